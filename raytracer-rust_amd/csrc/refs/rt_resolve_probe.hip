// rt_resolve_probe.hip -- the kernels behind a finished path (k_resolve, k_gather_strips, k_gather_accum) on caller-supplied buffers.
// Compiled into the tests' reference build only (build.build_device_variant("refs"), -DMI355RT_REFS): the product library and its kernel
// hash do not contain it.
//
// Nothing is restated here: mi355rt_debug_resolve / mi355rt_debug_gather fill ResolveParams / GatherParams / GatherAccumParams from their
// arguments and call the shipped launch_resolve / launch_gather_strips / launch_gather_accum (rt_kernels.hip), the launchers the renders
// call, and the magic pair of `width` is the library's magic_div (rt_prepare.h); tests/test_gpu_resolve_stage.py checks every pixel's place under a
// row table.
// Every pointer is a DEVICE address of the current device and is used as it is: the caller sizes the buffers
// (tests/test_gpu_resolve_stage.py states the extents next to each call).  Both calls wait for the kernel before they return.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../device/rt_device.h"
#include "../device/rt_host.h"

namespace mi355rt {

struct ResolveProbeArgs {                              // 64 B; device.ResolveProbeArgs has the same layout
    uint64_t radiance, out_packed, out_linear, accum, out_row;   // ResolveParams' pointers (out_linear, accum, out_row may be 0)
    uint32_t accum_load, band_pixel0, band_pixels, spp;
    float inv_spp;
    uint32_t width;                                     // with out_row: the image width (its magic pair is computed here); else unused
};
static_assert(sizeof(ResolveProbeArgs) == 64, "ResolveProbeArgs");
struct ResolveMaskedProbeArgs {                        // 88 B; device.ResolveMaskedProbeArgs has the same layout
    ResolveProbeArgs plain;
    uint64_t cam_mask;                                  // ResolveParams.cam_mask: band_pixels words, one per band pixel (0: no table)
    float miss[3];                                      // ResolveParams.miss
    uint32_t pad;
};
static_assert(sizeof(ResolveMaskedProbeArgs) == 88, "ResolveMaskedProbeArgs");
struct GatherProbeArgs {                                // 64 B; device.GatherProbeArgs has the same layout
    uint64_t src_row;                                   // n_rows entries
    uint64_t src_packed, dst_packed, src_linear, dst_linear;     // GatherParams (src_packed 0: no k_gather_strips launch)
    uint64_t accum_src, accum_dst;                      // GatherAccumParams (accum_src 0: no k_gather_accum launch)
    uint32_t n_rows, width;
};
static_assert(sizeof(GatherProbeArgs) == 64, "GatherProbeArgs");

}  // namespace mi355rt

using namespace mi355rt;

// One k_resolve launch for both entries below; cam_mask / miss as ResolveParams takes them.
static int resolve_probe(const ResolveProbeArgs& a, const uint32_t* cam_mask, const float* miss);

// Not in the public header; the reference build's diagnostic entries.
extern "C" int mi355rt_debug_resolve(const void* args) {
    return guard([&]() -> int {
    if (!args) return fail(MI355RT_ERR_INVALID, "debug_resolve: null");
    return resolve_probe(*static_cast<const ResolveProbeArgs*>(args), nullptr, nullptr);
    });
}
// ... and with the band's camera-mask words: a pixel whose word is 0 is resolved from `miss`, its samples are not read (k_resolve, RESOLVE_SKIP).
extern "C" int mi355rt_debug_resolve_masked(const void* args) {
    return guard([&]() -> int {
    if (!args) return fail(MI355RT_ERR_INVALID, "debug_resolve_masked: null");
    const ResolveMaskedProbeArgs m = *static_cast<const ResolveMaskedProbeArgs*>(args);
    return resolve_probe(m.plain, reinterpret_cast<const uint32_t*>(m.cam_mask), m.miss);
    });
}
static int resolve_probe(const ResolveProbeArgs& a, const uint32_t* cam_mask, const float* miss) {
    {
    if (!a.radiance || !a.out_packed || !a.spp) return fail(MI355RT_ERR_INVALID, "debug_resolve: radiance, out_packed and spp are required");
    if ((uint64_t)a.band_pixel0 + a.band_pixels >= (1ull << 31)) return fail(MI355RT_ERR_INVALID, "debug_resolve: pixel numbers stay below 2^31");
    if (a.out_row && !a.width) return fail(MI355RT_ERR_INVALID, "debug_resolve: out_row needs the width");
    if (a.accum_load && !a.accum) return fail(MI355RT_ERR_INVALID, "debug_resolve: accum_load without accum");
    if (a.accum & 15u) return fail(MI355RT_ERR_INVALID, "debug_resolve: accum must start on 16 bytes");
    ResolveParams r{};
    r.radiance = reinterpret_cast<const float*>(a.radiance);
    r.out_packed = reinterpret_cast<uint32_t*>(a.out_packed);
    r.out_linear = reinterpret_cast<float*>(a.out_linear);
    r.accum = reinterpret_cast<float*>(a.accum);
    r.accum_load = a.accum_load;
    r.band_pixel0 = a.band_pixel0; r.band_pixels = a.band_pixels; r.spp = a.spp;
    r.inv_spp = a.inv_spp;
    r.out_row = reinterpret_cast<const uint32_t*>(a.out_row);
    r.width = a.width;
    magic_div(a.width, r.width_mul, r.width_shift);
    r.cam_mask = cam_mask;
    if (miss) { r.miss[0] = miss[0]; r.miss[1] = miss[1]; r.miss[2] = miss[2]; }
    if (a.band_pixels && launch_resolve(r, nullptr) != 0) return fail(MI355RT_ERR_HIP, "debug_resolve: k_resolve launch failed");
    HIP_TRY(hipStreamSynchronize(nullptr));
    return MI355RT_OK;
    }
}

extern "C" int mi355rt_debug_gather(const void* args) {
    return guard([&]() -> int {
    if (!args) return fail(MI355RT_ERR_INVALID, "debug_gather: null");
    const GatherProbeArgs a = *static_cast<const GatherProbeArgs*>(args);
    if (!a.src_row || !a.width) return fail(MI355RT_ERR_INVALID, "debug_gather: the row table and the width are required");
    if (a.src_packed && !a.dst_packed) return fail(MI355RT_ERR_INVALID, "debug_gather: dst_packed");
    if ((a.src_linear != 0) != (a.dst_linear != 0)) return fail(MI355RT_ERR_INVALID, "debug_gather: the linear planes come together");
    if ((a.accum_src != 0) != (a.accum_dst != 0) || ((a.accum_src | a.accum_dst) & 15u))
        return fail(MI355RT_ERR_INVALID, "debug_gather: the sums come together and start on 16 bytes");
    if (a.src_packed) {
        GatherParams g{};
        g.src_row = reinterpret_cast<const uint32_t*>(a.src_row);
        g.src_packed = reinterpret_cast<const uint32_t*>(a.src_packed); g.dst_packed = reinterpret_cast<uint32_t*>(a.dst_packed);
        g.src_linear = reinterpret_cast<const uint32_t*>(a.src_linear); g.dst_linear = reinterpret_cast<uint32_t*>(a.dst_linear);
        g.n_rows = a.n_rows; g.width = a.width;
        if (launch_gather_strips(g, nullptr) != 0) return fail(MI355RT_ERR_HIP, "debug_gather: k_gather_strips launch failed");
    }
    if (a.accum_src) {
        GatherAccumParams ga{};
        ga.src_row = reinterpret_cast<const uint32_t*>(a.src_row);
        ga.src = reinterpret_cast<const uint32_t*>(a.accum_src); ga.dst = reinterpret_cast<uint32_t*>(a.accum_dst);
        ga.n_rows = a.n_rows; ga.width = a.width;
        if (launch_gather_accum(ga, nullptr) != 0) return fail(MI355RT_ERR_HIP, "debug_gather: k_gather_accum launch failed");
    }
    HIP_TRY(hipStreamSynchronize(nullptr));
    return MI355RT_OK;
    });
}
