// rt_view.hip -- camera views of the resident scene (mi355rt_context_view_rays, mi355rt_context_render_view): the rays of a pinhole or a thin lens
// are MADE on the device, in front of the radiance queries' path loop.
//
// Kernels (gfx950, wave64; a translation unit of its own: no other kernel is recompiled differently for it)
//   k_view_rays_<model>         one lane per pixel of the view: the ray of sample `sample`, written as the two float4 of a mi355rt_path_ray
//                               (origin, x; direction normalised ONCE, row) -- what mi355rt_context_trace_radiance and _trace_rays read.
//   k_view_paths_<model>[_mesh] radiance_paths (rt_radiance_paths.h: the loop of k_radiance_paths, not a copy) with the ray made in the refill instead
//                               of loaded: item = pixel * samples + (s - sample_begin); rng.start, block 0 of ray 0 for the jitter (words 0 / 1) and
//                               the lens (words 2 / 3; blocks j >= 1 of ray 0 for the rejected tries, which the render never draws), the model's ray
//                               maker, Ray::new's normalisation on top -- then the path stands at ray 0 exactly as the query's does.  One
//                               instantiation per model: a pinhole view does not pay for the rejection loop.
//   k_view_sum                  radiance_sum<true>: k_radiance_sum's chain, and color_to_u32(sqrt(mean)) per pixel where a packed image is asked for.
// The view arrives as kernel arguments (ViewParams: scalar loads of launch constants); nothing of the caller's is read for it.  The work per item is
// bounded: max_depth segments and at most VIEW_LENS_TRIES generator blocks, so there is no watchdog here either.
// Every formula below is include/mi355rt.h's definition, in float32 in the order written (-ffp-contract=off).
// Kernels and launch_* functions only: the entry points stand in rt_queries.cpp, which binds the context's scene to these launches.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rt_device.h"
#include "rt_view.h"

#include "rt_radiance_paths.h"                                                              // radiance_paths<HAS_MESH, Source>, radiance_sum<PACK>

namespace mi355rt {

DI f3 v3(const float (&a)[3]) { return mk(a[0], a[1], a[2]); }

// The ray of sample s of pixel (x, y): origin and the direction normalised once.  The generator here is the maker's own: the path loop starts the
// same stream again (the same arithmetic on the same words: the compiler keeps one copy) and stands at ray 0 of that sample.
template <uint32_t MODEL>
DI void view_make_ray(const ViewParams& V, uint32_t x, uint32_t y, uint32_t s, uint64_t ykey, f3& ro, f3& rd) {
    RngCtrT<true> rng;
    rng.start((uint32_t)ykey, (uint32_t)(ykey >> 32), x, s);
    float ju = 0.5f, jv = 0.5f;
    if (!V.centre) { rng.load_block0(); ju = rng.jitter_u(); jv = rng.jitter_v(); }         // (ray 0, block 0), words 0 / 1
    const float u = ((float)x + ju) / V.width_f, v = ((float)y + jv) / V.height_f;          // renderer.rs:96-99; IEEE division
    const f3 pos = v3(V.cam.position);
    if constexpr (MODEL == MI355RT_VIEW_PINHOLE) {
        ro = pos;
        rd = normalized(camera_raw(V.cam, u, v));                                           // camera.rs:33-42
    } else if constexpr (MODEL == MI355RT_VIEW_THIN_LENS) {
        float a = 0.0f, b = 0.0f;
        if (!V.centre) {                                                                    // the lens point: rejection in the unit disk, try j from words 2 / 3 of (ray 0, block j)
            uint32_t blk[4] = {rng.b0[0], rng.b0[1], rng.b0[2], rng.b0[3]};
            for (uint32_t j = 0u;;) {
                a = 2.0f * u32_to_f01(blk[2]) - 1.0f; b = 2.0f * u32_to_f01(blk[3]) - 1.0f;
                if (a * a + b * b < 1.0f) break;
                if (++j == VIEW_LENS_TRIES) { a = 0.0f; b = 0.0f; break; }                  // bounded work per item
                RngCtrT<true>::block(rng.w, j, blk);
            }
        }
        const f3 off = v3(V.cam.right) * (V.lens_radius * a) + v3(V.cam.true_up) * (V.lens_radius * b);
        ro = pos + off;
        rd = normalized(camera_raw(V.cam, u, v) * V.focus_distance - off);
    } else static_assert(MODEL == MI355RT_VIEW_PINHOLE || MODEL == MI355RT_VIEW_THIN_LENS, "a model needs its maker");
}

template <uint32_t MODEL>
DI void view_rays(const ViewParams& V, const ViewRays& R) {
    const uint32_t i = blockIdx.x * RADIANCE_BLOCK_THREADS + threadIdx.x;
    if (i >= R.n_pixels) return;                                                            // lanes past the image do nothing
    const uint32_t y = i / V.width, x = i - y * V.width;
    f3 ro, rd;
    view_make_ray<MODEL>(V, x, y, R.sample, (uint64_t)y + (((uint64_t)R.seed_hi << 32) | (uint64_t)R.seed_lo), ro, rd);
    float4* __restrict__ o = reinterpret_cast<float4*>(R.rays) + 2u * (size_t)i;
    o[0] = make_float4(ro.x, ro.y, ro.z, __uint_as_float(x));
    o[1] = make_float4(rd.x, rd.y, rd.z, __uint_as_float(y));
}

// The ray source of radiance_paths for a view: "ray" i of the loop is pixel i.  Ray::new normalises what the maker made (the render's second normalisation).
template <uint32_t MODEL>
struct MadeRays {
    typedef ViewParams Arg;                                                                 // the kernel's by-value view: scalar loads of launch constants
    const ViewParams& V;
    DI MadeRays(const RadianceParams&, const ViewParams& v) : V(v) {}
    DI PathStart start(uint32_t i, uint32_t s, uint64_t seed) const {
        PathStart a;
        const uint32_t y = i / V.width;
        a.x = i - y * V.width; a.ykey = (uint64_t)y + seed;
        view_make_ray<MODEL>(V, a.x, y, s, a.ykey, a.ro, a.rd);
        a.rd = normalized(a.rd);                                                            // Ray::new, ray.rs:12-17
        return a;
    }
};

#define MI_VIEW_KERNELS(NAME, MODEL) \
__global__ void __launch_bounds__(RADIANCE_BLOCK_THREADS) k_view_rays_##NAME(const ViewParams V, const ViewRays R) { view_rays<MODEL>(V, R); } \
__global__ void __launch_bounds__(RADIANCE_BLOCK_THREADS) k_view_paths_##NAME(const RadianceParams P, const ViewParams V) { radiance_paths<false, MadeRays<MODEL>>(P, V); } \
__global__ void __launch_bounds__(RADIANCE_BLOCK_THREADS) k_view_paths_##NAME##_mesh(const RadianceParams P, const ViewParams V) { radiance_paths<true, MadeRays<MODEL>>(P, V); }
MI_VIEW_KERNELS(pinhole, MI355RT_VIEW_PINHOLE)
MI_VIEW_KERNELS(thin_lens, MI355RT_VIEW_THIN_LENS)
#undef MI_VIEW_KERNELS

__global__ void __launch_bounds__(RADIANCE_BLOCK_THREADS) k_view_sum(const ViewSum S) { radiance_sum<true>(S.sum, S.out_packed); }

int launch_view_rays(const ViewParams& v, const ViewRays& r, uint32_t model, void* stream) {
    if (r.n_pixels == 0u) return 0;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((uint32_t)(((uint64_t)r.n_pixels + RADIANCE_BLOCK_THREADS - 1u) / RADIANCE_BLOCK_THREADS)), block(RADIANCE_BLOCK_THREADS);
    switch (model) {
    case MI355RT_VIEW_PINHOLE: hipLaunchKernelGGL(k_view_rays_pinhole, grid, block, 0, st, v, r); break;
    case MI355RT_VIEW_THIN_LENS: hipLaunchKernelGGL(k_view_rays_thin_lens, grid, block, 0, st, v, r); break;
    default: return -1;                                                                     // (plan_view refused it: a missing kernel is an error)
    }
    return (int)hipGetLastError();
}

int launch_view_paths(const RadianceParams& p, const ViewParams& v, const ViewSum& s, uint32_t model, bool has_mesh, uint32_t grid_paths, uint32_t grid_sum, void* stream) {
    if (p.n_items == 0u) return 0;
    hipStream_t st = (hipStream_t)stream;
    const dim3 block(RADIANCE_BLOCK_THREADS), grid(grid_paths);
    switch (model) {
    case MI355RT_VIEW_PINHOLE:
        if (has_mesh) hipLaunchKernelGGL(k_view_paths_pinhole_mesh, grid, block, 0, st, p, v); else hipLaunchKernelGGL(k_view_paths_pinhole, grid, block, 0, st, p, v);
        break;
    case MI355RT_VIEW_THIN_LENS:
        if (has_mesh) hipLaunchKernelGGL(k_view_paths_thin_lens_mesh, grid, block, 0, st, p, v); else hipLaunchKernelGGL(k_view_paths_thin_lens, grid, block, 0, st, p, v);
        break;
    default: return -1;
    }
    if (int e = (int)hipGetLastError()) return e;
    hipLaunchKernelGGL(k_view_sum, dim3(grid_sum), block, 0, st, s);
    return (int)hipGetLastError();
}

}  // namespace mi355rt
