// rt_range_wave_probe.h -- k_render_ctr_simple_qc's range arithmetic (rt_math.h) on whole waves whose lanes the caller chooses.
// Compiled into the tests' reference build only (included by rt_kernels_refs.hip behind rt_kernels.hip; -DMI355RT_REFS): the product library and its
// kernel hash do not contain it.
//
// Every range form tests its operands with a ballot over the wave's active lanes and sends the WHOLE wave to the guarded form, out of line, when one
// lane fails.  The enumerations of tools/verify/range_arithmetic.hip walk consecutive floats, so their waves are all inside or all outside a range but
// at a boundary.  Here a lane reads a record -- active or not, a raw direction, a ray origin -- and runs the shipped functions on it with the RANGE
// bits of one of three selectors: normalized_ranged, ray_direction, and, with that direction and the record's origin, hit_quad and hit_cube on two
// primitive records the caller supplies (as walk_list calls them: BOUNDED, `wide` from walk_origin_wide, the cube's reciprocals FIRST).  An inactive
// lane is outside the branch that calls them, as a lane that is not live is outside the walk: the ballots see a partial exec mask.
// tests/test_gpu_range_wave.py builds the waves (all lanes ordinary; one odd lane among 63 ordinary ones; half the lanes inactive) and compares every
// word of selectors 1 and 2 with selector 0, the guarded forms, and the directions with a numpy restatement.
#pragma once

#include <vector>

#include "../device/rt_host.h"

namespace mi355rt {

struct RangeProbeIn { float v[3], ro[3]; uint32_t flags, pad[9]; };                                    // 16 words; flags bit 0: the lane is active
struct RangeProbeOut { float once[3], rd[3], quad_hit, quad_t, cube_hit, cube_t, cube_po[3]; uint32_t quad_idx, cube_idx, pad; };   // 16 words; an inactive lane writes zeros
static_assert(sizeof(RangeProbeIn) == 64 && sizeof(RangeProbeOut) == 64, "range probe records");

template <uint32_t RANGE>
__global__ void __launch_bounds__(BLOCK_THREADS) k_probe_range_wave(const DevPrim* __restrict__ prims_, const RangeProbeIn* __restrict__ in, RangeProbeOut* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;                        // (the entry pads the records to whole workgroups)
    cprim_t prims = (cprim_t)(prims_);                                               // [0] the quad, [1] the cube: wave-uniform reads, as in the walk
    const RangeProbeIn r = in[i];
    RangeProbeOut o{};
    if ((r.flags & 1u) != 0u) {
        const f3 raw = mk(r.v[0], r.v[1], r.v[2]), ro = mk(r.ro[0], r.ro[1], r.ro[2]);
        const f3 once = normalized_ranged<true, RANGE>(raw);
        const f3 rd = ray_direction<true, RANGE>(raw);
        Cand cq; cand_reset(cq);
        const bool wide = walk_origin_wide(ro);
        const bool hq = hit_quad<true, true, RANGE>(prims, 0u, ro, rd, EPS, cq, wide);
        CandP cc; cand_reset(cc);
        const bool hc = hit_cube<true, true, true, RANGE>(prims + 1, 1u, ro, rd, EPS, cc);
        o.once[0] = once.x; o.once[1] = once.y; o.once[2] = once.z;
        o.rd[0] = rd.x; o.rd[1] = rd.y; o.rd[2] = rd.z;
        o.quad_hit = hq ? 1.0f : 0.0f; o.quad_t = cq.t; o.quad_idx = cq.idx;
        o.cube_hit = hc ? 1.0f : 0.0f; o.cube_t = cc.t; o.cube_idx = cc.idx;
        o.cube_po[0] = cc.po.x; o.cube_po[1] = cc.po.y; o.cube_po[2] = cc.po.z;
    }
    out[i] = o;
}

// selector 0: the guarded forms (RANGE 0: what every other kernel and the all-off library run); 1: the bits the library ships (MI355RT_QC_RANGE);
// 2: all four steps, so that a step whose define is 0 stays under test.
constexpr uint32_t RANGE_PROBE_BITS[3] = {0u, MI355RT_QC_RANGE, RANGE_RENORM_CLOSED | RANGE_NORM_RANGED | RANGE_QUAD_NOFIX | RANGE_CUBE_NOFIX};

}  // namespace mi355rt

// Not in the public header; the reference build's diagnostic entry.
// mi355rt_debug_range_wave: host pointers.  quad_d = the 16 words of a quad's DevPrim::d that hit_quad reads, cube_d = the first 28 of a cube's (w2o,
// zd, a pad word, o2w); records = n RangeProbeIn, 64 to a wave in the order given; out = n RangeProbeOut; range_bits (may be null) receives the RANGE
// bits behind `selector`.  The last workgroup is padded with inactive lanes.  Synchronous; every buffer is freed before it returns.
extern "C" int mi355rt_debug_range_wave(uint32_t selector, const float* quad_d, const float* cube_d, const void* records, uint32_t n, void* out, uint32_t* range_bits, int device) {
    using namespace mi355rt;
    return guard([&]() -> int {
    if (selector >= 3u || !quad_d || !cube_d || !records || !out || !n) return fail(MI355RT_ERR_INVALID, "debug_range_wave: selector / null / empty");
    if (n > (1u << 24)) return fail(MI355RT_ERR_INVALID, "debug_range_wave: at most 2^24 records");
    if (range_bits) *range_bits = RANGE_PROBE_BITS[selector];
    DevPrim prims[2] = {};
    prims[0].kind = MI355RT_PRIM_QUAD; prims[0].run_end = 1u;
    prims[1].kind = MI355RT_PRIM_CUBE; prims[1].run_end = 2u;
    for (int k = 0; k < 16; ++k) prims[0].d[k] = quad_d[k];
    for (int k = 0; k < 28; ++k) prims[1].d[k] = cube_d[k];
    const RangeProbeIn* in = static_cast<const RangeProbeIn*>(records);
    const uint32_t padded = (n + BLOCK_THREADS - 1u) / BLOCK_THREADS * BLOCK_THREADS;
    std::vector<RangeProbeIn> host(padded);                                         // (value-initialised: the padding's flags are 0)
    for (uint32_t i = 0; i < n; ++i) host[i] = in[i];
    HIP_TRY(hipSetDevice(device));
    DevBuf<RangeProbeIn> d_in; DevBuf<RangeProbeOut> d_out; DevBuf<DevPrim> d_prims;
    int rc = d_in.ensure(padded);
    if (!rc) rc = d_out.ensure(padded);
    if (!rc) rc = d_prims.ensure(2);
    hipError_t e = hipSuccess;
    if (!rc) e = hipMemcpy(d_in.p, host.data(), (size_t)padded * sizeof(RangeProbeIn), hipMemcpyHostToDevice);
    if (!rc && e == hipSuccess) e = hipMemcpy(d_prims.p, prims, sizeof(prims), hipMemcpyHostToDevice);
    if (!rc && e == hipSuccess) {
        const dim3 grid(padded / BLOCK_THREADS), block(BLOCK_THREADS);
        if (selector == 0u) hipLaunchKernelGGL(k_probe_range_wave<RANGE_PROBE_BITS[0]>, grid, block, 0, nullptr, d_prims.p, d_in.p, d_out.p);
        else if (selector == 1u) hipLaunchKernelGGL(k_probe_range_wave<RANGE_PROBE_BITS[1]>, grid, block, 0, nullptr, d_prims.p, d_in.p, d_out.p);
        else hipLaunchKernelGGL(k_probe_range_wave<RANGE_PROBE_BITS[2]>, grid, block, 0, nullptr, d_prims.p, d_in.p, d_out.p);
        e = hipGetLastError();
    }
    if (!rc && e == hipSuccess) e = hipMemcpy(out, d_out.p, (size_t)n * sizeof(RangeProbeOut), hipMemcpyDeviceToHost);
    if (!rc && e != hipSuccess) rc = fail(MI355RT_ERR_HIP, std::string("debug_range_wave: ") + hipGetErrorString(e));
    d_in.release(); d_out.release(); d_prims.release();
    return rc;
    });
}
