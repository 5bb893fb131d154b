// rt_probe.hip -- surface probes of the resident scene (mi355rt_context_probe_rays, mi355rt_context_probe_radiance): cosine-hemisphere rays leaving
// caller-supplied surface points are MADE on the device, in front of the radiance queries' path loop -- the radiance form of the ambient-occlusion pass.
//
// Kernels (gfx950, wave64; a translation unit of its own: no other kernel is recompiled differently for it)
//   k_probe_rays          one lane per probe: the ray of sample `sample`, written as the two float4 of a mi355rt_path_ray (origin, x; direction
//                         normalised ONCE, row) -- what mi355rt_context_trace_radiance and _trace_rays read.
//   k_probe_paths[_mesh]  radiance_paths (rt_radiance_paths.h: the loop of k_radiance_paths, not a copy) with the ray made in the refill instead of
//                         loaded: item = probe * samples + (s - sample_begin); the probe's two 16-byte loads, rng.start, the unit-ball point from
//                         words 1 / 2 / 3 of (ray 0, block j) -- the render draws only words 0 / 1 of block 0 there, and never the blocks j >= 1 --,
//                         the Lambert bounce's direction (diffuse_finish) and origin (scatter_origin), Ray::new's normalisation on top -- then the
//                         path stands at ray 0 exactly as the query's does.
//   k_probe_sum           radiance_sum<false>: k_radiance_sum's chain, instantiated here (no new branch in an old kernel).
// The work per item is bounded: max_depth segments and at most PROBE_TRIES generator blocks, so there is no watchdog here either.
// Every formula below is include/mi355rt.h's definition, in float32 in the order written (-ffp-contract=off); + - * / sqrt and compares only.
// Kernels and launch_* functions only: the entry points stand in rt_queries.cpp, which binds the context's scene to these launches.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rt_device.h"
#include "rt_probe.h"

#include "rt_radiance_paths.h"                                                              // radiance_paths<HAS_MESH, Source>, radiance_sum<PACK>

namespace mi355rt {

// What a probe record holds: position and normal (used as given) and the stream address.
struct ProbeRec { f3 pos, n; uint32_t x, row; };
DI ProbeRec probe_load(const float4* __restrict__ probes, uint32_t i) {
    const float4 r0 = probes[2u * (size_t)i], r1 = probes[2u * (size_t)i + 1u];
    ProbeRec b;
    b.pos = mk(r0.x, r0.y, r0.z); b.n = mk(r1.x, r1.y, r1.z);
    b.x = __float_as_uint(r0.w); b.row = __float_as_uint(r1.w);
    return b;
}

// The ray of sample s of a probe: the bounce a white Lambert surface at (P, N) would make, if that event were addressed at ray 0.  The generator
// here is the maker's own: the path loop starts the same stream again (the same arithmetic on the same words: the compiler keeps one copy).
DI void probe_make_ray(const ProbeRec& b, uint32_t s, uint64_t ykey, f3& ro, f3& rd) {
    RngCtrT<true> rng;
    rng.start((uint32_t)ykey, (uint32_t)(ykey >> 32), b.x, s);
    rng.load_block0();                                                                      // (ray 0, block 0): try 0
    uint32_t blk[4] = {rng.b0[0], rng.b0[1], rng.b0[2], rng.b0[3]};
    f3 p;
    for (uint32_t j = 0u;;) {                                                               // random_in_unit_sphere (vec3.rs:54-61), bounded: try j from words 1 / 2 / 3 of block j
        p = mk(u32_to_range11(blk[1]), u32_to_range11(blk[2]), u32_to_range11(blk[3]));
        if (len2(p) < 1.0f) break;
        if (++j == PROBE_TRIES) { p = mk(0.f, 0.f, 0.f); break; }                           // bounded work per item
        RngCtrT<true>::block(rng.w, j, blk);
    }
    Hit h; h.p = b.pos; h.n = b.n;
    ro = scatter_origin(h, EPS);                                                            // P + N * EPSILON
    rd = normalized(diffuse_finish(h, p));                                                  // material.rs:54-62: N + normalized(p), N where that is near zero
}

DI void probe_rays(const ProbeParams& B, const ProbeRaysOut& R) {
    const uint32_t i = blockIdx.x * RADIANCE_BLOCK_THREADS + threadIdx.x;
    if (i >= R.n) return;                                                                   // lanes past the probes do nothing
    const ProbeRec b = probe_load(reinterpret_cast<const float4*>(B.probes), i);
    f3 ro, rd;
    probe_make_ray(b, R.sample, (uint64_t)b.row + (((uint64_t)R.seed_hi << 32) | (uint64_t)R.seed_lo), ro, rd);
    float4* __restrict__ o = reinterpret_cast<float4*>(R.rays) + 2u * (size_t)i;
    o[0] = make_float4(ro.x, ro.y, ro.z, __uint_as_float(b.x));
    o[1] = make_float4(rd.x, rd.y, rd.z, __uint_as_float(b.row));
}

// The ray source of radiance_paths for probes: "ray" i of the loop is probe i.  Ray::new normalises what the maker made (the second normalisation).
struct ProbeRays {
    typedef ProbeParams Arg;
    const float4* __restrict__ probes;
    DI ProbeRays(const RadianceParams&, const ProbeParams& b) : probes(reinterpret_cast<const float4*>(b.probes)) {}
    DI PathStart start(uint32_t i, uint32_t s, uint64_t seed) const {
        const ProbeRec b = probe_load(probes, i);
        PathStart a;
        a.x = b.x; a.ykey = (uint64_t)b.row + seed;
        probe_make_ray(b, s, a.ykey, a.ro, a.rd);
        a.rd = normalized(a.rd);                                                            // Ray::new, ray.rs:12-17
        return a;
    }
};

__global__ void __launch_bounds__(RADIANCE_BLOCK_THREADS) k_probe_rays(const ProbeParams B, const ProbeRaysOut R) { probe_rays(B, R); }
__global__ void __launch_bounds__(RADIANCE_BLOCK_THREADS) k_probe_paths(const RadianceParams P, const ProbeParams B) { radiance_paths<false, ProbeRays>(P, B); }
__global__ void __launch_bounds__(RADIANCE_BLOCK_THREADS) k_probe_paths_mesh(const RadianceParams P, const ProbeParams B) { radiance_paths<true, ProbeRays>(P, B); }

__global__ void __launch_bounds__(RADIANCE_BLOCK_THREADS) k_probe_sum(const RadianceSum S) { radiance_sum<false>(S, nullptr); }

int launch_probe_rays(const ProbeParams& b, const ProbeRaysOut& r, void* stream) {
    if (r.n == 0u) return 0;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((uint32_t)(((uint64_t)r.n + RADIANCE_BLOCK_THREADS - 1u) / RADIANCE_BLOCK_THREADS)), block(RADIANCE_BLOCK_THREADS);
    hipLaunchKernelGGL(k_probe_rays, grid, block, 0, st, b, r);
    return (int)hipGetLastError();
}

int launch_probe_paths(const RadianceParams& p, const ProbeParams& b, const RadianceSum& s, bool has_mesh, uint32_t grid_paths, uint32_t grid_sum, void* stream) {
    if (p.n_items == 0u) return 0;
    hipStream_t st = (hipStream_t)stream;
    const dim3 block(RADIANCE_BLOCK_THREADS), grid(grid_paths);
    if (has_mesh) hipLaunchKernelGGL(k_probe_paths_mesh, grid, block, 0, st, p, b); else hipLaunchKernelGGL(k_probe_paths, grid, block, 0, st, p, b);
    if (int e = (int)hipGetLastError()) return e;
    hipLaunchKernelGGL(k_probe_sum, dim3(grid_sum), block, 0, st, s);
    return (int)hipGetLastError();
}

}  // namespace mi355rt
