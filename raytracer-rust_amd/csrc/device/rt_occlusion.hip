// rt_occlusion.hip -- occlusion queries against the resident scene (mi355rt_context_occluded, mi355rt_context_ambient_occlusion).
//
// Kernels (gfx950, wave64; a translation unit of its own: the render and query kernels are not recompiled differently for it)
//   k_occluded[_mesh]        one caller-supplied segment per lane: two 16-byte loads of the 32-byte record (the last word is t_max), Ray::new's one
//                            normalisation (ray.rs:12-17), the list walk below, ONE 4-byte store of 0 / 1.
//   k_ao_spread[_mesh]       ambient occlusion, the samples of a pixel across the lanes of a wave: 64 / samples whole pixels per wave (samples <= 64) or
//                            one pixel over samples / 64 iterations; every lane makes its sample's ray (pcg4d, rt_rng.h), the occluded lanes are
//                            counted by ballot + popcount and the first lane of a pixel's group stores the float.
//   k_ao_lane[_mesh]         the same result with a pixel per lane looping over its samples (the A/B form; diagnostic knob "ao_form").
// 256-thread workgroups over a plain grid; the work per lane is bounded (a list walk per sample, the stackless BVH walk follows child and
// escape links only, 16 tries per direction), so there is no work counter, no LDS, no atomic and no bounded wait -- and no watchdog.
//
// THE WALK is HittableList::hit (hittable.rs:45-58) through the per-primitive tests of the render kernels (rt_intersect.h is included, not
// copied; FAST forms chosen as walk_list<HAS_MESH> chooses them): closest_so_far starts at INFINITY and shrinks, whatever t_max is -- Mesh::hit
// hands it to the BVH as an object-space bound, so another start would prune other triangles.  The answer is (closest t) < t_max, strict, f32.
// The one shortcut: the wave leaves the LIST (never a mesh's tree) once every active lane holds an accepted candidate below its t_max -- and
// only lanes whose ray, like the scene's records (may_exit, decided by the host), lies inside OCCLUSION_BOUND count as decided: within that
// bound no test can produce a NaN candidate, later candidates are only accepted at or below the current one, and the final t is below t_max
// as well.  A lane outside the bound keeps its whole wave in the list; its answer is the comparison at the end, like everyone's.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rt_device.h"
#include "rt_occlusion.h"

#include "rt_math.h"
#include "rt_rng.h"
#include "rt_intersect.h"

namespace mi355rt {

// Every component of the origin inside the bound, the (normalised) direction of a length in [1/2, 2]: NaN fails every comparison.
DI bool ray_within_bound(f3 ro, f3 rd) {
    const float l2 = dot(rd, rd);
    return fabsf(ro.x) <= OCCLUSION_BOUND && fabsf(ro.y) <= OCCLUSION_BOUND && fabsf(ro.z) <= OCCLUSION_BOUND && l2 >= 0.25f && l2 <= 4.0f;
}

// Called by the lanes that have a ray (the ballot covers the active lanes; the list index is wave-uniform: scalar loads).
template <bool HAS_MESH>
DI bool occluded(cprim_t prims, uint32_t n_prims, const DevNode* __restrict__ nodes, const DevTri* __restrict__ tris, f3 ro, f3 rd, float t_max, bool may_exit) {
    Cand c; cand_reset(c);
    const bool bounded = may_exit && ray_within_bound(ro, rd);
    bool done = false;                                                                      // wave-uniform
    uint32_t i = 0;
    while (i < n_prims && !done) {
#define MI_RUN(KIND, CALL) if (!done && i < n_prims && prims[i].kind == (KIND)) { const uint32_t end = min(prims[i].run_end, n_prims); \
            do { CALL; done = __ballot(!(bounded & (c.t < t_max))) == 0ull; } while (++i < end && !done); }
        MI_RUN(MI355RT_PRIM_QUAD,   hit_quad<!HAS_MESH>(prims + i, i, ro, rd, EPS, c))
        MI_RUN(MI355RT_PRIM_CUBE,   hit_cube<!HAS_MESH>(prims + i, i, ro, rd, EPS, c))
        MI_RUN(MI355RT_PRIM_SPHERE, hit_sphere(prims + i, i, ro, rd, EPS, c))
        MI_RUN(MI355RT_PRIM_PLANE,  hit_plane(prims + i, i, ro, rd, EPS, c))
        if (HAS_MESH) { MI_RUN(MI355RT_PRIM_MESH, hit_mesh(prims + i, i, nodes, tris, ro, rd, EPS, c)) }
        else if (!done && i < n_prims && prims[i].kind >= MI355RT_PRIM_MESH) ++i;           // cannot happen (the host picks this form only for mesh-free lists); keeps the loop finite
#undef MI_RUN
    }
    return c.t < t_max;                                                                     // no candidate: c.t == +inf, below no t_max
}

template <bool HAS_MESH>
DI void occluded_segments(const OcclusionParams& P) {
    const uint32_t i = blockIdx.x * OCCLUSION_BLOCK_THREADS + threadIdx.x;
    if (i >= P.n) return;                                                                   // lanes past n do nothing
    const float4* __restrict__ r = reinterpret_cast<const float4*>(P.segments) + 2u * (size_t)i;
    const float4 r0 = r[0], r1 = r[1];
    const f3 ro = mk(r0.x, r0.y, r0.z);
    const f3 rd = normalized(mk(r1.x, r1.y, r1.z));                                         // Ray::new, ray.rs:12-17: once
    P.out[i] = occluded<HAS_MESH>((cprim_t)P.prims, P.n_prims, P.nodes, P.tris, ro, rd, r1.w, P.may_exit != 0u) ? 1u : 0u;
}

// The ray of sample s of the pixel (x, y) whose first hit is (p, n): a point of the unit ball by rejection (16 tries, then the zero vector)
// added to the normal; mi355rt.h spells out every operation.
// Try j draws pcg4d(x, y, s * 16 + j, seed).  The generator's LCG step (rt_rng.h) is taken once: the caller passes x, y and seed already stepped
// (constant per pixel), and the third word runs, (s * 16 + j) * A + C = (s * 16 * A + C) + j * A: the same integers mod 2^32, the same draws.
DI f3 ao_direction(uint32_t x_stepped, uint32_t y_stepped, uint32_t s, uint32_t seed_stepped, f3 n) {
    f3 v = mk(0.f, 0.f, 0.f);
    uint32_t z = lcg_step(s * 16u);
    for (uint32_t j = 0; j < 16u; ++j, z += LCG_A) {
        uint32_t w[4]; pcg4d_stepped(x_stepped, y_stepped, z, seed_stepped, w);
        const f3 c = mk(u32_to_f01(w[0]) * 2.0f - 1.0f, u32_to_f01(w[1]) * 2.0f - 1.0f, u32_to_f01(w[2]) * 2.0f - 1.0f);
        if (dot(c, c) < 1.0f) { v = c; break; }
    }
    return normalized(n + v);                                                               // Ray::new: once
}

template <bool HAS_MESH, bool SPREAD>
DI void ambient_occlusion(const AoLaunch& P) {
    // SPREAD: a group of g = min(samples, 64) consecutive lanes shares a pixel; lane `sub` of the group takes samples sub, sub + 64, ...
    // (256 / g pixels per workgroup; the pixel index is made from the block index so that no 32-bit lane index is ever formed: lanes = n * g may pass 2^32)
    const uint32_t lg = SPREAD ? min(P.log2_samples, 6u) : 0u;
    const uint32_t pixel = (blockIdx.x << (8u - lg)) + (threadIdx.x >> lg), sub = threadIdx.x & ((1u << lg) - 1u);
    static_assert(OCCLUSION_BLOCK_THREADS == 256, "the pixel index above shifts by log2 of the workgroup size");
    const bool inside = pixel < P.n;
    f3 p = mk(0.f, 0.f, 0.f), n = p; bool live = false; uint32_t x = 0u, y = 0u;
    if (inside) {
        const uint4* __restrict__ h = reinterpret_cast<const uint4*>(P.hits) + 3u * (size_t)pixel;
        const uint4 h0 = h[0], h1 = h[1]; const uint32_t prim = h[2].x;
        p = mk(__uint_as_float(h0.x), __uint_as_float(h0.y), __uint_as_float(h0.z));
        n = mk(__uint_as_float(h1.x), __uint_as_float(h1.y), __uint_as_float(h1.z));
        live = prim != MI355RT_NO_HIT;
        const uint32_t jrow = P.width_mul ? (__umulhi(pixel, P.width_mul) >> P.width_shift) : pixel;   // pixel / width (host magic pair, pixel < 2^31)
        x = pixel - jrow * P.width; y = P.rows[jrow];
    }
    const uint32_t xs = lcg_step(x), ys = lcg_step(y), seeds = lcg_step(P.seed);            // the generator's step on the words a pixel's tries share, once
    uint32_t count = 0u;
    if constexpr (SPREAD) {
        const uint32_t lane = threadIdx.x & 63u, first = lane - sub;                        // the group's first lane
        const uint64_t group = lg == 6u ? ~0ull : ((1ull << (1u << lg)) - 1ull);
        for (uint32_t s = sub; s < P.samples; s += 64u) {                                   // samples / g iterations, the same for every lane
            bool occ = false;
            if (live) occ = occluded<HAS_MESH>((cprim_t)P.prims, P.n_prims, P.nodes, P.tris, p, ao_direction(xs, ys, s, seeds, n), P.radius, P.may_exit != 0u);
            count += (uint32_t)__popcll((__ballot(occ) >> first) & group);
        }
        if (sub != 0u) return;
    } else {
        if (live) for (uint32_t s = 0; s < P.samples; ++s)
            count += occluded<HAS_MESH>((cprim_t)P.prims, P.n_prims, P.nodes, P.tris, p, ao_direction(xs, ys, s, seeds, n), P.radius, P.may_exit != 0u) ? 1u : 0u;
    }
    if (inside) P.out[pixel] = live ? 1.0f - (float)count / (float)P.samples : 1.0f;
}

__global__ void __launch_bounds__(OCCLUSION_BLOCK_THREADS) k_occluded(const OcclusionParams P) { occluded_segments<false>(P); }
__global__ void __launch_bounds__(OCCLUSION_BLOCK_THREADS) k_occluded_mesh(const OcclusionParams P) { occluded_segments<true>(P); }
__global__ void __launch_bounds__(OCCLUSION_BLOCK_THREADS) k_ao_spread(const AoLaunch P) { ambient_occlusion<false, true>(P); }
__global__ void __launch_bounds__(OCCLUSION_BLOCK_THREADS) k_ao_spread_mesh(const AoLaunch P) { ambient_occlusion<true, true>(P); }
__global__ void __launch_bounds__(OCCLUSION_BLOCK_THREADS) k_ao_lane(const AoLaunch P) { ambient_occlusion<false, false>(P); }
__global__ void __launch_bounds__(OCCLUSION_BLOCK_THREADS) k_ao_lane_mesh(const AoLaunch P) { ambient_occlusion<true, false>(P); }

int launch_occluded(const OcclusionParams& p, bool has_mesh, void* stream) {
    if (p.n == 0) return 0;
    const dim3 grid((uint32_t)(((uint64_t)p.n + OCCLUSION_BLOCK_THREADS - 1u) / OCCLUSION_BLOCK_THREADS)), block(OCCLUSION_BLOCK_THREADS);   // (64-bit: n up to 2^32 - 1)
    hipStream_t s = (hipStream_t)stream;
    if (has_mesh) hipLaunchKernelGGL(k_occluded_mesh, grid, block, 0, s, p); else hipLaunchKernelGGL(k_occluded, grid, block, 0, s, p);
    return (int)hipGetLastError();
}

int launch_ambient_occlusion(const AoLaunch& p, bool has_mesh, void* stream) {
    if (p.n == 0) return 0;
    const bool spread = p.form == AO_FORM_SPREAD;
    // spread: n pixels of min(samples, 64) lanes each (< 2^31 * 2^6 lanes: the block count fits 32 bits, and so does every pixel index a lane computes)
    const uint64_t lanes = spread ? ((uint64_t)p.n << (p.log2_samples < 6u ? p.log2_samples : 6u)) : (uint64_t)p.n;
    const dim3 grid((uint32_t)((lanes + OCCLUSION_BLOCK_THREADS - 1u) / OCCLUSION_BLOCK_THREADS)), block(OCCLUSION_BLOCK_THREADS);
    hipStream_t s = (hipStream_t)stream;
    if (spread) { if (has_mesh) hipLaunchKernelGGL(k_ao_spread_mesh, grid, block, 0, s, p); else hipLaunchKernelGGL(k_ao_spread, grid, block, 0, s, p); }
    else { if (has_mesh) hipLaunchKernelGGL(k_ao_lane_mesh, grid, block, 0, s, p); else hipLaunchKernelGGL(k_ao_lane, grid, block, 0, s, p); }
    return (int)hipGetLastError();
}

}  // namespace mi355rt
