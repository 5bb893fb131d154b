// rt_radiance.hip -- radiance queries against the resident scene (mi355rt_context_trace_radiance): whole paths along caller-supplied rays.
//
// Kernels (gfx950, wave64; a translation unit of its own: the render and query kernels are not recompiled differently for it)
//   k_radiance_paths[_mesh]  trace_ray (renderer.rs:19-65) for (ray, sample) pairs: work item i * samples + (s - sample_begin) is sample s of ray i.
//                            A wave owns a block of 64 * K consecutive items and lane l the items l, l + 64, ... of it.  One trip of the loop is one
//                            ray SEGMENT of the lane's current path -- hit, then scatter or terminate -- and a lane whose path ended stores its
//                            radiance (three floats at scratch[3 * item], one 12-byte store) and starts its next item at the top of the next trip:
//                            the lanes REFILL themselves, so a wave idles behind its longest run of K paths, not behind the longest path of every
//                            64.  The assignment is static (no atomics, no LDS, no cross-lane traffic): the result cannot depend on K.  K = 1 is
//                            one item per lane.  The ray record is read as two 16-byte loads, the direction normalised once (Ray::new).
//   k_radiance_sum           per ray, the ordered sum of the chunk's samples (renderer.rs:100) continuing from the stored sum, the float4 sum
//                            written back and, optionally, sum * (1 / sample_end) (renderer.rs:85,103).  k_resolve's DPP row chain (rt_kernels.hip),
//                            restated: a 16-lane row owns a ray, lane s of the row loads sample c + s, the sequential sum runs along the row.
// 256-thread workgroups over plain grids.  The work per item is bounded by max_depth (a list walk per segment, the stackless BVH walk follows
// child and escape links only), so there is no work counter and no bounded wait -- and no watchdog.
// The top-level list is read with the wave-uniform loop index through the constant address space (scalar loads), whatever the rays are; the
// pieces are the render kernels' (rt_intersect.h, rt_materials.h, rt_rng.h are included, not copied): hit_scene<HAS_MESH>, surface_scatter --
// every material, the unit-ball rejection as the plain per-lane loop --, miss_colour with the sky lookup, RngCtrT.  The fold is the render's:
// throughput * terminal, front to back; an exhausted depth gives throughput * BLACK.
// ADDRESSING (MI355RT_RNG_CTR): ykey = row + seed (64 bit), rng.start(ykey lo, ykey hi, x, s); the path stands at ray 0, whose block 0 is NOT
// drawn here (it belongs to whoever made the ray: words 0 / 1 are the render's pixel jitter); the scatter event after ray r draws from ray r + 1.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rt_host.h"
#include "rt_device.h"
#include "rt_radiance.h"

#include "rt_math.h"
#include "rt_rng.h"
#include "rt_intersect.h"
#include "rt_materials.h"

namespace mi355rt {

struct Rad3 { float x, y, z; };                                                             // 12 bytes: one global_store_dwordx3

template <bool HAS_MESH>
DI void radiance_paths(const RadianceParams& P) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = (uint64_t)blockIdx.x * (RADIANCE_BLOCK_THREADS / 64u) + (threadIdx.x >> 6);
    const uint64_t first = wave * (64u * (uint64_t)P.items_per_lane);                       // the wave's block of items: [first, first + count)
    if (first >= (uint64_t)P.n_items) return;                                               // (64 bit: the last workgroup's blocks may start past 2^32)
    const uint32_t first32 = (uint32_t)first;
    const uint32_t count = min(64u * P.items_per_lane, P.n_items - first32);                // <= 4096; first32 + count <= n_items: no index below wraps
    cprim_t prims = (cprim_t)P.prims;
    const float4* __restrict__ rays = reinterpret_cast<const float4*>(P.rays);
    Rad3* __restrict__ out = reinterpret_cast<Rad3*>(P.scratch);
    const uint64_t seed = ((uint64_t)P.seed_hi << 32) | (uint64_t)P.seed_lo;
    uint32_t next = lane;                                                                   // offset of the lane's next item within the block
    bool live = false;
    uint32_t item = 0u, depth = 0u;
    f3 ro = mk(0.f, 0.f, 0.f), rd = mk(0.f, 0.f, 1.f), thr = mk(1.f, 1.f, 1.f);
    RngCtrT<true> rng; rng.clear();
    for (;;) {
        if (!live) {
            if (next >= count) break;
            item = first32 + next; next += 64u;
            const uint32_t i = item / P.samples, s = P.sample_begin + (item - i * P.samples);  // one division per path (items reach 2^32 - 1: no magic pair)
            const float4 r0 = rays[2u * (size_t)i], r1 = rays[2u * (size_t)i + 1u];
            ro = mk(r0.x, r0.y, r0.z);
            rd = normalized(mk(r1.x, r1.y, r1.z));                                          // Ray::new, ray.rs:12-17: once
            const uint64_t ykey = (uint64_t)__float_as_uint(r1.w) + seed;
            rng.start((uint32_t)ykey, (uint32_t)(ykey >> 32), __float_as_uint(r0.w), s);     // the path stands at ray 0
            thr = mk(1.f, 1.f, 1.f); depth = 0u; live = true;
            if (P.max_depth == 0u) { out[item] = Rad3{0.f, 0.f, 0.f}; live = false; continue; }   // depth == 0 -> 1 * BLACK (renderer.rs:19-21)
        }
        // one segment: renderer.rs:24-36
        f3 term; bool fin = false;
        Hit h;
        if (!hit_scene<HAS_MESH>(prims, P.n_prims, P.nodes, P.tris, ro, rd, h)) { term = miss_colour(P.sky, P.sky_w, P.sky_h, P.miss, rd); fin = true; }
        else {
            float4 q0;
            if constexpr (HAS_MESH) q0 = reinterpret_cast<const float4*>(P.mats + (h.mat_ff & 0x7FFFFFFFu))[0];
            else q0 = h.q0;                                                                 // (the mesh-free finish_hit read it with the hit record)
            rng.next_event(); rng.load_block0();                                            // the event after ray r draws from ray r + 1
            f3 no, nd, atten, emitted;
            if (!surface_scatter(P.mats, P.textures, q0, h, rd, rng, no, nd, atten, emitted)) { term = emitted; fin = true; }
            else {
                thr = thr * atten; ro = no; rd = nd; ++depth;                               // scattered rays as surface_scatter returns them
                if (depth == P.max_depth) { term = mk(0.f, 0.f, 0.f); fin = true; }         // next level has depth == 0 (renderer.rs:20-22): throughput * BLACK
            }
        }
        if (fin) { const f3 L = thr * term; out[item] = Rad3{L.x, L.y, L.z}; live = false; }
    }
}

__global__ void __launch_bounds__(RADIANCE_BLOCK_THREADS) k_radiance_paths(const RadianceParams P) { radiance_paths<false>(P); }
__global__ void __launch_bounds__(RADIANCE_BLOCK_THREADS) k_radiance_paths_mesh(const RadianceParams P) { radiance_paths<true>(P); }

// The row chain of k_resolve (rt_kernels.hip): T = row_shr:1(T) + x, fifteen times.  Lane k's value is final after step k and every later step
// recomputes exactly the same sum, so no select is needed; lane 0 reads 0 from outside the row (bound_ctrl) and 0 + (acc + x0) is exact.  Samples
// past the chunk enter as +0, which leaves a sum unchanged -- unless the sum is -0: a running sum that started at +0 never is, and a stored sum
// that is -0 (only a caller could have put it there) becomes +0, which compares equal.
DI float radiance_row_shr1_zero(float v) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x111, 0xF, 0xF, true)); }
DI float radiance_row_ror1(float v) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x121, 0xF, 0xF, true)); }
__global__ void __launch_bounds__(RADIANCE_BLOCK_THREADS) k_radiance_sum(const RadianceSum S) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = ((uint64_t)blockIdx.x * RADIANCE_BLOCK_THREADS + threadIdx.x) >> 6;
    const uint32_t s = lane & 15u;
    const uint64_t ray = wave * 4u + (lane >> 4);                                           // this row's ray
    const bool valid = ray < (uint64_t)S.n_rays;
    const float* __restrict__ rad = S.scratch + 3u * (size_t)(valid ? ray : 0u) * S.samples;   // 3 floats per sample, a ray's samples back to back
    float4* __restrict__ accum = reinterpret_cast<float4*>(S.accum);
    f3 acc = mk(0.f, 0.f, 0.f);                                                             // meaningful in lane 0 of the row
    if (S.accum_load && valid) { const float4 a = accum[ray]; acc = mk(a.x, a.y, a.z); }
    for (uint32_t c = 0; c < S.samples; c += 16u) {
        f3 x = mk(0.f, 0.f, 0.f);
        if (valid && s < S.samples - c) {
            const float* q = rad + 3u * (size_t)(c + s);
            x = mk(__builtin_nontemporal_load(q), __builtin_nontemporal_load(q + 1), __builtin_nontemporal_load(q + 2));
        }
        if (s == 0u) x = acc + x;                                                           // renderer.rs:100 goes on where the previous 16 samples stopped
        f3 t = x;
#pragma unroll
        for (int k = 0; k < 15; ++k) t = mk(radiance_row_shr1_zero(t.x) + x.x, radiance_row_shr1_zero(t.y) + x.y, radiance_row_shr1_zero(t.z) + x.z);
        acc = mk(radiance_row_ror1(t.x), radiance_row_ror1(t.y), radiance_row_ror1(t.z));   // lane 0 <- lane 15: the sum so far
    }
    if (!valid || s != 0u) return;
    accum[ray] = make_float4(acc.x, acc.y, acc.z, 0.0f);
    if (S.out_linear) { const f3 mean = acc * S.inv_total; reinterpret_cast<Rad3*>(S.out_linear)[ray] = Rad3{mean.x, mean.y, mean.z}; }   // renderer.rs:103
}

int launch_radiance(const RadianceParams& p, const RadianceSum& s, bool has_mesh, uint32_t grid_paths, uint32_t grid_sum, void* stream) {
    if (p.n_items == 0u) return 0;
    hipStream_t st = (hipStream_t)stream;
    const dim3 block(RADIANCE_BLOCK_THREADS);
    if (has_mesh) hipLaunchKernelGGL(k_radiance_paths_mesh, dim3(grid_paths), block, 0, st, p); else hipLaunchKernelGGL(k_radiance_paths, dim3(grid_paths), block, 0, st, p);
    if (int e = (int)hipGetLastError()) return e;
    hipLaunchKernelGGL(k_radiance_sum, dim3(grid_sum), block, 0, st, s);
    return (int)hipGetLastError();
}

}  // namespace mi355rt

using namespace mi355rt;

// The three entry points of include/mi355rt.h, beside their kernels and behind the exception barrier.  What each does is the HIP-free half's
// (radiance_scratch_bytes, rt_prepare.cpp), the context's (context_trace_radiance, rt_api.cpp) and the host-buffer scaffold's (oneshot_trace_radiance, rt_oneshot.cpp).
extern "C" {

int mi355rt_radiance_scratch_bytes(uint32_t n_rays, uint32_t samples, uint64_t* out_bytes) {
    return guard([&]() -> int {
    return radiance_scratch_bytes(n_rays, samples, out_bytes);
    });
}

int mi355rt_context_trace_radiance(mi355rt_context* ctx, const mi355rt_radiance_params* params, const void* d_rays, uint32_t n_rays, void* d_accum, void* d_out_linear, void* d_scratch, void* hip_stream) {
    return guard([&]() -> int {
    return context_trace_radiance(ctx, params, d_rays, n_rays, d_accum, d_out_linear, d_scratch, hip_stream);
    });
}

int mi355rt_trace_radiance(const mi355rt_scene* scene, const mi355rt_radiance_params* params, const mi355rt_path_ray* rays, uint32_t n_rays, float* accum_in_out, float* out_linear) {
    return guard([&]() -> int {
    return oneshot_trace_radiance(scene, params, rays, n_rays, accum_in_out, out_linear);
    });
}

}  // extern "C"
