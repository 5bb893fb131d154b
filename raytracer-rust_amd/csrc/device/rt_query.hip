// rt_query.hip -- closest-hit ray queries against the resident scene (mi355rt_context_trace_rays, mi355rt_context_first_hits).
//
// Kernels (gfx950, wave64; a translation unit of its own: the render kernels of rt_kernels.hip are not recompiled differently for it)
//   k_query_rays[_mesh]     one caller-supplied ray per lane: two loads at the 16-byte halves of consecutive 32-byte records (written as 16-byte
//                           loads; the compiler drops the unread pad words: two global_load_dwordx3), Ray::new's one normalisation
//                           (ray.rs:12-17), HittableList::hit (hittable.rs:45-58), three 16-byte stores of the 48-byte record.
//   k_query_pixels[_mesh]   the same record for the ray through the centre of every selected pixel: the ray is made in the kernel
//                           (Camera::get_ray, camera.rs:33-42, then Ray::new) from the pixel index, nothing is read but the row table.
// 256-thread workgroups over a plain grid of ceil(n / 256): the work per ray is bounded (the list is walked once, the stackless BVH walk
// follows child and escape links only), so there is no work counter, no LDS, no atomic and no bounded wait -- and no watchdog.
// The top-level list is read with the wave-uniform loop index through the constant address space (scalar loads), whatever the rays are;
// `_mesh` is hit_scene<true>'s walk (per-lane BVH traversal), the other form hit_scene<false>'s (short division / reciprocals, the cube's
// object-space point carried) -- the functions, flags and therefore the bits of the render kernels (rt_intersect.h is included, not copied).
// The ray source is a template argument, not a branch: see DESIGN.md 4.6.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "rt_device.h"
#include "rt_query.h"

#include "rt_math.h"
#include "rt_rng.h"
#include "rt_intersect.h"
#include "rt_materials.h"

namespace mi355rt {

// hit_scene() (rt_intersect.h) with the winner's list index kept: the same candidate walk and the same finish_hit instantiation
// (each kind finishes through the shared tail on mesh-free lists, on its own with meshes), minus the material head nobody reads here.
template <bool HAS_MESH>
DI uint32_t query_hit(cprim_t prims, uint32_t n_prims, const DevNode* __restrict__ nodes, const DevTri* __restrict__ tris, f3 ro, f3 rd, Hit& best) {
    typename std::conditional<!HAS_MESH, CandP, Cand>::type c; cand_reset(c);
    walk_list<HAS_MESH>(prims, n_prims, nodes, tris, ro, rd, c);
    if (c.idx == CAND_NONE) return CAND_NONE;
    finish_hit<HAS_MESH, !HAS_MESH, false>((const DevPrim*)prims, tris, c, ro, rd, best);
    return c.idx;
}

template <bool HAS_MESH, bool CAMERA>
DI void query(const QueryParams& P) {
    const uint32_t i = blockIdx.x * QUERY_BLOCK_THREADS + threadIdx.x;
    if (i >= P.n) return;                                                               // lanes past n do nothing
    f3 ro, rd;
    if constexpr (CAMERA) {
        const uint32_t jrow = P.width_mul ? (__umulhi(i, P.width_mul) >> P.width_shift) : i;        // i / width (host magic pair, i < 2^31)
        const uint32_t x = i - jrow * P.width, y = P.rows[jrow];
        const float u = ((float)x + 0.5f) / P.width_f, v = ((float)y + 0.5f) / P.height_f;          // the pixel centre; IEEE division
        camera_ray(P.cam, u, v, ro, rd);                                                            // camera.rs:33-42, ray.rs:12-17
    } else {
        const float4* __restrict__ r = reinterpret_cast<const float4*>(P.rays) + 2u * (size_t)i;
        const float4 r0 = r[0], r1 = r[1];
        ro = mk(r0.x, r0.y, r0.z);
        rd = normalized(mk(r1.x, r1.y, r1.z));                                                      // Ray::new, ray.rs:12-17: once
    }
    Hit h;
    const uint32_t prim = query_hit<HAS_MESH>((cprim_t)P.prims, P.n_prims, P.nodes, P.tris, ro, rd, h);
    uint4 w0, w1, w2;
    if (prim != CAND_NONE) {
        w0 = make_uint4(__float_as_uint(h.p.x), __float_as_uint(h.p.y), __float_as_uint(h.p.z), __float_as_uint(h.t));
        w1 = make_uint4(__float_as_uint(h.n.x), __float_as_uint(h.n.y), __float_as_uint(h.n.z), h.mat_ff >> 31);
        w2 = make_uint4(prim, h.mat_ff & 0x7FFFFFFFu, 0u, 0u);
    } else {
        w0 = make_uint4(0u, 0u, 0u, __float_as_uint(__builtin_inff()));
        w1 = make_uint4(0u, 0u, 0u, 0u);
        w2 = make_uint4(MI355RT_NO_HIT, MI355RT_NO_HIT, 0u, 0u);
    }
    uint4* __restrict__ o = reinterpret_cast<uint4*>(P.hits) + 3u * (size_t)i;
    o[0] = w0; o[1] = w1; o[2] = w2;
}

__global__ void __launch_bounds__(QUERY_BLOCK_THREADS) k_query_rays(const QueryParams P) { query<false, false>(P); }
__global__ void __launch_bounds__(QUERY_BLOCK_THREADS) k_query_rays_mesh(const QueryParams P) { query<true, false>(P); }
__global__ void __launch_bounds__(QUERY_BLOCK_THREADS) k_query_pixels(const QueryParams P) { query<false, true>(P); }
__global__ void __launch_bounds__(QUERY_BLOCK_THREADS) k_query_pixels_mesh(const QueryParams P) { query<true, true>(P); }

int launch_query(const QueryParams& p, bool has_mesh, void* stream) {
    if (p.n == 0) return 0;
    const dim3 grid((uint32_t)(((uint64_t)p.n + QUERY_BLOCK_THREADS - 1u) / QUERY_BLOCK_THREADS)), block(QUERY_BLOCK_THREADS);   // (64-bit: n up to 2^32 - 1)
    hipStream_t s = (hipStream_t)stream;
    if (p.rays) {
        if (has_mesh) hipLaunchKernelGGL(k_query_rays_mesh, grid, block, 0, s, p); else hipLaunchKernelGGL(k_query_rays, grid, block, 0, s, p);
    } else {
        if (has_mesh) hipLaunchKernelGGL(k_query_pixels_mesh, grid, block, 0, s, p); else hipLaunchKernelGGL(k_query_pixels, grid, block, 0, s, p);
    }
    return (int)hipGetLastError();
}

}  // namespace mi355rt
