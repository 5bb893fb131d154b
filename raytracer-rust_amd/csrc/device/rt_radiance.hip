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
// The loop and the sum themselves stand in rt_radiance_paths.h as templates (radiance_paths<HAS_MESH, Source>, radiance_sum<PACK>), shared with the
// camera views (rt_view.hip), whose ray source makes the ray where this file's loads it; the kernels here are instruction for instruction what they
// were with the bodies in this file (profiles/isa_diff_views_vs_parent.txt).
// ADDRESSING (MI355RT_RNG_CTR): ykey = row + seed (64 bit), rng.start(ykey lo, ykey hi, x, s); the path stands at ray 0, whose block 0 is NOT
// drawn here (it belongs to whoever made the ray: words 0 / 1 are the render's pixel jitter); the scatter event after ray r draws from ray r + 1.
// Kernels and launch_* functions only: the entry points stand in rt_queries.cpp, which binds the context's scene to these launches.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rt_device.h"
#include "rt_radiance.h"

#include "rt_radiance_paths.h"                                                              // the loop and the sum, shared with rt_view.hip: radiance_paths<HAS_MESH, Source>, radiance_sum<PACK>

namespace mi355rt {

__global__ void __launch_bounds__(RADIANCE_BLOCK_THREADS) k_radiance_paths(const RadianceParams P) { radiance_paths<false, LoadedRays>(P, LoadedRays::Arg{}); }
__global__ void __launch_bounds__(RADIANCE_BLOCK_THREADS) k_radiance_paths_mesh(const RadianceParams P) { radiance_paths<true, LoadedRays>(P, LoadedRays::Arg{}); }

__global__ void __launch_bounds__(RADIANCE_BLOCK_THREADS) k_radiance_sum(const RadianceSum S) { radiance_sum<false>(S, nullptr); }

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
