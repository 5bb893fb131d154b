// rt_radiance.h -- launch interface of the radiance-query kernels (rt_radiance.hip): mi355rt_context_trace_radiance.
// Internal to libmi355rt.so, shared by rt_radiance.hip and rt_queries.cpp (the entry points; mi355rt_trace_radiance, the host-buffer call: rt_oneshot.cpp).
#pragma once
#include "rt_device.h"

namespace mi355rt {

// Whole paths along caller-supplied rays (renderer.rs:19-65), one (ray, sample) pair per work item; item i * samples + (s - sample_begin) leaves
// its radiance as three floats at scratch[3 * item].  The launch reads the scene arrays and its rays and writes the caller's scratch: no workspace
// of the context, no counters, no error word.
struct RadianceParams {
    const DevPrim* prims; const DevMat* mats; const DevNode* nodes; const DevTri* tris;
    const float* sky; const DevTexture* textures;   // as RenderParams: null sky = the constant miss colour
    const void* rays;            // n_rays mi355rt_path_ray records (32 B, 16-byte aligned)
    float* scratch;              // 3 floats per item
    uint32_t sky_w, sky_h, n_prims;
    uint32_t n_items;            // n_rays * samples (< 2^32: plan_radiance)
    uint32_t samples;            // sample_end - sample_begin
    uint32_t sample_begin, max_depth;
    uint32_t items_per_lane;     // K: a wave owns 64 * K consecutive items, lane l the items l, l + 64, ... of them (1 = one item per lane)
    uint32_t seed_lo, seed_hi;
    float miss[3];
};
// The ordered sum of a ray's samples (renderer.rs:100) over the chunk's scratch, continuing from the stored sum.
struct RadianceSum {
    const float* scratch;        // what the paths kernel wrote
    float* accum;                // n_rays float4 running sums: read when accum_load, always written
    float* out_linear;           // n_rays * 3 floats, sum * inv_total; may be null
    uint32_t n_rays, samples, accum_load;
    float inv_total;             // 1.0f / (float)sample_end
};
constexpr uint32_t RADIANCE_BLOCK_THREADS = 256;
constexpr uint32_t RADIANCE_ITEMS_MAX = 64;
// The shipped K (diagnostic knob "radiance_items", 0 = this): the fastest of {1, 2, 4, 8, 16} on cornell's camera rays, 800 x 600 x 16 at depth 30 --
// 3.34 / 2.88 / 2.49 / 2.40 / 2.62 ms per call, the spread of a figure below 3 % (profiles/radiance_bench.txt).
constexpr uint32_t RADIANCE_ITEMS_DEFAULT = 8;

// has_mesh: the list holds a mesh (set_scene knows) -- k_radiance_paths_mesh walks the BVHs per lane, k_radiance_paths is hit_scene's mesh-free instantiation.
// grid_paths / grid_sum: plan_radiance's (rt_prepare.h).  The sum is enqueued behind the paths on the same stream.
int launch_radiance(const RadianceParams& p, const RadianceSum& s, bool has_mesh, uint32_t grid_paths, uint32_t grid_sum, void* stream);

}  // namespace mi355rt
