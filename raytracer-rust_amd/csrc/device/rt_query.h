// rt_query.h -- launch interface of the ray-query kernels (rt_query.hip): mi355rt_context_trace_rays / mi355rt_context_first_hits.
// Internal to libmi355rt.so, shared by rt_query.hip and rt_queries.cpp.
#pragma once
#include "rt_device.h"

namespace mi355rt {

// One closest-hit query per lane against the resident scene: HittableList::hit with t_min = EPSILON, t_max = INFINITY (renderer.rs:24).
// The launch reads the scene arrays and its rays and writes records [0, n): no workspace, no counters, no error word.
struct QueryParams {
    const DevPrim* prims; const DevNode* nodes; const DevTri* tris;
    const void* rays;            // n mi355rt_ray records (32 B, 16-byte aligned); null: camera rays through pixel centres
    void* hits;                  // n mi355rt_hit records (48 B, 16-byte aligned), every word written
    const uint32_t* rows;        // camera form: local output row -> absolute image row y
    uint32_t n_prims;
    uint32_t n;                  // rays, or selected rows * width
    DevCamera cam;               // camera form
    uint32_t width, width_mul, width_shift;   // image width and its magic pair (pixel -> local row)
    float width_f, height_f;     // (float)width, (float)height: exact, both below 2^24
};
constexpr uint32_t QUERY_BLOCK_THREADS = 256;

// has_mesh: the list holds a mesh (set_scene knows) -- k_query_*_mesh walks the BVHs per lane, the other form is hit_scene's mesh-free instantiation.
int launch_query(const QueryParams& p, bool has_mesh, void* stream);

}  // namespace mi355rt
