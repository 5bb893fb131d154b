// rt_occlusion.h -- launch interface of the occlusion kernels (rt_occlusion.hip): mi355rt_context_occluded / mi355rt_context_ambient_occlusion.
// Internal to libmi355rt.so, shared by rt_occlusion.hip and rt_queries.cpp.  Both queries are defined in include/mi355rt.h.
#pragma once
#include "rt_device.h"

namespace mi355rt {

// One occlusion query per lane against the resident scene: is the closest hit of {origin, direction} nearer than t_max?  The launch reads the
// scene arrays and its segments and writes words [0, n): no workspace, no counters, no error word.
// may_exit (both launches): the host found every number the hit tests read from the scene inside +-OCCLUSION_BOUND (rt_prepare.h
// scene_within_occlusion_bound), so that a ray inside the same bound cannot produce a NaN candidate and a wave may leave the list once all its rays are
// decided.  0: the whole list is walked for every ray.
struct OcclusionParams {
    const DevPrim* prims; const DevNode* nodes; const DevTri* tris;
    const void* segments;        // n mi355rt_segment records (32 B, 16-byte aligned)
    uint32_t* out;               // n words, 0 / 1, every one written
    uint32_t n_prims;
    uint32_t n;
    uint32_t may_exit;
};

// Ambient occlusion at the first hits: `samples` occlusion queries per selected pixel, made and counted in the kernel.
enum : uint32_t { AO_FORM_SPREAD = 0, AO_FORM_PIXEL_PER_LANE = 1 };
struct AoLaunch {
    const DevPrim* prims; const DevNode* nodes; const DevTri* tris;
    const void* hits;            // n mi355rt_hit records (48 B, 16-byte aligned): what mi355rt_context_first_hits wrote for the same rows
    float* out;                  // n floats, every one written
    const uint32_t* rows;        // local output row -> absolute image row y (the first_hits table of the selection)
    uint32_t n_prims;
    uint32_t n;                  // selected rows * width (< 2^31)
    uint32_t width, width_mul, width_shift;   // image width and its magic pair (pixel -> local row)
    uint32_t samples, log2_samples;           // a power of two, 1 .. 256
    uint32_t seed;
    float radius;
    uint32_t may_exit;
    uint32_t form;               // AO_FORM_*: how (pixel, sample) pairs are dealt to lanes; the result does not depend on it
};
constexpr uint32_t OCCLUSION_BLOCK_THREADS = 256;
constexpr float OCCLUSION_BOUND = 65536.0f;    // 2^16: products of four such numbers and a division by EPSILON stay far below 2^127

// has_mesh: the list holds a mesh (set_scene knows) -- the `_mesh` kernels walk the BVHs per lane, the others are the mesh-free instantiation.
int launch_occluded(const OcclusionParams& p, bool has_mesh, void* stream);
int launch_ambient_occlusion(const AoLaunch& p, bool has_mesh, void* stream);

}  // namespace mi355rt
