// rt_denoise.h -- launch interface of the denoise kernels (rt_denoise.hip): mi355rt_context_denoise / mi355rt_denoise.
// Internal to libmi355rt.so, shared by rt_denoise.hip and rt_queries.cpp.  The filter itself is defined in include/mi355rt.h.
#pragma once
#include "rt_prepare.h"

namespace mi355rt {

// The scratch of one call, DENOISE_SCRATCH_PER_PIXEL bytes per pixel in three planes (n = width * rows):
//   [0, 32 n)     guides: two 16-byte words per pixel, {normal.xyz, miss word (0 / 1)} and {position.xyz, t}
//   [32 n, 48 n)  colour image A, {r, g, b, 0} per pixel: the input (level 0 reads it), then every second level's result
//   [48 n, 64 n)  colour image B
struct DenoiseLaunch {
    const float* in;             // rows * width * 3 floats (4-byte aligned); read by the prepass only
    const void* hits;            // rows * width mi355rt_hit records (48 B, 16-byte aligned); read by the prepass only
    void* scratch;               // 16-byte aligned
    float* out_linear;           // rows * width * 3 floats or null; may be `in`
    uint32_t* out_packed;        // rows * width words or null
    uint32_t width, rows;
    DenoisePlan plan;
    int staged;                  // the form of the levels with step 1 and 2: 1 (the product) = the tile and its halo staged in LDS, 0 = global gathers like the later levels
};
constexpr uint32_t DENOISE_BLOCK_THREADS = 256;
constexpr uint32_t DENOISE_TILE_W = 32, DENOISE_TILE_H = 8;      // one pixel per lane: a wave is two rows of 32 pixels

// Enqueues the prepass and one launch per level (levels == 0: one copy launch) on `stream`.  Returns 0 or the hipError_t of the first failed launch.
int launch_denoise(const DenoiseLaunch& d, void* stream);

}  // namespace mi355rt
