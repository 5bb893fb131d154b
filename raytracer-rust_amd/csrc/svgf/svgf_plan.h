// svgf_plan.h -- what the calls of include/mi355rt_svgf.h decide before a device is involved: the defaults of their params, every refusal, and
// the launch geometry.  No HIP in here or in svgf_plan.cpp: the plans run, and are tested, on a machine without a GPU.
// Part of libmi355rt_svgf.so; everything lives in namespace mi355rt_svgf, so that a host that loads the other two libraries as well sees no symbol twice.
#pragma once

#include <stdint.h>

#include <string>

#include "../../../include/mi355rt_svgf.h"

namespace mi355rt_svgf {

constexpr uint32_t TILE_W = 32, TILE_H = 8, BLOCK_THREADS = TILE_W * TILE_H;   // one pixel per lane: a wave is two rows of 32 pixels
#ifndef MI355RT_SVGF_MAX_BLOCKS                          // (the tests' variant library builds with 3, so that a small frame walks every tile loop more than once; the product never defines it)
#define MI355RT_SVGF_MAX_BLOCKS (1u << 20)
#endif
constexpr uint32_t MAX_BLOCKS = MI355RT_SVGF_MAX_BLOCKS;  // a workgroup takes tiles blockIdx.x, blockIdx.x + gridDim.x, ...
static_assert(MAX_BLOCKS >= 1u, "a grid has at least one workgroup");
constexpr uint32_t SCRATCH_PER_PIXEL = 64;               // guides 32, image A 16, image B 16
constexpr uint32_t SPATIAL_MARK = 0xBF800000u;           // -1.0f: what k_svgf_accumulate leaves in variance_out for a pixel k_svgf_spatial has to estimate (no variance is negative)

// The constants of one accumulate: a by-value kernel argument (scalar loads).  The camera is prev's, as given.
struct AccumulateConsts {
    float position[3], forward[3], right[3], true_up[3];
    float half_width, half_height;
    float prev_width_f, prev_height_f;                   // (float)W', (float)H'
    uint32_t width, height, prev_width, prev_height;     // W, H, W', H'; W' = H' = 0 without a previous frame
    uint32_t tiles_x, n_tiles;
    float max_history_f, normal_min, plane_tolerance;
    uint32_t has_prev;
    float min_temporal_f, sigma_plane;
    uint32_t normal_squarings;
};

struct AccumulatePlan {
    AccumulateConsts k;
    uint32_t grid;                                       // workgroups of BLOCK_THREADS lanes, of both kernels
};

struct FilterPlan {
    uint32_t width, height, tiles_x, n_tiles, grid, grid_px;   // grid: of the level kernels (tiles); grid_px: of the prepass and the copy (pixels)
    uint32_t levels, normal_squarings;
    float sl2, sigma_plane;                              // sl2 = sigma_luminance * sigma_luminance (f32)
    bool staged;                                         // the levels with step 1 and 2 stage their tile and halo in LDS
};

// MI355RT_OK and the plan, or MI355RT_ERR_INVALID and, in `why`, a text that names the argument.
int plan_accumulate(int hip_device, const mi355rt_view* cur, const mi355rt_view* prev, const mi355rt_svgf_accumulate_params* params,
                    const void* hits_cur, const void* color_cur, const void* hits_prev, const void* hist_prev, const void* moments_prev,
                    const void* hist_out, const void* moments_out, const void* variance_out, AccumulatePlan& plan, std::string& why);
int plan_filter(int hip_device, uint32_t width, uint32_t height, const mi355rt_svgf_filter_params* params,
                const void* hist_in, const void* variance_in, const void* hits, const void* scratch, const void* out_linear, const void* out_packed,
                FilterPlan& plan, std::string& why);
int plan_scratch_bytes(uint32_t width, uint32_t height, uint64_t* out_bytes, std::string& why);

// svgf_kernels.hip: the kernels on `stream` of the current device.  0 or the hipError_t of the first failed launch.
struct AccumulateBuffers {
    const void* hits_cur; const void* color_cur; const void* hits_prev; const void* hist_prev; const void* moments_prev;
    void* hist_out; void* moments_out; void* variance_out;
};
struct FilterBuffers {
    const void* hist_in; const void* variance_in; const void* hits; void* scratch; void* out_linear; void* out_packed;
};
int launch_accumulate(const AccumulatePlan& plan, const AccumulateBuffers& b, void* stream);
int launch_filter(const FilterPlan& plan, const FilterBuffers& b, void* stream);

}  // namespace mi355rt_svgf
