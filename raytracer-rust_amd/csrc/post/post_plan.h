// post_plan.h -- what mi355rt_post_reproject (include/mi355rt_post.h) decides before a device is involved: the defaults of its params, every
// refusal, and the launch geometry.  No HIP in here or in post_plan.cpp: the plan runs, and is tested, on a machine without a GPU.
// Part of libmi355rt_post.so; everything lives in namespace mi355rt_post, so that a host that loads libmi355rt.so as well sees no symbol twice.
#pragma once

#include <stdint.h>

#include <string>

#include "../../../include/mi355rt_post.h"

namespace mi355rt_post {

constexpr uint32_t REPROJECT_TILE_W = 32, REPROJECT_TILE_H = 8, REPROJECT_BLOCK_THREADS = REPROJECT_TILE_W * REPROJECT_TILE_H;
constexpr uint32_t REPROJECT_MAX_BLOCKS = 1u << 20;      // a workgroup takes tiles blockIdx.x, blockIdx.x + gridDim.x, ...

// The constants of one launch: a by-value kernel argument (scalar loads).  The camera is prev's, as given.
struct ReprojectConsts {
    float position[3], forward[3], right[3], true_up[3];
    float half_width, half_height;
    float prev_width_f, prev_height_f;                   // (float)W', (float)H'
    uint32_t width, height, prev_width, prev_height;     // W, H, W', H'; W' = H' = 0 without a previous frame
    uint32_t tiles_x, n_tiles;
    float max_history_f, normal_min, plane_tolerance;
    uint32_t has_prev;
};

struct ReprojectPlan {
    ReprojectConsts k;
    uint32_t grid;                                       // workgroups of REPROJECT_BLOCK_THREADS lanes
};

// MI355RT_OK and the plan, or MI355RT_ERR_INVALID and, in `why`, a text that names the argument.
int plan_reproject(int hip_device, const mi355rt_view* cur, const mi355rt_view* prev, const mi355rt_reproject_params* params,
                   const void* hits_cur, const void* color_cur, const void* hits_prev, const void* hist_prev,
                   const void* hist_out, const void* out_linear, const void* out_packed, ReprojectPlan& plan, std::string& why);

// post_reproject.hip: k_post_reproject on `stream` of the current device.  0 or the hipError_t of the launch.
struct ReprojectBuffers {
    const void* hits_cur; const void* color_cur; const void* hits_prev; const void* hist_prev;
    void* hist_out; void* out_linear; void* out_packed;
};
int launch_reproject(const ReprojectPlan& plan, const ReprojectBuffers& b, void* stream);

}  // namespace mi355rt_post
