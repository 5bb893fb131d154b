// post_plan.cpp -- the HIP-free half of mi355rt_post_reproject: defaults, refusals, launch geometry (post_plan.h).
#include "post_plan.h"

#include <cmath>
#include <cstring>

namespace mi355rt_post {

namespace {

const mi355rt_reproject_params defaults = {32u, 0u, 0.9f, 0.05f};

bool misaligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1u)) != 0u; }

// A view as the reprojection reads it: model known, a size, a finite camera.  "" or what is wrong with it.
std::string view_fault(const char* name, const mi355rt_view* v) {
    const std::string n(name);
    if (v->model != MI355RT_VIEW_PINHOLE && v->model != MI355RT_VIEW_THIN_LENS) return n + ".model is unknown";
    if (v->width == 0u) return n + ".width is 0";
    if (v->height == 0u) return n + ".height is 0";
    const mi355rt_camera& c = v->camera;
    for (int i = 0; i < 3; ++i)
        if (!std::isfinite(c.position[i]) || !std::isfinite(c.forward[i]) || !std::isfinite(c.right[i]) || !std::isfinite(c.true_up[i])) return n + ".camera must be finite";
    if (!std::isfinite(c.half_width) || !std::isfinite(c.half_height)) return n + ".camera must be finite";
    if ((uint64_t)v->width * v->height >= (1ull << 31)) return n + ".width * " + n + ".height must be below 2^31";
    return std::string();
}

}  // namespace

int plan_reproject(int hip_device, const mi355rt_view* cur, const mi355rt_view* prev, const mi355rt_reproject_params* params,
                   const void* hits_cur, const void* color_cur, const void* hits_prev, const void* hist_prev,
                   const void* hist_out, const void* out_linear, const void* out_packed, ReprojectPlan& plan, std::string& why) {
    const auto bad = [&why](const std::string& text) { why = "reproject: " + text; return MI355RT_ERR_INVALID; };
    plan = ReprojectPlan{};
    if (!cur) return bad("cur is null");
    { const std::string f = view_fault("cur", cur); if (!f.empty()) return bad(f); }
    if (prev) { const std::string f = view_fault("prev", prev); if (!f.empty()) return bad(f); }
    const mi355rt_reproject_params p = params ? *params : defaults;
    if (p.max_history < 1u || p.max_history > 65535u) return bad("params.max_history must be 1 .. 65535");
    if (p.flags != 0u) return bad("params.flags must be 0");
    if (!std::isfinite(p.normal_min) || p.normal_min < -1.0f || p.normal_min > 1.0f) return bad("params.normal_min must be finite and in [-1, 1]");
    if (!std::isfinite(p.plane_tolerance) || !(p.plane_tolerance > 0.0f)) return bad("params.plane_tolerance must be finite and positive");
    if (!hits_cur) return bad("d_hits_cur is null");
    if (!color_cur) return bad("d_color_cur is null");
    if (!hist_out) return bad("d_hist_out is null");
    if (misaligned_to(hits_cur, 16)) return bad("d_hits_cur must be 16-byte aligned");
    if (misaligned_to(color_cur, 4)) return bad("d_color_cur must be 4-byte aligned");
    if (misaligned_to(hist_out, 16)) return bad("d_hist_out must be 16-byte aligned");
    if (misaligned_to(out_linear, 4)) return bad("d_out_linear must be 4-byte aligned");
    if (misaligned_to(out_packed, 4)) return bad("d_out_packed must be 4-byte aligned");
    if (prev) {
        if (!hits_prev) return bad("d_hits_prev is null but prev is given");
        if (!hist_prev) return bad("d_hist_prev is null but prev is given");
        if (misaligned_to(hits_prev, 16)) return bad("d_hits_prev must be 16-byte aligned");
        if (misaligned_to(hist_prev, 16)) return bad("d_hist_prev must be 16-byte aligned");
        if (hist_out == hist_prev) return bad("d_hist_out must not be d_hist_prev (the taps gather neighbours)");
    } else {
        if (hits_prev) return bad("d_hits_prev is given without prev");
        if (hist_prev) return bad("d_hist_prev is given without prev");
    }
    if (hip_device < 0) return bad("hip_device is negative");

    ReprojectConsts& k = plan.k;
    k.width = cur->width; k.height = cur->height;
    if (prev) {
        const mi355rt_camera& c = prev->camera;
        std::memcpy(k.position, c.position, sizeof k.position); std::memcpy(k.forward, c.forward, sizeof k.forward);
        std::memcpy(k.right, c.right, sizeof k.right); std::memcpy(k.true_up, c.true_up, sizeof k.true_up);
        k.half_width = c.half_width; k.half_height = c.half_height;
        k.prev_width = prev->width; k.prev_height = prev->height;
        k.prev_width_f = (float)prev->width; k.prev_height_f = (float)prev->height;
        k.has_prev = 1u;
    }
    k.tiles_x = (k.width + REPROJECT_TILE_W - 1u) / REPROJECT_TILE_W;
    const uint64_t n_tiles = (uint64_t)k.tiles_x * ((k.height + REPROJECT_TILE_H - 1u) / REPROJECT_TILE_H);   // (< 2^31: every tile holds a pixel)
    k.n_tiles = (uint32_t)n_tiles;
    k.max_history_f = (float)p.max_history; k.normal_min = p.normal_min; k.plane_tolerance = p.plane_tolerance;
    plan.grid = k.n_tiles < REPROJECT_MAX_BLOCKS ? k.n_tiles : REPROJECT_MAX_BLOCKS;
    return MI355RT_OK;
}

}  // namespace mi355rt_post
