// svgf_plan.cpp -- the HIP-free half of libmi355rt_svgf.so: defaults, refusals, launch geometry (svgf_plan.h).
#include "svgf_plan.h"

#include <cmath>
#include <cstring>

namespace mi355rt_svgf {

namespace {

const mi355rt_svgf_accumulate_params accumulate_defaults = {32u, 0u, 0.9f, 0.05f, 4u, 5u, 0.05f, 0u};
const mi355rt_svgf_filter_params filter_defaults = {5u, 5u, 1.0f, 0.05f, 0u, 0u};

bool misaligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1u)) != 0u; }

// A view as the accumulation reads it: model known, a size, a finite camera.  "" or what is wrong with it.
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

uint32_t tiles_of(uint32_t width, uint32_t height, uint32_t& tiles_x) {
    tiles_x = (width + TILE_W - 1u) / TILE_W;
    return (uint32_t)((uint64_t)tiles_x * ((height + TILE_H - 1u) / TILE_H));    // (< 2^31: every tile holds a pixel)
}

}  // namespace

int plan_accumulate(int hip_device, const mi355rt_view* cur, const mi355rt_view* prev, const mi355rt_svgf_accumulate_params* params,
                    const void* hits_cur, const void* color_cur, const void* hits_prev, const void* hist_prev, const void* moments_prev,
                    const void* hist_out, const void* moments_out, const void* variance_out, AccumulatePlan& plan, std::string& why) {
    const auto bad = [&why](const std::string& text) { why = "accumulate: " + text; return MI355RT_ERR_INVALID; };
    plan = AccumulatePlan{};
    if (!cur) return bad("cur is null");
    { const std::string f = view_fault("cur", cur); if (!f.empty()) return bad(f); }
    if (prev) { const std::string f = view_fault("prev", prev); if (!f.empty()) return bad(f); }
    const mi355rt_svgf_accumulate_params p = params ? *params : accumulate_defaults;
    if (p.max_history < 1u || p.max_history > 65535u) return bad("params.max_history must be 1 .. 65535");
    if (p.flags != 0u) return bad("params.flags must be 0");
    if (!std::isfinite(p.normal_min) || p.normal_min < -1.0f || p.normal_min > 1.0f) return bad("params.normal_min must be finite and in [-1, 1]");
    if (!std::isfinite(p.plane_tolerance) || !(p.plane_tolerance > 0.0f)) return bad("params.plane_tolerance must be finite and positive");
    if (p.min_temporal < 1u || p.min_temporal > p.max_history) return bad("params.min_temporal must be 1 .. params.max_history");
    if (p.normal_squarings > 8u) return bad("params.normal_squarings must be 0 .. 8");
    if (!std::isfinite(p.sigma_plane) || !(p.sigma_plane > 0.0f)) return bad("params.sigma_plane must be finite and positive");
    if (p.reserved != 0u) return bad("params.reserved must be 0");
    if (!hits_cur) return bad("d_hits_cur is null");
    if (!color_cur) return bad("d_color_cur is null");
    if (!hist_out) return bad("d_hist_out is null");
    if (!moments_out) return bad("d_moments_out is null");
    if (!variance_out) return bad("d_variance_out is null");
    if (misaligned_to(hits_cur, 16)) return bad("d_hits_cur must be 16-byte aligned");
    if (misaligned_to(color_cur, 4)) return bad("d_color_cur must be 4-byte aligned");
    if (misaligned_to(hist_out, 16)) return bad("d_hist_out must be 16-byte aligned");
    if (misaligned_to(moments_out, 8)) return bad("d_moments_out must be 8-byte aligned");
    if (misaligned_to(variance_out, 4)) return bad("d_variance_out must be 4-byte aligned");
    if (prev) {
        if (!hits_prev) return bad("d_hits_prev is null but prev is given");
        if (!hist_prev) return bad("d_hist_prev is null but prev is given");
        if (!moments_prev) return bad("d_moments_prev is null but prev is given");
        if (misaligned_to(hits_prev, 16)) return bad("d_hits_prev must be 16-byte aligned");
        if (misaligned_to(hist_prev, 16)) return bad("d_hist_prev must be 16-byte aligned");
        if (misaligned_to(moments_prev, 8)) return bad("d_moments_prev must be 8-byte aligned");
        if (hist_out == hist_prev) return bad("d_hist_out must not be d_hist_prev (the taps gather neighbours)");
        if (moments_out == moments_prev) return bad("d_moments_out must not be d_moments_prev (the taps gather neighbours)");
    } else {
        if (hits_prev) return bad("d_hits_prev is given without prev");
        if (hist_prev) return bad("d_hist_prev is given without prev");
        if (moments_prev) return bad("d_moments_prev is given without prev");
    }
    if (hip_device < 0) return bad("hip_device is negative");

    AccumulateConsts& k = plan.k;
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
    k.n_tiles = tiles_of(k.width, k.height, k.tiles_x);
    k.max_history_f = (float)p.max_history; k.normal_min = p.normal_min; k.plane_tolerance = p.plane_tolerance;
    k.min_temporal_f = (float)p.min_temporal; k.sigma_plane = p.sigma_plane; k.normal_squarings = p.normal_squarings;
    plan.grid = k.n_tiles < MAX_BLOCKS ? k.n_tiles : MAX_BLOCKS;
    return MI355RT_OK;
}

int plan_filter(int hip_device, uint32_t width, uint32_t height, const mi355rt_svgf_filter_params* params,
                const void* hist_in, const void* variance_in, const void* hits, const void* scratch, const void* out_linear, const void* out_packed,
                FilterPlan& plan, std::string& why) {
    const auto bad = [&why](const std::string& text) { why = "filter: " + text; return MI355RT_ERR_INVALID; };
    plan = FilterPlan{};
    if (width == 0u) return bad("width is 0");
    if (height == 0u) return bad("height is 0");
    if ((uint64_t)width * height >= (1ull << 31)) return bad("width * height must be below 2^31");
    const mi355rt_svgf_filter_params p = params ? *params : filter_defaults;
    if (p.levels > 8u) return bad("params.levels must be 0 .. 8");
    if (p.normal_squarings > 8u) return bad("params.normal_squarings must be 0 .. 8");
    if (!std::isfinite(p.sigma_luminance) || !(p.sigma_luminance > 0.0f)) return bad("params.sigma_luminance must be finite and positive");
    const float sl2 = p.sigma_luminance * p.sigma_luminance;
    if (!std::isfinite(sl2) || !(sl2 > 0.0f)) return bad("params.sigma_luminance must have a finite, positive square");
    if (!std::isfinite(p.sigma_plane) || !(p.sigma_plane > 0.0f)) return bad("params.sigma_plane must be finite and positive");
    if ((p.flags & ~MI355RT_SVGF_GATHERS_ONLY) != 0u) return bad("params.flags has an unknown bit");
    if (p.reserved != 0u) return bad("params.reserved must be 0");
    if (!hist_in) return bad("d_hist_in is null");
    if (!variance_in) return bad("d_variance_in is null");
    if (!hits) return bad("d_hits is null");
    if (!scratch) return bad("d_scratch is null");
    if (!out_linear && !out_packed) return bad("d_out_linear and d_out_packed are both null");
    if (misaligned_to(hist_in, 16)) return bad("d_hist_in must be 16-byte aligned");
    if (misaligned_to(variance_in, 4)) return bad("d_variance_in must be 4-byte aligned");
    if (misaligned_to(hits, 16)) return bad("d_hits must be 16-byte aligned");
    if (misaligned_to(scratch, 16)) return bad("d_scratch must be 16-byte aligned");
    if (misaligned_to(out_linear, 4)) return bad("d_out_linear must be 4-byte aligned");
    if (misaligned_to(out_packed, 4)) return bad("d_out_packed must be 4-byte aligned");
    if (p.levels == 0u) {                                // the copy has no pass through the scratch, and a lane's output lies in another lane's history pixel
        if (out_linear == hist_in) return bad("d_out_linear must not be d_hist_in when params.levels is 0");
        if (out_packed == hist_in) return bad("d_out_packed must not be d_hist_in when params.levels is 0");
    }
    if (hip_device < 0) return bad("hip_device is negative");

    plan.width = width; plan.height = height;
    plan.n_tiles = tiles_of(width, height, plan.tiles_x);
    plan.grid = plan.n_tiles < MAX_BLOCKS ? plan.n_tiles : MAX_BLOCKS;
    plan.grid_px = (width * height + BLOCK_THREADS - 1u) / BLOCK_THREADS;
    plan.levels = p.levels; plan.normal_squarings = p.normal_squarings;
    plan.sl2 = sl2; plan.sigma_plane = p.sigma_plane;
    plan.staged = (p.flags & MI355RT_SVGF_GATHERS_ONLY) == 0u;
    return MI355RT_OK;
}

int plan_scratch_bytes(uint32_t width, uint32_t height, uint64_t* out_bytes, std::string& why) {
    const auto bad = [&why](const std::string& text) { why = "scratch_bytes: " + text; return MI355RT_ERR_INVALID; };
    if (!out_bytes) return bad("out_bytes is null");
    *out_bytes = 0u;
    if (width == 0u) return bad("width is 0");
    if (height == 0u) return bad("height is 0");
    if ((uint64_t)width * height >= (1ull << 31)) return bad("width * height must be below 2^31");
    *out_bytes = (uint64_t)width * height * SCRATCH_PER_PIXEL;
    return MI355RT_OK;
}

}  // namespace mi355rt_svgf
