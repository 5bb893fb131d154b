// rt_view.h -- launch interface of the view kernels (rt_view.hip): mi355rt_context_view_rays, mi355rt_context_render_view.
// Internal to libmi355rt.so, shared by rt_view.hip and rt_queries.cpp (the entry points).
#pragma once
#include "rt_device.h"
#include "rt_radiance.h"

namespace mi355rt {

// A view as its kernels read it: launch constants, passed as kernel arguments (scalar loads, no memory of the caller's is read for it).
// Pixel p = y * width + x of the view's own width x height image; sample s of it draws from rng.start(ykey lo, ykey hi, x, s), ykey = y + seed.
struct ViewParams {
    DevCamera cam;
    float width_f, height_f;     // (float)width, (float)height: u = (x + ju) / width_f, IEEE division
    uint32_t width;
    uint32_t centre;             // MI355RT_VIEW_CENTRE: both jitters 0.5, the lens point (0, 0)
    float lens_radius, focus_distance;   // the thin lens
};
// k_view_rays: the rays of one sample, width * height mi355rt_path_ray records.
struct ViewRays {
    void* rays;
    uint32_t n_pixels, sample, seed_lo, seed_hi;
};
// The sum of a view: k_radiance_sum's chain over the pixels (RadianceSum::n_rays = width * height) and the optional packed image.
struct ViewSum {
    RadianceSum sum;
    uint32_t* out_packed;        // width * height words, color_to_u32(sqrt(mean)); may be null
};
constexpr uint32_t VIEW_MODELS = 2;                // MI355RT_VIEW_PINHOLE, _THIN_LENS
constexpr uint32_t VIEW_LENS_TRIES = 64;           // rejected tries of the lens point after which it is (0, 0)

// model: MI355RT_VIEW_* (plan_view refused every other value).  The path kernels are instantiated per model and per has_mesh; p.rays is not read.
int launch_view_rays(const ViewParams& v, const ViewRays& r, uint32_t model, void* stream);
int launch_view_paths(const RadianceParams& p, const ViewParams& v, const ViewSum& s, uint32_t model, bool has_mesh, uint32_t grid_paths, uint32_t grid_sum, void* stream);

}  // namespace mi355rt
