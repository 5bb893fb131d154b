// rt_prepare.cpp -- scene preparation and the other HIP-free host code of libmi355rt.so (rt_prepare.h): no HIP call, no context.
// Compiled with the device sources' flags (-ffp-contract=off: cube_normal_table repeats the device's operation order).
#include "rt_prepare.h"
#include "rt_occlusion.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <initializer_list>
#include <limits>
#include <utility>

using namespace mi355rt;

namespace {
thread_local std::string g_err;
}  // namespace

namespace mi355rt {

int fail(int code, const std::string& msg) { g_err = msg; return code; }
int fail_noexcept(int code, const char* msg) noexcept { try { g_err.assign(msg); } catch (...) { g_err.clear(); } return code; }
std::string& last_error() { return g_err; }

// Options of ABI version 4 are accepted as well: version 5 added entry points (mi355rt_multi_context_*), no struct changed.
int select_rows(const mi355rt_settings& st, const mi355rt_options* o, RowSel& sel) {
    uint32_t rb = 0, re = st.height, strip = 1, parts = 1, part = 0;
    if (o) {
        if (o->abi_version != MI355RT_ABI_VERSION && o->abi_version != 4u) return fail(MI355RT_ERR_INVALID, "options.abi_version mismatch");
        rb = o->row_begin; re = o->row_end ? o->row_end : st.height;
        strip = o->strip_rows ? o->strip_rows : 1; parts = o->n_parts ? o->n_parts : 1; part = o->part;
        if (o->rng_mode != MI355RT_RNG_CTR && o->rng_mode != MI355RT_RNG_REF) return fail(MI355RT_ERR_INVALID, "options.rng_mode");
    }
    if (re > st.height || rb > re || part >= parts) return fail(MI355RT_ERR_INVALID, "row selection out of range");
    sel.rows.clear();
    for (uint32_t y = rb; y < re; ++y) if ((y / strip) % parts == part) sel.rows.push_back(y);
    return MI355RT_OK;
}

int check_settings(const mi355rt_settings* st) {
    if (!st) return fail(MI355RT_ERR_INVALID, "settings is null");
    if (st->width == 0 || st->height == 0 || st->samples_per_pixel == 0) return fail(MI355RT_ERR_INVALID, "width/height/spp must be > 0");
    if ((uint64_t)st->width * st->height >= (1ull << 31)) return fail(MI355RT_ERR_INVALID, "image too large");
    if (st->width >= (1u << 24) || st->height >= (1u << 24)) return fail(MI355RT_ERR_INVALID, "width/height must be < 2^24 (x as f32 is exact, renderer.rs:96)");
    if (st->samples_per_pixel >= (1u << 30)) return fail(MI355RT_ERR_INVALID, "samples_per_pixel too large");
    return MI355RT_OK;
}

static int check_denoise_size(uint32_t width, uint32_t rows) {
    if (width == 0) return fail(MI355RT_ERR_INVALID, "denoise: width is 0");
    if (rows == 0) return fail(MI355RT_ERR_INVALID, "denoise: rows is 0");
    if ((uint64_t)width * rows >= (1ull << 31)) return fail(MI355RT_ERR_INVALID, "denoise: width * rows must be below 2^31");
    return MI355RT_OK;
}

int plan_denoise(uint32_t width, uint32_t rows, const mi355rt_denoise_params* params, DenoisePlan& plan) {
    if (int rc = check_denoise_size(width, rows)) return rc;
    const mi355rt_denoise_params defaults = {5u, 5u, 2.0f, 0.05f};
    const mi355rt_denoise_params& p = params ? *params : defaults;
    if (p.levels > DENOISE_MAX_LEVELS) return fail(MI355RT_ERR_INVALID, "denoise: params.levels must be 0 .. 8");
    if (p.normal_squarings > DENOISE_MAX_SQUARINGS) return fail(MI355RT_ERR_INVALID, "denoise: params.normal_squarings must be 0 .. 8");
    if (!(p.sigma_color > 0.0f) || !std::isfinite(p.sigma_color)) return fail(MI355RT_ERR_INVALID, "denoise: params.sigma_color must be positive and finite");
    if (!(p.sigma_plane > 0.0f) || !std::isfinite(p.sigma_plane)) return fail(MI355RT_ERR_INVALID, "denoise: params.sigma_plane must be positive and finite");
    plan.levels = p.levels; plan.normal_squarings = p.normal_squarings; plan.sigma_plane = p.sigma_plane;
    for (uint32_t k = 0; k < DENOISE_MAX_LEVELS; ++k) {
        const float sigma = p.sigma_color * std::ldexp(1.0f, -(int)k);   // 2^-k is exact: one rounding
        const float sq = sigma * sigma;
        plan.inv_sigma2[k] = 1.0f / sq;
    }
    return MI355RT_OK;
}

int check_denoise_buffers(const void* linear_in, const void* hits, const void* scratch, const void* out_linear, const void* out_packed) {
    const auto misaligned = [](const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1u)) != 0u; };
    if (!linear_in) return fail(MI355RT_ERR_INVALID, "denoise: d_linear_in is null");
    if (!hits) return fail(MI355RT_ERR_INVALID, "denoise: d_hits is null");
    if (!scratch) return fail(MI355RT_ERR_INVALID, "denoise: d_scratch is null");
    if (!out_linear && !out_packed) return fail(MI355RT_ERR_INVALID, "denoise: d_out_linear and d_out_packed are both null");
    if (misaligned(hits, 16)) return fail(MI355RT_ERR_INVALID, "denoise: d_hits must be 16-byte aligned");
    if (misaligned(scratch, 16)) return fail(MI355RT_ERR_INVALID, "denoise: d_scratch must be 16-byte aligned");
    if (misaligned(linear_in, 4)) return fail(MI355RT_ERR_INVALID, "denoise: d_linear_in must be 4-byte aligned");
    if (misaligned(out_linear, 4)) return fail(MI355RT_ERR_INVALID, "denoise: d_out_linear must be 4-byte aligned");
    if (misaligned(out_packed, 4)) return fail(MI355RT_ERR_INVALID, "denoise: d_out_packed must be 4-byte aligned");
    return MI355RT_OK;
}

int denoise_scratch_bytes(uint32_t width, uint32_t rows, uint64_t* out_bytes) {
    if (!out_bytes) return fail(MI355RT_ERR_INVALID, "denoise: out_bytes is null");
    if (int rc = check_denoise_size(width, rows)) return rc;
    *out_bytes = (uint64_t)width * rows * DENOISE_SCRATCH_PER_PIXEL;
    return MI355RT_OK;
}

static bool misaligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1u)) != 0u; }

int check_occluded_args(bool have_ctx, bool have_scene, const void* segments, uint32_t n, const void* out) {
    if (n != 0u) {
        if (!segments) return fail(MI355RT_ERR_INVALID, "occluded: d_segments is null");
        if (!out) return fail(MI355RT_ERR_INVALID, "occluded: d_out_u32 is null");
        if (misaligned_to(segments, 16)) return fail(MI355RT_ERR_INVALID, "occluded: d_segments must be 16-byte aligned");
        if (misaligned_to(out, 4)) return fail(MI355RT_ERR_INVALID, "occluded: d_out_u32 must be 4-byte aligned");
    }
    if (!have_ctx) return fail(MI355RT_ERR_INVALID, "occluded: ctx is null");
    if (!have_scene) return fail(MI355RT_ERR_INVALID, "occluded: context has no scene");
    return MI355RT_OK;
}

int plan_ambient_occlusion(bool have_ctx, bool have_scene, const mi355rt_settings& st, const mi355rt_options* opt, const mi355rt_ao_params* params,
                           const void* hits, const void* out, RowSel& sel, AoPlan& plan) {
    const mi355rt_ao_params defaults = {16u, 0u, std::numeric_limits<float>::infinity(), 0u};
    const mi355rt_ao_params& p = params ? *params : defaults;
    if (p.samples == 0u || p.samples > 256u || (p.samples & (p.samples - 1u)) != 0u) return fail(MI355RT_ERR_INVALID, "ambient_occlusion: params.samples must be a power of two, 1 .. 256");
    if (!(p.radius > 0.0f)) return fail(MI355RT_ERR_INVALID, "ambient_occlusion: params.radius must be positive (or +inf), not NaN");
    if (p._pad != 0u) return fail(MI355RT_ERR_INVALID, "ambient_occlusion: params._pad must be 0");
    if (opt && opt->abi_version != MI355RT_ABI_VERSION && opt->abi_version != 4u) return fail(MI355RT_ERR_INVALID, "ambient_occlusion: options.abi_version mismatch");
    if (opt && (opt->flags & ~MI355RT_FLAG_FIXED_AABB) != 0u) return fail(MI355RT_ERR_INVALID, "ambient_occlusion: options.flags has unknown bits");
    if (!have_ctx) return fail(MI355RT_ERR_INVALID, "ambient_occlusion: ctx is null");
    if (!have_scene) return fail(MI355RT_ERR_INVALID, "ambient_occlusion: context has no scene");
    {   mi355rt_options rows_only{};                                 // rng_mode, seed and workspace_bytes are not this call's business
        if (opt) { rows_only = *opt; rows_only.rng_mode = MI355RT_RNG_CTR; }
        if (int rc = select_rows(st, opt ? &rows_only : nullptr, sel)) return rc; }
    if (opt && (opt->flags & MI355RT_FLAG_FIXED_AABB) != 0u)
        return fail(MI355RT_ERR_UNSUPPORTED, "ambient_occlusion: MI355RT_FLAG_FIXED_AABB is not built for ray queries (they answer as the reference does)");
    if (!sel.rows.empty()) {
        if (!hits) return fail(MI355RT_ERR_INVALID, "ambient_occlusion: d_hits is null");
        if (!out) return fail(MI355RT_ERR_INVALID, "ambient_occlusion: d_out_f32 is null");
        if (misaligned_to(hits, 16)) return fail(MI355RT_ERR_INVALID, "ambient_occlusion: d_hits must be 16-byte aligned");
        if (misaligned_to(out, 4)) return fail(MI355RT_ERR_INVALID, "ambient_occlusion: d_out_f32 must be 4-byte aligned");
    }
    plan.samples = p.samples; plan.seed = p.seed; plan.radius = p.radius;
    plan.log2_samples = 0u; while ((1u << plan.log2_samples) < p.samples) ++plan.log2_samples;
    return MI355RT_OK;
}

// The radiance query's plan for `who` ("trace_radiance"; "render_view": the views run the same loop over made rays -- rays_name null, `rays` not looked at;
// "probe_radiance": the probes run it over rays made from the caller's records -- rays_name "d_probes").
static int radiance_items_bytes(const char* who, const char* what, uint64_t n_rays, uint32_t samples, uint64_t* out_bytes) {
    if (!out_bytes) return fail(MI355RT_ERR_INVALID, std::string(who) + ": out_bytes is null");
    if (n_rays >= (1ull << 32) || n_rays * samples >= (1ull << 32)) return fail(MI355RT_ERR_INVALID, std::string(who) + ": " + what + " must stay below 2^32 (split the call)");
    *out_bytes = (n_rays * samples * 12u + 15u) & ~15ull;         // (n_rays < 2^32 is tested first, so the product of two 32-bit numbers does not wrap)
    return MI355RT_OK;
}

int radiance_scratch_bytes(uint32_t n_rays, uint32_t samples, uint64_t* out_bytes) {
    return radiance_items_bytes("trace_radiance", "n_rays * samples", n_rays, samples, out_bytes);
}

static int plan_radiance_for(const char* who, const char* what, const char* rays_name, bool have_ctx, bool have_scene, const mi355rt_radiance_params* params, const void* rays,
                             uint64_t n_rays, const void* accum, const void* out_linear, const void* out_packed, const void* scratch, uint32_t items_knob,
                             uint32_t default_items, RadiancePlan& plan) {
    const auto bad = [who](const char* text) { return fail(MI355RT_ERR_INVALID, std::string(who) + ": " + text); };
    if (!params) return bad("params is null");
    if (params->flags != 0u) return bad("params.flags must be 0");
    if (params->reserved != 0u) return bad("params.reserved must be 0");
    if (params->sample_begin >= params->sample_end) return bad("params.sample_begin must be below params.sample_end");
    plan = RadiancePlan{};
    plan.samples = params->sample_end - params->sample_begin;
    if (n_rays != 0u) {
        if (rays_name && !rays) return fail(MI355RT_ERR_INVALID, std::string(who) + ": " + rays_name + " is null");
        if (!accum) return bad("d_accum is null");
        if (!scratch) return bad("d_scratch is null");
        if (rays_name && misaligned_to(rays, 16)) return fail(MI355RT_ERR_INVALID, std::string(who) + ": " + rays_name + " must be 16-byte aligned");
        if (misaligned_to(accum, 16)) return bad("d_accum must be 16-byte aligned");
        if (misaligned_to(scratch, 16)) return bad("d_scratch must be 16-byte aligned");
        if (misaligned_to(out_linear, 4)) return bad("d_out_linear must be 4-byte aligned");
        if (misaligned_to(out_packed, 4)) return bad("d_out_packed must be 4-byte aligned");
        if (int rc = radiance_items_bytes(who, what, n_rays, plan.samples, &plan.scratch_bytes)) return rc;
    }
    if (!have_ctx) return bad("ctx is null");
    if (!have_scene) return bad("context has no scene");
    const uint32_t k = items_knob ? items_knob : default_items;
    if (k == 0u || k > RADIANCE_PLAN_ITEMS_MAX) return bad("items per lane out of range");
    plan.n_items = (uint32_t)n_rays * plan.samples;                  // (< 2^32: checked above)
    plan.items_per_lane = k;
    const uint64_t per_block = (uint64_t)RADIANCE_PLAN_BLOCK * k;
    plan.grid_paths = (uint32_t)(((uint64_t)plan.n_items + per_block - 1u) / per_block);
    plan.grid_sum = (uint32_t)((n_rays + RADIANCE_PLAN_BLOCK / 16u - 1u) / (RADIANCE_PLAN_BLOCK / 16u));
    plan.seed_lo = (uint32_t)params->seed; plan.seed_hi = (uint32_t)(params->seed >> 32);
    plan.accum_load = params->sample_begin > 0u ? 1u : 0u;
    plan.inv_total = 1.0f / (float)params->sample_end;               // renderer.rs:85
    return MI355RT_OK;
}

int plan_radiance(bool have_ctx, bool have_scene, const mi355rt_radiance_params* params, const void* rays, uint32_t n_rays, const void* accum,
                  const void* out_linear, const void* scratch, uint32_t items_knob, uint32_t default_items, RadiancePlan& plan) {
    return plan_radiance_for("trace_radiance", "n_rays * samples", "d_rays", have_ctx, have_scene, params, rays, n_rays, accum, out_linear, nullptr, scratch, items_knob,
                             default_items, plan);
}

// What a view itself can be refused for: everything but the buffers and the size of the call.
static int check_view(const char* who, const mi355rt_view* v) {
    const auto bad = [who](const char* text) { return fail(MI355RT_ERR_INVALID, std::string(who) + ": " + text); };
    if (!v) return bad("view is null");
    if (v->model != MI355RT_VIEW_PINHOLE && v->model != MI355RT_VIEW_THIN_LENS) return bad("view.model is unknown");
    if (v->width == 0u) return bad("view.width is 0");
    if (v->height == 0u) return bad("view.height is 0");
    if ((v->flags & ~MI355RT_VIEW_CENTRE) != 0u) return bad("view.flags has unknown bits");
    for (uint32_t r : v->reserved) if (r != 0u) return bad("view.reserved must be 0");
    const mi355rt_camera& c = v->camera;
    for (int i = 0; i < 3; ++i)
        if (!std::isfinite(c.position[i]) || !std::isfinite(c.forward[i]) || !std::isfinite(c.right[i]) || !std::isfinite(c.true_up[i])) return bad("view.camera must be finite");
    if (!std::isfinite(c.half_width) || !std::isfinite(c.half_height)) return bad("view.camera must be finite");
    if (v->model == MI355RT_VIEW_THIN_LENS) {
        if (!std::isfinite(v->lens_radius) || v->lens_radius < 0.0f) return bad("view.lens_radius must be finite and not negative");
        if (!std::isfinite(v->focus_distance) || !(v->focus_distance > 0.0f)) return bad("view.focus_distance must be finite and positive");
    } else {
        if (v->lens_radius != 0.0f) return bad("view.lens_radius must be 0 unless the model is the thin lens");       // (NaN != 0: refused too)
        if (v->focus_distance != 0.0f) return bad("view.focus_distance must be 0 unless the model is the thin lens");
    }
    return MI355RT_OK;
}

int view_scratch_bytes(const mi355rt_view* view, uint32_t samples, uint64_t* out_bytes) {
    if (!out_bytes) return fail(MI355RT_ERR_INVALID, "view_scratch_bytes: out_bytes is null");
    if (int rc = check_view("view_scratch_bytes", view)) return rc;
    return radiance_items_bytes("view_scratch_bytes", "view.width * view.height * samples", (uint64_t)view->width * view->height, samples, out_bytes);
}

int plan_view_rays(bool have_ctx, bool have_scene, const mi355rt_view* view, const void* rays, ViewPlan& plan) {
    if (int rc = check_view("view_rays", view)) return rc;
    plan = ViewPlan{};
    if (!rays) return fail(MI355RT_ERR_INVALID, "view_rays: d_rays is null");
    if (misaligned_to(rays, 16)) return fail(MI355RT_ERR_INVALID, "view_rays: d_rays must be 16-byte aligned");
    const uint64_t pixels = (uint64_t)view->width * view->height;
    if (pixels >= (1ull << 32)) return fail(MI355RT_ERR_INVALID, "view_rays: view.width * view.height must stay below 2^32 (split the call)");
    if (!have_ctx) return fail(MI355RT_ERR_INVALID, "view_rays: ctx is null");
    if (!have_scene) return fail(MI355RT_ERR_INVALID, "view_rays: context has no scene");
    plan.n_pixels = plan.r.n_items = (uint32_t)pixels; plan.r.samples = 1u;   // (launch_view_rays cuts its own grid: one lane per pixel)
    plan.centre = view->flags & MI355RT_VIEW_CENTRE;
    return MI355RT_OK;
}

int plan_view(bool have_ctx, bool have_scene, const mi355rt_view* view, const mi355rt_radiance_params* params, const void* accum, const void* out_linear,
              const void* out_packed, const void* scratch, uint32_t items_knob, uint32_t default_items, ViewPlan& plan) {
    if (int rc = check_view("render_view", view)) return rc;
    plan = ViewPlan{};
    const uint64_t pixels = (uint64_t)view->width * view->height;    // (> 0: check_view)
    if (int rc = plan_radiance_for("render_view", "view.width * view.height * samples", nullptr, have_ctx, have_scene, params, nullptr, pixels, accum, out_linear,
                                   out_packed, scratch, items_knob, default_items, plan.r)) return rc;
    plan.n_pixels = (uint32_t)pixels;
    plan.centre = view->flags & MI355RT_VIEW_CENTRE;
    return MI355RT_OK;
}

// The surface probes: a probe record is read as a ray record is (two 16-byte loads), so probe_radiance is the radiance query's plan under its own name.
int plan_probe_rays(bool have_ctx, bool have_scene, const void* probes, uint32_t n, const void* rays) {
    const auto bad = [](const char* text) { return fail(MI355RT_ERR_INVALID, std::string("probe_rays: ") + text); };
    if (n != 0u) {
        if (!probes) return bad("d_probes is null");
        if (!rays) return bad("d_rays is null");
        if (misaligned_to(probes, 16)) return bad("d_probes must be 16-byte aligned");
        if (misaligned_to(rays, 16)) return bad("d_rays must be 16-byte aligned");
    }
    if (!have_ctx) return bad("ctx is null");
    if (!have_scene) return bad("context has no scene");
    return MI355RT_OK;
}

int plan_probe(bool have_ctx, bool have_scene, const mi355rt_radiance_params* params, const void* probes, uint32_t n, const void* accum,
               const void* out_linear, const void* scratch, uint32_t items_knob, uint32_t default_items, RadiancePlan& plan) {
    return plan_radiance_for("probe_radiance", "n * samples", "d_probes", have_ctx, have_scene, params, probes, n, accum, out_linear, nullptr, scratch, items_knob,
                             default_items, plan);
}

// s = ceil(log2 d), mul = ceil(2^(31+s) / d) < 2^32, shift = s - 1.
void magic_div(uint32_t d, uint32_t& mul, uint32_t& shift) {
    if (d <= 1) { mul = 0; shift = 0; return; }
    uint32_t s = 0; while ((1ull << s) < d) ++s;
    const unsigned __int128 num = (unsigned __int128)1 << (31 + s);
    mul = (uint32_t)((num + d - 1) / d); shift = s - 1;
}

void row_tables(const std::vector<uint32_t>& rows, const std::vector<float>& cost, uint32_t groups, std::vector<uint32_t>& out) {
    const size_t n = rows.size();
    out.resize(3 * n);
    std::vector<uint32_t> sorted(n);
    for (size_t j = 0; j < n; ++j) sorted[j] = (uint32_t)j;
    if (!cost.empty())
        std::stable_sort(sorted.begin(), sorted.end(), [&](uint32_t a, uint32_t b) {
            const float ca = rows[a] < cost.size() ? cost[rows[a]] : 0.f, cb = rows[b] < cost.size() ? cost[rows[b]] : 0.f;
            return ca > cb; });
    groups = std::max(1u, std::min<uint32_t>(groups, (uint32_t)std::max<size_t>(n, 1)));
    size_t jp = 0;
    for (uint32_t g = 0; g < groups && !cost.empty(); ++g)
        for (size_t k = g; k < n; k += groups, ++jp) { out[n + jp] = rows[sorted[k]]; out[2 * n + jp] = sorted[k]; }
    for (size_t j = 0; j < n; ++j) {
        out[j] = rows[j];
        if (cost.empty()) { out[n + j] = rows[j]; out[2 * n + j] = (uint32_t)j; }
    }
}

int plan_render(const RenderPlanIn& in, RowSel& sel, RenderPlan& plan) {
    const mi355rt_settings& st = *in.settings;
    const mi355rt_options* opt = in.options;
    if (int rc = select_rows(st, opt, sel)) return rc;
    const bool fixed_aabb = opt && (opt->flags & MI355RT_FLAG_FIXED_AABB) != 0u;
    if (opt && (opt->flags & ~MI355RT_FLAG_FIXED_AABB) != 0u) return fail(MI355RT_ERR_INVALID, "options.flags has unknown bits");
    plan = RenderPlan{};
    plan.rng_mode = opt ? opt->rng_mode : (uint32_t)MI355RT_RNG_CTR;
    if (fixed_aabb && plan.rng_mode != MI355RT_RNG_CTR) return fail(MI355RT_ERR_INVALID, "MI355RT_FLAG_FIXED_AABB needs MI355RT_RNG_CTR (the replay mode reproduces the reference as it is)");
    uint32_t variant = in.variant;
    if (fixed_aabb && in.has_mesh) variant = VARIANT_TABLE[variant].fixed_aabb;     // without a mesh the flag changes nothing
    // The mesh-free lockstep kernels are compiled under the assumption that the list holds something and that a path may take a step (rt_kernels.hip,
    // render_ctr_lockstep); the two degenerate renders -- every sample is the miss colour / BLACK -- go to the plain per-lane loop, which assumes nothing.
    if ((in.n_prims == 0 || st.max_depth == 0) && VARIANT_TABLE[variant].family == FAMILY_LOCKSTEP && !(VARIANT_TABLE[variant].prims & (1u << MI355RT_PRIM_MESH)))
        variant = KERNEL_LOCKSTEP_MESH;
    plan.variant = variant; plan.fixed_aabb = fixed_aabb ? 1u : 0u;
    plan.seed = opt ? opt->seed : 0; plan.seed_lo = (uint32_t)plan.seed; plan.seed_hi = (uint32_t)(plan.seed >> 32);
    plan.spp = in.s1 - in.s0; plan.sample0 = in.s0; plan.accum_load = in.s0 != 0 ? 1u : 0u;
    plan.inv_spp = 1.0f / (float)in.s1;                                               // renderer.rs:85
    plan.width = st.width; plan.width_f = (float)st.width; plan.height_f = (float)st.height;   // exact: both below 2^24
    { volatile float one = 1.0f; plan.inv_width_rn = one / plan.width_f; plan.inv_height_rn = one / plan.height_f; }   // IEEE division on the host = RN(1/x), what recip_normal_range() returns on the device
    magic_div(plan.spp, plan.spp_mul, plan.spp_shift); magic_div(st.width, plan.width_mul, plan.width_shift);
    plan.total_pixels = (uint64_t)sel.rows.size() * st.width;
    plan.guided_mult = in.guided_mult; plan.row_probe = in.row_probe ? 1u : 0u;
    // What fills the device, or this context's share of it: with F frames in flight (F contexts, F streams) each launch takes 1 / F of the wave slots,
    // F launches are co-resident, and a frame whose last paths are draining shares every SIMD with frames in their steady state.  A full-size grid
    // leaves the next frame's workgroups waiting for the draining frame's to retire one by one ("tail").
    plan.resident = std::max(1u, in.block_slots[variant] / in.grid_div);
    const bool ordered = in.have_row_cost && plan.rng_mode == MI355RT_RNG_CTR;      // otherwise: image order
    if (sel.rows.empty()) { plan.order_groups = ordered ? WORK_SHARDS : 0u; return MI355RT_OK; }
    if (plan.rng_mode == MI355RT_RNG_REF) {
        if (in.have_accum || in.s0 != 0 || in.s1 != st.samples_per_pixel)
            return fail(MI355RT_ERR_INVALID, "progressive rendering needs MI355RT_RNG_CTR (the reference stream of a row is sequential over its pixels)");
        plan.band_pixels = plan.total_pixels; plan.n_bands = 1; plan.block_threads = 64;   // k_render_ref: one lane per row
        return MI355RT_OK;
    }
    // ---- band plan: the radiance workspace holds band_pixels * spp float4 ----
    const uint64_t ws_cap = (opt && opt->workspace_bytes) ? opt->workspace_bytes : (32ull << 30);   // 288 GB of HBM: default = the 2^31-sample band limit; only what a band needs is allocated
    const uint64_t max_samples = std::min<uint64_t>(ws_cap / 12, (1ull << 31) - 16 * RUN_LIMIT);     // the shard counters overshoot by at most one run per claiming wave's last try; 32-bit headroom
    if (max_samples < plan.spp) return fail(MI355RT_ERR_INVALID, "workspace_bytes too small for one pixel (needs spp * 12 bytes)");
    plan.band_pixels = in.row_probe ? st.width : std::min<uint64_t>(max_samples / plan.spp, plan.total_pixels);   // the probe: a band = a row
    plan.n_bands = (uint32_t)((plan.total_pixels + plan.band_pixels - 1) / plan.band_pixels);
    plan.order_groups = ordered ? WORK_SHARDS * std::min(64u, plan.n_bands) : 0u;   // the work shards of every band this launch is cut into
    plan.block_threads = VARIANT_TABLE[variant].block_threads;
    return MI355RT_OK;
}

RenderBand render_band(const RenderPlan& plan, uint32_t b) {
    RenderBand r;
    const uint64_t p0 = (uint64_t)b * plan.band_pixels;
    r.band_pixel0 = (uint32_t)p0; r.band_pixels = (uint32_t)std::min<uint64_t>(plan.band_pixels, plan.total_pixels - p0);
    r.band_samples = (uint32_t)((uint64_t)r.band_pixels * plan.spp);
    const bool wf = VARIANT_TABLE[plan.variant].family == FAMILY_WAVEFRONT;
    const uint32_t run_min = wf ? RUN_WAVEFRONT_MIN : BATCH_MIN, run_max = wf ? RUN_WAVEFRONT : BATCH_MAX;   // what the kernel's WorkCursorT is compiled with
    r.shard_samples = (r.band_samples + WORK_SHARDS - 1) / WORK_SHARDS;
    r.shard_samples = (r.shard_samples + run_max - 1) / run_max * run_max;           // shards begin on run boundaries (fixed runs then stay aligned)
    const uint32_t waves_per_block = plan.block_threads / 64;
    const uint32_t min_runs = (r.band_samples + run_min - 1) / run_min;               // never more waves than minimum-size runs
    r.grid = std::max(1u, std::min(plan.resident, (min_runs + waves_per_block - 1) / waves_per_block));
    r.guided_div = std::max(1u, plan.guided_mult * r.grid * waves_per_block / WORK_SHARDS);
    return r;
}

// (the row probe's counter blocks are laid out one per ROW = per band: halving would make more bands than blocks -- its caller returns the OOM)
bool halve_bands(RenderPlan& plan) {
    if (plan.band_pixels <= 1 || plan.row_probe) return false;
    plan.band_pixels = (plan.band_pixels + 1) / 2;
    plan.n_bands = (uint32_t)((plan.total_pixels + plan.band_pixels - 1) / plan.band_pixels);
    return true;
}

bool scene_within_occlusion_bound(const PreparedScene& s) {
    const auto inside = [](const float* v, size_t n) { for (size_t k = 0; k < n; ++k) if (!(std::fabs(v[k]) <= OCCLUSION_BOUND)) return false; return true; };
    for (const DevPrim& p : s.prims) {
        switch (p.kind) {                                            // the words the hit tests read (rt_device.h, DevPrim::d)
        case MI355RT_PRIM_SPHERE: if (!inside(p.d, 4)) return false; break;
        case MI355RT_PRIM_PLANE: if (!inside(p.d, 6)) return false; break;
        case MI355RT_PRIM_QUAD: if (!inside(p.d, 15)) return false; break;
        default: if (!inside(p.d, 15) || !inside(p.d + 16, 12)) return false; break;     // cube, mesh: w2o, zd, o2w
        }
    }
    for (const DevTri& t : s.tris) if (!inside(t.v0, 3) || !inside(t.e1, 3) || !inside(t.e2, 3)) return false;
    return true;
}

}  // namespace mi355rt

namespace {

// Re-lay the meshes' BVHs (any node order, explicit child indices -- the shape of BVHNode, bvh.rs:7-12) into the
// two-link form the kernels walk (rt_device.h, DevNode): every node carries where the walk goes when its box is hit
// (inner: the left child, bvh.rs:142) and where it goes otherwise / afterwards (the "escape": the next node of the
// reference's left-then-right recursion that is not below this one).  The links make the visit order independent of
// the storage order, so nodes are stored LEVEL BY LEVEL (level 0 of every mesh, then level 1, ...): the levels every
// ray touches come first and are the part the state-machine kernel keeps in LDS.  Triangles go into leaf-visit order.
struct MeshFlat {
    std::vector<uint32_t> order;                 // input node ids in BFS order
    std::vector<uint32_t> level_begin;           // order[level_begin[L] .. level_begin[L+1]) = level L
    std::vector<uint32_t> escape;                // per input node: input id of its escape node, NODE_END if none
    std::vector<uint32_t> first_tri;             // per input leaf: index of its first triangle in out_tris
    std::vector<uint32_t> global_id;             // per input node: index in the device array
};

int flatten_mesh(const mi355rt_scene* sc, const mi355rt_mesh& m, MeshFlat& f, std::vector<DevTri>& out_tris) {
    if ((uint64_t)m.first_triangle + m.triangle_count > sc->n_triangles || m.triangle_count == 0) return fail(MI355RT_ERR_INVALID, "mesh triangle range");
    if ((uint64_t)m.first_node + m.node_count > sc->n_nodes || m.node_count == 0) return fail(MI355RT_ERR_INVALID, "mesh node range (is the BVH missing? see mi355rt_bvh_build)");
    if ((uint64_t)m.first_index + m.index_count > sc->n_tri_indices) return fail(MI355RT_ERR_INVALID, "mesh index range");
    const mi355rt_bvh_node* nodes = sc->nodes + m.first_node;
    const uint32_t* indices = sc->tri_indices + m.first_index;
    const mi355rt_triangle* tris = sc->triangles + m.first_triangle;
    f.escape.assign(m.node_count, NODE_END); f.first_tri.assign(m.node_count, 0u); f.global_id.assign(m.node_count, NODE_END);
    // pre-order with an explicit stack (input depth is not trusted): escapes, leaf-order triangles, cycle check
    std::vector<uint8_t> seen(m.node_count, 0);
    std::vector<std::pair<uint32_t, uint32_t>> stack;   // (node, its escape)
    stack.emplace_back(0u, NODE_END);
    uint32_t visited = 0;
    while (!stack.empty()) {
        const auto [ni, esc] = stack.back(); stack.pop_back();
        if (ni >= m.node_count) return fail(MI355RT_ERR_INVALID, "BVH child index out of range");
        if (seen[ni] || ++visited > m.node_count) return fail(MI355RT_ERR_INVALID, "BVH has a cycle or shared nodes");
        seen[ni] = 1;
        f.escape[ni] = esc;
        const mi355rt_bvh_node& n = nodes[ni];
        if (n.index_count > 0) {
            if ((uint64_t)n.first_index + n.index_count > m.index_count) return fail(MI355RT_ERR_INVALID, "BVH leaf index range");
            f.first_tri[ni] = (uint32_t)out_tris.size();
            for (uint32_t k = 0; k < n.index_count; ++k) {
                const uint32_t id = indices[n.first_index + k];
                if (id >= m.triangle_count) return fail(MI355RT_ERR_INVALID, "BVH leaf triangle id out of range");
                const mi355rt_triangle& t = tris[id];
                DevTri dt;
                for (int c = 0; c < 3; ++c) { dt.v0[c] = t.v0[c]; dt.e1[c] = t.v1[c] - t.v0[c]; dt.e2[c] = t.v2[c] - t.v0[c]; dt.n[c] = t.normal[c]; }
                out_tris.push_back(dt);
            }
        } else {
            stack.emplace_back(n.right, esc);        // visited after the whole left subtree; it inherits the parent's escape
            stack.emplace_back(n.left, n.right);     // a left child escapes to its sibling
        }
    }
    // breadth-first order
    f.order.clear(); f.level_begin.clear();
    f.order.push_back(0u); f.level_begin.push_back(0u);
    for (size_t lb = 0; lb < f.order.size();) {
        const size_t le = f.order.size();
        for (size_t i = lb; i < le; ++i) {
            const mi355rt_bvh_node& n = nodes[f.order[i]];
            if (n.index_count == 0) { f.order.push_back(n.left); f.order.push_back(n.right); }
        }
        lb = le;
        if (f.order.size() > le) f.level_begin.push_back((uint32_t)le);
    }
    f.level_begin.push_back((uint32_t)f.order.size());
    return MI355RT_OK;
}

int flatten_meshes(const mi355rt_scene* sc, std::vector<DevNode>& out_nodes, std::vector<DevTri>& out_tris, std::vector<uint32_t>& roots) {
    std::vector<MeshFlat> flat(sc->n_meshes);
    size_t max_levels = 0, total = 0;
    for (uint32_t m = 0; m < sc->n_meshes; ++m) {
        int rc = flatten_mesh(sc, sc->meshes[m], flat[m], out_tris);
        if (rc) return rc;
        max_levels = std::max(max_levels, flat[m].level_begin.size() - 1);
        total += flat[m].order.size();
    }
    // the walk packs node indices into 26 bits (and addresses nodes / triangles with 32-bit byte offsets)
    if (total >= NODE_END || out_tris.size() > (1u << 26)) return fail(MI355RT_ERR_INVALID, "more than 2^26 BVH nodes or triangles");
    // Storage order: breadth-first, level by level across all meshes, until the LDS copy is full (LDS_NODE_CAP nodes: the
    // levels every ray touches); every subtree hanging below that front then follows in depth-first pre-order, so that a
    // walk through the global-memory part finds a node's left child right behind it (same or next cache line).
    uint32_t next = 0;
    for (size_t L = 0; L < max_levels && next < LDS_NODE_CAP; ++L)
        for (uint32_t m = 0; m < sc->n_meshes && next < LDS_NODE_CAP; ++m) {
            MeshFlat& f = flat[m];
            if (L + 1 >= f.level_begin.size()) continue;
            for (uint32_t i = f.level_begin[L]; i < f.level_begin[L + 1] && next < LDS_NODE_CAP; ++i) f.global_id[f.order[i]] = next++;
        }
    for (uint32_t m = 0; m < sc->n_meshes; ++m) {
        MeshFlat& f = flat[m];
        const mi355rt_bvh_node* nodes = sc->nodes + sc->meshes[m].first_node;
        std::vector<uint32_t> stack;
        for (uint32_t ni : f.order) {                                   // BFS order: parents before children
            if (f.global_id[ni] != NODE_END) continue;
            // ni is the root of an unplaced subtree (its parent was placed, or it is a mesh root beyond the cap)
            stack.assign(1, ni);
            while (!stack.empty()) {
                const uint32_t x = stack.back(); stack.pop_back();
                f.global_id[x] = next++;
                if (nodes[x].index_count == 0) { stack.push_back(nodes[x].right); stack.push_back(nodes[x].left); }
            }
        }
    }
    out_nodes.assign(total, DevNode{});
    roots.assign(sc->n_meshes, 0u);
    for (uint32_t m = 0; m < sc->n_meshes; ++m) {
        const MeshFlat& f = flat[m];
        const mi355rt_bvh_node* nodes = sc->nodes + sc->meshes[m].first_node;
        roots[m] = f.global_id[0];
        for (uint32_t ni : f.order) {
            const mi355rt_bvh_node& n = nodes[ni];
            DevNode& d = out_nodes[f.global_id[ni]];
            std::memcpy(d.bmin, n.bmin, 12); std::memcpy(d.bmax, n.bmax, 12);
            const uint32_t esc = f.escape[ni] == NODE_END ? NODE_END : f.global_id[f.escape[ni]];
            if (n.index_count == 0) { d.a = f.global_id[n.left]; d.b = esc; }
            else if (n.index_count <= NODE_MAX_LEAF) { d.a = f.first_tri[ni]; d.b = esc | (n.index_count << NODE_LINK_BITS); }
            else {
                // A leaf with more triangles than the count field holds (BVHNode::new makes them only at depth 25, bvh.rs:31;
                // a caller-built tree may have them anywhere): its box test stays where it is, as an inner node whose "left
                // child" is a chain of chunk leaves with infinite bounds.  An infinite box is hit by every ray (the slab test
                // leaves t_min / t_max untouched), so the chain only adds box tests that change nothing; a miss of the real
                // box skips the whole chain.  The chunks live behind the level-ordered part of the array.
                d.a = (uint32_t)out_nodes.size(); d.b = esc;
                const float inf = std::numeric_limits<float>::infinity();
                for (uint32_t k = 0; k < n.index_count; k += NODE_MAX_LEAF) {
                    const uint32_t cnt = std::min(NODE_MAX_LEAF, n.index_count - k);
                    const bool last = k + cnt == n.index_count;
                    DevNode c;
                    for (int x = 0; x < 3; ++x) { c.bmin[x] = -inf; c.bmax[x] = inf; }
                    c.a = f.first_tri[ni] + k;
                    c.b = (last ? esc : (uint32_t)out_nodes.size() + 1u) | (cnt << NODE_LINK_BITS);
                    out_nodes.push_back(c);       // may reallocate: `d` is not used after this loop
                }
            }
        }
    }
    if (out_nodes.size() >= NODE_END) return fail(MI355RT_ERR_INVALID, "more than 2^26 BVH nodes");
    return MI355RT_OK;
}

// Is a mesh untransformed?  world_to_object (column-major, w2o[4 * column + row]) with a diagonal of exact ones, exact zeros (of either sign) off the
// diagonal of the upper 3 x 3 and a zero translation: the case rt_intersect.h's ray_nonzero_finite() reasons about.
bool xform_is_identity(const float* w2o) {
    for (int k : {4, 8, 1, 9, 2, 6, 12, 13, 14}) if (w2o[k] != 0.0f) return false;            // (NaN != 0 too)
    return w2o[0] == 1.0f && w2o[5] == 1.0f && w2o[10] == 1.0f;
}

// The 6 world normals a cube hit can produce (cube.rs:105-136): normalized(world_to_object^T * (+-e_k, 0)) with
// exactly the device's operation order (xform_normal + normalized in rt_intersect.h / rt_math.h; this file is compiled
// with -ffp-contract=off too), so the kernel can select instead of recomputing sqrt and divide per hit.
void cube_normal_table(float* d) {
    const float EPS = 1e-4f;
    for (int k = 0; k < 3; ++k) for (int sgn = 0; sgn < 2; ++sgn) {
        volatile float n[3] = {0.0f, 0.0f, 0.0f};
        n[k] = sgn ? -1.0f : 1.0f;
        float v[3];
        for (int r = 0; r < 3; ++r) {
            volatile float a = d[4 * r + 0] * n[0], b = d[4 * r + 1] * n[1], c = d[4 * r + 2] * n[2];
            volatile float s1 = a + b; volatile float s2 = s1 + c; volatile float s3 = s2 + d[31 + r];
            v[r] = s3;
        }
        volatile float xx = v[0] * v[0], yy = v[1] * v[1], zz = v[2] * v[2];
        volatile float l2a = xx + yy; volatile float l2 = l2a + zz;
        const float l = std::sqrt((float)l2);
        float* out = d + 34 + 3 * (2 * k + sgn);
        if (l < EPS) { out[0] = v[0]; out[1] = v[1]; out[2] = v[2]; }
        else { volatile float inv = 1.0f / l; out[0] = v[0] * inv; out[1] = v[1] * inv; out[2] = v[2] * inv; }
    }
}

}  // namespace

namespace mi355rt {

int prepare_scene(const mi355rt_scene* sc, PreparedScene& out) {
    out = PreparedScene{};
    if (!sc) return fail(MI355RT_ERR_INVALID, "scene is null");
    const bool has_sky = sc->sky_rgb != nullptr;
    if (has_sky != (sc->sky_width != 0 && sc->sky_height != 0) || (!has_sky && (sc->sky_width || sc->sky_height)))
        return fail(MI355RT_ERR_INVALID, "sky_rgb / sky_width / sky_height are inconsistent");
    if (has_sky && ((uint64_t)sc->sky_width * sc->sky_height > (1ull << 28) || sc->sky_width >= (1u << 24) || sc->sky_height >= (1u << 24)))
        return fail(MI355RT_ERR_INVALID, "skybox too large");
    if (sc->n_primitives && !sc->primitives) return fail(MI355RT_ERR_INVALID, "primitives is null");
    if (sc->n_materials && !sc->materials) return fail(MI355RT_ERR_INVALID, "materials is null");
    if (sc->n_textures && !sc->textures) return fail(MI355RT_ERR_INVALID, "textures is null");
    for (uint32_t i = 0; i < sc->n_textures; ++i) {
        const mi355rt_texture& t = sc->textures[i];
        if (!t.rgba8 || t.width == 0 || t.height == 0 || t.width >= (1u << 24) || t.height >= (1u << 24)) return fail(MI355RT_ERR_INVALID, "texture: null image or bad size");
        out.n_texels += (uint64_t)t.width * t.height;
    }
    if (out.n_texels > (1ull << 30)) return fail(MI355RT_ERR_INVALID, "textures larger than 2^30 texels in total");
    for (uint32_t i = 0; i < sc->n_materials; ++i) {
        if (sc->materials[i].kind >= MI355RT_MAT_KIND_COUNT) return fail(MI355RT_ERR_INVALID, "material kind");
        if (sc->materials[i].kind == MI355RT_MAT_TEXTURE && sc->materials[i].texture >= sc->n_textures) return fail(MI355RT_ERR_INVALID, "material texture index");
    }

    if (sc->n_meshes && (!sc->meshes || !sc->nodes || !sc->triangles || (!sc->tri_indices && sc->n_tri_indices))) return fail(MI355RT_ERR_INVALID, "mesh arrays are null");
    { int rc = flatten_meshes(sc, out.nodes, out.tris, out.mesh_roots); if (rc) return rc; }
    std::vector<DevPrim>& prims = out.prims;
    prims.resize(sc->n_primitives);
    for (uint32_t i = 0; i < sc->n_primitives; ++i) {
        const mi355rt_primitive& p = sc->primitives[i];
        DevPrim& d = prims[i];
        std::memset(&d, 0, sizeof d);
        if (p.kind >= MI355RT_PRIM_KIND_COUNT) return fail(MI355RT_ERR_INVALID, "primitive kind");
        if (p.material >= sc->n_materials) return fail(MI355RT_ERR_INVALID, "primitive material index");
        d.kind = p.kind; d.material = p.material;
        std::memcpy(d.mat0, &sc->materials[p.material], 16);      // kind + albedo, beside the geometry (rt_device.h)
        // The reference cannot render a sphere of |radius| < 1e-4: sphere.rs:38 divides by the radius with `Vec3 / f32`, which panics
        // below EPSILON (vec3.rs:120-122) the first time the sphere is hit.  Refused here rather than rendered.
        if (p.kind == MI355RT_PRIM_SPHERE && std::fabs(p.data[3]) < 1e-4f)
            return fail(MI355RT_ERR_INVALID, "sphere radius |r| < 1e-4: the reference panics on it (Vec3 / f32, vec3.rs:120-122 via sphere.rs:38)");
        // The quad test divides by dot(normal, direction) with the short division of rt_math.h (div_bounded), proven equal to `/` for divisors of
        // magnitude <= 2^25.  The reference's constructor always stores a unit normal (quad.rs:26-79, n = normalize(e0 x e1)), so |divisor| <= ~1;
        // a caller that hands in a scaled normal would leave the proven range while the reference semantics (IEEE division) go on: refused.
        if (p.kind == MI355RT_PRIM_QUAD) {
            bool ok = true;
            for (int k = 9; k < 12; ++k) ok = ok && std::fabs(p.data[k]) <= 0x1p20f;                       // (false for NaN and infinities too)
            if (!ok) return fail(MI355RT_ERR_INVALID, "quad normal (data[9..11]) is not finite or larger than 2^20: the reference stores a unit normal (quad.rs:26-79)");
        }
        if (p.kind == MI355RT_PRIM_CUBE || p.kind == MI355RT_PRIM_MESH) {
            const float* o2w = p.data; const float* w2o = p.data + 16;
            float t[52] = {};                                 // matrix-shaped staging: w2o[16] column-major, o2w[12], zd[3], zn[3], the cube's normal table
            std::memcpy(t, w2o, 64);
            for (int c = 0; c < 4; ++c) for (int r = 0; r < 3; ++r) t[16 + 3 * c + r] = o2w[4 * c + r];
            volatile float zero = 0.0f;                       // keep the IEEE product (sign of zero, NaN) exactly
            for (int r = 0; r < 3; ++r) t[28 + r] = w2o[12 + r] * zero;
            for (int r = 0; r < 3; ++r) t[31 + r] = w2o[4 * r + 3] * zero;
            if (p.kind == MI355RT_PRIM_CUBE) cube_normal_table(t);
            // The record (rt_device.h): what the hit test reads -- the 3 x 3 part of w2o, its translation, zd -- as ONE run of 15 words, so that the
            // wave-uniform walk fetches it with one scalar load instead of ten pieces picked out of a 4 x 4 matrix.
            for (int c = 0; c < 4; ++c) for (int r = 0; r < 3; ++r) d.d[3 * c + r] = t[4 * c + r];
            for (int r = 0; r < 3; ++r) d.d[12 + r] = t[28 + r];
            for (int k = 16; k < 28; ++k) d.d[k] = t[k];
            for (int k = 31; k < 52; ++k) d.d[k] = t[k];
            if (p.kind == MI355RT_PRIM_CUBE)
                // (an entry that is NaN or infinite keeps the list: it makes the object-space direction NaN or infinite, never a finite magnitude of 2^126 or
                //  more, and the short reciprocal is exact on NaN and infinities -- rt_math.h recip_normal_range.  A cube of zero scale on one axis is such a record.)
                for (int k : {0, 1, 2, 3, 4, 5, 6, 7, 8, 12, 13, 14}) out.walk_bounded = out.walk_bounded && !(std::isfinite(d.d[k]) && std::fabs(d.d[k]) > WALK_CUBE_M_MAX);
            if (p.kind == MI355RT_PRIM_MESH) {
                if (p.mesh >= sc->n_meshes) return fail(MI355RT_ERR_INVALID, "primitive mesh index");
                d.node_begin = out.mesh_roots[p.mesh];
                out.all_meshes_identity = out.all_meshes_identity && xform_is_identity(w2o);
                out.all_meshes_shallow = out.all_meshes_shallow && sc->meshes[p.mesh].node_count <= WF_SHALLOW_NODES;
            }
        } else if (p.kind == MI355RT_PRIM_QUAD) {               // normal and plane constant first (what every ray needs), then base, e0, e1, the two 1 / |e|^2
            for (int k = 0; k < 4; ++k) d.d[k] = p.data[9 + k];
            for (int k = 0; k < 9; ++k) d.d[4 + k] = p.data[k];
            d.d[13] = p.data[13]; d.d[14] = p.data[14];
            out.walk_bounded = out.walk_bounded && std::fabs(d.d[3]) <= WALK_QUAD_D_MAX;                       // (false for NaN and infinities too)
        } else {
            std::memcpy(d.d, p.data, 32 * sizeof(float));
        }
    }
    for (uint32_t i = sc->n_primitives; i-- > 0;)               // runs of one kind: the list walk loops over a run without re-dispatching on the kind
        prims[i].run_end = (i + 1 < sc->n_primitives && prims[i + 1].kind == prims[i].kind) ? prims[i + 1].run_end : i + 1;
    for (const auto& pr : prims) out.n_mesh_prims += pr.kind == MI355RT_PRIM_MESH;
    for (uint32_t i = 0; i < sc->n_primitives; ++i) { out.scene_mats |= MATBIT(sc->materials[sc->primitives[i].material].kind); out.scene_prim_kinds |= 1u << sc->primitives[i].kind; }
    return MI355RT_OK;
}

uint32_t choose_variant(const PreparedScene& s, int forced_variant, uint32_t built_mask) {
    const uint32_t scene_mats = s.scene_mats, scene_prim_kinds = s.scene_prim_kinds;
    const bool has_mesh = s.n_mesh_prims != 0, all_meshes_identity = s.all_meshes_identity, all_meshes_shallow = s.all_meshes_shallow;
    auto render_ctr_variant_built = [&](uint32_t variant) { return ((built_mask >> variant) & 1u) != 0u; };   // (what rt_kernels.hip says of this library, passed in)
    auto covers = [&](uint32_t variant) { return (scene_mats & ~VARIANT_TABLE[variant].mats) == 0u; };
    auto kinds_covered = [&](uint32_t variant) { return (scene_prim_kinds & ~VARIANT_TABLE[variant].prims) == 0u; };       // likewise for the primitive kinds of the list (a mesh among them)
    // k_render_ctr_simple_qc tests its argument ranges once per walk instead of once per primitive (rt_intersect.h, BOUNDED), which needs bounded records.
    auto ranges_ok = [&](uint32_t variant) { return variant != KERNEL_LOCKSTEP_SIMPLE_QC || s.walk_bounded; };
    uint32_t chosen;
    // Scenes with meshes: the wavefront kernel (path state in LDS, stage queues).  No mesh: a lockstep kernel.  In both
    // families the most pruned instantiation whose material set covers the scene's (rt_device.h, VARIANT_TABLE): the branches of
    // the kinds a scene does not have are compiled out -- they set the register peak.  The library reads NO environment
    // variables; the diagnostic hook mi355rt_debug_set_knob("kernel", v) may name another variant this library was built with.
    // ... and, where the meshes are all untransformed (OBJ data in world space: teapot), the instantiation whose mesh_setup skips the matrix products.
    // ... and, for transformed meshes whose trees are all small (semesterbild), the instantiation with the shorter WALK rounds (rt_wavefront.h).
    if (has_mesh) chosen = covers(KERNEL_WAVEFRONT_NOMETAL) ? (all_meshes_identity ? KERNEL_WAVEFRONT_NOMETAL_IDENT : all_meshes_shallow ? KERNEL_WAVEFRONT_NOMETAL_SHALLOW : KERNEL_WAVEFRONT_NOMETAL)
                                                                  : KERNEL_WAVEFRONT;
    else {
        // Mesh-free lists run on a lockstep kernel -- unless the shading step diverges EXPENSIVELY: a rough conductor (ln, atan, two
        // sin_cos, the conductor's Fresnel term: ~400 instructions) next to another scattering material.  In lockstep a wave pays that branch
        // whenever any lane takes it (veach-mis: in 71 % of its iterations, for 6.8 lanes); the wavefront kernel's material-sorted SHADE
        // passes run it at ~57 lanes: veach-mis 18.30 -> 16.75 ms at 256 spp.  Cheap mixtures (Lambert + metal + dielectric + plastic)
        // measured 3-7 % FASTER in lockstep (tools/ab_fuzz_scene.py), and so stay there.
        const bool rough = (scene_mats & MATS_ROUGH) != 0u, other_scatter = (scene_mats & ~(MATS_ROUGH | MATS_TERMINAL)) != 0u;
        chosen = covers(KERNEL_LOCKSTEP_SIMPLE) ? (kinds_covered(KERNEL_LOCKSTEP_SIMPLE_QC) && ranges_ok(KERNEL_LOCKSTEP_SIMPLE_QC) ? KERNEL_LOCKSTEP_SIMPLE_QC : KERNEL_LOCKSTEP_SIMPLE)   // (... pruned to quads and cubes where the list holds nothing else: cornell)
                     : (rough && other_scatter && covers(KERNEL_WAVEFRONT_MESHFREE)) ? KERNEL_WAVEFRONT_MESHFREE
                     : covers(KERNEL_LOCKSTEP_NOSPEC) ? KERNEL_LOCKSTEP_NOSPEC : KERNEL_LOCKSTEP;
    }
    if (forced_variant >= 0) {
        const uint32_t v = (uint32_t)forced_variant;
        const bool ok = render_ctr_variant_built(v) && VARIANT_TABLE[v].forceable && covers(v) && kinds_covered(v) &&
                        !(VARIANT_TABLE[v].identity_meshes && !(has_mesh && all_meshes_identity));
        if (ok && ranges_ok(v)) chosen = v;
    }
    return chosen;
}

// Root-box test right at mesh set-up (reference build's state machine): when several meshes share the list (teapot +5..12 %; a single
// mesh loses 5-10 %).
uint32_t choose_inline_steps(const PreparedScene& s, int knob) { return knob >= 0 ? (uint32_t)knob : (s.n_mesh_prims >= 2 ? 1u : 0u); }

}  // namespace mi355rt

// ---- camera masks ----------------------------------------------------------------------------------------------------------------
namespace {

constexpr double MASK_INFLATE = 1e-3;       // in the primitive's own parameter space: ten times the tests' EPS (rt_math.h) of 1e-4
constexpr double MASK_DILATE = 1.0;         // pixels, on every side of the footprint
constexpr double MASK_TAN_MAX = 1e6;        // a corner further off the view axis than this many times its depth counts as reaching the camera plane

struct V3 { double x, y, z; };
V3 v3(const float* p) { return V3{(double)p[0], (double)p[1], (double)p[2]}; }
double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
V3 cross(V3 a, V3 b) { return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
double maxabs(V3 a) { return std::max(std::fabs(a.x), std::max(std::fabs(a.y), std::fabs(a.z))); }

// Rows r0, r1, r2 and a right-hand side: the x with r_k . x = b_k, by Cramer's rule.  false: not finite, or a determinant that is nothing but
// rounding of its own terms (|det| <= 1e-12 |r0| |r1| |r2|).
bool solve_rows(V3 r0, V3 r1, V3 r2, V3 b, V3& x) {
    const V3 c12 = cross(r1, r2), c20 = cross(r2, r0), c01 = cross(r0, r1);
    const double det = dot(r0, c12), scale = maxabs(r0) * maxabs(r1) * maxabs(r2);
    if (!std::isfinite(det) || !std::isfinite(scale) || !(std::fabs(det) > 1e-12 * scale)) return false;
    x = V3{(b.x * c12.x + b.y * c20.x + b.z * c01.x) / det, (b.x * c12.y + b.y * c20.y + b.z * c01.y) / det, (b.x * c12.z + b.y * c20.z + b.z * c01.z) / det};
    return std::isfinite(x.x) && std::isfinite(x.y) && std::isfinite(x.z);
}

// The world-space corners of the region in which the kernel's test can accept a hit, inflated by MASK_INFLATE.  false: in doubt.
// Quad (rt_intersect.h hit_quad): the hit point P lies in the plane n . P = d, and l0 = ((P - base) . e0) * inv0 and l1 = ((P - base) . e1) * inv1 lie in
// [-EPS, 1 + EPS].  The corners are the P with l0, l1 in {-delta, 1 + delta} -- for the records the loader makes (e0 orthogonal to e1, inv = 1 / |e|^2, the
// plane through base) these are base + s e0 + t e1; solving the three equations of the record itself also covers a record that is not of that form.
int quad_corners(const mi355rt::DevPrim& p, V3* out) {
    const V3 n = v3(p.d), base = v3(p.d + 4), e0 = v3(p.d + 7), e1 = v3(p.d + 10);
    const double d = p.d[3], inv0 = p.d[13], inv1 = p.d[14];
    const V3 r1 = V3{e0.x * inv0, e0.y * inv0, e0.z * inv0}, r2 = V3{e1.x * inv1, e1.y * inv1, e1.z * inv1};
    int k = 0;
    for (double a : {-MASK_INFLATE, 1.0 + MASK_INFLATE}) for (double b : {-MASK_INFLATE, 1.0 + MASK_INFLATE})
        if (!solve_rows(n, r1, r2, V3{d, a + dot(base, r1), b + dot(base, r2)}, out[k++])) return 0;
    return k;
}
// Cube (hit_cube): the object-space ray w2o * (ray) meets the box [-0.5, 0.5]^3, so the world ray meets the image of that box under the inverse of the
// record's w2o (the record's own o2w only rejects more: it enters the second range check).  The corners: M x + c = (+-(0.5 + delta))^3.
int cube_corners(const mi355rt::DevPrim& p, V3* out) {
    const float* m = p.d;                                    // d[3 * column + row], column 3 = the translation
    const V3 r0 = V3{m[0], m[3], m[6]}, r1 = V3{m[1], m[4], m[7]}, r2 = V3{m[2], m[5], m[8]}, c = v3(m + 9);
    const double h = 0.5 + MASK_INFLATE;
    int k = 0;
    for (double x : {-h, h}) for (double y : {-h, h}) for (double z : {-h, h})
        if (!solve_rows(r0, r1, r2, V3{x - c.x, y - c.y, z - c.z}, out[k++])) return 0;
    return k;
}

}  // namespace

namespace mi355rt {

void build_camera_masks(const PreparedScene& s, const DevCamera& cam, uint32_t width, uint32_t height, std::vector<uint32_t>& out) {
    out.clear();
    const size_t n_prims = s.prims.size();
    if (n_prims == 0 || n_prims > 32 || width == 0 || height == 0) return;
    out.assign((size_t)width * height, 0u);
    const uint32_t all = n_prims == 32 ? 0xFFFFFFFFu : (1u << n_prims) - 1u;
    uint32_t keep = 0u;                                      // the primitives in doubt: their bits go into every pixel at the end
    const V3 O = v3(cam.position), F = v3(cam.forward), R = v3(cam.right), U = v3(cam.true_up);
    const double hw = cam.half_width, hh = cam.half_height, W = width, H = height;
    // X - O = lambda (F + a R + b U): the rows of the system are the components, its columns F, R, U (no basis is assumed orthonormal).
    const V3 row0 = V3{F.x, R.x, U.x}, row1 = V3{F.y, R.y, U.y}, row2 = V3{F.z, R.z, U.z};
    const bool cam_ok = std::isfinite(hw) && std::isfinite(hh) && std::fabs(hw) > 0.0 && std::fabs(hh) > 0.0;
    for (size_t i = 0; i < n_prims; ++i) {
        const DevPrim& p = s.prims[i];
        const uint32_t bit = 1u << i;
        V3 corner[8];
        const int n = !cam_ok ? 0 : p.kind == MI355RT_PRIM_QUAD ? quad_corners(p, corner) : p.kind == MI355RT_PRIM_CUBE ? cube_corners(p, corner) : 0;
        if (n == 0) { keep |= bit; continue; }
        double px[8], py[8];
        int behind = 0; bool doubt = false;
        for (int k = 0; k < n; ++k) {
            V3 q;                                            // (lambda, lambda a, lambda b)
            if (!solve_rows(row0, row1, row2, V3{corner[k].x - O.x, corner[k].y - O.y, corner[k].z - O.z}, q)) { doubt = true; break; }
            const double off = std::fabs(q.y) + std::fabs(q.z);
            if (q.x < 0.0 && -q.x * MASK_TAN_MAX > off) { ++behind; continue; }            // safely behind the camera plane
            if (!(q.x > 0.0 && q.x * MASK_TAN_MAX > off)) { doubt = true; break; }         // in or near the camera plane
            // camera_raw (rt_materials.h): a = (2 u - 1) half_width, b = (1 - 2 v) half_height; a pixel is [x, x + 1] x [y, y + 1] of (u W, v H)
            px[k] = (q.y / q.x / hw + 1.0) * 0.5 * W; py[k] = (1.0 - q.z / q.x / hh) * 0.5 * H;
            if (!std::isfinite(px[k]) || !std::isfinite(py[k])) { doubt = true; break; }
        }
        if (!doubt && behind == n) continue;                 // every corner, so the whole convex region, lies behind the camera: no ray reaches it
        if (doubt || behind != 0) { keep |= bit; continue; } // it reaches the camera plane
        // The footprint is the convex hull of the projected corners, and a convex set's extent in x within a band of rows is reached on a segment between
        // two of its corners: per pixel row, the extent of all corner pairs' segments clipped to the dilated row, widened by the dilation.
        double ymin = py[0], ymax = py[0];
        for (int k = 1; k < n; ++k) { ymin = std::min(ymin, py[k]); ymax = std::max(ymax, py[k]); }
        const double ylo = std::floor(ymin - MASK_DILATE), yhi = std::floor(ymax + MASK_DILATE);
        if (yhi < 0.0 || ylo > H - 1.0) continue;
        const uint32_t y0 = (uint32_t)std::max(ylo, 0.0), y1 = (uint32_t)std::min(yhi, H - 1.0);
        for (uint32_t y = y0; y <= y1; ++y) {
            const double lo = (double)y - MASK_DILATE, hi = (double)y + 1.0 + MASK_DILATE;
            double xmin = std::numeric_limits<double>::infinity(), xmax = -xmin;
            for (int a = 0; a < n; ++a) for (int b = a; b < n; ++b) {
                double xa = px[a], ya = py[a], xb = px[b], yb = py[b];
                if (ya > yb) { std::swap(xa, xb); std::swap(ya, yb); }
                if (yb < lo || ya > hi) continue;
                const double dy = yb - ya;
                double x_lo = xa, x_hi = xb;                 // the segment's ends inside [lo, hi]
                if (dy > 0.0) {
                    if (ya < lo) x_lo = xa + (xb - xa) * ((lo - ya) / dy);
                    if (yb > hi) x_hi = xa + (xb - xa) * ((hi - ya) / dy);
                }
                xmin = std::min(xmin, std::min(x_lo, x_hi)); xmax = std::max(xmax, std::max(x_lo, x_hi));
            }
            if (!(xmin <= xmax)) continue;
            const double fx0 = std::floor(xmin - MASK_DILATE), fx1 = std::floor(xmax + MASK_DILATE);
            if (fx1 < 0.0 || fx0 > W - 1.0) continue;
            const uint32_t x0 = (uint32_t)std::max(fx0, 0.0), x1 = (uint32_t)std::min(fx1, W - 1.0);
            uint32_t* row = out.data() + (size_t)y * width;
            for (uint32_t x = x0; x <= x1; ++x) row[x] |= bit;
        }
    }
    if (keep != 0u) for (uint32_t& w : out) w |= keep & all;
}

void gather_camera_masks(const std::vector<uint32_t>& absolute, uint32_t width, const uint32_t* rows_processing, size_t n_rows, std::vector<uint32_t>& out) {
    out.resize(n_rows * (size_t)width);
    for (size_t j = 0; j < n_rows; ++j) std::memcpy(out.data() + j * width, absolute.data() + (size_t)rows_processing[j] * width, (size_t)width * sizeof(uint32_t));
}

}  // namespace mi355rt
