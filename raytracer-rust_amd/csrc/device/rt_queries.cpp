// rt_queries.cpp -- the calls of include/mi355rt.h that read the resident scene and leave the render's workspaces alone, part of libmi355rt.so:
// the ray queries (rt_query.hip), the occlusion queries (rt_occlusion.hip), the radiance queries (rt_radiance.hip), the camera views (rt_view.hip),
// the surface probes (rt_probe.hip), the denoiser (rt_denoise.hip) and the three *_scratch_bytes calls.  Each entry point opens with the exception
// barrier and does its work itself: the refusals and the plan are rt_prepare.cpp's (no HIP in it), the kernels and their launch_* functions stand in the
// .hip files, and this file binds the context's scene to the launch (rt_context.h).
// THE PROTOCOL of every call here: it reads the scene arrays only -- no workspace, no counters, no error word of its own -- so it neither waits on
// `done` nor records it, and may run beside a render of the same context on another stream.  mi355rt_context_set_share is not consulted: the
// kernels are plain grids that end with their work.
#include "rt_context.h"
#include "rt_query.h"
#include "rt_denoise.h"
#include "rt_occlusion.h"
#include "rt_radiance.h"
#include "rt_view.h"
#include "rt_probe.h"

namespace {

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0u; }

// What every query does once its refusals are behind it: the context's device, and the word of an earlier asynchronous render on this context that failed.
int query_begin(mi355rt_context* ctx) {
    HIP_TRY(hipSetDevice(ctx->device));
    return report_device_error(ctx);
}

// The device table (local output row -> absolute y) of a row selection, one per selection seen since set_scene; `sel.rows` is taken when a new one is made.
// On return the table's upload is ordered before what is enqueued on `stream` next.
int query_row_table(mi355rt_context* ctx, RowSel& sel, hipStream_t stream, mi355rt_context::QueryRows*& table) {
    table = nullptr;
    for (auto& t : ctx->query_rows) if (t.rows == sel.rows) { table = &t; break; }
    if (!table) {
        if (ctx->query_rows.size() >= 16) { HIP_TRY(hipDeviceSynchronize()); ctx->query_rows_release(); }   // a caller that keeps changing its selection: start over
        mi355rt_context::QueryRows t;
        t.rows.swap(sel.rows); t.stream = stream;
        if (hipMalloc((void**)&t.d, t.rows.size() * sizeof(uint32_t)) != hipSuccess) return fail(MI355RT_ERR_OOM, "hipMalloc(first_hits row table)");
        ctx->query_rows.push_back(std::move(t));                     // (the vector's storage moves with it: the upload's source stays where it is)
        table = &ctx->query_rows.back();
        if (hipEventCreateWithFlags(&table->ready, hipEventDisableTiming) != hipSuccess ||
            hipMemcpyAsync(table->d, table->rows.data(), table->rows.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream) != hipSuccess ||
            hipEventRecord(table->ready, stream) != hipSuccess) {
            (void)hipDeviceSynchronize();                            // a table that may not have arrived is not kept
            (void)hipFree(table->d); if (table->ready) (void)hipEventDestroy(table->ready);
            ctx->query_rows.pop_back();
            return fail(MI355RT_ERR_HIP, "first_hits: row table upload failed");
        }
    } else if (table->stream != stream) HIP_TRY(hipStreamWaitEvent(stream, table->ready, 0));
    return MI355RT_OK;
}

// The launch constants of the radiance family's shared loop and sum (rt_radiance_paths.h), from the plan of rt_prepare.cpp: the callers' rays
// (trace_radiance), or none -- a view or the probes make them (p.rays is not read).
RadianceParams radiance_params(const mi355rt_context* ctx, const RadiancePlan& plan, const mi355rt_radiance_params* params, const void* d_rays, void* d_scratch) {
    RadianceParams p{};
    bind_geometry(ctx, p); bind_shading(ctx, p);
    p.rays = d_rays; p.scratch = (float*)d_scratch; p.n_items = plan.n_items; p.samples = plan.samples; p.sample_begin = params->sample_begin;
    p.max_depth = params->max_depth; p.items_per_lane = plan.items_per_lane; p.seed_lo = plan.seed_lo; p.seed_hi = plan.seed_hi;
    return p;
}
RadianceSum radiance_sum(const RadiancePlan& plan, uint32_t n_rays, const void* d_scratch, void* d_accum, void* d_out_linear) {
    RadianceSum s{};
    s.scratch = (const float*)d_scratch; s.accum = (float*)d_accum; s.out_linear = (float*)d_out_linear; s.n_rays = n_rays; s.samples = plan.samples;
    s.accum_load = plan.accum_load; s.inv_total = plan.inv_total;
    return s;
}

void view_params(const mi355rt_view* view, const ViewPlan& plan, ViewParams& v) {
    static_assert(sizeof(DevCamera) == sizeof(mi355rt_camera) && sizeof(mi355rt_view) == 96 && sizeof(mi355rt_view) % 16 == 0, "a view carries set_scene's camera");
    std::memcpy(&v.cam, &view->camera, sizeof v.cam);
    v.width_f = (float)view->width; v.height_f = (float)view->height; v.width = view->width; v.centre = plan.centre;
    v.lens_radius = view->lens_radius; v.focus_distance = view->focus_distance;
}

}  // namespace

extern "C" {

// ---- ray queries (rt_query.hip): what does a ray hit in the resident scene? ------------------------------------------------------
int mi355rt_context_trace_rays(mi355rt_context* ctx, const void* d_rays, uint32_t n_rays, void* d_hits, void* hip_stream) {
    return guard([&]() -> int {
    static_assert(sizeof(mi355rt_ray) == 32 && sizeof(mi355rt_hit) == 48, "the query kernels read a ray as two 16-byte halves and write a record as three 16-byte words");
    if (!ctx || !ctx->have_scene) return fail(MI355RT_ERR_INVALID, "context has no scene");
    if (n_rays == 0) return MI355RT_OK;
    if (!d_rays || !d_hits) return fail(MI355RT_ERR_INVALID, "trace_rays: d_rays / d_hits is null");
    if (!aligned16(d_rays) || !aligned16(d_hits)) return fail(MI355RT_ERR_INVALID, "trace_rays: d_rays / d_hits must be 16-byte aligned");
    if (int rc = query_begin(ctx)) return rc;
    QueryParams q{};
    bind_geometry(ctx, q);
    q.rays = d_rays; q.hits = d_hits; q.n = n_rays;
    if (launch_query(q, ctx->has_mesh, hip_stream) != 0) return fail(MI355RT_ERR_HIP, "k_query_rays launch failed");
    return MI355RT_OK;
    });
}

int mi355rt_context_first_hits(mi355rt_context* ctx, const mi355rt_options* opt, void* d_hits, void* hip_stream) {
    return guard([&]() -> int {
    if (!ctx || !ctx->have_scene) return fail(MI355RT_ERR_INVALID, "context has no scene");
    if (!d_hits) return fail(MI355RT_ERR_INVALID, "first_hits: d_hits is null");
    if (!aligned16(d_hits)) return fail(MI355RT_ERR_INVALID, "first_hits: d_hits must be 16-byte aligned");
    if (opt && (opt->flags & ~MI355RT_FLAG_FIXED_AABB) != 0u) return fail(MI355RT_ERR_INVALID, "options.flags has unknown bits");
    const mi355rt_settings& st = ctx->settings;
    RowSel sel;
    {   mi355rt_options rows_only{};                                 // rng_mode, seed and workspace_bytes are not this call's business
        if (opt) { rows_only = *opt; rows_only.rng_mode = MI355RT_RNG_CTR; }
        const int rc = select_rows(st, opt ? &rows_only : nullptr, sel); if (rc) return rc; }
    if (opt && (opt->flags & MI355RT_FLAG_FIXED_AABB) != 0u)
        return fail(MI355RT_ERR_UNSUPPORTED, "first_hits: MI355RT_FLAG_FIXED_AABB is not built for ray queries (they answer as the reference does)");
    if (sel.rows.empty()) return MI355RT_OK;
    if (int rc = query_begin(ctx)) return rc;
    mi355rt_context::QueryRows* table = nullptr;
    if (int rc = query_row_table(ctx, sel, (hipStream_t)hip_stream, table)) return rc;
    QueryParams q{};
    bind_geometry(ctx, q);
    q.rays = nullptr; q.hits = d_hits; q.rows = table->d; q.n = (uint32_t)(table->rows.size() * (size_t)st.width);   // (< 2^31: check_settings)
    q.cam = ctx->cam; q.width = st.width; q.width_f = (float)st.width; q.height_f = (float)st.height;
    magic_div(st.width, q.width_mul, q.width_shift);
    if (launch_query(q, ctx->has_mesh, hip_stream) != 0) return fail(MI355RT_ERR_HIP, "k_query_pixels launch failed");
    return MI355RT_OK;
    });
}

// ---- occlusion queries (rt_occlusion.hip): does anything lie in front of t_max? -----------------------------------------------------------
// Every refusal is rt_prepare.cpp's, before any HIP call.
int mi355rt_context_occluded(mi355rt_context* ctx, const void* d_segments, uint32_t n, void* d_out, void* hip_stream) {
    return guard([&]() -> int {
    static_assert(sizeof(mi355rt_segment) == 32, "the kernel reads a segment as two 16-byte halves");
    if (int rc = check_occluded_args(ctx != nullptr, ctx && ctx->have_scene, d_segments, n, d_out)) return rc;
    if (n == 0) return MI355RT_OK;
    if (int rc = query_begin(ctx)) return rc;
    OcclusionParams q{};
    bind_geometry(ctx, q);
    q.segments = d_segments; q.out = (uint32_t*)d_out; q.n = n; q.may_exit = ctx->occlusion_may_exit ? 1u : 0u;
    if (launch_occluded(q, ctx->has_mesh, hip_stream) != 0) return fail(MI355RT_ERR_HIP, "k_occluded launch failed");
    return MI355RT_OK;
    });
}

int mi355rt_context_ambient_occlusion(mi355rt_context* ctx, const mi355rt_options* opt, const mi355rt_ao_params* params, const void* d_hits, void* d_out,
                                      void* hip_stream) {
    return guard([&]() -> int {
    static_assert(sizeof(mi355rt_hit) == 48 && sizeof(mi355rt_ao_params) == 16, "the kernel reads a hit record as three 16-byte words");
    RowSel sel; AoPlan plan{};
    const mi355rt_settings no_settings{};
    if (int rc = plan_ambient_occlusion(ctx != nullptr, ctx && ctx->have_scene, ctx ? ctx->settings : no_settings, opt, params, d_hits, d_out, sel, plan)) return rc;
    if (sel.rows.empty()) return MI355RT_OK;
    const mi355rt_settings& st = ctx->settings;
    if (int rc = query_begin(ctx)) return rc;
    mi355rt_context::QueryRows* table = nullptr;
    if (int rc = query_row_table(ctx, sel, (hipStream_t)hip_stream, table)) return rc;
    AoLaunch a{};
    bind_geometry(ctx, a);
    a.hits = d_hits; a.out = (float*)d_out; a.rows = table->d; a.n = (uint32_t)(table->rows.size() * (size_t)st.width);   // (< 2^31: check_settings)
    a.width = st.width; magic_div(st.width, a.width_mul, a.width_shift);
    a.samples = plan.samples; a.log2_samples = plan.log2_samples; a.seed = plan.seed; a.radius = plan.radius;
    a.may_exit = ctx->occlusion_may_exit ? 1u : 0u; a.form = (uint32_t)ctx->knob_ao_form;
    if (launch_ambient_occlusion(a, ctx->has_mesh, hip_stream) != 0) return fail(MI355RT_ERR_HIP, "k_ao launch failed");
    return MI355RT_OK;
    });
}

// ---- radiance queries (rt_radiance.hip): whole paths along the caller's rays ----------------------------------------------------------------
// Every refusal, the item count and the grids are rt_prepare.cpp's (plan_radiance), before any HIP call.
int mi355rt_radiance_scratch_bytes(uint32_t n_rays, uint32_t samples, uint64_t* out_bytes) {
    return guard([&]() -> int { return radiance_scratch_bytes(n_rays, samples, out_bytes); });
}

int mi355rt_context_trace_radiance(mi355rt_context* ctx, const mi355rt_radiance_params* params, const void* d_rays, uint32_t n_rays, void* d_accum,
                                   void* d_out_linear, void* d_scratch, void* hip_stream) {
    return guard([&]() -> int {
    static_assert(sizeof(mi355rt_path_ray) == 32 && sizeof(mi355rt_radiance_params) == 32, "the kernel reads a ray as two 16-byte halves");
    static_assert(RADIANCE_PLAN_BLOCK == RADIANCE_BLOCK_THREADS && RADIANCE_PLAN_ITEMS_MAX == RADIANCE_ITEMS_MAX, "plan_radiance cuts the grids the kernels are launched on");
    RadiancePlan plan{};
    if (int rc = plan_radiance(ctx != nullptr, ctx && ctx->have_scene, params, d_rays, n_rays, d_accum, d_out_linear, d_scratch,
                               ctx ? (uint32_t)ctx->knob_radiance_items : 0u, RADIANCE_ITEMS_DEFAULT, plan)) return rc;
    if (n_rays == 0) return MI355RT_OK;
    if (int rc = query_begin(ctx)) return rc;
    const RadianceParams p = radiance_params(ctx, plan, params, d_rays, d_scratch);
    const RadianceSum s = radiance_sum(plan, n_rays, d_scratch, d_accum, d_out_linear);
    if (launch_radiance(p, s, ctx->has_mesh, plan.grid_paths, plan.grid_sum, hip_stream) != 0) return fail(MI355RT_ERR_HIP, "k_radiance launch failed");
    return MI355RT_OK;
    });
}

// ---- camera views (rt_view.hip): the rays of a pinhole or a thin lens made on the device, in front of the radiance queries' loop ----
// Every refusal and the grids are rt_prepare.cpp's (plan_view_rays, plan_view), before any HIP call.
int mi355rt_view_scratch_bytes(const mi355rt_view* view, uint32_t samples, uint64_t* out_bytes) {
    return guard([&]() -> int { return view_scratch_bytes(view, samples, out_bytes); });
}

int mi355rt_context_view_rays(mi355rt_context* ctx, const mi355rt_view* view, uint32_t sample, uint64_t seed, void* d_rays, void* hip_stream) {
    return guard([&]() -> int {
    ViewPlan plan{};
    if (int rc = plan_view_rays(ctx != nullptr, ctx && ctx->have_scene, view, d_rays, plan)) return rc;
    if (int rc = query_begin(ctx)) return rc;
    ViewParams v{}; view_params(view, plan, v);
    ViewRays r{};
    r.rays = d_rays; r.n_pixels = plan.n_pixels; r.sample = sample; r.seed_lo = (uint32_t)seed; r.seed_hi = (uint32_t)(seed >> 32);
    if (launch_view_rays(v, r, view->model, hip_stream) != 0) return fail(MI355RT_ERR_HIP, "k_view_rays launch failed");
    return MI355RT_OK;
    });
}

int mi355rt_context_render_view(mi355rt_context* ctx, const mi355rt_view* view, const mi355rt_radiance_params* params, void* d_accum, void* d_out_linear,
                                void* d_out_packed, void* d_scratch, void* hip_stream) {
    return guard([&]() -> int {
    ViewPlan plan{};
    if (int rc = plan_view(ctx != nullptr, ctx && ctx->have_scene, view, params, d_accum, d_out_linear, d_out_packed, d_scratch,
                           ctx ? (uint32_t)ctx->knob_radiance_items : 0u, RADIANCE_ITEMS_DEFAULT, plan)) return rc;
    if (int rc = query_begin(ctx)) return rc;
    const RadianceParams p = radiance_params(ctx, plan.r, params, nullptr, d_scratch);
    ViewParams v{}; view_params(view, plan, v);
    ViewSum s{};
    s.sum = radiance_sum(plan.r, plan.n_pixels, d_scratch, d_accum, d_out_linear); s.out_packed = (uint32_t*)d_out_packed;
    if (launch_view_paths(p, v, s, view->model, ctx->has_mesh, plan.r.grid_paths, plan.r.grid_sum, hip_stream) != 0) return fail(MI355RT_ERR_HIP, "k_view launch failed");
    return MI355RT_OK;
    });
}

// ---- surface probes (rt_probe.hip): cosine-hemisphere rays made on the device from the caller's points and normals, in front of the same loop ----
// Every refusal and the grids are rt_prepare.cpp's (plan_probe_rays, plan_probe), before any HIP call.
int mi355rt_context_probe_rays(mi355rt_context* ctx, const void* d_probes, uint32_t n, uint32_t sample, uint64_t seed, void* d_rays, void* hip_stream) {
    return guard([&]() -> int {
    static_assert(sizeof(mi355rt_probe) == 32 && sizeof(mi355rt_probe) == sizeof(mi355rt_path_ray), "the kernel reads a probe as two 16-byte halves");
    if (int rc = plan_probe_rays(ctx != nullptr, ctx && ctx->have_scene, d_probes, n, d_rays)) return rc;
    if (n == 0) return MI355RT_OK;
    if (int rc = query_begin(ctx)) return rc;
    ProbeParams b{}; b.probes = d_probes;
    ProbeRaysOut r{};
    r.rays = d_rays; r.n = n; r.sample = sample; r.seed_lo = (uint32_t)seed; r.seed_hi = (uint32_t)(seed >> 32);
    if (launch_probe_rays(b, r, hip_stream) != 0) return fail(MI355RT_ERR_HIP, "k_probe_rays launch failed");
    return MI355RT_OK;
    });
}

int mi355rt_context_probe_radiance(mi355rt_context* ctx, const mi355rt_radiance_params* params, const void* d_probes, uint32_t n, void* d_accum,
                                   void* d_out_linear, void* d_scratch, void* hip_stream) {
    return guard([&]() -> int {
    RadiancePlan plan{};
    if (int rc = plan_probe(ctx != nullptr, ctx && ctx->have_scene, params, d_probes, n, d_accum, d_out_linear, d_scratch,
                            ctx ? (uint32_t)ctx->knob_radiance_items : 0u, RADIANCE_ITEMS_DEFAULT, plan)) return rc;
    if (n == 0) return MI355RT_OK;
    if (int rc = query_begin(ctx)) return rc;
    const RadianceParams p = radiance_params(ctx, plan, params, nullptr, d_scratch);
    ProbeParams b{}; b.probes = d_probes;
    const RadianceSum s = radiance_sum(plan, n, d_scratch, d_accum, d_out_linear);
    if (launch_probe_paths(p, b, s, ctx->has_mesh, plan.grid_paths, plan.grid_sum, hip_stream) != 0) return fail(MI355RT_ERR_HIP, "k_probe launch failed");
    return MI355RT_OK;
    });
}

// ---- the denoiser (rt_denoise.hip): an a-trous filter over a linear image, guided by first-hit records --------------------------------
// The context names the device and carries the error word of its renders; nothing of it is read or written by the kernels.  What is decided
// before a device is involved -- the arguments, the per-level constants -- is rt_prepare.cpp's.
int mi355rt_denoise_scratch_bytes(uint32_t width, uint32_t rows, uint64_t* out_bytes) {
    return guard([&]() -> int { return denoise_scratch_bytes(width, rows, out_bytes); });
}

int mi355rt_context_denoise(mi355rt_context* ctx, uint32_t width, uint32_t rows, const mi355rt_denoise_params* params, const void* d_linear_in,
                            const void* d_hits, void* d_scratch, void* d_out_linear, void* d_out_packed, void* hip_stream) {
    return guard([&]() -> int {
    static_assert(sizeof(mi355rt_hit) == 48 && sizeof(mi355rt_denoise_params) == 16, "the prepass reads a hit record as three 16-byte words");
    if (!ctx) return fail(MI355RT_ERR_INVALID, "denoise: ctx is null");
    DenoiseLaunch d{};
    if (int rc = check_denoise_buffers(d_linear_in, d_hits, d_scratch, d_out_linear, d_out_packed)) return rc;
    if (int rc = plan_denoise(width, rows, params, d.plan)) return rc;
    if (int rc = query_begin(ctx)) return rc;
    d.in = (const float*)d_linear_in; d.hits = d_hits; d.scratch = d_scratch;
    d.out_linear = (float*)d_out_linear; d.out_packed = (uint32_t*)d_out_packed; d.width = width; d.rows = rows; d.staged = ctx->knob_denoise_staged;
    if (launch_denoise(d, hip_stream) != 0) return fail(MI355RT_ERR_HIP, "k_denoise launch failed");
    return MI355RT_OK;
    });
}

}  // extern "C"
