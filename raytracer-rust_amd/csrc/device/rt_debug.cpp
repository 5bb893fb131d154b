// rt_debug.cpp -- the diagnostic side of libmi355rt.so, none of it part of the public header: the mi355rt_debug_* hooks (what set_scene chose, what a
// render would launch, the raw counters and tables of the last render, one scatter / one hit per record through the render kernels' device functions)
// and the knobs (apply_knob, the process-wide defaults that mi355rt_context_create applies).  The context struct comes with rt_context.h.
#include <algorithm>
#include <map>
#include <mutex>
#include <string>

#include "rt_context.h"
#include "rt_radiance.h"

namespace {

// Diagnostic knobs (mi355rt_debug_set_knob; not part of the public header).  They replace the environment variables earlier
// rounds read at set_scene: a product library should not change behaviour with the caller's environment.
std::mutex g_knob_mutex;
std::map<std::string, int> g_default_knobs;
int apply_knob(mi355rt_context* ctx, const std::string& name, int v) {
    if (name == "kernel") { if (v < -1 || v >= (int)KERNEL_VARIANTS) return fail(MI355RT_ERR_INVALID, "knob kernel"); ctx->forced_variant = v; }
    else if (name == "inline_steps") { if (v < -1 || v > 8) return fail(MI355RT_ERR_INVALID, "knob inline_steps"); ctx->knob_inline_steps = v; }
    else if (name == "grid_div") { if (v < 1 || v > 16) return fail(MI355RT_ERR_INVALID, "knob grid_div"); ctx->grid_div = (uint32_t)v; }
    else if (name == "guided_mult") { if (v < 1 || v > 64) return fail(MI355RT_ERR_INVALID, "knob guided_mult"); ctx->guided_mult = (uint32_t)v; }
    else if (name == "trav_min") { if (v < 1 || v > 64) return fail(MI355RT_ERR_INVALID, "knob trav_min"); ctx->trav_min = (uint32_t)v; }
    else if (name == "spin_idle") { if (v < 1) return fail(MI355RT_ERR_INVALID, "knob spin_idle"); ctx->spin_limit_idle = (uint32_t)v; }
    else if (name == "spin_entry") { if (v < 1) return fail(MI355RT_ERR_INVALID, "knob spin_entry"); ctx->spin_limit_entry = (uint32_t)v; }
    else if (name == "wave_times") ctx->want_wave_times = v != 0;
    else if (name == "cam_cull") { if (v < -1 || v > 1) return fail(MI355RT_ERR_INVALID, "knob cam_cull"); ctx->knob_cam_cull = v; }
    else if (name == "resolve_skip") { if (v < 0 || v > 1) return fail(MI355RT_ERR_INVALID, "knob resolve_skip"); ctx->knob_resolve_skip = v; }
    else if (name == "denoise_staged") { if (v < 0 || v > 1) return fail(MI355RT_ERR_INVALID, "knob denoise_staged"); ctx->knob_denoise_staged = v; }
    else if (name == "ao_form") { if (v < 0 || v > 1) return fail(MI355RT_ERR_INVALID, "knob ao_form"); ctx->knob_ao_form = v; }
    else if (name == "radiance_items") { if (v < 0 || v > (int)RADIANCE_ITEMS_MAX) return fail(MI355RT_ERR_INVALID, "knob radiance_items"); ctx->knob_radiance_items = v; }
    else if (name == "row_order") { if (v < -1 || v > 1) return fail(MI355RT_ERR_INVALID, "knob row_order"); ctx->knob_row_order = v; }
    else return fail(MI355RT_ERR_INVALID, "unknown knob " + name);
    return MI355RT_OK;
}

}  // namespace

void mi355rt::apply_default_knobs(mi355rt_context* ctx) {
    std::lock_guard<std::mutex> g(g_knob_mutex);                        // process-wide diagnostic defaults (mi355rt_debug_set_knob(NULL, ...))
    for (const auto& kv : g_default_knobs) (void)apply_knob(ctx, kv.first, kv.second);
}

extern "C" {

// Diagnostic hook (not part of the public header).  ctx != NULL: set one knob of that context (before set_scene).  ctx == NULL: a
// process-wide default applied to every context created afterwards -- also those the one-shot calls create; name == NULL clears
// all defaults.  Knobs: kernel (KERNEL_* of rt_device.h, -1 = automatic), guided_mult, spin_idle, spin_entry, wave_times, row_order,
// cam_cull (0: k_render_ctr_simple_qc gets no camera masks), resolve_skip (0: k_resolve gets none), radiance_items (K of k_radiance_paths, 0 = the default), and for the reference build's state machine inline_steps, trav_min.
int mi355rt_debug_set_knob(mi355rt_context* ctx, const char* name, int value) {
    return guard([&]() -> int {
    if (ctx) return name ? apply_knob(ctx, name, value) : fail(MI355RT_ERR_INVALID, "knob name is null");
    std::lock_guard<std::mutex> g(g_knob_mutex);
    if (!name) { g_default_knobs.clear(); return MI355RT_OK; }
    mi355rt_context probe;                                            // validate name and range on a scratch context
    const int rc = apply_knob(&probe, name, value);
    if (rc == MI355RT_OK) g_default_knobs[name] = value;
    return rc;
    });
}
// 1 when this library holds the counter-mode kernel `variant` (the retired mesh kernels exist in the reference build only)
int mi355rt_debug_has_variant(uint32_t variant) { return render_ctr_variant_built(variant) ? 1 : 0; }

// Diagnostic hook (not part of the public header): which counter-mode kernel set_scene selected (KERNEL_* in rt_device.h).
int mi355rt_debug_kernel_variant(mi355rt_context* ctx, uint32_t* out) {
    return guard([&]() -> int {
    if (!ctx || !out || !ctx->have_scene) return fail(MI355RT_ERR_INVALID, "context has no scene");
    *out = ctx->variant;
    return MI355RT_OK;
    });
}

// Diagnostic hook (not part of the public header): the entry point the resident scene is launched on -- its kernel's name (a static string), how many of
// its workgroups the device holds per CU, and its VGPRs.  Variant 14 has two (rt_device.h ENTRY_*): with and without a sky texture.  Returns the name, or
// null for a context without a scene (nothing in here allocates or throws).
const char* mi355rt_debug_kernel_entry(mi355rt_context* ctx, uint32_t* out_blocks_per_cu, uint32_t* out_vgprs) {
    if (!ctx || !out_blocks_per_cu || !out_vgprs || !ctx->have_scene) return nullptr;
    const uint32_t e = ctx->entry();
    *out_blocks_per_cu = (uint32_t)ctx->blocks_per_cu[e][ctx->variant]; *out_vgprs = (uint32_t)ctx->vgprs[e][ctx->variant];
    return entry_kernel_name(ctx->variant, e);
}
// ... and the same choice without a device or a context: the name of the kernel a scene on `variant` is launched on, with or without a sky texture.
const char* mi355rt_debug_entry_kernel(uint32_t variant, int has_sky) {
    return variant < KERNEL_VARIANTS ? entry_kernel_name(variant, variant_entry(variant, has_sky != 0)) : nullptr;
}

// Diagnostic hook (not part of the public header): what set_scene would upload and choose for `scene`, without a device -- no HIP call, no
// context.  forced_variant: the "kernel" knob, -1 = the automatic choice.  Two calls, as mi355rt_bvh_build: with the arrays null it only
// counts; with an array given, its n_* holds the capacity on entry.  prims / nodes / tris: DevPrim / DevNode / DevTri records (rt_device.h).
int mi355rt_debug_prepare_scene(const mi355rt_scene* scene, int forced_variant, uint32_t* out_variant, uint32_t* out_inline_steps,
                                void* prims, uint32_t* n_prims, void* nodes, uint32_t* n_nodes, void* tris, uint32_t* n_tris) {
    return guard([&]() -> int {
    if (!out_variant || !out_inline_steps || !n_prims || !n_nodes || !n_tris) return fail(MI355RT_ERR_INVALID, "debug_prepare_scene: null");
    if (forced_variant < -1 || forced_variant >= (int)KERNEL_VARIANTS) return fail(MI355RT_ERR_INVALID, "knob kernel");
    PreparedScene s;
    const int rc = prepare_scene(scene, s); if (rc) return rc;
    if ((prims && *n_prims < s.prims.size()) || (nodes && *n_nodes < s.nodes.size()) || (tris && *n_tris < s.tris.size())) return fail(MI355RT_ERR_INVALID, "debug_prepare_scene: capacity");
    if (prims && !s.prims.empty()) std::memcpy(prims, s.prims.data(), s.prims.size() * sizeof(DevPrim));
    if (nodes && !s.nodes.empty()) std::memcpy(nodes, s.nodes.data(), s.nodes.size() * sizeof(DevNode));
    if (tris && !s.tris.empty()) std::memcpy(tris, s.tris.data(), s.tris.size() * sizeof(DevTri));
    *n_prims = (uint32_t)s.prims.size(); *n_nodes = (uint32_t)s.nodes.size(); *n_tris = (uint32_t)s.tris.size();
    *out_variant = choose_variant(s, forced_variant, built_variants());
    *out_inline_steps = choose_inline_steps(s, -1);
    return MI355RT_OK;
    });
}

// Diagnostic hook (not part of the public header): the camera masks set_scene would build for `scene` under `camera` and `settings`, without a device.
// options null: the absolute table, one word per pixel of the image; otherwise the table a render with those options reads, the selected rows in
// processing order (image order: the processing-order experiment needs a device).  Two calls: with `out` null it only counts.  *n == 0: no table
// (more than 32 primitives, or a scene that another kernel than forced_variant / the automatic choice's k_render_ctr_simple_qc serves).
int mi355rt_debug_camera_masks(const mi355rt_scene* scene, const mi355rt_camera* camera, const mi355rt_settings* settings, const mi355rt_options* options,
                               int forced_variant, uint32_t* out, uint64_t capacity, uint64_t* n) {
    return guard([&]() -> int {
    if (!camera || !n) return fail(MI355RT_ERR_INVALID, "debug_camera_masks: null");
    if (forced_variant < -1 || forced_variant >= (int)KERNEL_VARIANTS) return fail(MI355RT_ERR_INVALID, "knob kernel");
    int rc = check_settings(settings); if (rc) return rc;
    PreparedScene s;
    rc = prepare_scene(scene, s); if (rc) return rc;
    std::vector<uint32_t> table, gathered;
    if (choose_variant(s, forced_variant, built_variants()) == KERNEL_LOCKSTEP_SIMPLE_QC) {
        DevCamera cam; std::memcpy(&cam, camera, sizeof cam);
        build_camera_masks(s, cam, settings->width, settings->height, table);
    }
    if (options && !table.empty()) {
        RowSel sel; rc = select_rows(*settings, options, sel); if (rc) return rc;
        gather_camera_masks(table, settings->width, sel.rows.data(), sel.rows.size(), gathered);
        table.swap(gathered);
    }
    *n = table.size();
    if (out) { if (capacity < table.size()) return fail(MI355RT_ERR_INVALID, "debug_camera_masks: capacity"); if (!table.empty()) std::memcpy(out, table.data(), table.size() * sizeof(uint32_t)); }
    return MI355RT_OK;
    });
}

// Diagnostic hook (not part of the public header): what a render with these inputs would launch, without a device -- no HIP call, no context -- by the
// plan_render, halve_bands, render_band and row_tables that render_samples calls.  args: the context's side of RenderPlanIn (device.PlanProbeArgs has
// the same layout); row_cost: a per-image-row cost of the caller's (n_cost entries, 0 = none: image order).  `halvings` "the band did not fit" steps
// are taken first; *halved = how many of them existed.  out_plan: a RenderPlan.  Two calls, as mi355rt_debug_prepare_scene: with bands / tables null
// it only counts (*n_bands RenderBand records, 3 x *n_rows table entries); with an array given, its n_* holds the capacity on entry.
struct PlanProbeArgs { uint32_t s0, s1, have_accum, variant, has_mesh, n_prims, row_probe, grid_div, guided_mult, block_slots[KERNEL_VARIANTS]; };
int mi355rt_debug_plan_render(const mi355rt_settings* settings, const mi355rt_options* options, const void* args, const float* row_cost, uint32_t n_cost,
                              uint32_t halvings, void* out_plan, uint32_t* halved, void* bands, uint32_t* n_bands, uint32_t* tables, uint32_t* n_rows) {
    return guard([&]() -> int {
    if (!args || !out_plan || !halved || !n_bands || !n_rows || (n_cost && !row_cost)) return fail(MI355RT_ERR_INVALID, "debug_plan_render: null");
    int rc = check_settings(settings); if (rc) return rc;
    const PlanProbeArgs a = *static_cast<const PlanProbeArgs*>(args);
    if (a.variant >= KERNEL_VARIANTS) return fail(MI355RT_ERR_INVALID, "knob kernel");
    if (a.s1 <= a.s0) return fail(MI355RT_ERR_INVALID, "sample_end must be greater than sample_begin");
    if (a.grid_div < 1u || a.grid_div > 16u) return fail(MI355RT_ERR_INVALID, "share_of must be 1 .. 16");
    if (a.guided_mult < 1u || a.guided_mult > 64u) return fail(MI355RT_ERR_INVALID, "knob guided_mult");
    const RenderPlanIn in{settings, options, a.s0, a.s1, a.have_accum != 0u, a.variant, a.has_mesh != 0u, a.n_prims, n_cost != 0u, a.row_probe != 0u,
                          a.block_slots, a.grid_div, a.guided_mult};
    RowSel sel; RenderPlan plan;
    rc = plan_render(in, sel, plan); if (rc) return rc;
    for (*halved = 0; *halved < halvings && halve_bands(plan); ) ++*halved;
    const bool counter_mode = plan.rng_mode == MI355RT_RNG_CTR;      // (the replay mode's one launch has no band record)
    if (bands && counter_mode && plan.n_bands) {
        if (*n_bands < plan.n_bands) return fail(MI355RT_ERR_INVALID, "debug_plan_render: capacity");
        if (plan.block_threads == 0u) return fail(MI355RT_ERR_INVALID, "debug_plan_render: a retired variant has no launch");
        for (uint32_t b = 0; b < plan.n_bands; ++b) static_cast<RenderBand*>(bands)[b] = render_band(plan, b);
    }
    *n_bands = counter_mode ? plan.n_bands : 0u;
    if (tables) {
        if (*n_rows < sel.rows.size()) return fail(MI355RT_ERR_INVALID, "debug_plan_render: capacity");
        std::vector<uint32_t> t;
        row_tables(sel.rows, plan.order_groups ? std::vector<float>(row_cost, row_cost + n_cost) : std::vector<float>(), plan.order_groups, t);
        if (!t.empty()) std::memcpy(tables, t.data(), t.size() * sizeof(uint32_t));
    }
    *n_rows = (uint32_t)sel.rows.size();
    std::memcpy(out_plan, &plan, sizeof plan);
    return MI355RT_OK;
    });
}

// Diagnostic hook (not part of the public header): the STATS_WORDS (40) raw device counters of the last render.
int mi355rt_debug_read_counters(mi355rt_context* ctx, unsigned long long* out40) {
    return guard([&]() -> int {
    if (!ctx || !out40 || !ctx->stats.p) return fail(MI355RT_ERR_INVALID, "no counters");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpy(out40, ctx->stats.p, STATS_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return MI355RT_OK;
    });
}

// Diagnostic hook (not part of the public header): the row tables of the last render on this context -- 3 x n entries (natural, processing,
// out_row; see rt_prepare.h row_tables()) -- and the per-image-row cost the processing order was built from (`cost`, `height` entries; may be null).
int mi355rt_debug_read_row_tables(mi355rt_context* ctx, uint32_t* tables, uint32_t capacity_entries, uint32_t* n_rows, float* cost, uint32_t cost_capacity, uint32_t* n_cost) {
    return guard([&]() -> int {
    if (!ctx || !n_rows) return fail(MI355RT_ERR_INVALID, "null");
    const size_t n = ctx->rows_host.size();
    *n_rows = (uint32_t)n;
    if (tables) { if (capacity_entries < 3 * n || ctx->tables_host.size() != 3 * n) return fail(MI355RT_ERR_INVALID, "row tables: capacity"); std::memcpy(tables, ctx->tables_host.data(), 3 * n * sizeof(uint32_t)); }
    if (n_cost) *n_cost = (uint32_t)ctx->row_cost.size();
    if (cost) { if (cost_capacity < ctx->row_cost.size()) return fail(MI355RT_ERR_INVALID, "row cost: capacity"); std::memcpy(cost, ctx->row_cost.data(), ctx->row_cost.size() * sizeof(float)); }
    return MI355RT_OK;
    });
}

int mi355rt_debug_read_wave_times(mi355rt_context* ctx, unsigned long long* out, uint32_t capacity_waves, uint32_t* n_waves) {
    return guard([&]() -> int {
    if (!ctx || !out || !n_waves) return fail(MI355RT_ERR_INVALID, "null");
    HIP_TRY(hipSetDevice(ctx->device));
    const uint32_t n = std::min(capacity_waves, ctx->wave_times_n);
    if (n) HIP_TRY(hipMemcpy(out, ctx->wave_times.p, (size_t)n * WAVE_TIME_WORDS * 8, hipMemcpyDeviceToHost));
    *n_waves = n;
    return MI355RT_OK;
    });
}

// Diagnostic hooks (not part of the public header): one Material::scatter / one HittableList::hit per record through the
// device functions of the render kernels, on the context's resident scene.  Host pointers in and out; records are the
// 16- / 6- / 12-word PODs of rt_device.h.
int mi355rt_debug_scatter(mi355rt_context* ctx, const void* in_records, uint32_t n, void* out_records) {
    return guard([&]() -> int {
    if (!ctx || !ctx->have_scene || !in_records || !out_records) return fail(MI355RT_ERR_INVALID, "debug_scatter: null / no scene");
    HIP_TRY(hipSetDevice(ctx->device));
    const DebugScatterIn* in = static_cast<const DebugScatterIn*>(in_records);
    for (uint32_t i = 0; i < n; ++i) if (in[i].material >= ctx->n_mats) return fail(MI355RT_ERR_INVALID, "debug_scatter: material index");
    DevBuf<DebugScatterIn> d_in; DevBuf<DebugScatterOut> d_out;
    int rc = d_in.ensure(n); if (!rc) rc = d_out.ensure(n);
    if (!rc && n) {
        if (hipMemcpy(d_in.p, in, n * sizeof(DebugScatterIn), hipMemcpyHostToDevice) != hipSuccess || launch_debug_scatter(ctx->mats.p, ctx->textures.p, d_in.p, d_out.p, n, nullptr) != 0 ||
            hipMemcpy(out_records, d_out.p, n * sizeof(DebugScatterOut), hipMemcpyDeviceToHost) != hipSuccess) rc = fail(MI355RT_ERR_HIP, "debug_scatter");
    }
    d_in.release(); d_out.release();
    return rc;
    });
}

int mi355rt_debug_hit(mi355rt_context* ctx, const void* in_rays, uint32_t n, void* out_records) {
    return guard([&]() -> int {
    if (!ctx || !ctx->have_scene || !in_rays || !out_records) return fail(MI355RT_ERR_INVALID, "debug_hit: null / no scene");
    HIP_TRY(hipSetDevice(ctx->device));
    DevBuf<DebugHitIn> d_in; DevBuf<DebugHitOut> d_out;
    int rc = d_in.ensure(n); if (!rc) rc = d_out.ensure(n);
    if (!rc && n) {
        if (hipMemcpy(d_in.p, in_rays, n * sizeof(DebugHitIn), hipMemcpyHostToDevice) != hipSuccess ||
            launch_debug_hit(ctx->prims.p, ctx->n_prims, ctx->nodes.p, ctx->tris.p, d_in.p, d_out.p, n, nullptr) != 0 ||
            hipMemcpy(out_records, d_out.p, n * sizeof(DebugHitOut), hipMemcpyDeviceToHost) != hipSuccess) rc = fail(MI355RT_ERR_HIP, "debug_hit");
    }
    d_in.release(); d_out.release();
    return rc;
    });
}

}  // extern "C"
