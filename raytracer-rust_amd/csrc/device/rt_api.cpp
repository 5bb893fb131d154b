// rt_api.cpp -- implementation of the device half of include/mi355rt.h (libmi355rt.so).
//
// Replaces `render_scene(&scene, &camera, &render_settings) -> Vec<u32>` (src/renderer.rs:67,
// called from src/main.rs:57).  There is NO CPU fallback in this library: without a HIP device every
// render entry point returns MI355RT_ERR_NO_DEVICE.  What happens to a scene before a device is involved -- validation, the BVH re-lay, the
// primitive records, the choice of the kernel variant -- and what a render call launches -- its refusals, the variant, the bands and their grids -- is
// rt_prepare.cpp, which has no HIP in it; this file uploads and launches: the context's life cycle, set_scene with its probes, the renders, the
// share, timing and check.  The context struct is rt_context.h's; the calls that only read the resident scene (queries, views, probes, the denoiser)
// are rt_queries.cpp, the mi355rt_debug_* hooks and the knobs rt_debug.cpp.  The calls with host buffers (mi355rt_render and its kin) are clients of
// the public functions and live in rt_oneshot.cpp.
#include <algorithm>
#include <new>
#include <string>

#include "rt_context.h"

// Compares the host copy of the context's error word with what has already been reported.  The copy is refreshed in stream order
// behind every render, so after a wait on `done` it covers every render enqueued so far; without a wait it covers those that
// have finished.
// `this_render`: the caller has just waited for the render it enqueued itself (the stats path), so the failure is that render's; otherwise it
// belongs to an earlier, asynchronous render on this context.  The word names the kernel(s) and the wait(s) that gave up (rt_device.h, err_tag).
int mi355rt::report_device_error(mi355rt_context* ctx, bool this_render) {
    if (!ctx->h_err) return MI355RT_OK;
    const unsigned long long now = *(volatile unsigned long long*)ctx->h_err;
    const unsigned long long count = now & 0xFFFFFFFFull;
    if (count == ctx->err_reported) return MI355RT_OK;
    const unsigned long long n = count - ctx->err_reported;
    ctx->err_reported = count;
    static const struct { uint32_t bit; const char* what; } waits[] = {
        {WAIT_WF_IDLE, "idle: no progress in the workgroup"}, {WAIT_WF_RING, "ring entry: a reserved ticket was never written, or an entry never emptied"},
        {WAIT_WF_FOLLOWED, "waves that followed their workgroup's error flag out"}};
    std::string kernels, which;
    for (uint32_t v = 0; v < KERNEL_VARIANTS; ++v) if ((ctx->launched_variants >> v) & 1u)
        kernels += std::string(kernels.empty() ? "" : ", ") + entry_kernel_name(v, (ctx->launched_sky_entries >> v) & 1u ? ENTRY_SKY : ENTRY_PLAIN) + " (variant " + std::to_string(v) + ")";
    ctx->launched_variants = 0; ctx->launched_sky_entries = 0;
    for (const auto& w : waits) if ((now >> 32) & w.bit) which += std::string(which.empty() ? "" : "; ") + w.what;
    return fail(MI355RT_ERR_HIP, "kernel watchdog: " + std::to_string(n) + " wave(s) gave up a bounded wait " + (this_render ? "in this render" : "in an earlier render on this context") +
                                 " -- that image is incomplete [kernel(s) launched on this context since the last report: " + (kernels.empty() ? "?" : kernels) + "; wait: " + (which.empty() ? "?" : which) +
                                 "; limits: " + std::to_string(ctx->spin_limit_idle) + " idle polls, " + std::to_string(ctx->spin_limit_entry) + " polls of a ring entry]");
}

namespace {

// The upload of a prepared scene (rt_prepare.h: validated and laid out without HIP) and what the context keeps of it.
int build_device_scene(mi355rt_context* ctx, const mi355rt_scene* sc, const mi355rt_camera* camera, const mi355rt_settings* st) {
    PreparedScene s;
    int rc = prepare_scene(sc, s); if (rc) return rc;
    const bool has_sky = sc->sky_rgb != nullptr;
    if ((rc = ctx->prims.ensure(s.prims.size()))) return rc;
    if ((rc = ctx->mats.ensure(sc->n_materials))) return rc;
    if ((rc = ctx->nodes.ensure(s.nodes.size()))) return rc;
    if ((rc = ctx->tris.ensure(s.tris.size()))) return rc;
    static_assert(sizeof(DevMat) == sizeof(mi355rt_material), "material layout is shared with the ABI");
    if (!s.prims.empty()) HIP_TRY(hipMemcpy(ctx->prims.p, s.prims.data(), s.prims.size() * sizeof(DevPrim), hipMemcpyHostToDevice));
    if (sc->n_materials) HIP_TRY(hipMemcpy(ctx->mats.p, sc->materials, sc->n_materials * sizeof(DevMat), hipMemcpyHostToDevice));
    if (!s.nodes.empty()) HIP_TRY(hipMemcpy(ctx->nodes.p, s.nodes.data(), s.nodes.size() * sizeof(DevNode), hipMemcpyHostToDevice));
    if (!s.tris.empty()) HIP_TRY(hipMemcpy(ctx->tris.p, s.tris.data(), s.tris.size() * sizeof(DevTri), hipMemcpyHostToDevice));
    ctx->n_prims = sc->n_primitives; ctx->n_mats = sc->n_materials; ctx->n_nodes = s.nodes.size();
    std::memcpy(ctx->miss, sc->miss_color, 12);
    ctx->sky_w = ctx->sky_h = 0;
    if (has_sky) {
        const size_t nf = (size_t)sc->sky_width * sc->sky_height * 3;
        if ((rc = ctx->sky.ensure(nf))) return rc;
        HIP_TRY(hipMemcpy(ctx->sky.p, sc->sky_rgb, nf * sizeof(float), hipMemcpyHostToDevice));
        ctx->sky_w = sc->sky_width; ctx->sky_h = sc->sky_height;
    }
    if (sc->n_textures) {
        if ((rc = ctx->texels.ensure((size_t)s.n_texels))) return rc;
        if ((rc = ctx->textures.ensure(sc->n_textures))) return rc;
        std::vector<DevTexture> table(sc->n_textures);
        size_t off = 0;
        for (uint32_t i = 0; i < sc->n_textures; ++i) {
            const mi355rt_texture& t = sc->textures[i];
            const size_t n = (size_t)t.width * t.height;
            HIP_TRY(hipMemcpy(ctx->texels.p + off, t.rgba8, n * 4, hipMemcpyHostToDevice));
            table[i] = DevTexture{ctx->texels.p + off, t.width, t.height};
            off += n;
        }
        HIP_TRY(hipMemcpy(ctx->textures.p, table.data(), table.size() * sizeof(DevTexture), hipMemcpyHostToDevice));
    }
    ctx->has_mesh = s.n_mesh_prims != 0;
    ctx->occlusion_may_exit = scene_within_occlusion_bound(s);
    ctx->variant = choose_variant(s, ctx->forced_variant, built_variants());
    ctx->inline_steps = choose_inline_steps(s, ctx->knob_inline_steps);
    ctx->cam_mask_abs.clear(); ctx->cam_mask_host.clear();                    // (clear keeps the allocations: the next table is written in place)
    if (ctx->variant == KERNEL_LOCKSTEP_SIMPLE_QC && ctx->knob_cam_cull != 0) {
        static_assert(sizeof(DevCamera) == sizeof(mi355rt_camera), "camera layout is shared with the ABI");
        DevCamera cam; std::memcpy(&cam, camera, sizeof cam);
        build_camera_masks(s, cam, st->width, st->height, ctx->cam_mask_abs);
        ctx->cam_mask_w = st->width; ctx->cam_mask_h = st->height;
    }
    return MI355RT_OK;
}

}  // namespace

extern "C" {

const char* mi355rt_last_error(void) { return last_error().c_str(); }
uint32_t mi355rt_abi_version(void) { return MI355RT_ABI_VERSION; }

int mi355rt_rows_selected(const mi355rt_settings* settings, const mi355rt_options* options, uint32_t* out_rows) {
    return guard([&]() -> int {
    int rc = check_settings(settings); if (rc) return rc;
    if (!out_rows) return fail(MI355RT_ERR_INVALID, "out_rows is null");
    RowSel sel; rc = select_rows(*settings, options, sel); if (rc) return rc;
    *out_rows = (uint32_t)sel.rows.size();
    return MI355RT_OK;
    });
}

int mi355rt_context_create(int hip_device, mi355rt_context** out_ctx) {
    return guard([&]() -> int {
    if (!out_ctx) return fail(MI355RT_ERR_INVALID, "out_ctx is null");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(MI355RT_ERR_NO_DEVICE, "no HIP device visible (this library has no CPU path)");
    if (hip_device < 0 || hip_device >= n) return fail(MI355RT_ERR_NO_DEVICE, "hip_device out of range");
    HIP_TRY(hipSetDevice(hip_device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, hip_device));
    mi355rt_context* ctx = new (std::nothrow) mi355rt_context();
    if (!ctx) return fail(MI355RT_ERR_OOM, "host allocation failed");
    ctx->device = hip_device;
    ctx->cu_count = prop.multiProcessorCount;
    for (uint32_t v = 0; v < KERNEL_VARIANTS; ++v) {
        if (!render_ctr_variant_built(v)) continue;                    // the retired mesh kernels exist in the tests' reference build only
        for (uint32_t e = 0; e < KERNEL_ENTRIES; ++e)
        if (query_render_ctr_occupancy(v, e, &ctx->blocks_per_cu[e][v], &ctx->vgprs[e][v], &ctx->sgprs) != 0 || ctx->blocks_per_cu[e][v] <= 0) {
            delete ctx;
            return fail(MI355RT_ERR_HIP, std::string("kernel image not usable on this device (") + prop.gcnArchName + "); built for gfx950");
        }
    }
    for (auto& e : ctx->ev) if (hipEventCreate(&e) != hipSuccess) { delete ctx; return fail(MI355RT_ERR_HIP, "hipEventCreate"); }
    if (hipEventCreateWithFlags(&ctx->done, hipEventDisableTiming) != hipSuccess) { delete ctx; return fail(MI355RT_ERR_HIP, "hipEventCreate"); }
    if (ctx->errword.ensure(1) != MI355RT_OK || hipMemset(ctx->errword.p, 0, sizeof(unsigned long long)) != hipSuccess ||
        hipHostMalloc((void**)&ctx->h_err, sizeof(unsigned long long), hipHostMallocDefault) != hipSuccess) { mi355rt_context_destroy(ctx); return fail(MI355RT_ERR_HIP, "error word allocation"); }
    *ctx->h_err = 0ull;
    apply_default_knobs(ctx);                                        // process-wide diagnostic defaults (mi355rt_debug_set_knob(NULL, ...): rt_debug.cpp)
    *out_ctx = ctx;
    return MI355RT_OK;
    });
}

void mi355rt_context_destroy(mi355rt_context* ctx) {                 // (nothing in here allocates or throws: HIP calls and destructors of PODs' containers)
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    ctx->prims.release(); ctx->mats.release(); ctx->nodes.release(); ctx->tris.release(); ctx->rows.release();
    ctx->radiance.release(); ctx->counters.release(); ctx->stats.release(); ctx->fold_stack.release(); ctx->wave_times.release(); ctx->sky.release();
    ctx->textures.release(); ctx->texels.release(); ctx->errword.release(); ctx->query_rows_release();
    if (ctx->h_err) (void)hipHostFree(ctx->h_err);
    for (auto& e : ctx->ev) if (e) (void)hipEventDestroy(e);
    if (ctx->done) (void)hipEventDestroy(ctx->done);
    for (auto& e : ctx->pool) if (e) (void)hipEventDestroy(e);
    delete ctx;
}

static int render_samples(mi355rt_context* ctx, const mi355rt_options* opt, uint32_t s0, uint32_t s1, void* d_accum,
                          void* d_out_packed, void* d_out_linear, void* hip_stream, mi355rt_stats* stats, unsigned long long* d_row_counters = nullptr);

int mi355rt_context_set_scene(mi355rt_context* ctx, const mi355rt_scene* scene, const mi355rt_camera* camera,
                              const mi355rt_settings* settings) {
    return guard([&]() -> int {
    if (!ctx) return fail(MI355RT_ERR_INVALID, "ctx is null");
    if (!camera) return fail(MI355RT_ERR_INVALID, "camera is null");
    int rc = check_settings(settings); if (rc) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    ctx->have_scene = false; ctx->rows_valid = false;
    ctx->query_rows_release();                                       // (the tables belong to the old settings)
    rc = build_device_scene(ctx, scene, camera, settings); if (rc) return rc;
    static_assert(sizeof(DevCamera) == sizeof(mi355rt_camera), "camera layout is shared with the ABI");
    std::memcpy(&ctx->cam, camera, sizeof(DevCamera));
    ctx->settings = *settings;
    ctx->have_scene = true;
    // The probe renders below are set_scene's own business: they stay out of the caller's timing pool (mi355rt_context_set_timing).
    struct TimingOff { mi355rt_context* c; bool was; ~TimingOff() { c->timing = was; } } timing_off{ctx, ctx->timing};
    ctx->timing = false;
    // The materials only say that the mesh-free wavefront kernel MAY pay (a rough conductor next to another scattering material).  Whether
    // it does depends on how much the paths scatter: veach-mis bounces 1.5 times per path and gains 13 %; a scene of the same materials that is
    // mostly sky (1.1 rays per path) has nothing to sort and lost 14 % to the queues (profiles/r03_ab_meshfree_wavefront_fuzz_scenes.txt).
    // A probe decides: the same view at 64 pixels across, 4 samples per pixel, on the lockstep kernel -- deterministic (counter RNG), a
    // fraction of a millisecond -- and the wavefront form is kept when a path traces at least PROBE_RAYS_PER_PATH rays.
    // Both probes below render with the context's settings (and, the first, its variant) swapped for the probe's.  Whatever way they are left --
    // a return code, a HIP failure, a C++ exception out of render_samples' host allocations -- ProbeScope puts the full-size settings back, drops
    // the row tables of the probe size, frees the probe's device buffers and, unless the probe was committed, leaves the context WITHOUT a scene:
    // a context that kept have_scene with 64-pixel-wide settings would render a probe-sized image into the caller's full-size buffer.
    struct ProbeScope {
        mi355rt_context* c; mi355rt_settings full; uint32_t variant; uint32_t* d_tmp = nullptr; unsigned long long* d_cnt = nullptr; bool committed = false;
        ProbeScope(mi355rt_context* ctx) : c(ctx), full(ctx->settings), variant(ctx->variant) {}
        ~ProbeScope() {
            c->settings = full; c->rows_valid = false;
            if (d_tmp) (void)hipFree(d_tmp);
            if (d_cnt) (void)hipFree(d_cnt);
            if (!committed) { c->variant = variant; c->have_scene = false; c->row_cost.clear(); }
        }
    };
    if (ctx->variant == KERNEL_WAVEFRONT_MESHFREE && ctx->forced_variant < 0) {
        constexpr double PROBE_RAYS_PER_PATH = 1.6;       // veach-mis with max_bounces 1 / 2 / 3 / 16: 1.00 / 1.90 / 2.20 / 2.48 rays per path, wavefront +5.5 / -4.0 / -6.5 / -10.2 %
                                                          // against lockstep (profiles/r03_probe_calibration.txt): break-even near 1.5
        ProbeScope scope(ctx);
        mi355rt_settings probe = scope.full;
        probe.width = std::min(scope.full.width, 64u);
        probe.height = std::max(1u, std::min(scope.full.height, (uint32_t)((uint64_t)probe.width * scope.full.height / scope.full.width)));
        probe.samples_per_pixel = std::min(scope.full.samples_per_pixel, 4u);
        if (hipMalloc((void**)&scope.d_tmp, (size_t)probe.width * probe.height * 4) != hipSuccess) { scope.d_tmp = nullptr; return fail(MI355RT_ERR_OOM, "hipMalloc(probe)"); }
        ctx->settings = probe; ctx->variant = KERNEL_LOCKSTEP_NOSPEC;
        mi355rt_stats st{};
        rc = render_samples(ctx, nullptr, 0, probe.samples_per_pixel, nullptr, scope.d_tmp, nullptr, nullptr, &st);
        if (rc) return rc;
        ctx->variant = ((double)st.rays >= PROBE_RAYS_PER_PATH * (double)std::max<uint64_t>(st.samples, 1)) ? KERNEL_WAVEFRONT_MESHFREE : KERNEL_LOCKSTEP_NOSPEC;
        scope.committed = true;
    }
    // Row costs for the processing order (see mi355rt_context::row_cost): the same view at <= 64 x 96 pixels, 4 samples per pixel, one small
    // launch per probe row with its own {paths, rays} counters, all enqueued back to back and read after ONE wait -- deterministic (counter
    // RNG), a few milliseconds.  Only the diagnostic knob turns it on (measured, profiles/r04/ab_processing_order.txt: +-0.5 % on full frames --
    // the tail of a launch is old paths that waited in thin queues, not the rows handed out last).
    ctx->row_cost.clear();
    if (ctx->knob_row_order == 1) {
        ProbeScope scope(ctx);
        mi355rt_settings probe = scope.full;
        probe.width = std::min(scope.full.width, 64u);
        probe.height = std::min(scope.full.height, 96u);
        probe.samples_per_pixel = std::min(scope.full.samples_per_pixel, 4u);
        std::vector<unsigned long long> h_cnt(STATS_WORDS * (size_t)probe.height);
        if (hipMalloc((void**)&scope.d_tmp, (size_t)probe.width * probe.height * 4) != hipSuccess) { scope.d_tmp = nullptr; return fail(MI355RT_ERR_OOM, "hipMalloc(row probe)"); }
        if (hipMalloc((void**)&scope.d_cnt, h_cnt.size() * 8) != hipSuccess) { scope.d_cnt = nullptr; return fail(MI355RT_ERR_OOM, "hipMalloc(row probe)"); }
        HIP_TRY(hipMemset(scope.d_cnt, 0, h_cnt.size() * 8));
        ctx->settings = probe;
        rc = render_samples(ctx, nullptr, 0, probe.samples_per_pixel, nullptr, scope.d_tmp, nullptr, nullptr, nullptr, scope.d_cnt);
        if (rc) return rc;
        HIP_TRY(hipMemcpy(h_cnt.data(), scope.d_cnt, h_cnt.size() * 8, hipMemcpyDeviceToHost));                    // (waits for the launches)
        if ((rc = report_device_error(ctx))) return rc;
        ctx->row_cost.resize(scope.full.height);
        for (uint32_t y = 0; y < scope.full.height; ++y) {
            const uint32_t i = (uint32_t)std::min<uint64_t>(probe.height - 1, (uint64_t)y * probe.height / scope.full.height);
            ctx->row_cost[y] = (float)((double)h_cnt[STATS_WORDS * (size_t)i + 1] / (double)std::max<unsigned long long>(h_cnt[STATS_WORDS * (size_t)i], 1ull));
        }
        scope.committed = true;
    }
    return MI355RT_OK;
    });
}

// Samples [s0, s1) of every selected pixel.  The classic call is (0, settings.spp, no accumulator).  What is launched -- every refusal, the variant,
// the bands, each band's grid -- is plan_render's (rt_prepare.cpp, no HIP); this function enqueues it.  A refused call has touched neither the
// stream nor the context's row tables.
// d_row_counters (set_scene's row-cost probe only): one launch per selected ROW, each with its own block of device counters ({paths, rays, ...})
// at d_row_counters + STATS_WORDS * row, nothing resolved, nothing waited for.
static int render_samples(mi355rt_context* ctx, const mi355rt_options* opt, uint32_t s0, uint32_t s1, void* d_accum,
                          void* d_out_packed, void* d_out_linear, void* hip_stream, mi355rt_stats* stats, unsigned long long* d_row_counters) {
    if (!ctx || !ctx->have_scene) return fail(MI355RT_ERR_INVALID, "context has no scene");
    if (!d_out_packed) return fail(MI355RT_ERR_INVALID, "d_out_packed is null");
    HIP_TRY(hipSetDevice(ctx->device));
    if (int erc = report_device_error(ctx)) return erc;              // an earlier asynchronous render on this context failed (no wait: what has finished so far)
    const mi355rt_settings& st = ctx->settings;
    uint32_t block_slots[KERNEL_VARIANTS];
    for (uint32_t v = 0; v < KERNEL_VARIANTS; ++v) block_slots[v] = (uint32_t)(ctx->cu_count * ctx->blocks_per_cu[variant_entry(v, ctx->sky_w != 0)][v]);   // (of the entry point that launch_render_ctr picks)
    const RenderPlanIn in{&st, opt, s0, s1, d_accum != nullptr, ctx->variant, ctx->has_mesh, ctx->n_prims, !ctx->row_cost.empty(), d_row_counters != nullptr,
                          block_slots, ctx->grid_div, ctx->guided_mult};
    RowSel sel; RenderPlan plan;
    int rc = plan_render(in, sel, plan); if (rc) return rc;

    hipStream_t stream = (hipStream_t)hip_stream;
    if (ctx->have_last && ctx->last_stream != stream) HIP_TRY(hipStreamWaitEvent(stream, ctx->done, 0));   // the previous render owned the workspaces
    const bool same_rows = ctx->rows_valid && sel.rows == ctx->rows_host && plan.order_groups == ctx->order_groups;
    if (!same_rows) {
        if (ctx->have_last) HIP_TRY(hipEventSynchronize(ctx->done));   // a previous call's row-table upload may still read tables_host
        ctx->rows_host.swap(sel.rows);
        static const std::vector<float> no_cost;
        row_tables(ctx->rows_host, plan.order_groups ? ctx->row_cost : no_cost, plan.order_groups, ctx->tables_host);
        // the camera masks of these rows, in processing order (set_scene's probes render with other settings: the table is not theirs)
        ctx->cam_mask_host.clear();
        if (!ctx->cam_mask_abs.empty() && ctx->cam_mask_w == st.width && ctx->cam_mask_h == st.height)
            gather_camera_masks(ctx->cam_mask_abs, st.width, ctx->tables_host.data() + ctx->rows_host.size(), ctx->rows_host.size(), ctx->cam_mask_host);
        ctx->order_groups = plan.order_groups;
        ctx->rows_valid = false;
    }
    const uint32_t variant = plan.variant;
    const uint32_t n_rows = (uint32_t)ctx->rows_host.size();
    if (stats) { std::memset(stats, 0, sizeof *stats); stats->rows_rendered = n_rows; stats->kernel_vgprs = (uint32_t)ctx->vgprs[variant_entry(variant, ctx->sky_w != 0)][variant]; stats->kernel_sgprs = (uint32_t)ctx->sgprs; }
    if (n_rows == 0) return MI355RT_OK;

    if (!same_rows) {
        if ((rc = ctx->rows.ensure(3 * (size_t)n_rows + ctx->cam_mask_host.size()))) return rc;
        HIP_TRY(hipMemcpyAsync(ctx->rows.p, ctx->tables_host.data(), 3 * (size_t)n_rows * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
        if (!ctx->cam_mask_host.empty())
            HIP_TRY(hipMemcpyAsync(ctx->rows.p + 3 * (size_t)n_rows, ctx->cam_mask_host.data(), ctx->cam_mask_host.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
        ctx->rows_valid = true;
    }
    const uint32_t* d_rows_natural = ctx->rows.p;
    const uint32_t* d_rows_processing = ctx->rows.p + n_rows;
    const uint32_t* d_out_row = ctx->order_groups ? ctx->rows.p + 2 * (size_t)n_rows : nullptr;      // null: processing order == output order
    if ((rc = ctx->stats.ensure(STATS_WORDS))) return rc;
    HIP_TRY(hipMemsetAsync(ctx->stats.p, 0, STATS_WORDS * sizeof(unsigned long long), stream));

    double render_ms = 0, resolve_ms = 0, total_ms = 0;
    uint32_t grid_blocks = 0;

    if (plan.rng_mode == MI355RT_RNG_REF) {
        if ((rc = ctx->fold_stack.ensure((size_t)n_rows * std::max(st.max_depth, 1u) * 3))) return rc;
        RefParams rp{};
        bind_geometry(ctx, rp); bind_shading(ctx, rp);
        rp.rows = d_rows_natural; rp.out_packed = (uint32_t*)d_out_packed; rp.out_linear = (float*)d_out_linear; rp.fold_stack = ctx->fold_stack.p; rp.stats = ctx->stats.p;
        rp.n_mats = ctx->n_mats; rp.n_rows = n_rows; rp.cam = ctx->cam;
        rp.width = st.width; rp.height = st.height; rp.spp = st.samples_per_pixel; rp.max_depth = st.max_depth;
        rp.seed_lo = plan.seed_lo; rp.seed_hi = plan.seed_hi;
        if (stats) HIP_TRY(hipEventRecord(ctx->ev[0], stream));
        if (launch_render_ref(rp, stream) != 0) return fail(MI355RT_ERR_HIP, "k_render_ref launch failed");
        if (stats) {
            HIP_TRY(hipEventRecord(ctx->ev[1], stream));
            HIP_TRY(hipEventSynchronize(ctx->ev[1]));
            float ms = 0; HIP_TRY(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
            render_ms = total_ms = ms;
        }
        grid_blocks = n_rows;
    } else {
        // Only what a band needs is allocated.  When even that does not fit (another tenant on the GPU, a small device),
        // halve the band and try again: more, smaller bands give the same image (tiling invariance), just more launches.
        for (;;) {
            rc = ctx->radiance.ensure((size_t)(plan.band_pixels * plan.spp * 3));
            if (rc != MI355RT_ERR_OOM || !halve_bands(plan)) break;
            (void)hipGetLastError();
        }
        if (rc) return rc;
        const size_t ctr_words = (size_t)WORK_SHARDS * WORK_SHARD_STRIDE;            // per band
        if ((rc = ctx->counters.ensure((size_t)plan.n_bands * ctr_words))) return rc;
        HIP_TRY(hipMemsetAsync(ctx->counters.p, 0, (size_t)plan.n_bands * ctr_words * sizeof(uint32_t), stream));

        RenderParams p{};
        bind_geometry(ctx, p); bind_shading(ctx, p);
        p.rows = d_rows_processing; p.radiance = ctx->radiance.p; p.stats = ctx->stats.p;
        p.n_mats = ctx->n_mats; p.cam = ctx->cam;
        p.width = st.width; p.height = st.height; p.spp = plan.spp; p.max_depth = st.max_depth;
        p.width_f = plan.width_f; p.height_f = plan.height_f; p.inv_width_rn = plan.inv_width_rn; p.inv_height_rn = plan.inv_height_rn;
        p.seed_lo = plan.seed_lo; p.seed_hi = plan.seed_hi; p.sample0 = plan.sample0;
        p.spp_mul = plan.spp_mul; p.spp_shift = plan.spp_shift; p.width_mul = plan.width_mul; p.width_shift = plan.width_shift;
        p.trav_min = ctx->trav_min; p.inline_steps = ctx->inline_steps;
        p.lds_nodes = (uint32_t)std::min<size_t>(ctx->n_nodes, LDS_NODE_CAP);    // (the wavefront kernel clamps to its own WF_LDS_NODES)
        p.err = ctx->errword.p; p.spin_limit_idle = ctx->spin_limit_idle; p.spin_limit_entry = ctx->spin_limit_entry;
        // the masks lie behind the three row tables; p.rows is the second of them (n_rows * (1 + width) < 2^31 + 2^24 words)
        p.cam_mask_off = (variant == KERNEL_LOCKSTEP_SIMPLE_QC && ctx->cam_mask_host.size() == (size_t)n_rows * st.width) ? 2u * n_rows : 0u;
        ResolveParams r{};
        r.radiance = ctx->radiance.p; r.out_packed = (uint32_t*)d_out_packed; r.out_linear = (float*)d_out_linear;
        r.spp = plan.spp; r.inv_spp = plan.inv_spp;
        r.accum = (float*)d_accum; r.accum_load = plan.accum_load;
        r.out_row = d_out_row; r.width = st.width; r.width_mul = plan.width_mul; r.width_shift = plan.width_shift;
        // The resolve reads no sample of a pixel that no camera ray leaves with a hit: there k_render_ctr_simple_qc stored 1 * miss for every sample (HitStock::append).
        // Only that entry stores a constant -- the twin with the sky lookup stores a texel -- and the row-cost probe resolves nothing.
        const bool resolve_skip = p.cam_mask_off != 0u && p.sky == nullptr && !d_row_counters && ctx->knob_resolve_skip != 0;
        std::memcpy(r.miss, ctx->miss, 12);
        for (uint32_t b = 0; b < plan.n_bands; ++b) {
            const RenderBand band = render_band(plan, b);
            p.band_pixel0 = band.band_pixel0; p.band_samples = band.band_samples; p.shard_samples = band.shard_samples; p.guided_div = band.guided_div;
            p.batch_counter = ctx->counters.p + (size_t)b * ctr_words;
            if (d_row_counters) p.stats = d_row_counters + STATS_WORDS * (size_t)b;   // (a whole counter block per row: diagnostic builds write all of it)
            p.wave_times = nullptr;
            if (ctx->want_wave_times) {
                ctx->wave_times_n = band.grid * (plan.block_threads / 64);
                if ((rc = ctx->wave_times.ensure((size_t)ctx->wave_times_n * WAVE_TIME_WORDS))) return rc;
                HIP_TRY(hipMemsetAsync(ctx->wave_times.p, 0, (size_t)ctx->wave_times_n * WAVE_TIME_WORDS * 8, stream));
                p.wave_times = ctx->wave_times.p;
            }
            grid_blocks = std::max(grid_blocks, band.grid);
            r.band_pixel0 = band.band_pixel0; r.band_pixels = band.band_pixels;
            r.cam_mask = resolve_skip ? p.rows + p.cam_mask_off + band.band_pixel0 : nullptr;   // (the words the render kernel reads for this band)
            hipEvent_t pe0 = nullptr, pe1 = nullptr, pe2 = nullptr;
            if (ctx->timing && !stats) { pe0 = ctx->pool_get(); pe1 = ctx->pool_get(); pe2 = ctx->pool_get(); if (!pe0 || !pe1 || !pe2) return fail(MI355RT_ERR_HIP, "event pool"); }
            if (stats) HIP_TRY(hipEventRecord(ctx->ev[0], stream));
            if (pe0) HIP_TRY(hipEventRecord(pe0, stream));
            if (launch_render_ctr(p, variant, band.grid, stream) != 0) return fail(MI355RT_ERR_HIP, "k_render_ctr launch failed");
            ctx->launched_variants |= 1u << variant;
            if (variant_entry(variant, p.sky != nullptr) == ENTRY_SKY) ctx->launched_sky_entries |= 1u << variant;
            if (stats) HIP_TRY(hipEventRecord(ctx->ev[1], stream));
            if (pe1) HIP_TRY(hipEventRecord(pe1, stream));
            if (!d_row_counters && launch_resolve(r, stream) != 0) return fail(MI355RT_ERR_HIP, "k_resolve launch failed");
            if (pe2) { HIP_TRY(hipEventRecord(pe2, stream)); ++ctx->timed_launches; }
            if (stats) {
                HIP_TRY(hipEventRecord(ctx->ev[2], stream));
                HIP_TRY(hipEventSynchronize(ctx->ev[2]));
                float a = 0, c = 0;
                HIP_TRY(hipEventElapsedTime(&a, ctx->ev[0], ctx->ev[1]));
                HIP_TRY(hipEventElapsedTime(&c, ctx->ev[1], ctx->ev[2]));
                render_ms += a; resolve_ms += c; total_ms += a + c;
            }
        }
    }
    // the context's error word, behind the kernels and in front of `done`: whoever waits on `done` (or finds it complete) sees it
    HIP_TRY(hipMemcpyAsync(ctx->h_err, ctx->errword.p, sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipEventRecord(ctx->done, stream));
    ctx->last_stream = stream; ctx->have_last = true;
    if (stats) {
        unsigned long long h[2] = {0, 0};
        HIP_TRY(hipMemcpyAsync(h, ctx->stats.p, sizeof h, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (int erc = report_device_error(ctx, true)) return erc;    // a wave of THIS render gave up: the image is incomplete
        stats->render_kernel_ms = render_ms; stats->resolve_kernel_ms = resolve_ms; stats->total_ms = total_ms;
        stats->samples = h[0]; stats->rays = h[1];
        stats->bands = plan.n_bands; stats->grid_blocks = grid_blocks; stats->block_threads = plan.block_threads;
    }
    return MI355RT_OK;
}

int mi355rt_context_set_share(mi355rt_context* ctx, uint32_t share_of) {
    return guard([&]() -> int {
    if (!ctx) return fail(MI355RT_ERR_INVALID, "ctx is null");
    if (share_of < 1u || share_of > 16u) return fail(MI355RT_ERR_INVALID, "share_of must be 1 .. 16");
    ctx->grid_div = share_of;
    return MI355RT_OK;
    });
}

int mi355rt_context_render(mi355rt_context* ctx, const mi355rt_options* opt, void* d_out_packed, void* d_out_linear,
                           void* hip_stream, mi355rt_stats* stats) {
    return guard([&]() -> int {
    if (!ctx || !ctx->have_scene) return fail(MI355RT_ERR_INVALID, "context has no scene");
    return render_samples(ctx, opt, 0, ctx->settings.samples_per_pixel, nullptr, d_out_packed, d_out_linear, hip_stream, stats);
    });
}

int mi355rt_context_render_progressive(mi355rt_context* ctx, const mi355rt_options* opt, uint32_t sample_begin, uint32_t sample_end,
                                       void* d_accum, void* d_out_packed, void* d_out_linear, void* hip_stream, mi355rt_stats* stats) {
    return guard([&]() -> int {
    if (!d_accum) return fail(MI355RT_ERR_INVALID, "d_accum is null");
    if (sample_end <= sample_begin) return fail(MI355RT_ERR_INVALID, "sample_end must be greater than sample_begin");
    return render_samples(ctx, opt, sample_begin, sample_end, d_accum, d_out_packed, d_out_linear, hip_stream, stats);
    });
}

int mi355rt_context_set_timing(mi355rt_context* ctx, int enable) {
    return guard([&]() -> int {
    if (!ctx) return fail(MI355RT_ERR_INVALID, "ctx is null");
    ctx->timing = enable != 0; ctx->pool_used = 0; ctx->timed_launches = 0;
    return MI355RT_OK;
    });
}

int mi355rt_context_read_timing(mi355rt_context* ctx, double* render_kernel_ms, double* resolve_kernel_ms, uint32_t* launches) {
    return guard([&]() -> int {
    if (!ctx) return fail(MI355RT_ERR_INVALID, "ctx is null");
    HIP_TRY(hipSetDevice(ctx->device));
    double a = 0, c = 0;
    for (size_t i = 0; i + 2 < ctx->pool_used; i += 3) {
        HIP_TRY(hipEventSynchronize(ctx->pool[i + 2]));
        float x = 0, y = 0;
        HIP_TRY(hipEventElapsedTime(&x, ctx->pool[i], ctx->pool[i + 1]));
        HIP_TRY(hipEventElapsedTime(&y, ctx->pool[i + 1], ctx->pool[i + 2]));
        a += x; c += y;
    }
    if (render_kernel_ms) *render_kernel_ms = a;
    if (resolve_kernel_ms) *resolve_kernel_ms = c;
    if (launches) *launches = ctx->timed_launches;
    ctx->pool_used = 0; ctx->timed_launches = 0;
    return mi355rt_context_check(ctx);                               // the timed renders must also have been COMPLETE renders
    });
}

int mi355rt_context_check(mi355rt_context* ctx) {
    return guard([&]() -> int {
    if (!ctx) return fail(MI355RT_ERR_INVALID, "ctx is null");
    HIP_TRY(hipSetDevice(ctx->device));
    if (ctx->have_last) HIP_TRY(hipEventSynchronize(ctx->done));     // every render enqueued so far has finished and left its error word
    return report_device_error(ctx);
    });
}

}  // extern "C"
