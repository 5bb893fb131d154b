// rt_api.cpp -- implementation of the device half of include/mi355rt.h (libmi355rt.so).
//
// Replaces `render_scene(&scene, &camera, &render_settings) -> Vec<u32>` (src/renderer.rs:67,
// called from src/main.rs:57).  There is NO CPU fallback in this library: without a HIP device every
// render entry point returns MI355RT_ERR_NO_DEVICE.  What happens to a scene before a device is involved -- validation, the BVH re-lay, the
// primitive records, the choice of the kernel variant -- and what a render call launches -- its refusals, the variant, the bands and their grids -- is
// rt_prepare.cpp, which has no HIP in it; this file uploads and launches: the context, its renders, its queries and the debug hooks.  The
// calls with host buffers (mi355rt_render and its kin) are clients of this file's public functions and live in rt_oneshot.cpp.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../../include/mi355rt.h"
#include "rt_device.h"
#include "rt_host.h"
#include "rt_query.h"
#include "rt_denoise.h"
#include "rt_occlusion.h"
#include "rt_radiance.h"
#include "rt_view.h"
#include "rt_probe.h"

using namespace mi355rt;

struct mi355rt_context;
static int report_device_error(mi355rt_context* ctx, bool this_render = false);

struct mi355rt_context {
    int device = 0;
    int cu_count = 0;
    int blocks_per_cu[KERNEL_ENTRIES][KERNEL_VARIANTS] = {}, vgprs[KERNEL_ENTRIES][KERNEL_VARIANTS] = {}, sgprs = 0;   // per entry point (rt_device.h ENTRY_*): with / without a sky texture
    uint32_t entry() const { return variant_entry(variant, sky_w != 0); }   // the entry point the resident scene is launched on
    uint32_t variant = KERNEL_LOCKSTEP;  // chosen per scene in set_scene
    bool has_mesh = false;
    bool occlusion_may_exit = false;     // every number the hit tests read from the scene lies inside OCCLUSION_BOUND: the occlusion kernels may leave the list early (rt_prepare.h)
    uint32_t grid_div = 1;               // this context launches 1 / grid_div of the grid that fills the device: the caller keeps grid_div frames in flight, each on its own
                                         // context and stream, so that their persistent kernels are co-resident (see render_samples; mi355rt_context_set_share)
    uint32_t guided_mult = 16;           // run length = (left in shard) / (guided_mult * waves per shard); 16 measured best at 1/8-image launches
    uint32_t inline_steps = 0;           // 1 when several meshes share the list (many rays miss a mesh's root box: teapot +5..12 %), 0 for a single mesh (semesterbild -10 % otherwise)
    uint32_t trav_min = 24;              // measured optimum 24-32 on semesterbild / teapot (tools/ab_kernel.py)
    bool have_scene = false;
    mi355rt_settings settings{};
    DevCamera cam{};
    float miss[3] = {0.5f, 0.5f, 0.5f};
    uint32_t n_prims = 0, n_mats = 0; size_t n_nodes = 0;
    DevBuf<DevPrim> prims; DevBuf<DevMat> mats; DevBuf<DevNode> nodes; DevBuf<DevTri> tris;
    DevBuf<uint32_t> rows; DevBuf<float> radiance; DevBuf<uint32_t> counters; DevBuf<unsigned long long> stats;
    DevBuf<float> fold_stack;
    DevBuf<float> sky; uint32_t sky_w = 0, sky_h = 0;      // equirect HDR skybox (renderer.rs:40-54); sky_w == 0: none
    DevBuf<DevTexture> textures; DevBuf<uint32_t> texels;  // MI355RT_MAT_TEXTURE images: table + all texels in one buffer
    DevBuf<unsigned long long> wave_times; uint32_t wave_times_n = 0;   // diagnostics (MI355RT_WAVE_TIMES=1)
    std::vector<uint32_t> rows_host;     // the selected rows (absolute y, ascending = the order of the output buffer)
    std::vector<uint32_t> tables_host;   // source of the async upload of the three row tables (rt_prepare.h row_tables()); must outlive the copy
    // Camera masks (rt_prepare.h build_camera_masks; k_render_ctr_simple_qc's camera pass).  cam_mask_abs: the table of the scene, the camera and the
    // settings of set_scene, one word per pixel of the image (empty: none -- another kernel, more than 32 primitives, or the knob); cam_mask_host: its rows
    // in the processing order of rows_host, rebuilt with the row tables and uploaded behind them into `rows` (same lifetime as tables_host); empty: the
    // kernel gets no table.
    std::vector<uint32_t> cam_mask_abs, cam_mask_host; uint32_t cam_mask_w = 0, cam_mask_h = 0;
    int knob_cam_cull = -1;              // diagnostic knob "cam_cull": -1 / 1 on, 0 off (no table: the camera pass tests every primitive)
    int knob_resolve_skip = 1;           // diagnostic knob "resolve_skip": 1 (the product) = k_resolve gets the band's camera masks and reads no sample of a pixel whose word is 0; 0 = it reads every sample
    bool rows_valid = false;             // ctx->rows already holds the tables of rows_host (same selection and grouping as the last call)
    // Processing order (an experiment of round 4, opt-in).  The persistent kernels hand out a band's samples front to back, and a
    // launch ends with the paths of the rows handed out LAST.  The idea: process the rows in order of DECREASING expected cost -- cheap rows
    // (sky) last -- dealt over the work shards so that every shard ends with cheap rows, and a launch does not end on its longest paths.  The image cannot change: draws are keyed by absolute row / x /
    // sample, the resolve kernel writes each pixel where it belongs (ResolveParams.out_row).  `row_cost` = rays per path of each image
    // row, measured by set_scene with a small probe render of the same view; empty = natural order.
    std::vector<float> row_cost;
    int knob_denoise_staged = 1;         // diagnostic knob "denoise_staged": 1 (the product) = the denoiser's levels with step 1 and 2 stage their tile in LDS; 0 = they gather like the later levels (the A/B of DESIGN.md 4.7)
    int knob_ao_form = 0;                // diagnostic knob "ao_form": AO_FORM_* of rt_occlusion.h; 0 (the product) = a pixel's samples across the lanes of a wave, 1 = a pixel per lane (the A/B of DESIGN.md 4.8)
    int knob_radiance_items = 0;         // diagnostic knob "radiance_items": K of rt_radiance.h, 1 .. 64 items per lane of k_radiance_paths; 0 (the product) = RADIANCE_ITEMS_DEFAULT (the A/B of DESIGN.md 4.12)
    int knob_row_order = -1;             // diagnostic knob "row_order": 1 on; -1 / 0 off (NOT shipped as a default: no measured gain, see set_scene)
    uint32_t order_groups = 0;           // how many groups the cached tables were dealt over (work shards x bands)
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    // The workspaces (rows, radiance, counters, stats) belong to one render at a time.  `done` is recorded behind the last
    // operation of every render; a render enqueued on ANOTHER stream waits on it first, so two streams can never touch
    // the workspaces concurrently (same stream: in-order execution already guarantees it).
    hipEvent_t done = nullptr; hipStream_t last_stream = nullptr; bool have_last = false;
    bool want_wave_times = false;        // diagnostic knob "wave_times" (stamps builds)
    // Sticky error word.  A wave of the wavefront kernel that gives up a bounded wait (RenderParams.spin_limit_*) adds 1 to `errword`
    // and leaves paths unfinished.  The word is never reset by a render; its value is copied into the pinned host word `h_err`
    // behind the kernels of EVERY render (8 bytes, in stream order, before `done`), and whichever entry point looks next --
    // the same call when it synchronises for stats, mi355rt_context_check, mi355rt_context_read_timing, or the next render on
    // this context -- compares it with what has been reported and returns MI355RT_ERR_HIP once per failed render.
    DevBuf<unsigned long long> errword; unsigned long long* h_err = nullptr; unsigned long long err_reported = 0;
    uint32_t spin_limit_idle = SPIN_LIMIT_IDLE, spin_limit_entry = SPIN_LIMIT_ENTRY;   // diagnostic knobs "spin_idle" / "spin_entry"
    uint32_t launched_variants = 0;      // bit v: kernel variant v was launched since the last failure report (names the kernel in the message)
    uint32_t launched_sky_entries = 0;   // bit v: ... on its entry point for scenes with a sky texture
    int forced_variant = -1;             // diagnostic knob "kernel": applied by set_scene when the scene allows it
    int knob_inline_steps = -1;          // diagnostic knob "inline_steps" (reference build's state machine)
    // timing pool (mi355rt_context_set_timing): event triples recorded around every kernel pair without
    // synchronising; mi355rt_context_read_timing sums them after the caller's own stream sync.
    bool timing = false;
    std::vector<hipEvent_t> pool; size_t pool_used = 0;
    uint32_t timed_launches = 0;
    // Row tables of mi355rt_context_first_hits (local output row -> absolute y), one per row selection seen since set_scene.  They are the queries' own:
    // a query never touches `rows` above, which belongs to the render in flight.  A table is written once (its host copy outlives the upload) and
    // never changed, so queries on any streams may read it; `ready` orders the upload before a query on another stream.
    struct QueryRows { std::vector<uint32_t> rows; uint32_t* d = nullptr; hipEvent_t ready = nullptr; hipStream_t stream = nullptr; };
    std::vector<QueryRows> query_rows;
    void query_rows_release() {                                      // (hipFree waits for the device: no query still reads a table)
        for (auto& t : query_rows) { if (t.d) (void)hipFree(t.d); if (t.ready) (void)hipEventDestroy(t.ready); }
        query_rows.clear();
    }
    hipEvent_t pool_get() {
        if (pool_used == pool.size()) { hipEvent_t e = nullptr; if (hipEventCreate(&e) != hipSuccess) return nullptr; pool.push_back(e); }
        return pool[pool_used++];
    }
};

// Compares the host copy of the context's error word with what has already been reported.  The copy is refreshed in stream order
// behind every render, so after a wait on `done` it covers every render enqueued so far; without a wait it covers those that
// have finished.
// `this_render`: the caller has just waited for the render it enqueued itself (the stats path), so the failure is that render's; otherwise it
// belongs to an earlier, asynchronous render on this context.  The word names the kernel(s) and the wait(s) that gave up (rt_device.h, err_tag).
static int report_device_error(mi355rt_context* ctx, bool this_render) {
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

// 1 bit per counter-mode variant this library holds (rt_kernels.hip): what choose_variant (rt_prepare.h) may be made to force.
uint32_t built_variants() {
    uint32_t mask = 0u;
    for (uint32_t v = 0; v < KERNEL_VARIANTS; ++v) if (render_ctr_variant_built(v)) mask |= 1u << v;
    return mask;
}

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
    {   std::lock_guard<std::mutex> g(g_knob_mutex);                    // process-wide diagnostic defaults (mi355rt_debug_set_knob(NULL, ...))
        for (const auto& kv : g_default_knobs) (void)apply_knob(ctx, kv.first, kv.second); }
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
        rp.prims = ctx->prims.p; rp.mats = ctx->mats.p; rp.nodes = ctx->nodes.p; rp.tris = ctx->tris.p; rp.rows = d_rows_natural;
        rp.sky = ctx->sky_w ? ctx->sky.p : nullptr; rp.sky_w = ctx->sky_w; rp.sky_h = ctx->sky_h; rp.textures = ctx->textures.p;
        rp.out_packed = (uint32_t*)d_out_packed; rp.out_linear = (float*)d_out_linear; rp.fold_stack = ctx->fold_stack.p; rp.stats = ctx->stats.p;
        rp.n_prims = ctx->n_prims; rp.n_mats = ctx->n_mats; rp.n_rows = n_rows;
        std::memcpy(rp.miss, ctx->miss, 12); rp.cam = ctx->cam;
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
        p.prims = ctx->prims.p; p.mats = ctx->mats.p; p.nodes = ctx->nodes.p; p.tris = ctx->tris.p; p.rows = d_rows_processing;
        p.sky = ctx->sky_w ? ctx->sky.p : nullptr; p.sky_w = ctx->sky_w; p.sky_h = ctx->sky_h; p.textures = ctx->textures.p;
        p.radiance = ctx->radiance.p; p.stats = ctx->stats.p;
        p.n_prims = ctx->n_prims; p.n_mats = ctx->n_mats;
        std::memcpy(p.miss, ctx->miss, 12); p.cam = ctx->cam;
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

// ---- ray queries (rt_query.hip): what does a ray hit in the resident scene? ------------------------------------------------------
// They read the scene arrays only -- no workspace, no counters, no error word of their own -- so they neither wait on `done` nor
// record it, and may run beside a render of the same context on another stream.  mi355rt_context_set_share is not consulted: the
// kernels are plain grids that end with their rays.
static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0u; }
static void query_scene(const mi355rt_context* ctx, QueryParams& q) {
    q.prims = ctx->prims.p; q.nodes = ctx->nodes.p; q.tris = ctx->tris.p; q.n_prims = ctx->n_prims;
}

int mi355rt_context_trace_rays(mi355rt_context* ctx, const void* d_rays, uint32_t n_rays, void* d_hits, void* hip_stream) {
    return guard([&]() -> int {
    static_assert(sizeof(mi355rt_ray) == 32 && sizeof(mi355rt_hit) == 48, "the query kernels read a ray as two 16-byte halves and write a record as three 16-byte words");
    if (!ctx || !ctx->have_scene) return fail(MI355RT_ERR_INVALID, "context has no scene");
    if (n_rays == 0) return MI355RT_OK;
    if (!d_rays || !d_hits) return fail(MI355RT_ERR_INVALID, "trace_rays: d_rays / d_hits is null");
    if (!aligned16(d_rays) || !aligned16(d_hits)) return fail(MI355RT_ERR_INVALID, "trace_rays: d_rays / d_hits must be 16-byte aligned");
    HIP_TRY(hipSetDevice(ctx->device));
    if (int erc = report_device_error(ctx)) return erc;              // an earlier asynchronous render on this context failed
    QueryParams q{};
    query_scene(ctx, q);
    q.rays = d_rays; q.hits = d_hits; q.n = n_rays;
    if (launch_query(q, ctx->has_mesh, hip_stream) != 0) return fail(MI355RT_ERR_HIP, "k_query_rays launch failed");
    return MI355RT_OK;
    });
}

// The device table (local output row -> absolute y) of a row selection, one per selection seen since set_scene; `sel.rows` is taken when a new one is made.
// On return the table's upload is ordered before what is enqueued on `stream` next.
static int query_row_table(mi355rt_context* ctx, RowSel& sel, hipStream_t stream, mi355rt_context::QueryRows*& table) {
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
    HIP_TRY(hipSetDevice(ctx->device));
    if (int erc = report_device_error(ctx)) return erc;              // an earlier asynchronous render on this context failed
    mi355rt_context::QueryRows* table = nullptr;
    if (int rc = query_row_table(ctx, sel, (hipStream_t)hip_stream, table)) return rc;
    QueryParams q{};
    query_scene(ctx, q);
    q.rays = nullptr; q.hits = d_hits; q.rows = table->d; q.n = (uint32_t)(table->rows.size() * (size_t)st.width);   // (< 2^31: check_settings)
    q.cam = ctx->cam; q.width = st.width; q.width_f = (float)st.width; q.height_f = (float)st.height;
    magic_div(st.width, q.width_mul, q.width_shift);
    if (launch_query(q, ctx->has_mesh, hip_stream) != 0) return fail(MI355RT_ERR_HIP, "k_query_pixels launch failed");
    return MI355RT_OK;
    });
}

// ---- occlusion queries (rt_occlusion.hip): does anything lie in front of t_max? -----------------------------------------------------------
// The protocol of the ray queries: they read the scene arrays only, neither wait on `done` nor record it, and do not consult set_share.
// Every refusal is rt_prepare.cpp's, before any HIP call.
int mi355rt_context_occluded(mi355rt_context* ctx, const void* d_segments, uint32_t n, void* d_out, void* hip_stream) {
    return guard([&]() -> int {
    static_assert(sizeof(mi355rt_segment) == 32, "the kernel reads a segment as two 16-byte halves");
    if (int rc = check_occluded_args(ctx != nullptr, ctx && ctx->have_scene, d_segments, n, d_out)) return rc;
    if (n == 0) return MI355RT_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    if (int erc = report_device_error(ctx)) return erc;              // an earlier asynchronous render on this context failed
    OcclusionParams q{};
    q.prims = ctx->prims.p; q.nodes = ctx->nodes.p; q.tris = ctx->tris.p; q.n_prims = ctx->n_prims;
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
    HIP_TRY(hipSetDevice(ctx->device));
    if (int erc = report_device_error(ctx)) return erc;              // an earlier asynchronous render on this context failed
    mi355rt_context::QueryRows* table = nullptr;
    if (int rc = query_row_table(ctx, sel, (hipStream_t)hip_stream, table)) return rc;
    AoLaunch a{};
    a.prims = ctx->prims.p; a.nodes = ctx->nodes.p; a.tris = ctx->tris.p; a.n_prims = ctx->n_prims;
    a.hits = d_hits; a.out = (float*)d_out; a.rows = table->d; a.n = (uint32_t)(table->rows.size() * (size_t)st.width);   // (< 2^31: check_settings)
    a.width = st.width; magic_div(st.width, a.width_mul, a.width_shift);
    a.samples = plan.samples; a.log2_samples = plan.log2_samples; a.seed = plan.seed; a.radius = plan.radius;
    a.may_exit = ctx->occlusion_may_exit ? 1u : 0u; a.form = (uint32_t)ctx->knob_ao_form;
    if (launch_ambient_occlusion(a, ctx->has_mesh, hip_stream) != 0) return fail(MI355RT_ERR_HIP, "k_ao launch failed");
    return MI355RT_OK;
    });
}

// ---- radiance queries (rt_radiance.hip): whole paths along the caller's rays ----------------------------------------------------------------
// What mi355rt_context_trace_radiance does with its context: the entry point itself stands with its kernels in rt_radiance.hip, behind the barrier, as
// rt_noise.hip's do; this half needs the context struct.  The protocol of the ray queries: the call reads the scene arrays only, neither waits on
// `done` nor records it, and does not consult set_share.  Every refusal, the item count and the grids are rt_prepare.cpp's (plan_radiance), before any HIP call.
}  // extern "C"
int mi355rt::context_trace_radiance(mi355rt_context* ctx, const mi355rt_radiance_params* params, const void* d_rays, uint32_t n_rays, void* d_accum,
                                    void* d_out_linear, void* d_scratch, void* hip_stream) {
    static_assert(sizeof(mi355rt_path_ray) == 32 && sizeof(mi355rt_radiance_params) == 32, "the kernel reads a ray as two 16-byte halves");
    static_assert(RADIANCE_PLAN_BLOCK == RADIANCE_BLOCK_THREADS && RADIANCE_PLAN_ITEMS_MAX == RADIANCE_ITEMS_MAX, "plan_radiance cuts the grids the kernels are launched on");
    RadiancePlan plan{};
    if (int rc = plan_radiance(ctx != nullptr, ctx && ctx->have_scene, params, d_rays, n_rays, d_accum, d_out_linear, d_scratch,
                               ctx ? (uint32_t)ctx->knob_radiance_items : 0u, RADIANCE_ITEMS_DEFAULT, plan)) return rc;
    if (n_rays == 0) return MI355RT_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    if (int erc = report_device_error(ctx)) return erc;              // an earlier asynchronous render on this context failed
    RadianceParams p{};
    p.prims = ctx->prims.p; p.mats = ctx->mats.p; p.nodes = ctx->nodes.p; p.tris = ctx->tris.p; p.n_prims = ctx->n_prims;
    p.sky = ctx->sky_w ? ctx->sky.p : nullptr; p.sky_w = ctx->sky_w; p.sky_h = ctx->sky_h; p.textures = ctx->textures.p;
    std::memcpy(p.miss, ctx->miss, sizeof p.miss);
    p.rays = d_rays; p.scratch = (float*)d_scratch; p.n_items = plan.n_items; p.samples = plan.samples; p.sample_begin = params->sample_begin;
    p.max_depth = params->max_depth; p.items_per_lane = plan.items_per_lane; p.seed_lo = plan.seed_lo; p.seed_hi = plan.seed_hi;
    RadianceSum s{};
    s.scratch = (const float*)d_scratch; s.accum = (float*)d_accum; s.out_linear = (float*)d_out_linear; s.n_rays = n_rays; s.samples = plan.samples;
    s.accum_load = plan.accum_load; s.inv_total = plan.inv_total;
    if (launch_radiance(p, s, ctx->has_mesh, plan.grid_paths, plan.grid_sum, hip_stream) != 0) return fail(MI355RT_ERR_HIP, "k_radiance launch failed");
    return MI355RT_OK;
}

// ---- camera views (rt_view.hip): the rays of a pinhole or a thin lens made on the device, in front of the radiance queries' loop ----
// The context halves of mi355rt_context_view_rays / mi355rt_context_render_view, whose entry points stand with their kernels in rt_view.hip, behind
// the barrier.  The protocol of the ray queries; every refusal and the grids are rt_prepare.cpp's (plan_view_rays, plan_view), before any HIP call.
static void view_params(const mi355rt_view* view, const ViewPlan& plan, ViewParams& v) {
    static_assert(sizeof(DevCamera) == sizeof(mi355rt_camera) && sizeof(mi355rt_view) == 96 && sizeof(mi355rt_view) % 16 == 0, "a view carries set_scene's camera");
    std::memcpy(&v.cam, &view->camera, sizeof v.cam);
    v.width_f = (float)view->width; v.height_f = (float)view->height; v.width = view->width; v.centre = plan.centre;
    v.lens_radius = view->lens_radius; v.focus_distance = view->focus_distance;
}
int mi355rt::context_view_rays(mi355rt_context* ctx, const mi355rt_view* view, uint32_t sample, uint64_t seed, void* d_rays, void* hip_stream) {
    ViewPlan plan{};
    if (int rc = plan_view_rays(ctx != nullptr, ctx && ctx->have_scene, view, d_rays, plan)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    if (int erc = report_device_error(ctx)) return erc;              // an earlier asynchronous render on this context failed
    ViewParams v{}; view_params(view, plan, v);
    ViewRays r{};
    r.rays = d_rays; r.n_pixels = plan.n_pixels; r.sample = sample; r.seed_lo = (uint32_t)seed; r.seed_hi = (uint32_t)(seed >> 32);
    if (launch_view_rays(v, r, view->model, hip_stream) != 0) return fail(MI355RT_ERR_HIP, "k_view_rays launch failed");
    return MI355RT_OK;
}
int mi355rt::context_render_view(mi355rt_context* ctx, const mi355rt_view* view, const mi355rt_radiance_params* params, void* d_accum, void* d_out_linear,
                                 void* d_out_packed, void* d_scratch, void* hip_stream) {
    ViewPlan plan{};
    if (int rc = plan_view(ctx != nullptr, ctx && ctx->have_scene, view, params, d_accum, d_out_linear, d_out_packed, d_scratch,
                           ctx ? (uint32_t)ctx->knob_radiance_items : 0u, RADIANCE_ITEMS_DEFAULT, plan)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    if (int erc = report_device_error(ctx)) return erc;              // an earlier asynchronous render on this context failed
    RadianceParams p{};
    p.prims = ctx->prims.p; p.mats = ctx->mats.p; p.nodes = ctx->nodes.p; p.tris = ctx->tris.p; p.n_prims = ctx->n_prims;
    p.sky = ctx->sky_w ? ctx->sky.p : nullptr; p.sky_w = ctx->sky_w; p.sky_h = ctx->sky_h; p.textures = ctx->textures.p;
    std::memcpy(p.miss, ctx->miss, sizeof p.miss);
    p.rays = nullptr; p.scratch = (float*)d_scratch; p.n_items = plan.r.n_items; p.samples = plan.r.samples; p.sample_begin = params->sample_begin;
    p.max_depth = params->max_depth; p.items_per_lane = plan.r.items_per_lane; p.seed_lo = plan.r.seed_lo; p.seed_hi = plan.r.seed_hi;
    ViewParams v{}; view_params(view, plan, v);
    ViewSum s{};
    s.sum.scratch = (const float*)d_scratch; s.sum.accum = (float*)d_accum; s.sum.out_linear = (float*)d_out_linear; s.sum.n_rays = plan.n_pixels;
    s.sum.samples = plan.r.samples; s.sum.accum_load = plan.r.accum_load; s.sum.inv_total = plan.r.inv_total; s.out_packed = (uint32_t*)d_out_packed;
    if (launch_view_paths(p, v, s, view->model, ctx->has_mesh, plan.r.grid_paths, plan.r.grid_sum, hip_stream) != 0) return fail(MI355RT_ERR_HIP, "k_view launch failed");
    return MI355RT_OK;
}

// ---- surface probes (rt_probe.hip): cosine-hemisphere rays made on the device from the caller's points and normals, in front of the same loop ----
// The context halves of mi355rt_context_probe_rays / mi355rt_context_probe_radiance, whose entry points stand with their kernels in rt_probe.hip,
// behind the barrier.  The protocol of the ray queries; every refusal and the grids are rt_prepare.cpp's (plan_probe_rays, plan_probe), before any HIP call.
int mi355rt::context_probe_rays(mi355rt_context* ctx, const void* d_probes, uint32_t n, uint32_t sample, uint64_t seed, void* d_rays, void* hip_stream) {
    static_assert(sizeof(mi355rt_probe) == 32 && sizeof(mi355rt_probe) == sizeof(mi355rt_path_ray), "the kernel reads a probe as two 16-byte halves");
    if (int rc = plan_probe_rays(ctx != nullptr, ctx && ctx->have_scene, d_probes, n, d_rays)) return rc;
    if (n == 0) return MI355RT_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    if (int erc = report_device_error(ctx)) return erc;              // an earlier asynchronous render on this context failed
    ProbeParams b{}; b.probes = d_probes;
    ProbeRaysOut r{};
    r.rays = d_rays; r.n = n; r.sample = sample; r.seed_lo = (uint32_t)seed; r.seed_hi = (uint32_t)(seed >> 32);
    if (launch_probe_rays(b, r, hip_stream) != 0) return fail(MI355RT_ERR_HIP, "k_probe_rays launch failed");
    return MI355RT_OK;
}
int mi355rt::context_probe_radiance(mi355rt_context* ctx, const mi355rt_radiance_params* params, const void* d_probes, uint32_t n, void* d_accum,
                                    void* d_out_linear, void* d_scratch, void* hip_stream) {
    RadiancePlan plan{};
    if (int rc = plan_probe(ctx != nullptr, ctx && ctx->have_scene, params, d_probes, n, d_accum, d_out_linear, d_scratch,
                            ctx ? (uint32_t)ctx->knob_radiance_items : 0u, RADIANCE_ITEMS_DEFAULT, plan)) return rc;
    if (n == 0) return MI355RT_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    if (int erc = report_device_error(ctx)) return erc;              // an earlier asynchronous render on this context failed
    RadianceParams p{};
    p.prims = ctx->prims.p; p.mats = ctx->mats.p; p.nodes = ctx->nodes.p; p.tris = ctx->tris.p; p.n_prims = ctx->n_prims;
    p.sky = ctx->sky_w ? ctx->sky.p : nullptr; p.sky_w = ctx->sky_w; p.sky_h = ctx->sky_h; p.textures = ctx->textures.p;
    std::memcpy(p.miss, ctx->miss, sizeof p.miss);
    p.rays = nullptr; p.scratch = (float*)d_scratch; p.n_items = plan.n_items; p.samples = plan.samples; p.sample_begin = params->sample_begin;
    p.max_depth = params->max_depth; p.items_per_lane = plan.items_per_lane; p.seed_lo = plan.seed_lo; p.seed_hi = plan.seed_hi;
    ProbeParams b{}; b.probes = d_probes;
    RadianceSum s{};
    s.scratch = (const float*)d_scratch; s.accum = (float*)d_accum; s.out_linear = (float*)d_out_linear; s.n_rays = n; s.samples = plan.samples;
    s.accum_load = plan.accum_load; s.inv_total = plan.inv_total;
    if (launch_probe_paths(p, b, s, ctx->has_mesh, plan.grid_paths, plan.grid_sum, hip_stream) != 0) return fail(MI355RT_ERR_HIP, "k_probe launch failed");
    return MI355RT_OK;
}
extern "C" {

// ---- the denoiser (rt_denoise.hip): an a-trous filter over a linear image, guided by first-hit records --------------------------------
// The context names the device and carries the error word of its renders; nothing of it is read or written by the kernels, so the
// call neither waits on `done` nor records it.  What is decided before a device is involved -- the arguments, the per-level constants -- is
// rt_prepare.cpp's.
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
    HIP_TRY(hipSetDevice(ctx->device));
    if (int erc = report_device_error(ctx)) return erc;              // an earlier asynchronous render on this context failed
    d.in = (const float*)d_linear_in; d.hits = d_hits; d.scratch = d_scratch;
    d.out_linear = (float*)d_out_linear; d.out_packed = (uint32_t*)d_out_packed; d.width = width; d.rows = rows; d.staged = ctx->knob_denoise_staged;
    if (launch_denoise(d, hip_stream) != 0) return fail(MI355RT_ERR_HIP, "k_denoise launch failed");
    return MI355RT_OK;
    });
}

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
