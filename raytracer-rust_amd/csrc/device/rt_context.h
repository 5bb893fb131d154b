// rt_context.h -- struct mi355rt_context and what the three sources that see it share: rt_api.cpp (the context's life cycle, set_scene, the renders),
// rt_queries.cpp (the calls that read the resident scene and leave the render's workspaces alone) and rt_debug.cpp (the mi355rt_debug_* hooks and the
// knobs).  Nothing else may include it: rt_multi.cpp and rt_oneshot.cpp are clients of the public functions.  Not part of the public header.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstring>
#include <vector>

#include "../../../include/mi355rt.h"
#include "rt_device.h"
#include "rt_host.h"

using namespace mi355rt;             // (the struct is the public header's, at global scope; each of the three sources says the same)

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

namespace mi355rt {

// Compares the host copy of the context's error word with what has already been reported (rt_api.cpp).
int report_device_error(mi355rt_context* ctx, bool this_render = false);
// The process-wide knob defaults of mi355rt_debug_set_knob(NULL, ...), applied to a context that mi355rt_context_create has just made (rt_debug.cpp).
void apply_default_knobs(mi355rt_context* ctx);

// 1 bit per counter-mode variant this library holds (rt_kernels.hip): what choose_variant (rt_prepare.h) may be made to force.
inline uint32_t built_variants() {
    uint32_t mask = 0u;
    for (uint32_t v = 0; v < KERNEL_VARIANTS; ++v) if (render_ctr_variant_built(v)) mask |= 1u << v;
    return mask;
}

// The resident scene as a launch sees it, filled by field name into whichever parameter struct the kernel reads (RefParams, RenderParams, QueryParams,
// OcclusionParams, AoLaunch, RadianceParams): the geometry words every kernel has, and the shading words of the kernels that follow a path.  The
// structs themselves stay apart -- a shared sub-struct would move the offsets of every kernel's scalar loads.
template <class Params> void bind_geometry(const mi355rt_context* ctx, Params& p) {
    p.prims = ctx->prims.p; p.nodes = ctx->nodes.p; p.tris = ctx->tris.p; p.n_prims = ctx->n_prims;
}
template <class Params> void bind_shading(const mi355rt_context* ctx, Params& p) {
    p.mats = ctx->mats.p; p.sky = ctx->sky_w ? ctx->sky.p : nullptr; p.sky_w = ctx->sky_w; p.sky_h = ctx->sky_h; p.textures = ctx->textures.p;
    std::memcpy(p.miss, ctx->miss, sizeof p.miss);
}

}  // namespace mi355rt
