// rt_prepare.h -- the HIP-free half of libmi355rt.so's host code (rt_prepare.cpp): everything that reads caller-supplied data before a
// device is involved.  The thread-local last error and the exception barrier of every extern "C" entry point, the row-selection rule of
// mi355rt_options, scene preparation -- validation, the BVH re-lay, the DevPrim records and the choice of the kernel variant -- and the plans of the
// calls: what a render, the denoiser and the occlusion queries refuse and launch.
// Includes the public header, rt_device.h and the standard library only, so that it also compiles and runs without ROCm (the CPU tests
// through mi355rt_debug_prepare_scene, the sanitizer driver directly).  Not part of the public header.
#pragma once

#include <cstdint>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../../include/mi355rt.h"
#include "rt_device.h"

namespace mi355rt {

// Sets this thread's mi355rt_last_error() text and returns `code`.
int fail(int code, const std::string& msg);
int fail_noexcept(int code, const char* msg) noexcept;
std::string& last_error();       // this thread's text: what mi355rt_last_error() returns

// The exception barrier of every extern "C" entry point (mi355rt.h: "nothing aborts, nothing throws across the ABI"; the caller may
// be a Rust frame -- src/renderer.rs:67 is called from src/main.rs:57 -- into which a C++ exception must not unwind):
// std::bad_alloc / std::length_error -> MI355RT_ERR_OOM, anything else -> MI355RT_ERR_HIP with what() in mi355rt_last_error().
template <class F> int guard(F&& f) noexcept {
    try { return f(); }
    catch (const std::bad_alloc&) { return fail_noexcept(MI355RT_ERR_OOM, "host allocation failed (std::bad_alloc)"); }
    catch (const std::length_error&) { return fail_noexcept(MI355RT_ERR_OOM, "host allocation failed (std::length_error)"); }
    catch (const std::exception& e) {
        try { return fail(MI355RT_ERR_HIP, std::string("unexpected C++ exception: ") + e.what()); } catch (...) { return fail_noexcept(MI355RT_ERR_HIP, "unexpected C++ exception"); }
    }
    catch (...) { return fail_noexcept(MI355RT_ERR_HIP, "unexpected C++ exception"); }
}

struct RowSel { std::vector<uint32_t> rows; };

// The rows `o` selects (mi355rt.h, mi355rt_options), ascending = the order of the output buffers.
int select_rows(const mi355rt_settings& st, const mi355rt_options* o, RowSel& sel);
int check_settings(const mi355rt_settings* st);

// The denoiser (mi355rt.h, mi355rt_context_denoise): what the host decides before a launch.
constexpr uint32_t DENOISE_MAX_LEVELS = 8, DENOISE_MAX_SQUARINGS = 8;
constexpr uint64_t DENOISE_SCRATCH_PER_PIXEL = 64;
struct DenoisePlan {
    uint32_t levels, normal_squarings;
    float sigma_plane;
    float inv_sigma2[DENOISE_MAX_LEVELS];                            // a_k = 1 / (sigma_k * sigma_k), sigma_k = sigma_color * 2^-k: f32, one rounding per operation
};
// width, rows and the parameters (null: the defaults) -> the plan; MI355RT_ERR_INVALID and a text that names the argument otherwise.
int plan_denoise(uint32_t width, uint32_t rows, const mi355rt_denoise_params* params_or_null, DenoisePlan& plan);
// The pointer rules of mi355rt_context_denoise: input, hits and scratch given, at least one output, hits and scratch 16-byte aligned, the rest 4-byte aligned.
int check_denoise_buffers(const void* linear_in, const void* hits, const void* scratch, const void* out_linear, const void* out_packed);
int denoise_scratch_bytes(uint32_t width, uint32_t rows, uint64_t* out_bytes);

// The occlusion queries (mi355rt.h, mi355rt_context_occluded / mi355rt_context_ambient_occlusion): every refusal, decided before any HIP call.
// What does not depend on the context comes first -- pointers, parameters, the options' version and flags -- then the context and its scene, then what
// needs the scene's settings: the row selection, MI355RT_FLAG_FIXED_AABB (MI355RT_ERR_UNSUPPORTED) and the buffers of a non-empty selection.
int check_occluded_args(bool have_ctx, bool have_scene, const void* segments, uint32_t n, const void* out);
struct AoPlan { uint32_t samples, log2_samples, seed; float radius; };
// st: the settings of set_scene (read only when have_scene).  sel: the selected rows; empty = nothing to do.
int plan_ambient_occlusion(bool have_ctx, bool have_scene, const mi355rt_settings& st, const mi355rt_options* options_or_null,
                           const mi355rt_ao_params* params_or_null, const void* hits, const void* out, RowSel& sel, AoPlan& plan);

// The radiance query (mi355rt.h, mi355rt_context_trace_radiance): every refusal, the scratch size, the item count and the two grids,
// decided before any HIP call.  Refusals in this order (MI355RT_ERR_INVALID and a text that names the argument): the parameters -- null, flags,
// reserved, sample_begin >= sample_end --; with n_rays > 0 the pointers (d_rays / d_accum / d_scratch null or not 16-byte aligned, d_out_linear not
// 4-byte aligned) and n_rays * samples >= 2^32; then the context and its scene.  n_rays == 0 passes with n_items == 0: nothing to launch.
constexpr uint32_t RADIANCE_PLAN_BLOCK = 256, RADIANCE_PLAN_ITEMS_MAX = 64;      // (rt_radiance.h: RADIANCE_BLOCK_THREADS, RADIANCE_ITEMS_MAX; rt_queries.cpp asserts it)
struct RadiancePlan {
    uint64_t scratch_bytes;                                          // what mi355rt_radiance_scratch_bytes(n_rays, samples) reports
    uint32_t n_items, samples, items_per_lane;                       // n_rays * samples; sample_end - sample_begin; K
    uint32_t grid_paths, grid_sum;                                   // workgroups of 256: ceil(n_items / (256 * K)); ceil(n_rays / 16)
    uint32_t seed_lo, seed_hi, accum_load;                           // accum_load: sample_begin > 0
    float inv_total;                                                 // 1.0f / (float)sample_end
};
// 12 bytes per (ray, sample) pair, rounded up to a multiple of 16; MI355RT_ERR_INVALID for a null out_bytes or n_rays * samples >= 2^32.
int radiance_scratch_bytes(uint32_t n_rays, uint32_t samples, uint64_t* out_bytes);
// items_knob: the diagnostic knob "radiance_items" (0 = default_items).
int plan_radiance(bool have_ctx, bool have_scene, const mi355rt_radiance_params* params, const void* rays, uint32_t n_rays, const void* accum,
                  const void* out_linear_or_null, const void* scratch, uint32_t items_knob, uint32_t default_items, RadiancePlan& plan);

// The camera views (mi355rt.h, mi355rt_context_view_rays / mi355rt_context_render_view): every refusal, the scratch size and the grids,
// decided before any HIP call.  Refusals in this order (MI355RT_ERR_INVALID and a text that names the argument): the view -- null, model, width /
// height 0, flags, reserved, a camera field that is not finite, the lens fields --; then for view_rays d_rays (null, 16 bytes) and width * height >= 2^32,
// for render_view everything plan_radiance refuses about the params and the pointers, d_out_packed off 4 bytes and width * height * samples >= 2^32;
// then the context and its scene.
struct ViewPlan {
    RadiancePlan r;                                                  // of width * height "rays"; view_rays: n_items = the pixels, no grids
    uint32_t n_pixels, centre;                                       // width * height; MI355RT_VIEW_CENTRE set
};
int view_scratch_bytes(const mi355rt_view* view, uint32_t samples, uint64_t* out_bytes);
int plan_view_rays(bool have_ctx, bool have_scene, const mi355rt_view* view, const void* rays, ViewPlan& plan);
int plan_view(bool have_ctx, bool have_scene, const mi355rt_view* view, const mi355rt_radiance_params* params, const void* accum, const void* out_linear_or_null,
              const void* out_packed_or_null, const void* scratch, uint32_t items_knob, uint32_t default_items, ViewPlan& plan);

// The surface probes (mi355rt.h, mi355rt_context_probe_rays / mi355rt_context_probe_radiance), decided before any HIP call.
// plan_probe is plan_radiance under the call's own name, with d_probes in the place of d_rays.  plan_probe_rays refuses, with n > 0, a null or
// misaligned (16 bytes) d_probes, then d_rays; then the context and its scene.  n == 0 passes: nothing to launch.
int plan_probe_rays(bool have_ctx, bool have_scene, const void* probes, uint32_t n, const void* rays);
int plan_probe(bool have_ctx, bool have_scene, const mi355rt_radiance_params* params, const void* probes, uint32_t n, const void* accum,
               const void* out_linear_or_null, const void* scratch, uint32_t items_knob, uint32_t default_items, RadiancePlan& plan);

// The render call (mi355rt_context_render / mi355rt_context_render_progressive): every refusal, the variant that is launched, the
// bands the radiance workspace is cycled through and the geometry of each band's launch, decided before any HIP call.
// q = n / d for every n < 2^31 as umulhi(n, mul) >> shift (mul == 0 encodes d == 1).
void magic_div(uint32_t d, uint32_t& mul, uint32_t& shift);
// The three row tables of one selection, n entries each: [0, n) natural = absolute y of local output row j; [n, 2n) processing = absolute y
// of the row processed jp-th; [2n, 3n) out_row = the local output row that processing row jp is.  `cost` (per absolute image row, may be
// empty) orders the processing: rows sorted by decreasing cost (stable: equal costs keep image order) and dealt round-robin over `groups`
// consecutive ranges -- the launch's work shards (x bands) -- so that every range runs from its dearest rows to its cheapest.
void row_tables(const std::vector<uint32_t>& rows, const std::vector<float>& cost, uint32_t groups, std::vector<uint32_t>& out);
struct RenderPlanIn {                                                // what a render reads of its context and its caller
    const mi355rt_settings* settings;                                // of set_scene (checked there)
    const mi355rt_options* options;                                  // may be null
    uint32_t s0, s1;                                                 // samples [s0, s1) of every selected pixel, s0 < s1
    bool have_accum;                                                 // running sums were given (progressive rendering)
    uint32_t variant; bool has_mesh; uint32_t n_prims;               // of the resident scene
    bool have_row_cost;                                              // set_scene measured a cost per image row (the processing order)
    bool row_probe;                                                  // set_scene's row-cost probe: a band = a row, no halving
    const uint32_t* block_slots;                                     // per variant: workgroups the device holds at once (CUs x workgroups per CU)
    uint32_t grid_div, guided_mult;                                  // mi355rt_context_set_share; the knob "guided_mult"
};
struct RenderPlan {                                                  // plain words (device.RenderPlan has the same layout)
    uint64_t seed, total_pixels, band_pixels;                        // total_pixels: of the selection; band_pixels: of every band but the last
    uint32_t rng_mode, fixed_aabb, variant;                          // variant: the one that is launched (the flag form; k_render_ctr_mesh for the two degenerate renders)
    uint32_t order_groups;                                           // groups the processing order is dealt over: WORK_SHARDS x min(64, bands before any halving); 0 = image order
    uint32_t spp, n_bands, block_threads;                            // spp: samples per pixel of THIS launch
    float width_f, height_f, inv_width_rn, inv_height_rn, inv_spp;   // RenderParams / ResolveParams words that are arithmetic on the settings
    uint32_t spp_mul, spp_shift, width_mul, width_shift, accum_load, sample0, seed_lo, seed_hi;
    uint32_t width, resident, guided_mult, row_probe;                // what render_band cuts a band's launch with (resident: workgroups this context may launch)
};
static_assert(sizeof(RenderPlan) == 120, "RenderPlan is read as plain words by mi355rt_debug_plan_render's caller");
struct RenderBand { uint32_t band_pixel0, band_pixels, band_samples, shard_samples, grid, guided_div; };   // RenderParams / ResolveParams words and the grid of band b
// Refusals in this order (MI355RT_ERR_INVALID and today's texts): what select_rows refuses; unknown flag bits; MI355RT_FLAG_FIXED_AABB without
// MI355RT_RNG_CTR; then an EMPTY selection is MI355RT_OK (sel.rows empty, n_bands 0: nothing to launch) whatever follows; with MI355RT_RNG_REF a
// progressive call; with MI355RT_RNG_CTR a workspace below one pixel.  MI355RT_RNG_REF plans one "band" of one lane per row.
int plan_render(const RenderPlanIn& in, RowSel& sel, RenderPlan& plan);
RenderBand render_band(const RenderPlan& plan, uint32_t b);          // b < n_bands; MI355RT_RNG_CTR
// The workspace of a band did not fit: bands of half the pixels (the same image: tiling invariance).  false = there is no smaller plan (one pixel; the row probe).
bool halve_bands(RenderPlan& plan);

// A validated scene in the form the device holds it (rt_device.h), still in host memory, and what the choice of the kernel reads.
struct PreparedScene {
    // DO NOT REORDER these four, and keep mesh_roots alive with them: they are freed last to first, behind the upload, exactly as build_device_scene's
    // locals were.  Another order of frees changes what the allocator trims and maps again on every set_scene: with prims first, teapot's set_scene
    // took 0.57 .. 0.59 ms instead of 0.41 in two processes of three; with mesh_roots freed early, up to 0.43 (profiles/bench_scene_prepare_vs_parent.txt).
    std::vector<DevNode> nodes; std::vector<DevTri> tris;
    std::vector<uint32_t> mesh_roots;                                // per mesh: its root in `nodes` (DevPrim::node_begin of the primitives that use it)
    std::vector<DevPrim> prims;
    uint64_t n_texels = 0;                                           // of all textures together
    uint32_t scene_mats = 0u;                                        // which material kinds a ray can meet (bit k = MI355RT_MAT_k): those the primitives refer to
    uint32_t scene_prim_kinds = 0u;                                  // ... and which primitive kinds the list holds (bit k = MI355RT_PRIM_k)
    uint32_t n_mesh_prims = 0;
    bool all_meshes_identity = true, all_meshes_shallow = true;
    // Every quad's plane constant is at most WALK_QUAD_D_MAX in magnitude, and every cube's 3 x 3 part of world_to_object and its zd at most
    // WALK_CUBE_M_MAX where it is finite (a plane constant that is NaN or infinite is outside): what k_render_ctr_simple_qc's list walk takes for granted (rt_intersect.h, hit_quad / hit_cube
    // with BOUNDED).  A list that is not goes to k_render_ctr_simple, whose range tests are per primitive.
    bool walk_bounded = true;
};
constexpr float WALK_QUAD_D_MAX = 0x1p99f, WALK_CUBE_M_MAX = 0x1p100f;

// Validates `sc` and builds `out` from it; MI355RT_ERR_INVALID (and the text) for anything a kernel could not be launched on.
int prepare_scene(const mi355rt_scene* sc, PreparedScene& out);
// Every number the hit tests read from the scene -- the primitive records' test words, the triangles' vertices and edges -- is inside
// +-OCCLUSION_BOUND (rt_occlusion.h; NaN is outside): the condition under which the occlusion kernels may leave the list early.
bool scene_within_occlusion_bound(const PreparedScene& s);
// The counter-mode kernel (KERNEL_* of rt_device.h) that serves the scene.  forced_variant: the diagnostic knob "kernel", -1 = none;
// built_mask: bit v = this library holds variant v (rt_kernels.hip, render_ctr_variant_built).
uint32_t choose_variant(const PreparedScene& s, int forced_variant, uint32_t built_mask);
// RenderParams.inline_steps for the scene.  knob: the diagnostic knob "inline_steps", -1 = none.
uint32_t choose_inline_steps(const PreparedScene& s, int knob);

// Camera masks (k_render_ctr_simple_qc's camera pass): one word per pixel in absolute order y * width + x, bit i set = a camera ray of
// that pixel may hit primitive i.  A clear bit is a proof: the screen footprint of the region in which the kernel's test of that primitive can accept
// a hit, inflated and dilated by far more than any rounding, does not reach the pixel's jitter square.  Whatever is in doubt -- a primitive that reaches the camera plane,
// a record that is not finite, a degenerate matrix, a kind other than quad or cube -- keeps its bit in every pixel.  `out` is resized and filled in place
// (a context calls this on every set_scene: its allocation is kept).  Lists of more than 32 primitives get no table: `out` comes back empty.
void build_camera_masks(const PreparedScene& s, const DevCamera& cam, uint32_t width, uint32_t height, std::vector<uint32_t>& out);
// The table the kernel reads: the rows `rows_processing` (absolute y, in the order they are processed) of the absolute table, back to back.
void gather_camera_masks(const std::vector<uint32_t>& absolute, uint32_t width, const uint32_t* rows_processing, size_t n_rows, std::vector<uint32_t>& out);

}  // namespace mi355rt
