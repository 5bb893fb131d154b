// rt_oneshot.cpp -- the calls of include/mi355rt.h that take host buffers and give host buffers back, part of libmi355rt.so:
// mi355rt_render, mi355rt_render_multi, mi355rt_render_progressive, mi355rt_render_progressive_multi, mi355rt_trace_rays, mi355rt_occluded,
// mi355rt_trace_radiance and mi355rt_denoise.  Each is a client of the resident API and of nothing else (neither context struct is visible here): the checks that
// need no device, a context (or a multi context) of its own, device buffers, the resident call, the copy back.  What they share stands
// once: Call owns the context and the buffers of one call and gives them up on every way out; upload / copy_back name the buffer that
// failed; render_chunks is what the two progressive calls do once they hold their context, query what the queries do; run_parts
// (rt_host.h) deals mi355rt_render_multi's devices over threads.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../../include/mi355rt.h"
#include "rt_host.h"

using namespace mi355rt;

namespace {

const char* const NO_DEVICE = "no HIP device visible (this library has no CPU path)";

// What one call holds on the device: its context (or multi context) and its allocations.  The destructor frees the allocations, then destroys
// the context with the calling thread's last-error text kept -- the destroy may overwrite the message of the failure being reported -- so
// nothing stays allocated whether the call is left by a return code or by an exception on its way to the barrier.
struct Call {
    mi355rt_context* ctx = nullptr;
    mi355rt_multi_context* multi = nullptr;
    void* held[5] = {}; size_t n_held = 0;
    Call() = default; Call(const Call&) = delete;
    ~Call() {
        for (size_t i = 0; i < n_held; ++i) (void)hipFree(held[i]);
        if (multi) mi355rt_multi_context_destroy(multi);              // (keeps the message itself)
        std::string keep; keep.swap(last_error());                    // (swap never throws)
        mi355rt_context_destroy(ctx);
        last_error().swap(keep);
    }
    // n elements on the current device, freed with the call.
    template <class T> int alloc(T*& p, size_t n, const char* name) {
        void* v = nullptr;
        if (n_held == sizeof held / sizeof held[0] || hipMalloc(&v, n * sizeof(T)) != hipSuccess) return fail(MI355RT_ERR_OOM, std::string("hipMalloc(") + name + ")");
        held[n_held++] = v; p = static_cast<T*>(v);
        return MI355RT_OK;
    }
};

template <class T> int upload(T* d, const T* h, size_t n, const char* name) {
    return hipMemcpy(d, h, n * sizeof(T), hipMemcpyHostToDevice) == hipSuccess ? MI355RT_OK : fail(MI355RT_ERR_HIP, std::string("upload ") + name);
}
template <class T> int copy_back(T* h, const T* d, size_t n, const char* name) {      // (waits for what the null stream was given)
    return hipMemcpy(h, d, n * sizeof(T), hipMemcpyDeviceToHost) == hipSuccess ? MI355RT_OK : fail(MI355RT_ERR_HIP, std::string("copy back ") + name);
}

// The image of a render on the device: packed words and, when the caller wants them, linear floats; between the two, a progressive call's sums.
struct Image {
    uint32_t* packed = nullptr; float* linear = nullptr; float* accum = nullptr;
    int alloc(Call& call, size_t npix, bool want_linear, bool want_accum = false) {
        if (int rc = call.alloc(packed, npix, "out_packed")) return rc;
        if (want_accum) if (int rc = call.alloc(accum, npix * 4, "accum")) return rc;
        return want_linear ? call.alloc(linear, npix * 3, "out_linear") : MI355RT_OK;
    }
    int fetch(uint32_t* out_packed, float* out_linear, size_t npix) const {
        if (int rc = copy_back(out_packed, packed, npix, "packed")) return rc;
        return out_linear ? copy_back(out_linear, linear, npix * 3, "linear") : MI355RT_OK;
    }
};

// The two progressive calls from their context on: the scene, the image (on `device` for a multi context, whose sums stay on its parts; a single
// context's are the call's), the chunks -- each waits (stats); the outputs are copied back after a chunk the caller looks at, and after the last.
// *stats receives the running total, also of a failure or an early stop: times and counts summed, the launch figures the last chunk's (a multi context's are 0).
int render_chunks(Call& call, int device, const mi355rt_scene* scene, const mi355rt_camera* camera, const mi355rt_settings* settings, const mi355rt_options* opt,
                  size_t n_rows, uint32_t chunk_spp, mi355rt_progress_fn on_chunk, void* user, uint32_t* out_packed, float* out_linear, mi355rt_stats* stats) {
    mi355rt_stats total{};
    const int rc = [&]() -> int {
        if (int rc = call.multi ? mi355rt_multi_context_set_scene(call.multi, scene, camera, settings) : mi355rt_context_set_scene(call.ctx, scene, camera, settings)) return rc;
        const size_t npix = n_rows * settings->width;
        if (!npix) return MI355RT_OK;
        if (call.multi && hipSetDevice(device) != hipSuccess) return fail(MI355RT_ERR_HIP, "hipSetDevice(hip_devices[0])");
        Image img;
        if (int rc = img.alloc(call, npix, out_linear != nullptr, !call.multi)) return rc;
        const uint32_t spp = settings->samples_per_pixel;
        for (uint32_t s0 = 0; s0 < spp; ) {
            const uint32_t s1 = s0 + std::min(chunk_spp, spp - s0);
            mi355rt_stats st{};
            if (int rc = call.multi ? mi355rt_multi_context_render_progressive(call.multi, opt, s0, s1, nullptr, img.packed, img.linear, nullptr, &st)
                                    : mi355rt_context_render_progressive(call.ctx, opt, s0, s1, img.accum, img.packed, img.linear, nullptr, &st)) return rc;
            total.render_kernel_ms += st.render_kernel_ms; total.resolve_kernel_ms += st.resolve_kernel_ms; total.total_ms += st.total_ms;
            total.samples += st.samples; total.rays += st.rays; total.bands += st.bands;
            total.rows_rendered = st.rows_rendered; total.grid_blocks = st.grid_blocks; total.block_threads = st.block_threads;
            total.kernel_vgprs = st.kernel_vgprs; total.kernel_sgprs = st.kernel_sgprs;
            if (on_chunk || s1 == spp) if (int rc = img.fetch(out_packed, out_linear, npix)) return rc;
            s0 = s1;
            if (on_chunk && on_chunk(user, s1, spp, out_packed) != 0) break;               // the caller stops early: outputs hold s1 samples
        }
        return MI355RT_OK;
    }();
    if (stats) *stats = total;
    return rc;
}

// The queries: a context on device 0, the scene uploaded (set_scene wants a view; a query does not look at it), n records up, one query, n records back.
// A record of the result is out_per elements of Out; in_out: the result's buffer is uploaded first (running sums).  `run` gets the call, for what else it holds on the device.
template <class In, class Out, class Query>
int query(const mi355rt_scene* scene, const In* in, const char* in_name, uint32_t n, Out* out, const char* out_name, Query&& run, size_t out_per = 1, bool in_out = false) {
    Call call;
    if (int rc = mi355rt_context_create(0, &call.ctx)) return rc;
    const mi355rt_camera no_camera{}; const mi355rt_settings one_pixel{1, 1, 1, 1};
    if (int rc = mi355rt_context_set_scene(call.ctx, scene, &no_camera, &one_pixel)) return rc;
    In* d_in = nullptr; Out* d_out = nullptr;
    if (int rc = call.alloc(d_in, n, in_name)) return rc;
    if (int rc = call.alloc(d_out, n * out_per, out_name)) return rc;
    if (int rc = upload(d_in, in, n, in_name)) return rc;
    if (in_out) if (int rc = upload(d_out, out, n * out_per, out_name)) return rc;
    if (int rc = run(call, d_in, d_out)) return rc;
    return copy_back(out, d_out, n * out_per, out_name);
}

}  // namespace

extern "C" {

int mi355rt_render(const mi355rt_scene* scene, const mi355rt_camera* camera, const mi355rt_settings* settings,
                   const mi355rt_options* opt, uint32_t* out_packed, float* out_linear, mi355rt_stats* stats) {
    return guard([&]() -> int {
    if (!out_packed) return fail(MI355RT_ERR_INVALID, "out_packed_rgb is null");
    if (int rc = check_settings(settings)) return rc;
    uint32_t n_rows = 0;
    if (int rc = mi355rt_rows_selected(settings, opt, &n_rows)) return rc;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return fail(MI355RT_ERR_NO_DEVICE, NO_DEVICE);
    Call call;
    if (int rc = mi355rt_context_create(dev, &call.ctx)) return rc;
    if (int rc = mi355rt_context_set_scene(call.ctx, scene, camera, settings)) return rc;
    const size_t npix = (size_t)n_rows * settings->width;
    if (!npix) return MI355RT_OK;                                      // (*stats stays as it was)
    Image img;
    if (int rc = img.alloc(call, npix, out_linear != nullptr)) return rc;
    mi355rt_stats local{};                                             // stats even when the caller wants none: the render then waits and reports the watchdog itself
    if (int rc = mi355rt_context_render(call.ctx, opt, img.packed, img.linear, nullptr, stats ? stats : &local)) return rc;
    return img.fetch(out_packed, out_linear, npix);
    });
}

// One host process, several GPUs (the shape of the reference's own host: a single `main`, src/main.rs:22-89).
// Row strips are dealt round-robin over `hip_devices` exactly as the one-process-per-GPU path deals them over ranks
// (options.strip_rows; 0 -> 4); every device gets the full scene, renders its strips on its own host thread and
// copies them straight into the caller's row-major image -- the exchange step is the device-to-host copy, no
// collective.  The image is bit-identical to the one-device image (draws are keyed by absolute row / x / sample).
// Not built on the multi context: one context per device per call, no peer copies and no gather kernel.
int mi355rt_render_multi(const mi355rt_scene* scene, const mi355rt_camera* camera, const mi355rt_settings* settings,
                         const mi355rt_options* opt, const int* hip_devices, uint32_t n_devices,
                         uint32_t* out_packed, float* out_linear, mi355rt_stats* stats) {
    return guard([&]() -> int {
    if (!out_packed) return fail(MI355RT_ERR_INVALID, "out_packed_rgb is null");
    if (!hip_devices || n_devices == 0) return fail(MI355RT_ERR_INVALID, "hip_devices is empty");
    if (int rc = check_settings(settings)) return rc;
    mi355rt_options base{};                                            // (its own rule, not base_options: n_parts > 1 is all it refuses)
    if (opt) base = *opt; else { base.abi_version = MI355RT_ABI_VERSION; base.rng_mode = MI355RT_RNG_CTR; }
    if (base.n_parts > 1) return fail(MI355RT_ERR_INVALID, "render_multi deals the strips itself: leave options.n_parts / part at 0");
    if (base.strip_rows == 0) base.strip_rows = 4;
    RowSel all;                                                        // the rows the caller's buffer holds (row window)
    if (int rc = select_rows(*settings, &base, all)) return rc;
    int visible = 0;
    if (hipGetDeviceCount(&visible) != hipSuccess || visible == 0) return fail(MI355RT_ERR_NO_DEVICE, NO_DEVICE);
    for (uint32_t d = 0; d < n_devices; ++d)
        if (hip_devices[d] < 0 || hip_devices[d] >= visible) return fail(MI355RT_ERR_INVALID, "hip_devices entry out of range");
    const uint32_t W = settings->width, row0 = all.rows.empty() ? 0u : all.rows.front();
    struct Part { int rc = MI355RT_OK; std::string err; mi355rt_stats st{}; };
    std::vector<Part> parts(n_devices);
    auto render_part = [&](uint32_t d) -> int {
        mi355rt_options o = base; o.n_parts = n_devices; o.part = d;
        RowSel sel;
        if (int rc = select_rows(*settings, &o, sel)) return rc;
        if (sel.rows.empty()) return MI355RT_OK;
        const size_t npix = sel.rows.size() * (size_t)W;
        std::vector<uint32_t> h_packed(npix); std::vector<float> h_linear(out_linear ? npix * 3 : 0);
        Call call; Image img;
        if (int rc = mi355rt_context_create(hip_devices[d], &call.ctx)) return rc;
        if (int rc = mi355rt_context_set_scene(call.ctx, scene, camera, settings)) return rc;
        if (int rc = img.alloc(call, npix, out_linear != nullptr)) return rc;
        if (int rc = mi355rt_context_render(call.ctx, &o, img.packed, img.linear, nullptr, &parts[d].st)) return rc;
        if (int rc = img.fetch(h_packed.data(), out_linear ? h_linear.data() : nullptr, npix)) return rc;
        for (size_t j = 0; j < sel.rows.size(); ++j) {                 // de-interleave: local row j is image row sel.rows[j]
            const size_t dst = (size_t)(sel.rows[j] - row0) * W;
            std::memcpy(out_packed + dst, h_packed.data() + j * W, (size_t)W * 4);
            if (out_linear) std::memcpy(out_linear + dst * 3, h_linear.data() + j * W * 3, (size_t)W * 12);
        }
        return MI355RT_OK;
    };
    // One part, on whatever thread runs it: nothing may leave by exception (on a worker thread that would be std::terminate).
    run_parts(n_devices, [&](size_t d) noexcept {
        parts[d].rc = guard([&]() -> int { return render_part((uint32_t)d); });
        if (parts[d].rc) { try { parts[d].err = last_error(); } catch (...) {} }
    });
    mi355rt_stats total{};
    for (uint32_t d = 0; d < n_devices; ++d) {
        if (parts[d].rc) return fail(parts[d].rc, "device " + std::to_string(hip_devices[d]) + ": " + parts[d].err);
        const mi355rt_stats& s = parts[d].st;
        total.render_kernel_ms = std::max(total.render_kernel_ms, s.render_kernel_ms);     // the devices run side by side
        total.resolve_kernel_ms = std::max(total.resolve_kernel_ms, s.resolve_kernel_ms);
        total.total_ms = std::max(total.total_ms, s.total_ms);
        total.samples += s.samples; total.rays += s.rays; total.rows_rendered += s.rows_rendered; total.bands += s.bands;
        total.grid_blocks = std::max(total.grid_blocks, s.grid_blocks); total.block_threads = s.block_threads ? s.block_threads : total.block_threads;
        total.kernel_vgprs = s.kernel_vgprs ? s.kernel_vgprs : total.kernel_vgprs; total.kernel_sgprs = s.kernel_sgprs ? s.kernel_sgprs : total.kernel_sgprs;
    }
    if (stats) *stats = total;
    return MI355RT_OK;
    });
}

// Host-buffer progressive render: what a preview window (src/main.rs:60-75) would be fed from.
int mi355rt_render_progressive(const mi355rt_scene* scene, const mi355rt_camera* camera, const mi355rt_settings* settings,
                               const mi355rt_options* opt, uint32_t chunk_spp, mi355rt_progress_fn on_chunk, void* user,
                               uint32_t* out_packed, float* out_linear, mi355rt_stats* stats) {
    return guard([&]() -> int {
    if (!out_packed) return fail(MI355RT_ERR_INVALID, "out_packed_rgb is null");
    if (chunk_spp == 0) return fail(MI355RT_ERR_INVALID, "chunk_spp is 0");
    if (int rc = check_settings(settings)) return rc;
    uint32_t n_rows = 0;
    if (int rc = mi355rt_rows_selected(settings, opt, &n_rows)) return rc;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return fail(MI355RT_ERR_NO_DEVICE, NO_DEVICE);
    Call call;
    if (int rc = mi355rt_context_create(dev, &call.ctx)) return rc;
    return render_chunks(call, dev, scene, camera, settings, opt, n_rows, chunk_spp, on_chunk, user, out_packed, out_linear, stats);
    });
}

// Its multi-device twin, on a multi context.
int mi355rt_render_progressive_multi(const mi355rt_scene* scene, const mi355rt_camera* camera, const mi355rt_settings* settings,
                                     const mi355rt_options* opt, const int* hip_devices, uint32_t n_devices, uint32_t chunk_spp,
                                     mi355rt_progress_fn on_chunk, void* user, uint32_t* out_packed, float* out_linear, mi355rt_stats* stats) {
    return guard([&]() -> int {
    if (!out_packed) return fail(MI355RT_ERR_INVALID, "out_packed_rgb is null");
    if (chunk_spp == 0) return fail(MI355RT_ERR_INVALID, "chunk_spp is 0");
    if (!hip_devices || n_devices == 0) return fail(MI355RT_ERR_INVALID, "hip_devices is empty");
    if (int rc = check_settings(settings)) return rc;
    mi355rt_options base;
    if (int rc = base_options(opt, "render_progressive_multi", base)) return rc;
    RowSel all;
    if (int rc = select_rows(*settings, &base, all)) return rc;
    if (base.rng_mode != MI355RT_RNG_CTR)
        return fail(MI355RT_ERR_INVALID, "progressive rendering needs MI355RT_RNG_CTR (the reference stream of a row is sequential over its pixels)");
    DeviceScope scope;                                                 // (before the call's owner: the device is put back last)
    Call call;
    if (int rc = mi355rt_multi_context_create(hip_devices, n_devices, &call.multi)) return rc;   // (no device: MI355RT_ERR_NO_DEVICE, no CPU path)
    return render_chunks(call, hip_devices[0], scene, camera, settings, &base, all.rows.size(), chunk_spp, on_chunk, user, out_packed, out_linear, stats);
    });
}

int mi355rt_trace_rays(const mi355rt_scene* scene, const mi355rt_ray* rays, uint32_t n_rays, mi355rt_hit* out_hits) {
    return guard([&]() -> int {
    if (!scene) return fail(MI355RT_ERR_INVALID, "scene is null");
    if (n_rays && (!rays || !out_hits)) return fail(MI355RT_ERR_INVALID, "trace_rays: rays / out_hits is null");
    if (n_rays == 0) return MI355RT_OK;
    return query(scene, rays, "rays", n_rays, out_hits, "hits", [&](Call& call, const mi355rt_ray* d_rays, mi355rt_hit* d_hits) {
        return mi355rt_context_trace_rays(call.ctx, d_rays, n_rays, d_hits, nullptr); });
    });
}

int mi355rt_occluded(const mi355rt_scene* scene, const mi355rt_segment* segments, uint32_t n, uint32_t* out) {
    return guard([&]() -> int {
    if (!scene) return fail(MI355RT_ERR_INVALID, "occluded: scene is null");
    if (n && !segments) return fail(MI355RT_ERR_INVALID, "occluded: segments is null");
    if (n && !out) return fail(MI355RT_ERR_INVALID, "occluded: out is null");
    if (n == 0) return MI355RT_OK;
    return query(scene, segments, "segments", n, out, "words", [&](Call& call, const mi355rt_segment* d_seg, uint32_t* d_out) {
        return mi355rt_context_occluded(call.ctx, d_seg, n, d_out, nullptr); });
    });
}

// The rays go up, the running sums go up (when the call continues them) and come back; the scratch and the optional means are the call's own.
int mi355rt_trace_radiance(const mi355rt_scene* scene, const mi355rt_radiance_params* params, const mi355rt_path_ray* rays, uint32_t n_rays,
                           float* accum_in_out, float* out_linear) {
    return guard([&]() -> int {
    if (!scene) return fail(MI355RT_ERR_INVALID, "trace_radiance: scene is null");
    if (!params) return fail(MI355RT_ERR_INVALID, "trace_radiance: params is null");
    if (params->flags != 0u) return fail(MI355RT_ERR_INVALID, "trace_radiance: params.flags must be 0");
    if (params->reserved != 0u) return fail(MI355RT_ERR_INVALID, "trace_radiance: params.reserved must be 0");
    if (params->sample_begin >= params->sample_end) return fail(MI355RT_ERR_INVALID, "trace_radiance: params.sample_begin must be below params.sample_end");
    if (n_rays && !rays) return fail(MI355RT_ERR_INVALID, "trace_radiance: rays is null");
    if (n_rays && !accum_in_out) return fail(MI355RT_ERR_INVALID, "trace_radiance: accum_in_out is null");
    if (n_rays == 0) return MI355RT_OK;
    uint64_t scratch_bytes = 0;
    if (int rc = radiance_scratch_bytes(n_rays, params->sample_end - params->sample_begin, &scratch_bytes)) return rc;
    return query(scene, rays, "rays", n_rays, accum_in_out, "accum", [&](Call& call, const mi355rt_path_ray* d_rays, float* d_accum) -> int {
        unsigned char* d_scratch = nullptr; float* d_linear = nullptr;
        if (int rc = call.alloc(d_scratch, (size_t)scratch_bytes, "scratch")) return rc;
        if (out_linear) if (int rc = call.alloc(d_linear, (size_t)n_rays * 3, "out_linear")) return rc;
        if (int rc = mi355rt_context_trace_radiance(call.ctx, params, d_rays, n_rays, d_accum, d_linear, d_scratch, nullptr)) return rc;
        return out_linear ? copy_back(out_linear, d_linear, (size_t)n_rays * 3, "linear") : MI355RT_OK;
    }, 4, params->sample_begin > 0u);
    });
}

// Host buffers in, host buffers out: a context on device 0 (no scene), the image and the records uploaded, one call, the results copied back.
int mi355rt_denoise(uint32_t width, uint32_t rows, const mi355rt_denoise_params* params, const float* linear_in, const mi355rt_hit* hits,
                    float* out_linear, uint32_t* out_packed) {
    return guard([&]() -> int {
    DenoisePlan plan;
    if (!linear_in) return fail(MI355RT_ERR_INVALID, "denoise: linear_in is null");
    if (!hits) return fail(MI355RT_ERR_INVALID, "denoise: hits is null");
    if (!out_linear && !out_packed) return fail(MI355RT_ERR_INVALID, "denoise: out_linear and out_packed are both null");
    if (int rc = plan_denoise(width, rows, params, plan)) return rc;
    const size_t n = (size_t)width * rows;
    Call call;
    if (int rc = mi355rt_context_create(0, &call.ctx)) return rc;
    float* d_in = nullptr; float* d_lin = nullptr; mi355rt_hit* d_hits = nullptr; uint32_t* d_packed = nullptr; unsigned char* d_scratch = nullptr;
    if (int rc = call.alloc(d_in, n * 3, "image")) return rc;
    if (int rc = call.alloc(d_hits, n, "hits")) return rc;
    if (int rc = call.alloc(d_scratch, n * DENOISE_SCRATCH_PER_PIXEL, "scratch")) return rc;
    if (out_linear) if (int rc = call.alloc(d_lin, n * 3, "out_linear")) return rc;
    if (out_packed) if (int rc = call.alloc(d_packed, n, "out_packed")) return rc;
    if (int rc = upload(d_in, linear_in, n * 3, "image")) return rc;
    if (int rc = upload(d_hits, hits, n, "hits")) return rc;
    if (int rc = mi355rt_context_denoise(call.ctx, width, rows, params, d_in, d_hits, d_scratch, d_lin, d_packed, nullptr)) return rc;
    if (out_linear) if (int rc = copy_back(out_linear, d_lin, n * 3, "linear")) return rc;   // (waits for the kernels)
    return out_packed ? copy_back(out_packed, d_packed, n, "packed") : MI355RT_OK;
    });
}

}  // extern "C"
