// rt_render.cpp -- CLI stand-in for the reference's `main` (src/main.rs:22-89): load a Tungsten JSON
// scene, call the MI355X render loop through the C ABI exactly where main.rs:57 calls render_scene,
// save the PNG (main.rs:58).  The minifb preview window (main.rs:60-75) becomes --chunk: a PNG that refines.
//
//   rt_render <scene.json> [-o out.png] [--width W] [--height H] [--spp N] [--max-depth D]
//             [--rng ctr|ref] [--seed S] [--skip-unknown] [--chunk N] [--pfm out.pfm] [--exr out.exr] [--gpus N | --devices a,b,..]
//             [--denoise-out denoised.png]
//             [--view-position x,y,z --view-target x,y,z [--view-fov deg] [--lens-radius r --focus-distance d]]
//             [--noise-target T [--noise-floor F] [--noise-allow FRACTION] [--min-chunks K] [--max-spp N] [--noise-out map.pfm] [--noise-device]]
// --fix-aabb / --fix-wo3 switch on the two opt-in fixes (MI355RT_FLAG_FIXED_AABB, wo3_four_index_stride): not the reference's image.
// --gpus N deals row strips over HIP devices 0..N-1 from this one process (mi355rt_render_multi); --devices a,b,... names them
// (a device may repeat: the strip plan of N GPUs on a one-GPU machine).
// --chunk N renders N samples per pixel at a time and rewrites the PNG after every chunk (a preview that refines).
// --denoise-out PATH writes, besides -o, the final image filtered by mi355rt_context_denoise with its defaults, guided by the first hits of the
// same view (a context on the first device: set_scene, first_hits, denoise).  Without it nothing the tool writes changes.
// --noise-target T stops a chunked render when its estimated noise is low enough (mi355rt_noise_*, include/mi355rt.h): chunks of --chunk samples
// (default 16) until at most --noise-allow FRACTION of the pixels (default 0) have a relative standard error of the mean luminance above T, but
// not before --min-chunks K chunks (default 4) and not past --max-spp N samples (default: the scene's spp).  --noise-floor F is the estimate's
// floor (default 0.01).  T = 0 never stops on the estimate.  Every output is the image of the samples the run stopped at, bit-identical to a
// one-shot render of that many; --noise-out PATH.pfm writes the per-pixel error map (grey, NaN where the pixel is not finite).  No preview is
// written between chunks.  One line `noise: samples=S chunks=K rendered=R above=A nonfinite=F max=.. mean=.. converged=0|1 wall_ms=.. kernel_ms=..`
// reports the stop (R >= S: what the device traced, the speculative chunk included; kernel_ms covers all of R).
// --noise-device (only with --noise-target) takes the estimate on the device, beside the running sums (mi355rt_noise_device_*): the same images,
// the same map and the same verdict, mean= equal up to the rounding of another order of summation; no copy of the sums leaves the device.
// --view-position x,y,z --view-target x,y,z renders the loaded scene through a VIEW (mi355rt_context_render_view) after set_scene with the scene's own
// camera: a pinhole at that position looking at that target (world up 0,1,0; Camera::new, src/camera.rs:14-31), with the scene's own field of view
// or --view-fov degrees at the aspect width / height; --lens-radius r --focus-distance d make it a thin lens.  The image
// keeps the scene's size, samples, depth and seed.  With the scene's own pose the PNG is the plain run's, byte for byte.  One GPU, the counter-mode
// generator, no --chunk, --denoise-out or --noise-target.  With no view option nothing the tool does changes.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <limits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "../../../include/mi355rt.h"

// The final linear image, filtered with the defaults and packed: out[width * height].  0, or 1 with the failure on stderr.
static int denoise_image(int hip_device, const mi355rt_scene* sc, const mi355rt_camera* cam, const mi355rt_settings* st, const float* linear, uint32_t* out) {
    const size_t n = (size_t)st->width * st->height;
    uint64_t scratch_bytes = 0;
    mi355rt_context* ctx = nullptr;
    void *d_lin = nullptr, *d_hits = nullptr, *d_scratch = nullptr, *d_packed = nullptr;
    const char* what = nullptr;
    int rc = mi355rt_denoise_scratch_bytes(st->width, st->height, &scratch_bytes);
    if (!rc && hipSetDevice(hip_device) != hipSuccess) what = "hipSetDevice";
    if (!rc && !what) rc = mi355rt_context_create(hip_device, &ctx);
    if (!rc && !what) rc = mi355rt_context_set_scene(ctx, sc, cam, st);
    if (!rc && !what && (hipMalloc(&d_lin, n * 12) != hipSuccess || hipMalloc(&d_hits, n * sizeof(mi355rt_hit)) != hipSuccess ||
                hipMalloc(&d_scratch, scratch_bytes) != hipSuccess || hipMalloc(&d_packed, n * 4) != hipSuccess)) what = "hipMalloc";
    if (!rc && !what && hipMemcpy(d_lin, linear, n * 12, hipMemcpyHostToDevice) != hipSuccess) what = "upload";
    if (!rc && !what) rc = mi355rt_context_first_hits(ctx, nullptr, d_hits, nullptr);
    if (!rc && !what) rc = mi355rt_context_denoise(ctx, st->width, st->height, nullptr, d_lin, d_hits, d_scratch, nullptr, d_packed, nullptr);
    if (!rc && !what && hipMemcpy(out, d_packed, n * 4, hipMemcpyDeviceToHost) != hipSuccess) what = "copy back";   // (waits for the kernels)
    if (rc) std::fprintf(stderr, "denoise failed (%d): %s\n", rc, mi355rt_last_error());
    else if (what) std::fprintf(stderr, "denoise failed: %s\n", what);
    (void)hipFree(d_lin); (void)hipFree(d_hits); (void)hipFree(d_scratch); (void)hipFree(d_packed);
    if (ctx) mi355rt_context_destroy(ctx);
    return (rc || what) ? 1 : 0;
}

// --noise-target: render chunk by chunk until mi355rt_noise_evaluate says converged, or max_spp samples are in.  One context on one device;
// the device never waits for the host's estimate: while the host looks at the sums of chunk k, chunk k + 1 is already running (one speculative
// chunk, thrown away when chunk k turns out to be enough).  Per chunk k = 1, 2, ...:
//   render stream:  mi355rt_context_render_progressive into the output pair [k & 1];  d_accum -> d_snap[k & 1] (device to device);  event E_k
//   copy stream:    wait E_k;  d_snap[k & 1] -> h_snap[k & 1] (pinned);  event F_k
//   host:           enqueue chunk k + 1 FIRST (unless chunk k ended at max_spp), then wait F_k, mi355rt_noise_update, mi355rt_noise_evaluate.
// Chunk k's image is the pair [k & 1]; the speculative chunk k + 1 writes the other pair.  d_snap[k & 1], h_snap[k & 1] and the pair [k & 1]
// are next written by chunk k + 2, and chunk k + 2 is enqueued only after the host has waited for F_k and consumed snapshot k -- so two of
// each are enough and nothing is overwritten while it is still read.
// With --noise-device there are no snapshots and no copy stream.  Per chunk k, all on the render stream:
//   mi355rt_context_render_progressive into the output pair [k & 1];  event P_k;  mi355rt_noise_device_update(d_accum);  for k >= 2
//   mi355rt_noise_device_evaluate into the pinned summary [k & 1] (and the device error map [k & 1] with --noise-out);  event F_k
//   host:           enqueue chunk k + 1 first, as above, then wait F_k and read the 56 bytes.
// P_k .. F_k (timing events) bracket the estimate's kernels of chunk k: their sum over the chunks k >= 2 is the `noise device:` line.
// --view-*: the scene through a view.  out_packed[width * height], out_linear_or_null[width * height * 3].  0, or 1 with the failure on stderr.
// The samples go in chunks of at most 2^26 (pixel, sample) pairs -- any chunking of 0 .. N gives the words of one call --, so the scratch stays below 1 GB.
static int render_through_view(int hip_device, const mi355rt_scene* sc, const mi355rt_camera* cam, const mi355rt_settings* st, const mi355rt_options* opt,
                               const mi355rt_view* view, uint32_t* out_packed, float* out_linear_or_null, double* kernel_ms) {
    const size_t n = (size_t)view->width * view->height;
    const uint32_t spp = st->samples_per_pixel;
    const uint32_t chunk = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(spp, (1ull << 26) / n));
    uint64_t scratch_bytes = 0;
    mi355rt_context* ctx = nullptr;
    void *d_accum = nullptr, *d_lin = nullptr, *d_scratch = nullptr, *d_packed = nullptr;
    const char* what = nullptr;
    int rc = mi355rt_view_scratch_bytes(view, chunk, &scratch_bytes);
    if (!rc) rc = mi355rt_context_create(hip_device, &ctx);
    if (!rc && hipSetDevice(hip_device) != hipSuccess) what = "hipSetDevice";
    if (!rc && !what) rc = mi355rt_context_set_scene(ctx, sc, cam, st);
    if (!rc && !what && (hipMalloc(&d_accum, n * 16) != hipSuccess || hipMalloc(&d_lin, n * 12) != hipSuccess || hipMalloc(&d_scratch, scratch_bytes) != hipSuccess ||
                         hipMalloc(&d_packed, n * 4) != hipSuccess)) what = "hipMalloc";
    hipEvent_t e0 = nullptr, e1 = nullptr;                                          // device time of all the chunks' kernels
    if (!rc && !what && (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess || hipEventRecord(e0, nullptr) != hipSuccess)) what = "hipEvent";
    for (uint32_t s = 0; !rc && !what && s < spp; s += chunk) {
        const mi355rt_radiance_params prm = {s, std::min(spp, s + chunk), st->max_depth, 0u, opt->seed, 0ull};
        rc = mi355rt_context_render_view(ctx, view, &prm, d_accum, d_lin, d_packed, d_scratch, nullptr);
    }
    float ms = 0.0f;
    if (!rc && !what && (hipEventRecord(e1, nullptr) != hipSuccess || hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess)) what = "hipEvent";
    *kernel_ms = ms;
    if (!rc && !what && hipMemcpy(out_packed, d_packed, n * 4, hipMemcpyDeviceToHost) != hipSuccess) what = "copy back";
    if (!rc && !what && out_linear_or_null && hipMemcpy(out_linear_or_null, d_lin, n * 12, hipMemcpyDeviceToHost) != hipSuccess) what = "copy back";
    if (!rc && !what) rc = mi355rt_context_check(ctx);
    if (rc) std::fprintf(stderr, "render_view failed (%d): %s\n", rc, mi355rt_last_error());
    else if (what) std::fprintf(stderr, "render_view failed: %s\n", what);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    (void)hipFree(d_accum); (void)hipFree(d_lin); (void)hipFree(d_scratch); (void)hipFree(d_packed);
    if (ctx) mi355rt_context_destroy(ctx);
    return (rc || what) ? 1 : 0;
}

// Camera::new (src/camera.rs:14-31) as the scene loader states it (csrc/host/scene_loader.cpp, camera_new): float32, one rounding per operation, the
// tangent correctly rounded through double.  fov_deg < 0: keep half_width / half_height of `own`.
static mi355rt_camera view_camera(const float (&pos)[3], const float (&at)[3], float fov_deg, float aspect, const mi355rt_camera& own) {
    struct V { float x, y, z; };
    const auto norm = [](V a) { const float l = std::sqrt(a.x * a.x + a.y * a.y + a.z * a.z); if (l < 1e-4f) return a; const float r = 1.0f / l; return V{a.x * r, a.y * r, a.z * r}; };
    const auto cross = [](V a, V b) { return V{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; };
    const V forward = norm(V{at[0] - pos[0], at[1] - pos[1], at[2] - pos[2]});
    const V right = norm(cross(forward, norm(V{0.0f, 1.0f, 0.0f})));
    const V up = norm(cross(right, forward));
    mi355rt_camera c = own;
    c.position[0] = pos[0]; c.position[1] = pos[1]; c.position[2] = pos[2];
    c.forward[0] = forward.x; c.forward[1] = forward.y; c.forward[2] = forward.z;
    c.right[0] = right.x; c.right[1] = right.y; c.right[2] = right.z;
    c.true_up[0] = up.x; c.true_up[1] = up.y; c.true_up[2] = up.z;
    if (fov_deg >= 0.0f) {
        const float fov_rad = fov_deg * 3.14159265358979323846f / 180.0f;
        c.half_height = (float)std::tan((double)(fov_rad / 2.0f));
        c.half_width = c.half_height * aspect;
    }
    return c;
}

static bool parse_xyz(const char* s, float (&out)[3]) {
    for (int k = 0; k < 3; ++k) {
        char* e = nullptr;
        out[k] = (float)std::strtod(s, &e);
        if (e == s || *e != (k < 2 ? ',' : '\0')) return false;
        s = e + 1;
    }
    return true;
}

struct ConvergeArgs { uint32_t chunk, max_spp; mi355rt_noise_params params; std::string noise_out; bool on_device; };
struct ConvergeResult { mi355rt_noise_summary summary; uint32_t rendered; double wall_ms, render_ms, resolve_ms, update_ms, evaluate_ms, pass_ms; uint32_t passes; };

static int render_converging(int hip_device, const mi355rt_scene* sc, const mi355rt_camera* cam, const mi355rt_settings* st, const mi355rt_options* opt,
                             const ConvergeArgs& a, uint32_t* out_packed, float* out_linear_or_null, ConvergeResult* res) {
    const size_t n = (size_t)st->width * st->height;
    mi355rt_context* ctx = nullptr; mi355rt_noise_state* noise = nullptr; mi355rt_noise_device* noise_dev = nullptr;
    void *d_accum = nullptr, *d_packed[2] = {}, *d_linear[2] = {}, *d_snap[2] = {}, *h_snap[2] = {}, *d_err[2] = {}, *h_sum[2] = {};
    hipStream_t s_render = nullptr, s_copy = nullptr; hipEvent_t E[2] = {}, F[2] = {}, P[2] = {};
    std::vector<float> error_map(a.noise_out.empty() ? 0 : n);
    const char* what = nullptr; int rc = 0, host_rc = 0;
    *res = ConvergeResult{};
    auto hip_ok = [&](hipError_t e, const char* w) { if (e != hipSuccess && !what) what = w; return e == hipSuccess; };
    const auto t0 = std::chrono::steady_clock::now();
    rc = mi355rt_context_create(hip_device, &ctx);                                      // (first: without a device its message says so)
    if (!rc) hip_ok(hipSetDevice(hip_device), "hipSetDevice");
    if (!what && !rc) rc = mi355rt_context_set_scene(ctx, sc, cam, st);
    if (!what && !rc) rc = mi355rt_context_set_timing(ctx, 1);
    if (!what && !rc && !a.on_device) host_rc = mi355rt_noise_create(st->width, st->height, &noise);
    if (!what && !rc && a.on_device) rc = mi355rt_noise_device_create(hip_device, st->width, st->height, &noise_dev);
    if (!what && !rc && !host_rc) {
        hip_ok(hipMalloc(&d_accum, n * 16), "hipMalloc");
        for (int i = 0; i < 2 && !what; ++i) {
            hip_ok(hipMalloc(&d_packed[i], n * 4), "hipMalloc"); hip_ok(hipMalloc(&d_linear[i], n * 12), "hipMalloc");
            if (a.on_device) {
                hip_ok(hipHostMalloc(&h_sum[i], sizeof(mi355rt_noise_summary), hipHostMallocDefault), "hipHostMalloc");
                if (!a.noise_out.empty()) hip_ok(hipMalloc(&d_err[i], n * 4), "hipMalloc");
                hip_ok(hipEventCreate(&P[i]), "hipEventCreate"); hip_ok(hipEventCreate(&F[i]), "hipEventCreate");
                continue;
            }
            hip_ok(hipMalloc(&d_snap[i], n * 16), "hipMalloc");
            hip_ok(hipHostMalloc(&h_snap[i], n * 16, hipHostMallocDefault), "hipHostMalloc");
            hip_ok(hipEventCreateWithFlags(&E[i], hipEventDisableTiming), "hipEventCreate"); hip_ok(hipEventCreateWithFlags(&F[i], hipEventDisableTiming), "hipEventCreate");
        }
        hip_ok(hipStreamCreateWithFlags(&s_render, hipStreamNonBlocking), "hipStreamCreate");
        if (!a.on_device) hip_ok(hipStreamCreateWithFlags(&s_copy, hipStreamNonBlocking), "hipStreamCreate");
    }
    // chunk k covers samples [begin(k), end(k)); the last one may be shorter
    auto end_of = [&](uint32_t k) { const uint64_t e = (uint64_t)k * a.chunk; return e < a.max_spp ? (uint32_t)e : a.max_spp; };
    auto enqueue = [&](uint32_t k) {
        const int i = (int)(k & 1u);
        rc = mi355rt_context_render_progressive(ctx, opt, end_of(k - 1), end_of(k), d_accum, d_packed[i], d_linear[i], s_render, nullptr);
        if (rc) return;
        if (a.on_device) {
            hip_ok(hipEventRecord(P[i], s_render), "hipEventRecord");
            rc = mi355rt_noise_device_update(noise_dev, d_accum, end_of(k), s_render);
            if (!rc && k >= 2) rc = mi355rt_noise_device_evaluate(noise_dev, &a.params, d_err[i], h_sum[i], s_render);
            if (rc) return;
            hip_ok(hipEventRecord(F[i], s_render), "hipEventRecord");
            res->rendered = end_of(k);
            return;
        }
        hip_ok(hipMemcpyAsync(d_snap[i], d_accum, n * 16, hipMemcpyDeviceToDevice, s_render), "snapshot");
        hip_ok(hipEventRecord(E[i], s_render), "hipEventRecord");
        hip_ok(hipStreamWaitEvent(s_copy, E[i], 0), "hipStreamWaitEvent");
        hip_ok(hipMemcpyAsync(h_snap[i], d_snap[i], n * 16, hipMemcpyDeviceToHost, s_copy), "snapshot copy");
        hip_ok(hipEventRecord(F[i], s_copy), "hipEventRecord");
        res->rendered = end_of(k);
    };
    uint32_t k = 1;
    if (!what && !rc && !host_rc) enqueue(1);
    for (; !what && !rc && !host_rc; ++k) {
        const bool last = end_of(k) >= a.max_spp;
        if (!last) enqueue(k + 1);                                                      // the device stays busy while the host estimates
        if (what || rc) break;
        if (!hip_ok(hipEventSynchronize(F[k & 1u]), "hipEventSynchronize")) break;
        if (a.on_device) {
            if (k >= 2) {
                float ms = 0.0f;
                if (!hip_ok(hipEventElapsedTime(&ms, P[k & 1u], F[k & 1u]), "hipEventElapsedTime")) break;
                res->pass_ms += ms; res->passes += 1;
                std::memcpy(&res->summary, h_sum[k & 1u], sizeof res->summary);
                std::printf("  %u / %u samples per pixel: above=%llu max=%.6g mean=%.6g\n", end_of(k), a.max_spp, (unsigned long long)res->summary.above,
                            res->summary.max_error, res->summary.mean_error);
            } else {
                res->summary.chunks = 1; res->summary.samples = end_of(k); res->summary.pixels = n;
                std::printf("  %u / %u samples per pixel\n", end_of(k), a.max_spp);
            }
            if (res->summary.converged || last) break;
            continue;
        }
        const auto u0 = std::chrono::steady_clock::now();
        host_rc = mi355rt_noise_update(noise, static_cast<const float*>(h_snap[k & 1u]), end_of(k));
        const auto u1 = std::chrono::steady_clock::now();
        res->update_ms += std::chrono::duration<double, std::milli>(u1 - u0).count();
        if (host_rc) break;
        if (k >= 2) {
            host_rc = mi355rt_noise_evaluate(noise, &a.params, error_map.empty() ? nullptr : error_map.data(), &res->summary);
            res->evaluate_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - u1).count();
            if (host_rc) break;
            std::printf("  %u / %u samples per pixel: above=%llu max=%.6g mean=%.6g\n", end_of(k), a.max_spp, (unsigned long long)res->summary.above,
                        res->summary.max_error, res->summary.mean_error);
        } else {
            res->summary.chunks = 1; res->summary.samples = end_of(k); res->summary.pixels = n;    // (a run that ends after one chunk has no estimate)
            std::printf("  %u / %u samples per pixel\n", end_of(k), a.max_spp);
        }
        if (res->summary.converged || last) break;
    }
    // chunk k is the result.  Wait for everything enqueued (the speculative chunk included) before anything is read or freed.
    if (s_render) hip_ok(hipStreamSynchronize(s_render), "hipStreamSynchronize");
    if (s_copy) hip_ok(hipStreamSynchronize(s_copy), "hipStreamSynchronize");
    if (!what && !rc && !host_rc) rc = mi355rt_context_check(ctx);
    if (!what && !rc && !host_rc) {
        uint32_t launches = 0;
        rc = mi355rt_context_read_timing(ctx, &res->render_ms, &res->resolve_ms, &launches);
        hip_ok(hipMemcpy(out_packed, d_packed[k & 1u], n * 4, hipMemcpyDeviceToHost), "copy back");
        if (out_linear_or_null) hip_ok(hipMemcpy(out_linear_or_null, d_linear[k & 1u], n * 12, hipMemcpyDeviceToHost), "copy back");
        if (d_err[k & 1u] && res->summary.chunks >= 2) hip_ok(hipMemcpy(error_map.data(), d_err[k & 1u], n * 4, hipMemcpyDeviceToHost), "copy back");
    }
    res->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (rc) std::fprintf(stderr, "render failed (%d): %s\n", rc, mi355rt_last_error());
    else if (host_rc) std::fprintf(stderr, "noise estimate failed (%d): %s\n", host_rc, mi355rt_host_last_error());
    else if (what) std::fprintf(stderr, "render failed: %s: %s\n", what, hipGetErrorString(hipGetLastError()));
    for (int i = 0; i < 2; ++i) {
        (void)hipFree(d_packed[i]); (void)hipFree(d_linear[i]); (void)hipFree(d_snap[i]); if (h_snap[i]) (void)hipHostFree(h_snap[i]);
        (void)hipFree(d_err[i]); if (h_sum[i]) (void)hipHostFree(h_sum[i]);
        if (E[i]) (void)hipEventDestroy(E[i]);
        if (F[i]) (void)hipEventDestroy(F[i]);
        if (P[i]) (void)hipEventDestroy(P[i]);
    }
    (void)hipFree(d_accum);
    if (s_render) (void)hipStreamDestroy(s_render);
    if (s_copy) (void)hipStreamDestroy(s_copy);
    mi355rt_noise_device_destroy(noise_dev);                                            // (both streams have been waited for)
    if (ctx) mi355rt_context_destroy(ctx);
    int failed = (rc || host_rc || what) ? 1 : 0;
    if (!failed && !a.noise_out.empty()) {                                              // the error map as grey RGB; NaN where the pixel is non-finite
        std::vector<float> rgb(n * 3);
        for (size_t p = 0; p < n; ++p) rgb[3 * p] = rgb[3 * p + 1] = rgb[3 * p + 2] = error_map[p];
        if (res->summary.chunks < 2) { std::fprintf(stderr, "--noise-out: the run ended after one chunk, there is no estimate to write\n"); failed = 1; }
        else if (mi355rt_write_pfm(a.noise_out.c_str(), rgb.data(), st->width, st->height) != MI355RT_OK) { std::fprintf(stderr, "%s\n", mi355rt_host_last_error()); failed = 1; }
    }
    mi355rt_noise_free(noise);
    return failed;
}

static const char USAGE[] = "usage: %s <scene.json> [-o out.png] [--width W] [--height H] [--spp N] [--max-depth D] [--rng ctr|ref] [--seed S] [--skip-unknown] [--chunk N] [--pfm out.pfm] [--exr out.exr] [--gpus N | --devices a,b,..] [--fix-aabb] [--fix-wo3] [--denoise-out denoised.png]"
                            " [--view-position x,y,z --view-target x,y,z [--view-fov deg] [--lens-radius r --focus-distance d]]"
                            " [--noise-target T [--noise-floor F] [--noise-allow FRACTION] [--min-chunks K] [--max-spp N] [--noise-out map.pfm] [--noise-device]]\n";

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, USAGE, argv[0]); return 2; }
    std::string scene_path = argv[1], out_path = "render_pt.png", pfm_path, exr_path, denoise_path;
    mi355rt_load_overrides ov{}; mi355rt_options opt{}; uint32_t chunk = 0, gpus = 1; std::vector<int> device_list;
    opt.abi_version = MI355RT_ABI_VERSION; opt.rng_mode = MI355RT_RNG_CTR; opt.strip_rows = 1; opt.n_parts = 1;
    ConvergeArgs cv{}; cv.params = {0.02, 0.01, 4u, 0u, 0ull};                          // the library's defaults
    float view_pos[3] = {}, view_at[3] = {}, view_fov = -1.0f, lens_radius = 0.0f, focus_distance = 0.0f;
    bool have_view_pos = false, have_view_at = false, view_option = false, have_lens = false, have_focus = false;
    bool noise = false, noise_option = false, noise_device = false, multi_option = false; double noise_allow = 0.0;
    auto usage = [&](const char* why) { std::fprintf(stderr, USAGE, argv[0]); std::fprintf(stderr, "%s\n", why); return 2; };
    for (int i = 2; i < argc; ++i) {
        auto next = [&]() -> const char* { if (i + 1 >= argc) { std::fprintf(stderr, "missing value for %s\n", argv[i]); std::exit(2); } return argv[++i]; };
        if (!std::strcmp(argv[i], "-o")) out_path = next();
        else if (!std::strcmp(argv[i], "--width")) ov.width = (uint32_t)std::atoi(next());
        else if (!std::strcmp(argv[i], "--height")) ov.height = (uint32_t)std::atoi(next());
        else if (!std::strcmp(argv[i], "--spp")) ov.samples_per_pixel = (uint32_t)std::atoi(next());
        else if (!std::strcmp(argv[i], "--max-depth")) ov.max_depth = (uint32_t)std::atoi(next());
        else if (!std::strcmp(argv[i], "--rng")) opt.rng_mode = std::strcmp(next(), "ref") ? MI355RT_RNG_CTR : MI355RT_RNG_REF;
        else if (!std::strcmp(argv[i], "--seed")) opt.seed = std::strtoull(next(), nullptr, 0);
        else if (!std::strcmp(argv[i], "--skip-unknown")) ov.skip_unknown_primitives = 1;
        else if (!std::strcmp(argv[i], "--chunk")) chunk = (uint32_t)std::atoi(next());
        else if (!std::strcmp(argv[i], "--pfm")) pfm_path = next();
        else if (!std::strcmp(argv[i], "--exr")) exr_path = next();
        else if (!std::strcmp(argv[i], "--denoise-out")) denoise_path = next();
        else if (!std::strcmp(argv[i], "--noise-target")) { cv.params.threshold = std::atof(next()); noise = true; }
        else if (!std::strcmp(argv[i], "--noise-floor")) { cv.params.floor = std::atof(next()); noise_option = true; }
        else if (!std::strcmp(argv[i], "--noise-allow")) { noise_allow = std::atof(next()); noise_option = true; }
        else if (!std::strcmp(argv[i], "--min-chunks")) { cv.params.min_chunks = (uint32_t)std::atoi(next()); noise_option = true; }
        else if (!std::strcmp(argv[i], "--max-spp")) { cv.max_spp = (uint32_t)std::atoi(next()); noise_option = true; }
        else if (!std::strcmp(argv[i], "--noise-out")) { cv.noise_out = next(); noise_option = true; }
        else if (!std::strcmp(argv[i], "--noise-device")) noise_device = true;
        else if (!std::strcmp(argv[i], "--gpus")) { gpus = (uint32_t)std::atoi(next()); multi_option = true; }
        else if (!std::strcmp(argv[i], "--devices")) {
            multi_option = true;
            for (const char* q = next(); *q;) { char* e = nullptr; const long d = std::strtol(q, &e, 10); if (e == q) { std::fprintf(stderr, "--devices wants a comma-separated list of device numbers\n"); return 2; }
                                                device_list.push_back((int)d); q = (*e == ',') ? e + 1 : e; if (*e && *e != ',') { std::fprintf(stderr, "--devices wants a comma-separated list of device numbers\n"); return 2; } }
            gpus = (uint32_t)device_list.size();
        }
        else if (!std::strcmp(argv[i], "--view-position")) { if (!parse_xyz(next(), view_pos)) return usage("--view-position wants x,y,z"); have_view_pos = true; }
        else if (!std::strcmp(argv[i], "--view-target")) { if (!parse_xyz(next(), view_at)) return usage("--view-target wants x,y,z"); have_view_at = true; }
        else if (!std::strcmp(argv[i], "--view-fov")) { view_fov = (float)std::atof(next()); view_option = true; if (!(view_fov > 0.0f && view_fov < 180.0f)) return usage("--view-fov wants degrees, 0 .. 180"); }
        else if (!std::strcmp(argv[i], "--lens-radius")) { lens_radius = (float)std::atof(next()); view_option = have_lens = true; }
        else if (!std::strcmp(argv[i], "--focus-distance")) { focus_distance = (float)std::atof(next()); view_option = have_focus = true; }
        else if (!std::strcmp(argv[i], "--fix-aabb")) opt.flags |= MI355RT_FLAG_FIXED_AABB;
        else if (!std::strcmp(argv[i], "--fix-wo3")) ov.wo3_four_index_stride = 1;
        else { std::fprintf(stderr, "unknown option %s\n", argv[i]); return 2; }
    }
    if (gpus == 0) { std::fprintf(stderr, "--gpus / --devices: at least one device\n"); return 2; }
    if (noise_option && !noise) return usage(cv.noise_out.empty() ? "--noise-floor, --noise-allow, --min-chunks and --max-spp go with --noise-target" : "--noise-out needs --noise-target");
    if (noise_device && !noise) return usage("--noise-device needs --noise-target");
    cv.on_device = noise_device;
    if (noise) {
        if (multi_option) return usage("--noise-target renders on one GPU: it cannot be combined with --gpus or --devices");
        if (opt.rng_mode == MI355RT_RNG_REF) return usage("--noise-target needs the counter-mode generator: it cannot be combined with --rng ref");
        if (!(cv.params.threshold >= 0.0) || !(cv.params.threshold < 1e300)) return usage("--noise-target wants a number >= 0");
        if (!(noise_allow >= 0.0 && noise_allow <= 1.0)) return usage("--noise-allow wants a fraction of the pixels, 0 .. 1");
        // 0 = never stop on the estimate (render --max-spp samples): the library wants a threshold > 0, and `err > the smallest double` is `err > 0`
        if (cv.params.threshold == 0.0) cv.params.threshold = std::numeric_limits<double>::denorm_min();
        if (!(cv.params.floor >= 0.0) || !(cv.params.floor < 1e300)) return usage("--noise-floor wants a number >= 0");
        if (cv.params.min_chunks < 2) return usage("--min-chunks wants at least 2: one chunk has no spread");
        cv.chunk = chunk ? chunk : 16;
    }
    const bool through_view = have_view_pos || have_view_at;
    if (have_view_pos != have_view_at || (view_option && !through_view)) return usage("a view needs both --view-position and --view-target; --view-fov, --lens-radius and --focus-distance go with them");
    if (through_view) {
        if (have_lens != have_focus) return usage("--lens-radius and --focus-distance go together");
        if (multi_option || chunk || noise || !denoise_path.empty() || opt.rng_mode == MI355RT_RNG_REF || opt.flags)
            return usage("a view renders on one GPU with the counter-mode generator: it cannot be combined with --gpus, --devices, --chunk, --noise-target, --denoise-out, --rng ref or --fix-aabb");
    }
    const bool multi = gpus > 1 || !device_list.empty();
    if (multi && chunk) { std::fprintf(stderr, "--chunk (progressive preview) renders on one GPU: it cannot be combined with --gpus %u\n", gpus); return 2; }
    std::printf("Attempting to load scene from: %s\n", scene_path.c_str());
    auto t0 = std::chrono::steady_clock::now();
    mi355rt_loaded_scene* ls = nullptr;
    if (mi355rt_scene_load_json(scene_path.c_str(), &ov, &ls) != MI355RT_OK) { std::fprintf(stderr, "%s\n", mi355rt_host_last_error()); return 1; }
    const mi355rt_scene* sc = mi355rt_loaded_scene_get(ls);
    const mi355rt_settings* st = mi355rt_loaded_scene_settings(ls);
    std::printf("Scene loaded. Objects: %u. Image: %ux%u, Samples: %u, Max Depth: %u\n", sc->n_primitives, st->width, st->height,
                st->samples_per_pixel, st->max_depth);
    std::vector<uint32_t> buffer((size_t)st->width * st->height);
    std::vector<float> linear(pfm_path.empty() && exr_path.empty() && denoise_path.empty() ? 0 : (size_t)st->width * st->height * 3);
    float* lin = linear.empty() ? nullptr : linear.data();
    mi355rt_stats stats{};
    std::printf("Rendering frame (%ux%u) with %u AA samples...\n", st->width, st->height, st->samples_per_pixel);
    struct Preview { const char* path; uint32_t w, h; } pv{out_path.c_str(), st->width, st->height};
    auto on_chunk = [](void* user, uint32_t done, uint32_t total, const uint32_t* packed) -> int {
        const Preview* p = static_cast<const Preview*>(user);
        std::printf("  %u / %u samples per pixel\n", done, total);
        if (done < total) (void)mi355rt_write_png(p->path, packed, p->w, p->h);       // the final image is written below
        return 0;
    };
    std::vector<int> devices = device_list;
    if (devices.empty()) for (uint32_t d = 0; d < gpus; ++d) devices.push_back((int)d);
    if (multi) { opt.strip_rows = 4; opt.n_parts = 0; }
    const auto t_render = std::chrono::steady_clock::now();
    if (noise) {
        if (cv.max_spp == 0) cv.max_spp = st->samples_per_pixel;
        const uint64_t n_px = (uint64_t)st->width * st->height;
        cv.params.allowed_above = (uint64_t)std::floor(noise_allow * (double)n_px);
        ConvergeResult cr;
        if (render_converging(devices[0], sc, mi355rt_loaded_scene_camera(ls), st, &opt, cv, buffer.data(), lin, &cr)) { mi355rt_scene_free(ls); return 1; }
        std::printf("noise: samples=%u chunks=%u rendered=%u above=%llu nonfinite=%llu max=%.9g mean=%.9g converged=%u wall_ms=%.3f kernel_ms=%.3f\n",
                    cr.summary.samples, cr.summary.chunks, cr.rendered, (unsigned long long)cr.summary.above, (unsigned long long)cr.summary.nonfinite,
                    cr.summary.max_error, cr.summary.mean_error, cr.summary.converged, cr.wall_ms, cr.render_ms + cr.resolve_ms);
        if (cv.on_device) std::printf("noise device: pass_ms=%.3f per chunk (update + evaluate of %u chunks, device time)\n", cr.passes ? cr.pass_ms / cr.passes : 0.0, cr.passes);
        else std::printf("noise host: update_ms=%.3f evaluate_ms=%.3f per chunk (%u updates, %u evaluations)\n", cr.update_ms / cr.summary.chunks,
                         cr.summary.chunks > 1 ? cr.evaluate_ms / (cr.summary.chunks - 1) : 0.0, cr.summary.chunks, cr.summary.chunks - 1);
        if (!cv.noise_out.empty()) std::printf("Noise map saved as '%s'\n", cv.noise_out.c_str());
        stats.samples = n_px * cr.rendered; stats.render_kernel_ms = cr.render_ms; stats.resolve_kernel_ms = cr.resolve_ms; stats.total_ms = cr.render_ms + cr.resolve_ms;
    }
    if (through_view) {
        mi355rt_view view{};
        view.camera = view_camera(view_pos, view_at, view_fov, (float)st->width / (float)st->height, *mi355rt_loaded_scene_camera(ls));
        view.model = have_lens ? MI355RT_VIEW_THIN_LENS : MI355RT_VIEW_PINHOLE;
        view.width = st->width; view.height = st->height; view.lens_radius = lens_radius; view.focus_distance = focus_distance;
        double view_ms = 0.0;
        if (render_through_view(devices[0], sc, mi355rt_loaded_scene_camera(ls), st, &opt, &view, buffer.data(), lin, &view_ms)) { mi355rt_scene_free(ls); return 1; }
        // (the view's path and sum kernels together, by device events: it has no kernel of its own for the resolve, and counts no rays)
        stats.samples = (uint64_t)st->width * st->height * st->samples_per_pixel; stats.render_kernel_ms = view_ms; stats.total_ms = view_ms;
    }
    int rc = (noise || through_view) ? MI355RT_OK : multi ? mi355rt_render_multi(sc, mi355rt_loaded_scene_camera(ls), st, &opt, devices.data(), gpus, buffer.data(), lin, &stats)
           : chunk ? mi355rt_render_progressive(sc, mi355rt_loaded_scene_camera(ls), st, &opt, chunk, on_chunk, &pv, buffer.data(), lin, &stats)
                   : mi355rt_render(sc, mi355rt_loaded_scene_camera(ls), st, &opt, buffer.data(), lin, &stats);   // <- src/main.rs:57
    if (rc != MI355RT_OK) { std::fprintf(stderr, "render failed (%d): %s\n", rc, mi355rt_last_error()); mi355rt_scene_free(ls); return 1; }
    // The call's wall time includes context creation, scene upload, workspace allocation and the copy back; the kernel
    // figures are device time (with --gpus: the maximum over the devices, which run side by side).
    const double wall_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_render).count();
    std::printf("Rendered in %.3f seconds (%.1f Msamples/s end to end; kernels %.3f ms path tracing + %.3f ms resolve%s = %.1f Msamples/s; %.2f rays/sample)\n",
                wall_s, wall_s > 0 ? (double)stats.samples / wall_s / 1e6 : 0.0, stats.render_kernel_ms, stats.resolve_kernel_ms,
                multi ? " (max over devices)" : "",
                stats.total_ms > 0 ? (double)stats.samples / stats.total_ms / 1e3 : 0.0, stats.samples ? (double)stats.rays / (double)stats.samples : 0.0);
    if (mi355rt_write_png(out_path.c_str(), buffer.data(), st->width, st->height) != MI355RT_OK) { std::fprintf(stderr, "%s\n", mi355rt_host_last_error()); mi355rt_scene_free(ls); return 1; }
    std::printf("Image saved as '%s'\n", out_path.c_str());
    if (lin && !exr_path.empty() && mi355rt_write_exr(exr_path.c_str(), lin, st->width, st->height) != MI355RT_OK) { std::fprintf(stderr, "%s\n", mi355rt_host_last_error()); mi355rt_scene_free(ls); return 1; }
    if (lin && !pfm_path.empty() && mi355rt_write_pfm(pfm_path.c_str(), lin, st->width, st->height) != MI355RT_OK) { std::fprintf(stderr, "%s\n", mi355rt_host_last_error()); mi355rt_scene_free(ls); return 1; }
    if (!denoise_path.empty()) {
        std::vector<uint32_t> denoised(buffer.size());
        if (denoise_image(devices[0], sc, mi355rt_loaded_scene_camera(ls), st, lin, denoised.data())) { mi355rt_scene_free(ls); return 1; }
        if (mi355rt_write_png(denoise_path.c_str(), denoised.data(), st->width, st->height) != MI355RT_OK) { std::fprintf(stderr, "%s\n", mi355rt_host_last_error()); mi355rt_scene_free(ls); return 1; }
        std::printf("Denoised image saved as '%s'\n", denoise_path.c_str());
    }
    mi355rt_scene_free(ls);
    std::printf("Total %.3f s\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    return 0;
}
