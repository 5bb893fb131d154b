// rt_multi.cpp -- the resident multi-device form of include/mi355rt.h (mi355rt_multi_context_*), part of libmi355rt.so.
//
// One host process drives several GPUs (the reference's host is a single `main`, src/main.rs:57) and keeps across calls what
// mi355rt_render_multi (rt_oneshot.cpp) rebuilds on every call.  Every entry of the device list is one PART: its own mi355rt_context (scene uploaded
// once), a non-blocking stream, a staging buffer for its rows (packed, and linear when asked for; it only grows) and a done-event.
// The destination device (the first entry) keeps a staging area with every part's rows back to back and the row table of
// k_gather_strips (src_row[r] = the staging row of output row r), uploaded only when the row selection changes.
//
// Stream / event protocol of one render; S = the caller's stream on the destination device:
//   1. `entry` is recorded on S -- behind a wait on the previous render's `done` when S is not that render's stream -- and every part
//      stream waits on it: a part never overwrites its staging while the previous render's copies still read it;
//   2. every part enqueues mi355rt_context_render of its strips into its staging, on its own stream, without stats, and records its
//      done-event;
//   3. S waits on every part's done-event and issues one hipMemcpyPeerAsync per part and output into the destination staging -- also
//      for a part on the destination device itself, so that a one-GPU machine runs the path a node runs;
//   4. one k_gather_strips launch on S writes every row to its place in the caller's image;
//   5. `done` is recorded on S.
// With stats, the call then waits for `done` once and reads every part's timing pool (mi355rt_context_set_timing / read_timing): the
// parts are never serialised by the per-render stats path of mi355rt_context_render.
//
// Progressive rendering (mi355rt_multi_context_render_progressive) runs the same five steps.  Every part keeps its running sums (`accum`: a
// float4 per pixel of its strips, on its own device, only grown) and in step 2 enqueues mi355rt_context_render_progressive into them instead
// of mi355rt_context_render; the sums stay on the part between chunks.  When the caller asks for the sums, step 3 adds one peer copy per part
// straight from `accum` into a staging area of the destination (`stage_accum`, the same row order as the image staging) and step 4 one
// k_gather_accum launch with the same row table.  The sequence (the sample_end and the options of the last chunk) is kept here, so that a
// chunk that does not continue it is refused before anything is enqueued.  The one-shot form with host buffers,
// mi355rt_render_progressive_multi, is a client of these entry points and lives in rt_oneshot.cpp.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <string>
#include <vector>

#include "../../../include/mi355rt.h"
#include "rt_device.h"
#include "rt_host.h"

using namespace mi355rt;

extern "C" int mi355rt_debug_read_counters(mi355rt_context* ctx, unsigned long long* out40);   // rt_debug.cpp: the device counters of the last render

namespace {

struct Part {
    int device = 0;
    mi355rt_context* ctx = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;
    DevBuf<uint32_t> packed; DevBuf<float> linear;    // this part's rows, on `device`
    DevBuf<float> accum;                              // this part's running sums of a progressive sequence: 4 floats per pixel of its rows, on `device`
    double kernel_ms = 0;                             // render + resolve kernel ms of the last render with stats (diagnostic hook below)
};

std::string part_name(const Part& p, size_t i) { return "device " + std::to_string(p.device) + " (part " + std::to_string(i) + ")"; }
int part_fail(int rc, const Part& p, size_t i) { return fail(rc, part_name(p, i) + ": " + mi355rt_last_error()); }

}  // namespace

struct mi355rt_multi_context {
    std::vector<Part> parts;
    int dest = 0;                                     // hip_devices[0]: where the outputs live
    bool have_scene = false;
    mi355rt_settings settings{};
    hipEvent_t entry = nullptr, done = nullptr;       // on `dest`
    hipStream_t last_stream = nullptr; bool have_last = false;
    DevBuf<uint32_t> stage_packed; DevBuf<float> stage_linear; DevBuf<uint32_t> src_row;   // on `dest`
    std::vector<uint32_t> src_row_host;               // what src_row holds; the source of its upload, so it must outlive the copy
    bool table_valid = false;
    DevBuf<float> stage_accum;                        // on `dest`: every part's sums back to back (progressive calls given d_accum)
    // The progressive sequence: while `seq_on`, the next chunk may begin at `seq_end` if its key (row selection, rng_mode, seed, flags)
    // equals `seq_key`; anything else must start at 0.
    bool seq_on = false; uint32_t seq_end = 0; mi355rt_options seq_key{};
};

namespace {

// Waits for everything this multi context has enqueued: the last render's assembly and every part stream (a render that failed half
// way may have left part renders that `done` does not cover).
int drain(mi355rt_multi_context* m) {
    HIP_TRY(hipSetDevice(m->dest));
    if (m->have_last) HIP_TRY(hipEventSynchronize(m->done));
    for (Part& p : m->parts) {
        if (!p.stream) continue;
        HIP_TRY(hipSetDevice(p.device));
        HIP_TRY(hipStreamSynchronize(p.stream));
    }
    return MI355RT_OK;
}

void release(mi355rt_multi_context* m) noexcept {     // (HIP calls and frees only)
    for (Part& p : m->parts) {
        if (p.ctx) mi355rt_context_destroy(p.ctx);
        (void)hipSetDevice(p.device);
        p.packed.release(); p.linear.release(); p.accum.release();
        if (p.stream) (void)hipStreamDestroy(p.stream);
        if (p.done) (void)hipEventDestroy(p.done);
    }
    (void)hipSetDevice(m->dest);
    m->stage_packed.release(); m->stage_linear.release(); m->src_row.release(); m->stage_accum.release();
    if (m->entry) (void)hipEventDestroy(m->entry);
    if (m->done) (void)hipEventDestroy(m->done);
    delete m;
}

// Peer access from `a` to `b`, where the hardware allows it.  Already enabled (torch and other libraries share this process-wide state)
// is fine; it is never disabled.
int enable_peer(int a, int b) {
    int can = 0;
    HIP_TRY(hipDeviceCanAccessPeer(&can, a, b));
    if (!can) return MI355RT_OK;
    HIP_TRY(hipSetDevice(a));
    const hipError_t e = hipDeviceEnablePeerAccess(b, 0);
    if (e == hipErrorPeerAccessAlreadyEnabled) { (void)hipGetLastError(); return MI355RT_OK; }
    HIP_TRY(e);
    return MI355RT_OK;
}

// A progressive chunk: samples [s0, s1) into every part's sums; the caller's sums (d_accum) receive them when not null.
struct Chunk { uint32_t s0 = 0, s1 = 0; void* d_accum = nullptr; };

// Steps 1-5 of the header comment, for a whole frame (chunk == null) or one progressive chunk.  The caller has checked its arguments and
// holds a DeviceScope.
int render_parts(mi355rt_multi_context* m, const mi355rt_options& base, const Chunk* chunk, void* d_out_packed, void* d_out_linear,
                 void* hip_stream, mi355rt_stats* stats, std::chrono::steady_clock::time_point t0) {
    const mi355rt_settings& st = m->settings;
    RowSel all;                                                        // the window: the rows the caller's buffers hold
    if (int rc = select_rows(st, &base, all)) return rc;
    const size_t N = m->parts.size(), W = st.width, n_rows = all.rows.size();
    const bool want_accum = chunk && chunk->d_accum;
    if (stats) { std::memset(stats, 0, sizeof *stats); }
    // Every part's rows (the strips it is dealt) and where they start in the destination staging; the row table of the gather.
    std::vector<RowSel> sel(N);
    std::vector<size_t> offset(N);
    std::vector<uint32_t> table(n_rows);
    size_t staged = 0;
    for (size_t i = 0; i < N; ++i) {
        mi355rt_options o = base; o.n_parts = (uint32_t)N; o.part = (uint32_t)i;
        if (int rc = select_rows(st, &o, sel[i])) return rc;
        offset[i] = staged;
        for (size_t j = 0; j < sel[i].rows.size(); ++j) table[sel[i].rows[j] - base.row_begin] = (uint32_t)(staged + j);
        staged += sel[i].rows.size();
    }
    if (n_rows == 0) {
        if (stats) stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        return MI355RT_OK;
    }
    const bool same_table = m->table_valid && table == m->src_row_host;
    bool grow = !same_table || m->stage_packed.n < n_rows * W || (d_out_linear && m->stage_linear.n < n_rows * W * 3) ||
                (want_accum && m->stage_accum.n < n_rows * W * 4);
    for (size_t i = 0; i < N; ++i) {
        const size_t np = sel[i].rows.size() * W;
        grow = grow || (np && (m->parts[i].packed.n < np || (d_out_linear && m->parts[i].linear.n < np * 3) || (chunk && m->parts[i].accum.n < np * 4)));
    }
    if (grow) {                                                        // a buffer is replaced, or the table's host copy is rewritten:
        if (int rc = drain(m)) return rc;                              // nothing enqueued earlier may still use them
        for (size_t i = 0; i < N; ++i) {
            const size_t np = sel[i].rows.size() * W;
            if (!np) continue;
            Part& p = m->parts[i];
            HIP_TRY(hipSetDevice(p.device));
            if (int rc = p.packed.ensure(np)) return rc;
            if (d_out_linear) if (int rc = p.linear.ensure(np * 3)) return rc;
            if (chunk) if (int rc = p.accum.ensure(np * 4)) return rc;  // (a chunk that continues a sequence selects the same rows: no growth)
        }
        HIP_TRY(hipSetDevice(m->dest));
        if (int rc = m->stage_packed.ensure(n_rows * W)) return rc;
        if (d_out_linear) if (int rc = m->stage_linear.ensure(n_rows * W * 3)) return rc;
        if (want_accum) if (int rc = m->stage_accum.ensure(n_rows * W * 4)) return rc;
        if (int rc = m->src_row.ensure(n_rows)) return rc;
    }
    hipStream_t S = (hipStream_t)hip_stream;
    HIP_TRY(hipSetDevice(m->dest));
    if (m->have_last && m->last_stream != S) HIP_TRY(hipStreamWaitEvent(S, m->done, 0));    // the previous render (another stream) owns the buffers
    if (!same_table) {
        m->table_valid = false;
        m->src_row_host.swap(table);
        HIP_TRY(hipMemcpyAsync(m->src_row.p, m->src_row_host.data(), n_rows * sizeof(uint32_t), hipMemcpyHostToDevice, S));
        m->table_valid = true;
    }
    HIP_TRY(hipEventRecord(m->entry, S));
    for (size_t i = 0; i < N; ++i) {                                   // 2. the parts render
        if (sel[i].rows.empty()) continue;
        Part& p = m->parts[i];
        HIP_TRY(hipSetDevice(p.device));
        HIP_TRY(hipStreamWaitEvent(p.stream, m->entry, 0));
        if (int rc = mi355rt_context_set_timing(p.ctx, stats ? 1 : 0)) return part_fail(rc, p, i);
        mi355rt_options o = base; o.n_parts = (uint32_t)N; o.part = (uint32_t)i;
        float* lin = d_out_linear ? p.linear.p : nullptr;
        const int rc = chunk ? mi355rt_context_render_progressive(p.ctx, &o, chunk->s0, chunk->s1, p.accum.p, p.packed.p, lin, p.stream, nullptr)
                             : mi355rt_context_render(p.ctx, &o, p.packed.p, lin, p.stream, nullptr);
        if (rc) return part_fail(rc, p, i);
        HIP_TRY(hipEventRecord(p.done, p.stream));
    }
    HIP_TRY(hipSetDevice(m->dest));
    for (size_t i = 0; i < N; ++i) {                                   // 3. the exchange: copy engines, one copy per part and output
        const size_t np = sel[i].rows.size() * W;
        if (!np) continue;
        const Part& p = m->parts[i];
        HIP_TRY(hipStreamWaitEvent(S, p.done, 0));
        HIP_TRY(hipMemcpyPeerAsync(m->stage_packed.p + offset[i] * W, m->dest, p.packed.p, p.device, np * sizeof(uint32_t), S));
        if (d_out_linear) HIP_TRY(hipMemcpyPeerAsync(m->stage_linear.p + offset[i] * W * 3, m->dest, p.linear.p, p.device, np * 3 * sizeof(float), S));
        if (want_accum) HIP_TRY(hipMemcpyPeerAsync(m->stage_accum.p + offset[i] * W * 4, m->dest, p.accum.p, p.device, np * 4 * sizeof(float), S));
    }
    GatherParams g{};                                                  // 4. every row to its place
    g.src_row = m->src_row.p; g.src_packed = m->stage_packed.p; g.dst_packed = (uint32_t*)d_out_packed;
    g.src_linear = d_out_linear ? reinterpret_cast<const uint32_t*>(m->stage_linear.p) : nullptr; g.dst_linear = (uint32_t*)d_out_linear;
    g.n_rows = (uint32_t)n_rows; g.width = (uint32_t)W;
    if (launch_gather_strips(g, S) != 0) return fail(MI355RT_ERR_HIP, "k_gather_strips launch failed");
    if (want_accum) {
        GatherAccumParams ga{};
        ga.src_row = m->src_row.p; ga.src = reinterpret_cast<const uint32_t*>(m->stage_accum.p); ga.dst = (uint32_t*)chunk->d_accum;
        ga.n_rows = (uint32_t)n_rows; ga.width = (uint32_t)W;
        if (launch_gather_accum(ga, S) != 0) return fail(MI355RT_ERR_HIP, "k_gather_accum launch failed");
    }
    HIP_TRY(hipEventRecord(m->done, S));                               // 5.
    m->last_stream = S; m->have_last = true;
    if (!stats) return MI355RT_OK;
    HIP_TRY(hipEventSynchronize(m->done));
    const double wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    for (size_t i = 0; i < N; ++i) {
        if (sel[i].rows.empty()) continue;
        Part& p = m->parts[i];
        double a = 0, c = 0; uint32_t launches = 0;
        if (int rc = mi355rt_context_read_timing(p.ctx, &a, &c, &launches)) return part_fail(rc, p, i);   // (also reports a failed render)
        (void)mi355rt_context_set_timing(p.ctx, 0);
        unsigned long long h[STATS_WORDS] = {};
        if (int rc = mi355rt_debug_read_counters(p.ctx, h)) return part_fail(rc, p, i);
        p.kernel_ms = a + c;
        stats->render_kernel_ms = std::max(stats->render_kernel_ms, a);              // the parts run side by side
        stats->resolve_kernel_ms = std::max(stats->resolve_kernel_ms, c);
        stats->samples += h[0]; stats->rays += h[1];
        stats->rows_rendered += (uint32_t)sel[i].rows.size();
        stats->bands += launches ? launches : 1u;                                    // (the replay mode launches one kernel, outside the timing pool)
    }
    stats->total_ms = wall;
    return MI355RT_OK;
}

}  // namespace

extern "C" {

int mi355rt_multi_context_create(const int* hip_devices, uint32_t n_devices, mi355rt_multi_context** out) {
    return guard([&]() -> int {
    if (!out) return fail(MI355RT_ERR_INVALID, "out is null");
    *out = nullptr;
    if (!hip_devices || n_devices == 0) return fail(MI355RT_ERR_INVALID, "hip_devices is empty");
    int visible = 0;
    if (hipGetDeviceCount(&visible) != hipSuccess || visible <= 0) return fail(MI355RT_ERR_NO_DEVICE, "no HIP device visible (this library has no CPU path)");
    for (uint32_t d = 0; d < n_devices; ++d)
        if (hip_devices[d] < 0 || hip_devices[d] >= visible) return fail(MI355RT_ERR_INVALID, "hip_devices entry out of range");
    DeviceScope scope;
    mi355rt_multi_context* m = new mi355rt_multi_context();
    struct Owner { mi355rt_multi_context* m; ~Owner() { if (m) release(m); } } owner{m};
    m->dest = hip_devices[0];
    m->parts.resize(n_devices);
    for (uint32_t i = 0; i < n_devices; ++i) {
        Part& p = m->parts[i];
        p.device = hip_devices[i];
        if (int rc = mi355rt_context_create(p.device, &p.ctx)) { p.ctx = nullptr; return part_fail(rc, p, i); }
        HIP_TRY(hipSetDevice(p.device));
        HIP_TRY(hipStreamCreateWithFlags(&p.stream, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&p.done, hipEventDisableTiming));
    }
    HIP_TRY(hipSetDevice(m->dest));
    HIP_TRY(hipEventCreateWithFlags(&m->entry, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&m->done, hipEventDisableTiming));
    std::vector<int> peers;
    for (const Part& p : m->parts)
        if (p.device != m->dest && std::find(peers.begin(), peers.end(), p.device) == peers.end()) peers.push_back(p.device);
    for (int d : peers) {
        if (int rc = enable_peer(m->dest, d)) return rc;
        if (int rc = enable_peer(d, m->dest)) return rc;
    }
    *out = m; owner.m = nullptr;
    return MI355RT_OK;
    });
}

void mi355rt_multi_context_destroy(mi355rt_multi_context* m) {
    if (!m) return;
    (void)guard([&]() -> int {
        DeviceScope scope;
        const std::string keep = mi355rt_last_error();                // (a failure being reported stays readable after the clean-up)
        (void)drain(m);
        release(m);
        return fail(MI355RT_OK, keep);
    });
}

int mi355rt_multi_context_set_scene(mi355rt_multi_context* m, const mi355rt_scene* scene, const mi355rt_camera* camera,
                                    const mi355rt_settings* settings) {
    return guard([&]() -> int {
    if (!m) return fail(MI355RT_ERR_INVALID, "multi context is null");
    if (!camera) return fail(MI355RT_ERR_INVALID, "camera is null");
    if (int rc = check_settings(settings)) return rc;
    DeviceScope scope;
    m->seq_on = false;                                                 // a new scene ends a progressive sequence, whatever follows
    if (int rc = drain(m)) return rc;                                  // the parts' buffers are about to be replaced
    m->have_scene = false; m->table_valid = false;
    struct Result { int rc = MI355RT_OK; std::string err; };
    std::vector<Result> res(m->parts.size());
    // One part, on whatever thread runs it: nothing may leave by exception (on a worker thread that would be std::terminate).
    run_parts(m->parts.size(), [&](size_t i) noexcept {               // (rt_host.h: a host thread per further part)
        const int rc = guard([&]() -> int {
            const int r = mi355rt_context_set_scene(m->parts[i].ctx, scene, camera, settings);
            if (r) res[i].err = mi355rt_last_error();
            return r;
        });
        res[i].rc = rc;
        if (rc && res[i].err.empty()) { try { res[i].err = mi355rt_last_error(); } catch (...) {} }
    });
    for (size_t i = 0; i < m->parts.size(); ++i)
        if (res[i].rc) return fail(res[i].rc, part_name(m->parts[i], i) + ": " + res[i].err);
    m->settings = *settings;
    m->have_scene = true;
    return MI355RT_OK;
    });
}

int mi355rt_multi_context_render(mi355rt_multi_context* m, const mi355rt_options* opt, void* d_out_packed, void* d_out_linear,
                                 void* hip_stream, mi355rt_stats* stats) {
    return guard([&]() -> int {
    const auto t0 = std::chrono::steady_clock::now();
    if (!m) return fail(MI355RT_ERR_INVALID, "multi context is null");
    if (!m->have_scene) return fail(MI355RT_ERR_INVALID, "multi context has no scene (mi355rt_multi_context_set_scene)");
    if (!d_out_packed) return fail(MI355RT_ERR_INVALID, "d_out_packed is null");
    mi355rt_options base;
    if (int rc = base_options(opt, "multi_context_render", base)) return rc;
    DeviceScope scope;
    const int rc = render_parts(m, base, nullptr, d_out_packed, d_out_linear, hip_stream, stats, t0);
    if (rc == MI355RT_ERR_HIP) m->seq_on = false;                      // a part failed -- perhaps an earlier chunk's watchdog: its sums are not to be continued
    return rc;
    });
}

int mi355rt_multi_context_render_progressive(mi355rt_multi_context* m, const mi355rt_options* opt, uint32_t sample_begin, uint32_t sample_end,
                                             void* d_accum, void* d_out_packed, void* d_out_linear, void* hip_stream, mi355rt_stats* stats) {
    return guard([&]() -> int {
    const auto t0 = std::chrono::steady_clock::now();
    if (!m) return fail(MI355RT_ERR_INVALID, "multi context is null");
    if (sample_end <= sample_begin) return fail(MI355RT_ERR_INVALID, "sample_end must be greater than sample_begin");
    if (!m->have_scene) return fail(MI355RT_ERR_INVALID, "multi context has no scene (mi355rt_multi_context_set_scene)");
    if (!d_out_packed) return fail(MI355RT_ERR_INVALID, "d_out_packed is null");
    mi355rt_options base;
    if (int rc = base_options(opt, "multi_context_render_progressive", base)) return rc;
    RowSel all;
    if (int rc = select_rows(m->settings, &base, all)) return rc;
    if (base.rng_mode != MI355RT_RNG_CTR)
        return fail(MI355RT_ERR_INVALID, "progressive rendering needs MI355RT_RNG_CTR (the reference stream of a row is sequential over its pixels)");
    if ((base.flags & ~MI355RT_FLAG_FIXED_AABB) != 0u) return fail(MI355RT_ERR_INVALID, "options.flags has unknown bits");
    mi355rt_options key{};                                             // what a continuation must keep
    key.row_begin = base.row_begin; key.row_end = base.row_end ? base.row_end : m->settings.height; key.strip_rows = base.strip_rows;
    key.rng_mode = base.rng_mode; key.seed = base.seed; key.flags = base.flags;
    if (sample_begin > 0) {
        const std::string at = "sample_begin " + std::to_string(sample_begin) + " continues a progressive sequence, but ";
        if (!m->seq_on)
            return fail(MI355RT_ERR_INVALID, at + "none is open on this multi context (never started, or ended by set_scene or a failure): start at 0");
        if (sample_begin != m->seq_end)
            return fail(MI355RT_ERR_INVALID, at + "the last chunk ended at sample " + std::to_string(m->seq_end) + ": continue there or start at 0");
        const mi355rt_options& k = m->seq_key;
        if (key.row_begin != k.row_begin || key.row_end != k.row_end || key.strip_rows != k.strip_rows)
            return fail(MI355RT_ERR_INVALID, at + "the row selection (row_begin, row_end, strip_rows) is not the sequence's: start at 0");
        if (key.rng_mode != k.rng_mode || key.seed != k.seed || key.flags != k.flags)
            return fail(MI355RT_ERR_INVALID, at + "rng_mode, seed or flags are not the sequence's: start at 0");
    }
    DeviceScope scope;
    m->seq_on = false;                                                 // from here on a failure ends the sequence
    const Chunk chunk{sample_begin, sample_end, d_accum};
    if (int rc = render_parts(m, base, &chunk, d_out_packed, d_out_linear, hip_stream, stats, t0)) return rc;
    m->seq_on = true; m->seq_end = sample_end; m->seq_key = key;
    return MI355RT_OK;
    });
}

int mi355rt_multi_context_check(mi355rt_multi_context* m) {
    return guard([&]() -> int {
    if (!m) return fail(MI355RT_ERR_INVALID, "multi context is null");
    DeviceScope scope;
    const int rc = [&]() -> int {
        if (m->have_last) { HIP_TRY(hipSetDevice(m->dest)); HIP_TRY(hipEventSynchronize(m->done)); }
        for (size_t i = 0; i < m->parts.size(); ++i)
            if (int rc = mi355rt_context_check(m->parts[i].ctx)) return part_fail(rc, m->parts[i], i);   // (waits for that part's last render)
        return MI355RT_OK;
    }();
    if (rc) m->seq_on = false;                                         // the sums of a failed chunk are not to be continued
    return rc;
    });
}

// Diagnostic hook (not part of the public header): render + resolve kernel ms of every part in the last render that was given stats.
int mi355rt_debug_multi_part_ms(mi355rt_multi_context* m, double* out, uint32_t capacity, uint32_t* n_parts) {
    return guard([&]() -> int {
    if (!m || !n_parts) return fail(MI355RT_ERR_INVALID, "null");
    *n_parts = (uint32_t)m->parts.size();
    if (out) for (size_t i = 0; i < m->parts.size() && i < capacity; ++i) out[i] = m->parts[i].kernel_ms;
    return MI355RT_OK;
    });
}

}  // extern "C"
