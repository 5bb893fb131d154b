// noise_estimate.cpp -- mi355rt_noise_*: the per-pixel noise estimate of a progressive render (include/mi355rt.h has the definition).
//
// Fed a host copy of mi355rt_context_render_progressive's running sums after every chunk, it keeps two double sums per pixel over the
// chunks' luminance sums (weighted batch means) and answers "is this image good enough yet?".  Not part of the reference: src/main.rs
// renders the file's spp and stops.  Pure CPU, double arithmetic in the order the header writes it (the library is built without
// contraction), so a restatement in numpy float64 is bit-identical.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "host_common.hpp"

struct mi355rt_noise_state {
    uint32_t width = 0, rows = 0;
    uint32_t chunks = 0, samples = 0;          // K, N
    std::vector<float> prev;                   // 3 per pixel: the last running sums
    std::vector<double> t, q;                  // per pixel: sum of Y, sum of Y*Y/n
};

namespace {
int refuse(const char* what) { return mi355rt_host::set_error(MI355RT_ERR_INVALID, what); }
}

extern "C" int mi355rt_noise_create(uint32_t width, uint32_t rows, mi355rt_noise_state** out) {
    return mi355rt_host::guard("noise_create", MI355RT_ERR_IO, [&]() -> int {
    if (!out) return refuse("noise_create: out is null");
    *out = nullptr;
    if (width == 0) return refuse("noise_create: width is 0");
    if (rows == 0) return refuse("noise_create: rows is 0");
    if ((uint64_t)width * rows >= (1ull << 31)) return refuse("noise_create: width * rows must be below 2^31");
    const size_t n = (size_t)width * rows;
    std::unique_ptr<mi355rt_noise_state> s(new mi355rt_noise_state());     // (a failed allocation leaves through the barrier: MI355RT_ERR_OOM)
    s->width = width; s->rows = rows;
    s->prev.assign(n * 3, 0.0f); s->t.assign(n, 0.0); s->q.assign(n, 0.0);
    *out = s.release();
    return MI355RT_OK;
    });
}

extern "C" void mi355rt_noise_free(mi355rt_noise_state* s) { delete s; }

extern "C" int mi355rt_noise_reset(mi355rt_noise_state* s) {
    return mi355rt_host::guard("noise_reset", MI355RT_ERR_IO, [&]() -> int {
    if (!s) return refuse("noise_reset: state is null");
    s->chunks = s->samples = 0;
    std::fill(s->prev.begin(), s->prev.end(), 0.0f);
    std::fill(s->t.begin(), s->t.end(), 0.0);
    std::fill(s->q.begin(), s->q.end(), 0.0);
    return MI355RT_OK;
    });
}

extern "C" int mi355rt_noise_update(mi355rt_noise_state* s, const float* accum, uint32_t samples_total) {
    return mi355rt_host::guard("noise_update", MI355RT_ERR_IO, [&]() -> int {
    if (!s) return refuse("noise_update: state is null");
    if (!accum) return refuse("noise_update: accum is null");
    if (samples_total <= s->samples)
        return mi355rt_host::set_error(MI355RT_ERR_INVALID, "noise_update: samples_total (" + std::to_string(samples_total) + ") must exceed the " +
                                                            std::to_string(s->samples) + " samples already seen");
    const double n = (double)(samples_total - s->samples);
    const size_t pixels = s->t.size();
    float* prev = s->prev.data(); double* T = s->t.data(); double* Q = s->q.data();
    for (size_t p = 0; p < pixels; ++p) {
        const float* a = accum + 4 * p;
        const double dr = (double)a[0] - (double)prev[3 * p], dg = (double)a[1] - (double)prev[3 * p + 1], db = (double)a[2] - (double)prev[3 * p + 2];
        const double y = (0.2126 * dr + 0.7152 * dg) + 0.0722 * db;
        T[p] += y;
        Q[p] += (y * y) / n;
        prev[3 * p] = a[0]; prev[3 * p + 1] = a[1]; prev[3 * p + 2] = a[2];
    }
    s->chunks += 1; s->samples = samples_total;
    return MI355RT_OK;
    });
}

extern "C" int mi355rt_noise_evaluate(const mi355rt_noise_state* s, const mi355rt_noise_params* params_or_null, float* out_error_or_null,
                                      mi355rt_noise_summary* out_summary) {
    return mi355rt_host::guard("noise_evaluate", MI355RT_ERR_IO, [&]() -> int {
    if (!s) return refuse("noise_evaluate: state is null");
    if (!out_summary) return refuse("noise_evaluate: out_summary is null");
    mi355rt_noise_params pr = {0.02, 0.01, 4u, 0u, 0ull};
    if (params_or_null) pr = *params_or_null;
    if (!(pr.threshold > 0.0) || !std::isfinite(pr.threshold)) return refuse("noise_evaluate: params.threshold must be > 0 and finite");
    if (!(pr.floor >= 0.0) || !std::isfinite(pr.floor)) return refuse("noise_evaluate: params.floor must be >= 0 and finite");
    if (pr.min_chunks < 2) return refuse("noise_evaluate: params.min_chunks must be >= 2");
    if (pr._pad != 0) return refuse("noise_evaluate: params._pad must be 0");
    if (s->chunks < 2) return refuse("noise_evaluate: needs at least 2 chunks (mi355rt_noise_update calls)");
    const double N = (double)s->samples, km1 = (double)(s->chunks - 1);
    const size_t pixels = s->t.size();
    uint64_t above = 0, nonfinite = 0;
    double max_error = 0.0, sum = 0.0;
    for (size_t p = 0; p < pixels; ++p) {
        const double T = s->t[p], Q = s->q[p];
        double err;
        if (!std::isfinite(T) || !std::isfinite(Q)) {
            err = std::numeric_limits<double>::quiet_NaN();
            ++nonfinite;
        } else {
            const double m = T / N;
            const double ss = Q - (T * T) / N;
            const double var = (ss > 0.0 ? ss : 0.0) / km1;
            const double se = std::sqrt(var / N);
            err = se / ((m > 0.0 ? m : 0.0) + pr.floor);
            if (std::isnan(err)) { err = std::numeric_limits<double>::quiet_NaN(); ++nonfinite; }   // 0 / 0: floor 0, neither signal nor variance
            else { if (err > pr.threshold) ++above; if (err > max_error) max_error = err; sum += err; }
        }
        if (out_error_or_null) out_error_or_null[p] = (float)err;
    }
    std::memset(out_summary, 0, sizeof *out_summary);
    out_summary->chunks = s->chunks; out_summary->samples = s->samples;
    out_summary->pixels = pixels; out_summary->above = above; out_summary->nonfinite = nonfinite;
    const uint64_t counted = pixels - nonfinite;
    out_summary->max_error = max_error;
    out_summary->mean_error = counted ? sum / (double)counted : 0.0;
    out_summary->converged = (s->chunks >= pr.min_chunks && above <= pr.allowed_above) ? 1u : 0u;
    return MI355RT_OK;
    });
}
