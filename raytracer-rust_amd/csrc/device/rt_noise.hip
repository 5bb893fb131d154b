// rt_noise.hip -- mi355rt_noise_device_*: the noise estimate of a progressive render on device memory, beside the running sums
// (defined in include/mi355rt.h, "noise estimate of a progressive render" and "the same estimate on the device").
//
// Kernels (gfx950, wave64; a translation unit of its own: no other kernel is recompiled differently for it)
//   k_noise_update     one pixel per lane over a plain grid: the pixel's running sums (one 16-byte read of d_accum, whose fourth word never
//                      enters the arithmetic) against prev, the luminance Y of the chunk into T and Q; prev and {T, Q} are one 16-byte word
//                      each, read and written once.  80 bytes per pixel.
//   k_noise_evaluate   one tile of NOISE_TILE consecutive pixels per workgroup, one pixel per lane: err from {T, Q} (16 bytes read), (float)err
//                      to the optional map (4 bytes written), and the tile's record -- above, nonfinite, the largest err, the tile tree's sum.
//   k_noise_finish     one workgroup: lane t adds the records of the tiles t, t + NOISE_TILE, ... in ascending order, the NOISE_TILE lane
//                      sums go through the tile tree once more, and lane 0 writes the 56 bytes of the summary with plain stores.
// No atomics and no polling waits; two workgroup barriers in a reduction, reached by every lane of the workgroup; the one loop (k_noise_finish)
// is bounded by the tile count.  The order of every addition depends on the pixel count alone.
// The arithmetic is the header's, operation for operation, in IEEE double: -ffp-contract=off keeps a*b+c two roundings, and the divisions
// and the square root are the compiler's correctly rounded forms (tests/test_gpu_noise_device.py compares them with the host's, word for word).
//
// The five entry points are defined here, beside their kernels; `reset`, `update` and `evaluate` only enqueue on the caller's stream, K and
// N live on the host side of the object, and every refusal is decided before any HIP call.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <memory>
#include <string>

#include "rt_host.h"
#include "rt_noise.h"

namespace mi355rt {

struct NoiseUpdate {
    const float4* accum; float4* prev; double2* tq;
    double n;                    // the samples of this chunk
    uint32_t pixels;
};
struct NoiseEvaluate {
    const double2* tq; float* out_error; NoisePartial* partials;
    double N, km1, floor, threshold;
    uint32_t pixels;
};
struct NoiseFinish {
    const NoisePartial* partials; mi355rt_noise_summary* out;
    uint64_t allowed_above;
    uint32_t n_tiles, pixels, chunks, samples, min_chunks;
};

__device__ __forceinline__ bool is_finite(double x) { return ((unsigned long long)__double_as_longlong(x) & 0x7FF0000000000000ull) != 0x7FF0000000000000ull; }

// The tile tree (mi355rt.h): within a wave lane i takes lane i + 32, then i + 16, ... i + 1 (as an exchange: both partners form the same sum,
// the addition commutes), the wave sums w0 .. w3 are then added as (w0 + w1) + (w2 + w3).  The result is valid in thread 0.
__device__ __forceinline__ void tile_reduce(double& sum, double& mx, unsigned long long& above, unsigned long long& nonfinite) {
    __shared__ double s_sum[NOISE_WAVES], s_max[NOISE_WAVES];
    __shared__ unsigned long long s_above[NOISE_WAVES], s_nonfinite[NOISE_WAVES];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        sum = sum + __shfl_xor(sum, off, 64);
        const double m = __shfl_xor(mx, off, 64);
        mx = m > mx ? m : mx;
        above += __shfl_xor(above, off, 64);
        nonfinite += __shfl_xor(nonfinite, off, 64);
    }
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0u) { s_sum[wave] = sum; s_max[wave] = mx; s_above[wave] = above; s_nonfinite[wave] = nonfinite; }
    __syncthreads();
    if (threadIdx.x == 0u) {
        static_assert(NOISE_WAVES == 4, "the tree below is written for four waves");
        sum = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
        const double a = s_max[0] > s_max[1] ? s_max[0] : s_max[1], b = s_max[2] > s_max[3] ? s_max[2] : s_max[3];
        mx = a > b ? a : b;
        above = (s_above[0] + s_above[1]) + (s_above[2] + s_above[3]);
        nonfinite = (s_nonfinite[0] + s_nonfinite[1]) + (s_nonfinite[2] + s_nonfinite[3]);
    }
    __syncthreads();                                                  // (a second reduction of the same workgroup would overwrite what thread 0 reads)
}

__global__ void __launch_bounds__(NOISE_TILE) k_noise_update(const NoiseUpdate U) {
    const uint32_t p = blockIdx.x * NOISE_TILE + threadIdx.x;         // (< 2^31: mi355rt_noise_device_create)
    if (p >= U.pixels) return;
    const float4 a = U.accum[p], pv = U.prev[p];
    double2 tq = U.tq[p];
    const double dr = (double)a.x - (double)pv.x, dg = (double)a.y - (double)pv.y, db = (double)a.z - (double)pv.z;
    const double y = (0.2126 * dr + 0.7152 * dg) + 0.0722 * db;
    tq.x = tq.x + y;
    tq.y = tq.y + (y * y) / U.n;
    U.tq[p] = tq;
    U.prev[p] = make_float4(a.x, a.y, a.z, 0.0f);
}

__global__ void __launch_bounds__(NOISE_TILE) k_noise_evaluate(const NoiseEvaluate E) {
    const uint32_t p = blockIdx.x * NOISE_TILE + threadIdx.x;
    double sum = 0.0, mx = 0.0;
    unsigned long long above = 0, nonfinite = 0;
    if (p < E.pixels) {
        const double2 tq = E.tq[p];
        const double T = tq.x, Q = tq.y;
        const double m = T / E.N;
        const double ss = Q - (T * T) / E.N;
        const double var = (ss > 0.0 ? ss : 0.0) / E.km1;
        const double se = sqrt(var / E.N);
        const double err = se / ((m > 0.0 ? m : 0.0) + E.floor);
        const bool bad = !is_finite(T) || !is_finite(Q) || err != err;    // T or Q not finite; 0 / 0 (floor 0, neither signal nor variance)
        if (bad) nonfinite = 1;
        else { sum = err; mx = err; above = err > E.threshold ? 1 : 0; }
        if (E.out_error) E.out_error[p] = bad ? __uint_as_float(0x7FC00000u) : (float)err;
    }
    tile_reduce(sum, mx, above, nonfinite);
    if (threadIdx.x == 0u) {
        NoisePartial r; r.sum = sum; r.max = mx; r.above = above; r.nonfinite = nonfinite;
        E.partials[blockIdx.x] = r;
    }
}

__global__ void __launch_bounds__(NOISE_TILE) k_noise_finish(const NoiseFinish F) {
    double sum = 0.0, mx = 0.0;
    unsigned long long above = 0, nonfinite = 0;
    for (uint32_t i = threadIdx.x; i < F.n_tiles; i += NOISE_TILE) {
        const NoisePartial r = F.partials[i];
        sum = sum + r.sum;
        mx = r.max > mx ? r.max : mx;
        above += r.above; nonfinite += r.nonfinite;
    }
    tile_reduce(sum, mx, above, nonfinite);
    if (threadIdx.x == 0u) {
        const unsigned long long counted = (unsigned long long)F.pixels - nonfinite;
        mi355rt_noise_summary* o = F.out;
        o->chunks = F.chunks; o->samples = F.samples;
        o->pixels = F.pixels; o->above = above; o->nonfinite = nonfinite;
        o->max_error = mx;
        o->mean_error = counted ? sum / (double)counted : 0.0;
        o->converged = (F.chunks >= F.min_chunks && above <= F.allowed_above) ? 1u : 0u;
        o->_pad = 0u;
    }
}

}  // namespace mi355rt

using namespace mi355rt;

struct mi355rt_noise_device {
    int device = 0;
    uint32_t width = 0, rows = 0, pixels = 0, n_tiles = 0;
    uint32_t chunks = 0, samples = 0;                                 // K, N: advanced when a call has been enqueued
    float4* prev = nullptr; double2* tq = nullptr; NoisePartial* partials = nullptr;
    ~mi355rt_noise_device() { (void)hipFree(prev); (void)hipFree(tq); (void)hipFree(partials); }
};

namespace {
int refuse(const char* what) { return fail(MI355RT_ERR_INVALID, what); }
bool misaligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1u)) != 0u; }
int clear_state(mi355rt_noise_device* s, hipStream_t stream) {
    HIP_TRY(hipMemsetAsync(s->prev, 0, (size_t)s->pixels * sizeof(float4), stream));
    HIP_TRY(hipMemsetAsync(s->tq, 0, (size_t)s->pixels * sizeof(double2), stream));
    return MI355RT_OK;
}
}  // namespace

extern "C" {

int mi355rt_noise_device_create(int hip_device, uint32_t width, uint32_t rows, mi355rt_noise_device** out) {
    return guard([&]() -> int {
    if (!out) return refuse("noise_device_create: out is null");
    *out = nullptr;
    if (width == 0) return refuse("noise_device_create: width is 0");
    if (rows == 0) return refuse("noise_device_create: rows is 0");
    if ((uint64_t)width * rows >= (1ull << 31)) return refuse("noise_device_create: width * rows must be below 2^31");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(MI355RT_ERR_NO_DEVICE, "no HIP device visible (this library has no CPU path)");
    if (hip_device < 0 || hip_device >= n) return fail(MI355RT_ERR_NO_DEVICE, "hip_device out of range");
    HIP_TRY(hipSetDevice(hip_device));
    std::unique_ptr<mi355rt_noise_device> s(new mi355rt_noise_device());
    s->device = hip_device; s->width = width; s->rows = rows;
    s->pixels = width * rows; s->n_tiles = (s->pixels + NOISE_TILE - 1u) / NOISE_TILE;
    HIP_TRY(hipMalloc((void**)&s->prev, (size_t)s->pixels * sizeof(float4)));
    HIP_TRY(hipMalloc((void**)&s->tq, (size_t)s->pixels * sizeof(double2)));
    HIP_TRY(hipMalloc((void**)&s->partials, (size_t)s->n_tiles * sizeof(NoisePartial)));
    if (int rc = clear_state(s.get(), nullptr)) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    *out = s.release();
    return MI355RT_OK;
    });
}

void mi355rt_noise_device_destroy(mi355rt_noise_device* s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    delete s;
}

int mi355rt_noise_device_reset(mi355rt_noise_device* s, void* hip_stream) {
    return guard([&]() -> int {
    if (!s) return refuse("noise_device_reset: state is null");
    HIP_TRY(hipSetDevice(s->device));
    if (int rc = clear_state(s, (hipStream_t)hip_stream)) return rc;
    s->chunks = s->samples = 0;
    return MI355RT_OK;
    });
}

int mi355rt_noise_device_update(mi355rt_noise_device* s, const void* d_accum, uint32_t samples_total, void* hip_stream) {
    return guard([&]() -> int {
    if (!d_accum) return refuse("noise_device_update: d_accum is null");                  // (what does not need the state comes first)
    if (misaligned(d_accum, 16)) return refuse("noise_device_update: d_accum must be 16-byte aligned");
    if (!s) return refuse("noise_device_update: state is null");
    if (samples_total <= s->samples)
        return fail(MI355RT_ERR_INVALID, "noise_device_update: samples_total (" + std::to_string(samples_total) + ") must exceed the " +
                                         std::to_string(s->samples) + " samples already seen");
    HIP_TRY(hipSetDevice(s->device));
    NoiseUpdate u{};
    u.accum = static_cast<const float4*>(d_accum); u.prev = s->prev; u.tq = s->tq;
    u.n = (double)(samples_total - s->samples); u.pixels = s->pixels;
    hipLaunchKernelGGL(k_noise_update, dim3(s->n_tiles), dim3(NOISE_TILE), 0, (hipStream_t)hip_stream, u);
    HIP_TRY(hipGetLastError());
    s->chunks += 1; s->samples = samples_total;
    return MI355RT_OK;
    });
}

int mi355rt_noise_device_evaluate(mi355rt_noise_device* s, const mi355rt_noise_params* params_or_null, void* d_out_error_or_null, void* d_out_summary, void* hip_stream) {
    return guard([&]() -> int {
    if (!d_out_summary) return refuse("noise_device_evaluate: d_out_summary is null");
    if (misaligned(d_out_summary, 8)) return refuse("noise_device_evaluate: d_out_summary must be 8-byte aligned");
    if (misaligned(d_out_error_or_null, 4)) return refuse("noise_device_evaluate: d_out_error must be 4-byte aligned");
    mi355rt_noise_params pr = {0.02, 0.01, 4u, 0u, 0ull};
    if (params_or_null) pr = *params_or_null;
    if (!(pr.threshold > 0.0) || !std::isfinite(pr.threshold)) return refuse("noise_device_evaluate: params.threshold must be > 0 and finite");
    if (!(pr.floor >= 0.0) || !std::isfinite(pr.floor)) return refuse("noise_device_evaluate: params.floor must be >= 0 and finite");
    if (pr.min_chunks < 2) return refuse("noise_device_evaluate: params.min_chunks must be >= 2");
    if (pr._pad != 0) return refuse("noise_device_evaluate: params._pad must be 0");
    if (!s) return refuse("noise_device_evaluate: state is null");
    if (s->chunks < 2) return refuse("noise_device_evaluate: needs at least 2 chunks (mi355rt_noise_device_update calls)");
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t stream = (hipStream_t)hip_stream;
    NoiseEvaluate e{};
    e.tq = s->tq; e.out_error = static_cast<float*>(d_out_error_or_null); e.partials = s->partials;
    e.N = (double)s->samples; e.km1 = (double)(s->chunks - 1u); e.floor = pr.floor; e.threshold = pr.threshold; e.pixels = s->pixels;
    hipLaunchKernelGGL(k_noise_evaluate, dim3(s->n_tiles), dim3(NOISE_TILE), 0, stream, e);
    HIP_TRY(hipGetLastError());
    NoiseFinish f{};
    f.partials = s->partials; f.out = static_cast<mi355rt_noise_summary*>(d_out_summary); f.allowed_above = pr.allowed_above;
    f.n_tiles = s->n_tiles; f.pixels = s->pixels; f.chunks = s->chunks; f.samples = s->samples; f.min_chunks = pr.min_chunks;
    hipLaunchKernelGGL(k_noise_finish, dim3(1), dim3(NOISE_TILE), 0, stream, f);
    HIP_TRY(hipGetLastError());
    return MI355RT_OK;
    });
}

}  // extern "C"
