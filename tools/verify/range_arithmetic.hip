// The proofs behind rt_math.h's range arithmetic (k_render_ctr_simple_qc), run on the SHIPPED functions: this file includes the product's headers and is
// built with the product's flags.  Every claim is enumerated over its whole argument space and compared with the guarded form it replaces.
//   (a) recip_nofix(x) == 1.0f / x           for all 2^32 x that recip3_nofix's class test lets through (normal numbers, NaN) below the caller's bound 2^126;
//                                             it differs among those the test sends away (zeros, infinities, denormals): the reason for the test.
//       recip3_nofix(x, 1.5, -3) == 1.0f / x  for all those x and all it sends away (its ballot takes the compiler's reciprocals), with and without FIRST
//   (b) renorm_scale(renorm_t(x)) == recip_normal_range(length_for_normalize(x)), with a length of at least EPS, for every x of all 2^32 that passes
//       renorm_in_range(); the guard passes exactly the 3073 floats of [1 - 2^-13, 1 + 2^-13]
//   (c) length_ranged(x) == length_for_normalize(x) >= EPS and recip_nofix(l) == recip_normal_range(l) for every x that passes norm_in_range(); the test
//       passes exactly the floats of [NORM_LO, NORM_HI]
//       normalized_ranged / ray_direction with the range forms == the guarded forms on vectors (u, 0.75, -0.5) * s for all 2^32 u (every wave mixes
//       lanes in and out of range: a wave of 64 consecutive u crosses into NaN, infinities, zeros and tiny vectors somewhere in the enumeration)
//   (d) div_bounded_nofix(a, b) == a / b for the pairs of significands enumerated (argv[1] chunks of 2^17 b x all 2^23 a), and on a table of special
//       values the quad's CANDIDATE PREDICATE and every ACCEPTED t equal those of a / b (a raw value may differ where the predicate rejects the lane)
// usage: range_arithmetic [division chunks, default 2]     exit code 0 = every check passed
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include "../../raytracer-rust_amd/csrc/device/rt_math.h"
#include "../../raytracer-rust_amd/csrc/device/rt_rng.h"
#include "../../raytracer-rust_amd/csrc/device/rt_intersect.h"
#include "../../raytracer-rust_amd/csrc/device/rt_materials.h"
using namespace mi355rt;
__device__ bool same(float a, float b) { const uint32_t x = __float_as_uint(a), y = __float_as_uint(b); return x == y || (((x & 0x7FFFFFFFu) > 0x7F800000u) && ((y & 0x7FFFFFFFu) > 0x7F800000u)); }
__device__ bool same3(f3 a, f3 b) { return same(a.x, b.x) && same(a.y, b.y) && same(a.z, b.z); }
#define GRID_STRIDE_ALL(i) for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < (1ull << 32); i += (uint64_t)gridDim.x * blockDim.x)
// out[0]: recip_nofix differs where the class test lets x through and |x| < 2^126; out[1]: it differs among those sent away; out[2] / out[3]: recip3_nofix<false> / <true> differ
__global__ void k_recip(unsigned long long* out) {
    GRID_STRIDE_ALL(i) {
        const uint32_t u = (uint32_t)i, e = (u >> 23) & 0xFFu, m = u & 0x7FFFFFu;
        const float x = __uint_as_float(u), want = 1.0f / x;
        const bool away = e == 0u || (e == 255u && m == 0u);                 // zeros and denormals; infinities
        const bool bounded = e <= 252u || e == 255u;                         // |x| < 2^126 (hit_cube's BOUNDED), NaN, infinity
        if (!same(want, recip_nofix(x))) { if (away) atomicAdd(&out[1], 1ull); else if (bounded) atomicAdd(&out[0], 1ull); }
        if (bounded) {
            float ix, iy, iz; recip3_nofix<false>(x, 1.5f, -3.0f, ix, iy, iz);
            if (!same(want, ix) || !same(iy, 1.0f / 1.5f) || !same(iz, 1.0f / -3.0f)) atomicAdd(&out[2], 1ull);
            recip3_nofix<true>(-3.0f, x, 1.5f, ix, iy, iz);
            if (!same(want, iy) || !same(iz, 1.0f / 1.5f) || !same(ix, 1.0f / -3.0f)) atomicAdd(&out[3], 1ull);
        }
    }
}
// out[0]: x passing the guard; out[1]: closed form differs; out[2]: a float of [1 - 2^-13, 1 + 2^-13] that fails the guard
__global__ void k_renorm(unsigned long long* out) {
    unsigned long long passed = 0;
    GRID_STRIDE_ALL(i) {
        const float x = __uint_as_float((uint32_t)i), t = renorm_t(x);
        const bool inside = x >= 1.0f - 0x1p-13f && x <= 1.0f + 0x1p-13f;
        if (!renorm_in_range(t)) { if (inside) atomicAdd(&out[2], 1ull); continue; }
        ++passed;
        const float l = length_for_normalize(x);
        if (l < EPS || __float_as_uint(renorm_scale(t)) != __float_as_uint(recip_normal_range(l))) atomicAdd(&out[1], 1ull);
    }
    if (passed) atomicAdd(&out[0], passed);
}
// out[0]: x passing the range test; out[1]: l or r differ from the guarded forms, or l < EPS; out[2]: a float of [NORM_LO, NORM_HI] that fails the test
__global__ void k_norm(unsigned long long* out) {
    unsigned long long passed = 0;
    GRID_STRIDE_ALL(i) {
        const float x = __uint_as_float((uint32_t)i);
        const bool inside = x >= NORM_LO && x <= NORM_HI;
        if (!norm_in_range(x)) { if (inside) atomicAdd(&out[2], 1ull); continue; }
        ++passed;
        const float l = length_ranged(x), lg = length_for_normalize(x);
        if (l < EPS || __float_as_uint(l) != __float_as_uint(lg) || __float_as_uint(recip_nofix(l)) != __float_as_uint(recip_normal_range(lg))) atomicAdd(&out[1], 1ull);
    }
    if (passed) atomicAdd(&out[0], passed);
}
// out[0]: normalized_ranged differs from normalized<true>; out[1]: ray_direction with both range forms differs from the guarded one; out[2]: the closed form alone
__global__ void k_vectors(unsigned long long* out) {
    const float scales[4] = {1.0f, 0x1p-14f, 0x1p60f, 0.0f};                 // ordinary; below 1e-4 (passed through); len2 beyond NORM_HI; the zero vector and NaN (0 * inf)
    GRID_STRIDE_ALL(i) {
        const float u = __uint_as_float((uint32_t)i);
        for (float s : scales) {
            const f3 a = mk(u * s, 0.75f * s, -0.5f * s);
            if (!same3(normalized_ranged<true, RANGE_NORM_RANGED>(a), normalized<true>(a))) atomicAdd(&out[0], 1ull);
            const f3 want = ray_direction<true>(a);
            if (!same3(ray_direction<true, RANGE_NORM_RANGED | RANGE_RENORM_CLOSED>(a), want)) atomicAdd(&out[1], 1ull);
            if (!same3(ray_direction<true, RANGE_RENORM_CLOSED>(a), want)) atomicAdd(&out[2], 1ull);
        }
    }
}
__global__ void __launch_bounds__(256) k_div(unsigned long long* out, uint32_t b_base) {
    const float b = __uint_as_float(0x3F800000u | (b_base + blockIdx.x * blockDim.x + threadIdx.x));
    unsigned long long bad = 0;
    for (uint32_t am = 0; am < (1u << 23); ++am) { const float a = __uint_as_float(0x3F800000u | am); bad += __float_as_uint(a / b) != __float_as_uint(div_bounded_nofix(a, b)); }
    if (bad) atomicAdd(&out[0], bad);
}
// hit_quad's use of t, in a wave that is not wide (|num| < 2^100; anything else is a wide wave, whose t is the compiler's division): the predicate and the
// accepted t against a / b.  denom = dot(n, rd) of a finite normal and a direction that is finite or NaN: no infinite b.
// out[0]: predicate or accepted t differ; out[1]: raw values that differ (allowed: those lanes are rejected)
__global__ void k_div_specials(unsigned long long* out) {
    const float as[] = {0.0f, -0.0f, 0x1p-149f, -0x1p-149f, 0x1.fffffcp-127f, 0x1p-126f, 0x1p-101f, 0x1p-100f, -0x1p-100f, 0x1.fffffep99f, -0x1.fffffep99f, 1.0f, -3.0f, 1e-4f, 555.0f,
                        0x1p100f, __builtin_inff(), -__builtin_inff(), __builtin_nanf("")};
    const float bs[] = {0.0f, -0.0f, 0x1p-149f, -0x1.fffffcp-127f, 0x1p-126f, 0x1p-25f, -0x1p-25f, 0x1.a36e2cp-14f /* below EPS */, 1e-4f, -1e-4f, 0x1.a36e3p-14f /* above EPS */,
                        0.7071068f, 1.0f, -1.0f, 3.0f, 0x1.fffffep24f, __builtin_nanf("")};
    const float tmaxs[] = {__builtin_inff(), 1000.0f, 1.0f};
    for (float a : as) for (float b : bs) {
        const bool wide = !(fabsf(a) < 0x1p100f);
        const float want = a / b, got = wide ? a / b : div_bounded_nofix(a, b);
        if (!same(want, got)) atomicAdd(&out[1], 1ull);
        for (float tmax : tmaxs) {
            const bool cw = !(fabsf(b) < EPS) & !((want <= EPS) | (want >= tmax)), cg = !(fabsf(b) < EPS) & !((got <= EPS) | (got >= tmax));
            if (cw != cg || (cw && !same(want, got))) atomicAdd(&out[0], 1ull);
        }
    }
}
int main(int argc, char** argv) {
    const int chunks = argc > 1 ? atoi(argv[1]) : 2;
    unsigned long long* d; if (hipMalloc(&d, 64) != hipSuccess) { printf("no device\n"); return 2; }
    unsigned long long h[8]; int fails = 0;
    auto fetch = [&]() { if (hipDeviceSynchronize() != hipSuccess) { printf("device error\n"); exit(3); } hipMemcpy(h, d, 64, hipMemcpyDeviceToHost); hipMemset(d, 0, 64); };
    hipMemset(d, 0, 64);
    hipLaunchKernelGGL(k_recip, dim3(2048), dim3(256), 0, 0, d); fetch();
    printf("recip_nofix: %llu differences among the normal numbers below 2^126 and NaN (want 0), %llu among zeros, infinities and denormals (the reason for the class test)\n", h[0], h[1]);
    printf("recip3_nofix: %llu differences over all x below 2^126, zeros, infinities, NaN (want 0), %llu with FIRST (want 0)\n", h[2], h[3]); fails += h[0] != 0 || h[1] == 0 || h[2] != 0 || h[3] != 0;
    hipLaunchKernelGGL(k_renorm, dim3(2048), dim3(256), 0, 0, d); fetch();
    printf("renorm_scale: %llu of 2^32 x pass the guard (want 3073), %llu differences from the guarded form among them (want 0), %llu floats of [1 - 2^-13, 1 + 2^-13] refused (want 0)\n", h[0], h[1], h[2]);
    fails += h[0] != 3073ull || h[1] != 0 || h[2] != 0;
    hipLaunchKernelGGL(k_norm, dim3(2048), dim3(256), 0, 0, d); fetch();
    const unsigned long long in_range = 126ull * (1ull << 23) + 1ull;                                  // [2^-26, 2^100]: 126 binades and the upper end
    printf("normalized_ranged: %llu of 2^32 x pass the range test (want %llu), %llu differences in length or reciprocal among them (want 0), %llu floats of the range refused (want 0)\n", h[0], in_range, h[1], h[2]);
    fails += h[0] != in_range || h[1] != 0 || h[2] != 0;
    hipLaunchKernelGGL(k_vectors, dim3(2048), dim3(256), 0, 0, d); fetch();
    printf("vectors: %llu differences of normalized_ranged, %llu of ray_direction with both forms, %llu with the closed form alone, over 4 x 2^32 vectors (want 0 0 0)\n", h[0], h[1], h[2]);
    fails += h[0] != 0 || h[1] != 0 || h[2] != 0;
    for (int c = 0; c < chunks && c < 64; ++c) hipLaunchKernelGGL(k_div, dim3(512), dim3(256), 0, 0, d, (uint32_t)(c * (64 / (chunks < 64 ? chunks : 64))) << 17);
    fetch();
    printf("div_bounded_nofix: %llu differences over %d x 2^17 b significands x all 2^23 a significands (want 0)\n", h[0], chunks); fails += h[0] != 0;
    hipLaunchKernelGGL(k_div_specials, dim3(1), dim3(1), 0, 0, d); fetch();
    printf("div_bounded_nofix: %llu differences in the quad's predicate or accepted t on the specials table (want 0); %llu raw values differ on rejected lanes\n", h[0], h[1]); fails += h[0] != 0;
    printf(fails ? "FAILED\n" : "all checks passed\n");
    return fails ? 1 : 0;
}
