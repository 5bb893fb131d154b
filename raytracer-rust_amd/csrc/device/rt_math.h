// rt_math.h -- device prelude (DI, EPS, Prof) and the f32 vector helpers of vec3.rs / color.rs, operation for operation
// Part of the device code of libmi355rt.so; included by rt_kernels.hip only (one translation unit: every kernel sees the same
// inlined device functions, and build.kernel_hash() covers every file of this directory).
#pragma once
#include "rt_device.h"

namespace mi355rt {


#define DI __device__ __forceinline__

constexpr float EPS = 1e-4f;                      // renderer.rs:17
constexpr float PI_F = 3.14159265358979323846f;   // std::f32::consts::PI

typedef const __attribute__((address_space(4))) DevPrim* cprim_t;   // wave-uniform reads -> s_load

// Diagnostic-only cycle stamps (build with -DMI355RT_STAMPS into a separate library; the product build
// compiles Prof to nothing).  Shares of wave time per section, summed over waves, land in stats[2..].
#ifdef MI355RT_STAMPS
struct Prof {
    unsigned long long acc[6]; unsigned long long last;
    unsigned long long cls[10];     // lockstep kernels: per branch of the shading step {iterations in which any lane takes it, lanes that take it}:
                                   // 0 rough conductor, 1 Lambert-style bounce (Lambert, checker, texture, plastic), 2 metal / dielectric, 3 camera ray, 4 every iteration / live lanes
    DI void begin() { for (int i = 0; i < 6; ++i) acc[i] = 0; for (int i = 0; i < 10; ++i) cls[i] = 0; last = now(); }
    DI void classes(bool cont, bool fresh, uint32_t kind) {
        const unsigned long long m[5] = {__ballot(cont && (kind == 6u || kind == 7u)), __ballot(cont && (kind == 0u || kind == 1u || kind == 5u || kind == 9u)),
                                         __ballot(cont && (kind == 2u || kind == 3u)), __ballot(fresh), __ballot(cont || fresh)};
        for (int i = 0; i < 5; ++i) { cls[2 * i] += m[i] != 0ull; cls[2 * i + 1] += (unsigned long long)__popcll(m[i]); }
    }
    DI static unsigned long long now() {
        unsigned long long t; __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) :: "memory");
        __builtin_amdgcn_sched_barrier(0); return t;
    }
    DI void mark(int i) { unsigned long long t = now(); acc[i] += t - last; last = t; }
};
#else
struct Prof { DI void begin() {} DI void mark(int) {} DI void classes(bool, bool, uint32_t) {} };
#endif


// ---------------------------------------------------------------------------------------------------
// vec3.rs
// ---------------------------------------------------------------------------------------------------
struct f3 { float x, y, z; };
DI f3 mk(float x, float y, float z) { f3 r; r.x = x; r.y = y; r.z = z; return r; }
DI f3 operator+(f3 a, f3 b) { return mk(a.x + b.x, a.y + b.y, a.z + b.z); }
DI f3 operator-(f3 a, f3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
DI f3 operator*(f3 a, float s) { return mk(a.x * s, a.y * s, a.z * s); }
DI f3 operator*(f3 a, f3 b) { return mk(a.x * b.x, a.y * b.y, a.z * b.z); }     // Color * Color
DI f3 operator/(f3 a, f3 b) { return mk(a.x / b.x, a.y / b.y, a.z / b.z); }     // Color / Color
DI f3 operator-(f3 a) { return mk(-a.x, -a.y, -a.z); }
DI f3 divf(f3 a, float s) { return mk(a.x / s, a.y / s, a.z / s); }
DI float dot(f3 a, f3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }            // vec3.rs:17-19
DI f3 cross(f3 a, f3 b) { return mk(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }  // :21-27
DI float len2(f3 a) { return a.x * a.x + a.y * a.y + a.z * a.z; }                 // :29-31
DI float len(f3 a) { return sqrtf(len2(a)); }                                     // :33-35
// 1.0f / x for 2^-126 <= |x| < 2^126, +-inf and NaN: v_rcp_f32, one Newton step, v_div_fixup_f32.  Equal to the compiler's correctly
// rounded division for EVERY such x -- compared exhaustively over all 2^32 bit patterns on the MI355X (tools/microbench/recip.hip,
// profiles/r03_microbench_reciprocal.txt: the only inputs where the two differ are denormals and |x| >= 2^126, whose reciprocal is a
// denormal) -- at about half the issue slots (7.5 instead of 14.8).  For callers that can bound their argument.
DI float recip_normal_range(float x) {
    float r = __builtin_amdgcn_rcpf(x);
    const float e = __builtin_fmaf(-x, r, 1.0f);
    r = __builtin_fmaf(e, r, r);
    return __builtin_amdgcn_div_fixupf(r, x, 1.0f);
}
// (the length is a square root: at most sqrt(FLT_MAX) = 1.8e19 < 2^126 or +inf / NaN, and at least EPS here)
// FASTN: with length_for_normalize() and recip_normal_range().  Same bits either way; the kernels of mesh-free lists gain 2-3 % from it
// in their shading step, the wavefront kernels with the BVH walk LOSE 0.4-1.5 % there (fewer instructions, one more spilled
// register) and gain only in mesh_setup (profiles/r03_ab_short_reciprocal.txt) -- so it is a template argument set site by site.
// a / b by the exact reciprocal and ONE correction: r = RN(1/b) (above), q0 = a*r, e = fma(-b, q0, a), q = fma(e, r, q0), v_div_fixup_f32 for
// infinities / NaN / zeros.  Equal to the compiler's correctly rounded division for all 2^23 x 2^23 pairs of significands (enumerated on the
// MI355X in 43 s: tools/microbench/div.hip, profiles/r03_microbench_division.txt); rounding commutes with scaling by powers of two while
// everything stays normal, so it IS a / b whenever 2^-25 <= |b| <= 2^25 and (a == 0 or 2^-100 <= |a| <= 2^100) -- 11 + 1.5 issue slots
// instead of 18.5.  For callers that can bound their arguments (or guard them with a ballot) and do not use the result elsewhere.
DI float div_bounded(float a, float b) {
    float r = __builtin_amdgcn_rcpf(b);
    { const float e = __builtin_fmaf(-b, r, 1.0f); r = __builtin_fmaf(e, r, r); }
    float q = a * r;
    { const float e = __builtin_fmaf(-b, q, a); q = __builtin_fmaf(e, r, q); }
    return __builtin_amdgcn_div_fixupf(q, b, a);
}

// div_bounded() with the reciprocal handed in (r must be RN(1/b), e.g. the host's 1.0f / b): for a divisor that is the same for the whole
// launch the reciprocal and its Newton step are not even hoisted into vector registers -- b and r stay scalar operands.
DI float div_by_rn(float a, float b, float r) {
    float q = a * r;
    { const float e = __builtin_fmaf(-b, q, a); q = __builtin_fmaf(e, r, q); }
    return __builtin_amdgcn_div_fixupf(q, b, a);
}

// "This value is computed here": an empty statement the optimizer cannot see through.  For a short form that a rare wave-uniform branch overwrites --
// without it the compiler sinks the short form into an `else` of that branch, and the common path is laid out behind the rare one (a taken branch per test).
DI void keep_computed(float& v) { asm volatile("" : "+v"(v)); }

// 1 / x, 1 / y, 1 / z for ANY arguments: the short form where every lane of the wave has all three in its range (zero counts as
// in range: v_div_fixup_f32 returns the infinity of the right sign), the compiler's division for the whole wave otherwise -- a
// wave-uniform branch, so the common case pays three short reciprocals and a range test (two 3-input min / max on the magnitudes).
// NaN components are ignored by the test and give NaN either way.  (The ballot covers the lanes that are active at the call.)
// BOUNDED (k_render_ctr_simple_qc's cube test): for callers that know every magnitude to be below 2^126 or NaN.  What is then left outside the short
// form's range is a denormal, and one v_cmp_class_f32 per component finds it.  A wave with a denormal lane takes the compiler's reciprocals, which the
// compiler lays out of line: the common path falls through the test into the short form.
// FIRST (the kernel compiled without the sky lookup): keep_computed() on the three short results, so that they run first, in front of the test, and a
// wave with a denormal overwrites them.  With the sky lookup's scalar registers in the loop this form had 13 SGPR spills instead of 6; without them none.
template <bool FASTR, bool BOUNDED = false, bool FIRST = false>
DI void recip3(float x, float y, float z, float& ix, float& iy, float& iz) {
    if constexpr (FASTR && BOUNDED) {
        constexpr int DENORMAL = 0x010 | 0x080;                                             // v_cmp_class_f32: negative denormal, positive denormal
        ix = recip_normal_range(x); iy = recip_normal_range(y); iz = recip_normal_range(z);
        if constexpr (FIRST) { keep_computed(ix); keep_computed(iy); keep_computed(iz); }
        // (__builtin_isfpclass, not __builtin_amdgcn_class: this compiler folds the latter's denormal classes to `false`; both select v_cmp_class_f32)
        const bool small = __builtin_isfpclass(x, DENORMAL) | __builtin_isfpclass(y, DENORMAL) | __builtin_isfpclass(z, DENORMAL);
        if (__builtin_expect(__ballot(small) != 0ull, 0)) { ix = 1.0f / x; iy = 1.0f / y; iz = 1.0f / z; }
        return;
    }
    if constexpr (FASTR) {
    const float ax = fabsf(x), ay = fabsf(y), az = fabsf(z);
    const float mx = fmaxf(fmaxf(ax, ay), az);
    const float mn = fminf(fminf(ax == 0.0f ? 1.0f : ax, ay == 0.0f ? 1.0f : ay), az == 0.0f ? 1.0f : az);
    if (__ballot((mn < 0x1p-126f) || (mx >= 0x1p126f)) == 0ull) { ix = recip_normal_range(x); iy = recip_normal_range(y); iz = recip_normal_range(z); return; }
    }
    ix = 1.0f / x; iy = 1.0f / y; iz = 1.0f / z;
}

// The length normalized() needs: bit-equal to sqrtf(x) for every x >= 2^-100, +inf and NaN; for 0 <= x < 2^-100 (a length below
// 1e-15) it returns 0, which normalized() treats like the true value -- both are below its 1e-4 pass-through threshold.  v_rsq_f32 +
// one residual correction instead of the compiler's expansion (denormal scaling, v_sqrt_f32, both neighbours tested): 9 instead of 17
// issue slots.  The contract was checked for EVERY x >= +0 and every NaN on the MI355X (tools/microbench/sqrt.hip, k_contract:
// 0 violations; profiles/r03_microbench_sqrt.txt).  x is a sum of squares here: never negative, never -0.
DI float length_for_normalize(float x) {
    const float y = __builtin_amdgcn_rsqf(x);
    const float g = x * y, h = 0.5f * y;
    const float d = __builtin_fmaf(-g, g, x);
    float s = __builtin_fmaf(d, h, g);
    s = (x < 0x1p-100f) ? 0.0f : s;
    return (x == __builtin_inff()) ? x : s;
}
template <bool FASTN = false>
DI f3 normalized(f3 a) {                                                          // :37-44
    if constexpr (FASTN) { const float l = length_for_normalize(len2(a)); if (l < EPS) return a; return a * recip_normal_range(l); }
    const float l = len(a); if (l < EPS) return a; return a * (FASTN ? recip_normal_range(l) : 1.0f / l);
}

// ---------------------------------------------------------------------------------------------------
// Range arithmetic (k_render_ctr_simple_qc only): the short forms above, without the work that only serves operands outside the range the kernel's
// values lie in.  Each form tests the range it is proven on -- one comparison and a ballot -- and a wave with a lane outside it takes the form above,
// out of line; so any operand still gives the bits it gave before.  tools/verify/range_arithmetic.hip enumerates every claim on these functions.
// RANGE (a template argument of ray_direction, diffuse_finish, hit_quad, hit_cube, recip3 and what passes it down; 0 everywhere else, which folds to the
// code as it was): one bit per step, each with a build define, MI355RT_QC_*, whose 0 builds the form before it (build.RANGE_OFF_DEFINES: all four).
//   RANGE_RENORM_CLOSED  ray_direction's second normalisation as a closed form of len2 (renorm_scale)
//   RANGE_NORM_RANGED    the first normalisation of a bounded vector without guards, pass-through selects and fix-up (normalized_ranged)
//   RANGE_QUAD_NOFIX     the quad's t without v_div_fixup_f32 (div_bounded_nofix)
//   RANGE_CUBE_NOFIX     the cube's three reciprocals without v_div_fixup_f32 (recip_nofix; recip3's class test also looks for zeros and infinities)
// The first and the last ship at 1.  RANGE_NORM_RANGED measures faster and stays at 0 because it changes the kernel's scalar spill figures, which
// tests/test_nosky_budget.py and tests/test_empty_pass_isa.py pin by equality; RANGE_QUAD_NOFIX stays at 0 because its gain was inside three times
// the spread.  What each measured: DESIGN.md 4.1 "Range arithmetic", profiles/bench_range_arithmetic_vs_parent.txt.
// ---------------------------------------------------------------------------------------------------
#ifndef MI355RT_QC_RENORM_CLOSED
#define MI355RT_QC_RENORM_CLOSED 1
#endif
#ifndef MI355RT_QC_NORM_RANGED
#define MI355RT_QC_NORM_RANGED 0                             // measured faster, not shipped: it moves the spill figures that existing tests pin (DESIGN.md 4.1 "Range arithmetic")
#endif
#ifndef MI355RT_QC_QUAD_NOFIX
#define MI355RT_QC_QUAD_NOFIX 0                              // inside the noise on top of step 1 (2.7 times the spread where the rule asks for 3): DESIGN.md 4.1
#endif
#ifndef MI355RT_QC_CUBE_NOFIX
#define MI355RT_QC_CUBE_NOFIX 1
#endif
enum : uint32_t { RANGE_RENORM_CLOSED = 1u, RANGE_NORM_RANGED = 2u, RANGE_QUAD_NOFIX = 4u, RANGE_CUBE_NOFIX = 8u };
#define MI355RT_QC_RANGE ((MI355RT_QC_RENORM_CLOSED != 0 ? RANGE_RENORM_CLOSED : 0u) | (MI355RT_QC_NORM_RANGED != 0 ? RANGE_NORM_RANGED : 0u) | (MI355RT_QC_QUAD_NOFIX != 0 ? RANGE_QUAD_NOFIX : 0u) | (MI355RT_QC_CUBE_NOFIX != 0 ? RANGE_CUBE_NOFIX : 0u))

// recip_normal_range() without its fix-up.  For a finite non-zero x whose reciprocal is a normal number v_div_fixup_f32(r, x, 1) returns |r| with the
// sign of x * 1, which is r: equal to 1.0f / x for every normal x below 2^126 in magnitude, and NaN for NaN.  What the fix-up served are zeros,
// infinities and denormals (x = 0: v_rcp gives inf, the Newton step inf * 0 = NaN): the caller keeps those out.
DI float recip_nofix(float x) {
    const float r = __builtin_amdgcn_rcpf(x);
    const float e = __builtin_fmaf(-x, r, 1.0f);
    return __builtin_fmaf(e, r, r);
}
// recip3<true, BOUNDED, FIRST> with recip_nofix(): the class test that sends a wave to the compiler's reciprocals looks for zeros and infinities beside
// the denormals -- the same v_cmp_class_f32 per component with a wider mask.  What it lets through is a normal number, below 2^126 by the caller's
// bound (hit_cube), or NaN.
template <bool FIRST = false>
DI void recip3_nofix(float x, float y, float z, float& ix, float& iy, float& iz) {
    constexpr int AWAY = 0x010 | 0x080 | 0x020 | 0x040 | 0x004 | 0x200;                     // v_cmp_class_f32: -denormal, +denormal, -0, +0, -inf, +inf
    ix = recip_nofix(x); iy = recip_nofix(y); iz = recip_nofix(z);
    if constexpr (FIRST) { keep_computed(ix); keep_computed(iy); keep_computed(iz); }
    const bool away = __builtin_isfpclass(x, AWAY) | __builtin_isfpclass(y, AWAY) | __builtin_isfpclass(z, AWAY);
    if (__builtin_expect(__ballot(away) != 0ull, 0)) { ix = 1.0f / x; iy = 1.0f / y; iz = 1.0f / z; }
}
// div_bounded() without its fix-up: the same q. For finite non-zero a and b whose quotient is a normal number the fix-up returns |q| with the sign of
// a * b, which is q -- so inside div_bounded()'s proven range (2^-25 <= |b| <= 2^25, 2^-100 <= |a| <= 2^100) this IS a / b.  Outside it: a == 0 gives
// a zero (q0 = 0 * r, e = 0, q = 0 -- possibly of the other sign than a / b's); b zero, denormal (v_rcp flushes it: r = inf) or NaN gives NaN or an
// infinity; an infinite a gives an infinity or NaN.  hit_quad's comment says why none of those lanes is accepted either way.
DI float div_bounded_nofix(float a, float b) {
    float r = __builtin_amdgcn_rcpf(b);
    { const float e = __builtin_fmaf(-b, r, 1.0f); r = __builtin_fmaf(e, r, r); }
    const float q = a * r;
    const float e = __builtin_fmaf(-b, q, a);
    return __builtin_fmaf(e, r, q);
}
// The second normalisation of ray_direction().  Its input went through normalized() once, so x = len2 is one of a handful of floats next to 1 (over
// 20 M random directions: 11 values within 1 +- 7 * 2^-24), and there RN(1 / RN(sqrt(x))) is a step function of x:
//   r = 1 - 2^-23 * floor((x - 1) * 2^22).
// (The square root halves the distance to 1 and the reciprocal mirrors it, each rounded to the float grid, which is 2^-23 wide above 1 and 2^-24 below.)
// The proof is an enumeration: the closed form equals recip_normal_range(length_for_normalize(x)) for every float x with |x - 1| <= 2^-13
// (tests/test_range_closed_form.py with numpy's correctly rounded sqrt and division; tools/verify/range_arithmetic.hip on the shipped functions, all 2^32 x).
// Every operation is exact: t = fma(x, 2^22, -2^22) = (x - 1) * 2^22 has at most 24 significant bits, floor(t) is an integer of magnitude at most 512,
// and 1 - floor(t) * 2^-23 is a float.  The guard |t| <= 512, that is |x - 1| <= 2^-13, is false for NaN and for a vector that normalized() passed
// through (a length below 1e-4: t = -2^22).
// (t as v_ldexp_f32 and an add of the literal -2^22, both exact: as one fma the two constants 2^22 and -2^22 cost a v_mov_b32 -- VOP3 takes no literal.)
DI float renorm_t(float x) { return __builtin_ldexpf(x, 22) - 0x1p22f; }
DI bool renorm_in_range(float t) { return fabsf(t) <= 512.0f; }
DI float renorm_scale(float t) { return __builtin_fmaf(-0x1p-23f, __builtin_floorf(t), 1.0f); }
// The first normalisation for a vector of bounded length: the unit-ball point (x = len2 < 1), n + unit (x <= 4 and rounding), a camera direction.
// One two-sided test of x -- med3(x, lo, hi) == x, false for NaN -- and inside it the straight line: v_rsq_f32 with its correction, v_rcp_f32 with its
// Newton step, three multiplies.  NORM_LO = 2^-26 > EPS^2 (1e-8 < 1.4902e-8): for x >= 2^-26 the length RN(sqrt(x)) is at least 2^-13 = 1.2207e-4 > EPS
// (sqrt is monotonic and exact at 2^-26), so normalized()'s pass-through `l < EPS` is false and its selects choose the scaled vector; x >= 2^-100 and
// x != inf, so length_for_normalize()'s two guards choose `s`.  NORM_HI = 2^100: the length is a normal number in [2^-13, 2^50], far below 2^126, and
// its reciprocal a normal number in [2^-50, 2^13], on which the fix-up is the identity (recip_nofix).  So for lo <= x <= hi, l and r are the values
// normalized<true>() computes, bit for bit (enumerated for every such x: tools/verify/range_arithmetic.hip).
constexpr float NORM_LO = 0x1p-26f, NORM_HI = 0x1p100f;
DI bool norm_in_range(float x) { return __builtin_amdgcn_fmed3f(x, NORM_LO, NORM_HI) == x; }
DI float length_ranged(float x) {
    const float y = __builtin_amdgcn_rsqf(x);
    const float g = x * y, h = 0.5f * y;
    const float d = __builtin_fmaf(-g, g, x);
    return __builtin_fmaf(d, h, g);
}
// A wave with a lane outside the range (a zero vector, one below 1e-4, NaN, an infinity, an idle lane's leftovers) takes normalized<true>() for all
// lanes, out of line: the short scale is computed first (keep_computed) and overwritten there, as recip3<BOUNDED> does.  Only the SCALE is merged, one
// register: normalized<true>() is a * normalize_scale(len2(a)), its pass-through a * 1.0f -- the same bits as `a` for every float (f32 denormals are
// not flushed in these kernels; tools/verify/range_arithmetic.hip runs tiny and denormal vectors through both).
DI float normalize_scale(float x) { const float l = length_for_normalize(x); return (l < EPS) ? 1.0f : recip_normal_range(l); }
template <bool FASTN = false, uint32_t RANGE = 0u>
DI f3 normalized_ranged(f3 a) {
    if constexpr (FASTN && (RANGE & RANGE_NORM_RANGED) != 0u) {
        const float x = len2(a);
        float r = recip_nofix(length_ranged(x));
        keep_computed(r);
        if (__builtin_expect(__ballot(!norm_in_range(x)) != 0ull, 0)) r = normalize_scale(x);
        return a * r;
    } else return normalized<FASTN>(a);
}
DI bool near_zero(f3 a) { const float S = 1e-8f; return fabsf(a.x) < S && fabsf(a.y) < S && fabsf(a.z) < S; }  // :63-66
DI bool has_nan(f3 a) { return (a.x != a.x) || (a.y != a.y) || (a.z != a.z); }
DI bool is_zero(f3 a) { return a.x == 0.0f && a.y == 0.0f && a.z == 0.0f; }
DI f3 nan3() { float n = __builtin_nanf(""); return mk(n, n, n); }
DI f3 splat(float v) { return mk(v, v, v); }
DI f3 sqrt3(f3 a) { return mk(sqrtf(a.x), sqrtf(a.y), sqrtf(a.z)); }
DI f3 to_world(f3 local, f3 normal) {                                             // vec3.rs:72-81
    f3 up = (fabsf(normal.z) < 0.999f) ? mk(0.f, 0.f, 1.f) : mk(0.f, 1.f, 0.f);
    f3 tangent = normalized(cross(normal, up));
    f3 bitangent = cross(normal, tangent);
    return (tangent * local.x + bitangent * local.y) + normal * local.z;
}
DI float clamp01(float v) { if (v < 0.0f) return 0.0f; if (v > 1.0f) return 1.0f; return v; }   // f32::clamp, NaN stays
DI uint32_t as_u32_sat(float v) {                                                 // Rust `as u32`
    if (!(v == v) || v <= 0.0f) return 0u;
    if (v >= 4294967296.0f) return 0xFFFFFFFFu;
    return (uint32_t)v;
}
DI int32_t as_i32_sat(float v) {                                                  // Rust `as i32`
    if (!(v == v)) return 0;
    if (v <= -2147483648.0f) return (int32_t)0x80000000;
    if (v >= 2147483648.0f) return 0x7FFFFFFF;
    return (int32_t)v;
}
DI uint32_t color_to_u32(f3 c) {                                                  // color.rs:87-93
    c.x = clamp01(c.x); c.y = clamp01(c.y); c.z = clamp01(c.z);
    return (as_u32_sat(c.x * 255.0f) << 16) | (as_u32_sat(c.y * 255.0f) << 8) | as_u32_sat(c.z * 255.0f);
}


}  // namespace mi355rt
