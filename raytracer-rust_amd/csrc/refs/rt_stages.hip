// rt_stages.hip -- the transcendental stages of the render path over enumerated inputs.  Compiled into the tests' reference build only
// (build.build_device_variant("refs"), -DMI355RT_REFS): the product library and its kernel hash do not contain it.
//
// mi355rt_debug_stages runs one stage on n elements.  Element i takes the index k = first + i * stride and makes its input from k by the
// rules below, which the oracle's oracle_debug_stages (oracle/rt_oracle.cpp) states word for word -- or it reads 4 explicit floats.  Only
// the results cross PCIe.  The stages call the shipped device functions of csrc/device as the render kernels call them:
//   LATTICE  ln(u1), theta_arg, theta = atan(sqrt(theta_arg)), sin / cos theta, sin / cos phi, phi of the rough conductor's sampling, both
//            forms (counter mode: the native f32 functions; reference-stream mode: double, rounded once) -- restated from scatter_pre, whose
//            lambdas are not reachable from outside; HALF below checks the shipped branch itself
//   HALF     the whole rough-conductor branch of scatter_pre<MATS_ALL>, driven by the real generators (RngCtr / RngRef) loaded with the words
//            that make the branch's two draws (u1, u2): raw direction, attenuation, the returned bool, and a signature of LATTICE's words
//   ACOS, ATAN2   acosf / atan2f as texture_lookup and miss_colour call them
//   TEX      texture_lookup on an RGBA8 texture whose texels encode their own (x, y); SKY: miss_colour on a sky whose floats are their index
//   ATAN2_EXACT, FMOD_EXACT   the structured atan2f sets with closed-form answers and fmodf(u + h, 1) against a - floorf(a), checked here
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "../device/rt_device.h"
#include "../device/rt_host.h"
#include "../device/rt_math.h"
#include "../device/rt_rng.h"
#include "../device/rt_intersect.h"
#include "../device/rt_materials.h"

namespace mi355rt {

enum : uint32_t { STAGE_LATTICE = 0, STAGE_HALF = 1, STAGE_ACOS = 2, STAGE_ATAN2 = 3, STAGE_TEX = 4, STAGE_SKY = 5, STAGE_ATAN2_EXACT = 6,
                  STAGE_FMOD_EXACT = 7, STAGE_COUNT = 8 };
constexpr uint64_t STAGE_ACOS_POS = 0x3F800009u;     // the non-negative floats up to 1 + 2^-20: ACOS index k < this is +bits(k), then -bits(k - this)
struct StageArgs {                                    // 96 B; the oracle's StageArgs and device.StageArgs have the same layout
    uint32_t stage, form;                             // form 0: counter mode, 1: reference-stream mode
    uint64_t first, stride;
    uint32_t ggx, axis, set, img_w;                   // HALF: rough-conductor kind, 0 = u1 runs over the lattice (u2 = fixed_u), 1 = u2 runs (u1 = fixed_u);
    uint32_t img_h, pad0;                             // ATAN2_EXACT: the set (0..7); TEX / SKY: image size
    float rough, fixed_u, h_offset, pad1;
    float n[4], rd[4];                                // HALF: the hit normal and the incoming direction
};
static_assert(sizeof(StageArgs) == 96, "StageArgs");
// Words per element of a stage's output; the exact stages write 3 words per call: mismatches, the smallest mismatching index, and (the
// diagonal sets of ATAN2_EXACT, 4..7) results one f32 step from the closed form, which are counted apart instead of as mismatches.
constexpr uint32_t stage_words(uint32_t stage) { return (stage == STAGE_ACOS || stage == STAGE_ATAN2) ? 1u : (stage >= STAGE_ATAN2_EXACT ? 0u : 8u); }

DI float stage_lattice_u(uint64_t k) { return u32_to_f01((uint32_t)k << 8); }          // k * 2^-24 for k < 2^24: every value u32_to_f01 has
DI float stage_acos_arg(uint64_t k) {
    return __uint_as_float(k < STAGE_ACOS_POS ? (uint32_t)k : 0x80000000u | (uint32_t)(k - STAGE_ACOS_POS));
}
DI f3 stage_dir(uint64_t k) {                                                           // a direction in [-1, 1)^3, pcg4d of the index
    uint32_t b[4];
    pcg4d((uint32_t)k, (uint32_t)(k >> 32), 0x9E3779B9u, 0x7F4A7C15u, b);
    return mk(u32_to_range11(b[0]), u32_to_range11(b[1]), u32_to_range11(b[2]));
}

// scatter_pre's rough-conductor sampling (rt_materials.h), in the form EXACT selects
template <bool EXACT> DI void stage_transcendentals(float u1_drawn, float u2, bool ggx, float rough, float (&o)[8]) {
    const float u1 = fmaxf(u1_drawn, 1e-6f);
    const float l = EXACT ? (float)log((double)u1) : logf(u1);
    float theta_arg;
    if (ggx) { float a = rough * rough; theta_arg = a * a * (-l) / (1.0f - u1); }
    else { theta_arg = -(rough * rough * l); }
    const float theta = EXACT ? (float)atan((double)sqrtf(theta_arg)) : atanf(sqrtf(theta_arg));
    const float phi = 2.0f * PI_F * u2;
    float st, ct, sp, cp;
    if (EXACT) { st = (float)sin((double)theta); ct = (float)cos((double)theta); sp = (float)sin((double)phi); cp = (float)cos((double)phi); }
    else { sincosf(theta, &st, &ct); sincosf(phi, &sp, &cp); }
    o[0] = l; o[1] = theta_arg; o[2] = theta; o[3] = st; o[4] = ct; o[5] = sp; o[6] = cp; o[7] = phi;
}
DI uint32_t stage_signature(const float (&t)[8]) {                                      // FNV-1a over the 8 words, every NaN as one word
    uint32_t h = 0x811C9DC5u;
    for (int w = 0; w < 8; ++w) h = (h ^ (t[w] != t[w] ? 0x7FC00000u : __float_as_uint(t[w]))) * 16777619u;
    return h;
}

// The shipped rough-conductor branch.  The generator of the form is loaded so that its two draws are (u1, u2): u32_to_f01 of the words
// (k << 8) gives back k * 2^-24, and every draw the renderer can make is such a value.
// (The generators are used as they are: the branch picks its libm form by the generator's type, so a wrapper type would take the other form.)
template <bool EXACT, class Rng> DI void stage_half(const StageArgs& A, const DevMat* __restrict__ mat, Rng& rng, float u1, float u2, uint32_t (&o)[8]) {
    Hit h;
    h.t = 1.0f; h.p = mk(0.f, 0.f, 0.f); h.n = mk(A.n[0], A.n[1], A.n[2]); h.mat_ff = 0x80000000u;
    const float4 q0 = reinterpret_cast<const float4*>(mat)[0];
    h.q0 = q0;
    float side = EPS, fuzz = 0.f;
    uint32_t ball = BALL_NONE;
    f3 raw = mk(0.f, 0.f, 0.f), atten = mk(0.f, 0.f, 0.f), emitted = mk(0.f, 0.f, 0.f);
    const bool ok = scatter_pre<MATS_ALL>(mat, nullptr, q0, h, mk(A.rd[0], A.rd[1], A.rd[2]), rng, side, raw, atten, emitted, ball, fuzz);
    float t[8];
    stage_transcendentals<EXACT>(u1, u2, A.ggx != 0u, A.rough, t);
    if (!ok) { raw = mk(0.f, 0.f, 0.f); atten = mk(0.f, 0.f, 0.f); }
    o[0] = __float_as_uint(raw.x); o[1] = __float_as_uint(raw.y); o[2] = __float_as_uint(raw.z);
    o[3] = __float_as_uint(atten.x); o[4] = __float_as_uint(atten.y); o[5] = __float_as_uint(atten.z);
    o[6] = __float_as_uint(ok ? 1.0f : 0.0f); o[7] = stage_signature(t);
}

__global__ void __launch_bounds__(256) k_debug_stages(const StageArgs A, const float* __restrict__ in, const DevMat* __restrict__ mat,
                                                      const DevTexture* __restrict__ tex, const float* __restrict__ sky, uint32_t* __restrict__ out,
                                                      uint64_t n) {
    const uint32_t W = stage_words(A.stage);
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t k = A.first + i * A.stride;
        const float4 e = in ? reinterpret_cast<const float4*>(in)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        uint32_t o[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
        if (A.stage == STAGE_LATTICE) {
            const float u = in ? e.x : stage_lattice_u(k);
            float t[8];
            if (A.form) stage_transcendentals<true>(u, u, A.ggx != 0u, A.rough, t);
            else stage_transcendentals<false>(u, u, A.ggx != 0u, A.rough, t);
            for (int w = 0; w < 8; ++w) o[w] = __float_as_uint(t[w]);
        } else if (A.stage == STAGE_HALF) {
            const uint32_t run = (uint32_t)k << 8, fixed = (uint32_t)(A.fixed_u * 16777216.0f) << 8;   // lattice values (the entry checks)
            uint32_t w1 = A.axis == 0u ? run : fixed, w2 = A.axis == 0u ? fixed : run;
            if (in) { w1 = (uint32_t)(e.x * 16777216.0f) << 8; w2 = (uint32_t)(e.y * 16777216.0f) << 8; }
            const float u1 = u32_to_f01(w1), u2 = u32_to_f01(w2);
            if (A.form) {
                RngRef rng;
                rng.idx = 0u; rng.buf[0] = w1; rng.buf[1] = w2;
                stage_half<true>(A, mat, rng, u1, u2, o);
            } else {
                RngCtr rng;
                rng.clear(); rng.b0[0] = w1; rng.b0[1] = w2;
                stage_half<false>(A, mat, rng, u1, u2, o);
            }
        } else if (A.stage == STAGE_ACOS) {
            o[0] = __float_as_uint(acosf(in ? e.x : stage_acos_arg(k)));
        } else if (A.stage == STAGE_ATAN2) {
            const f3 d = in ? mk(e.x, e.y, e.z) : stage_dir(k);
            o[0] = __float_as_uint(atan2f(d.z, d.x));
        } else if (A.stage == STAGE_TEX) {
            const f3 nn = in ? mk(e.x, e.y, e.z) : normalized(stage_dir(k));
            const f3 c = texture_lookup(tex, 0u, A.h_offset, nn);
            const float phi = atan2f(nn.z, nn.x);
            o[0] = __float_as_uint(c.x); o[1] = __float_as_uint(c.y); o[2] = __float_as_uint(c.z);
            o[3] = __float_as_uint(acosf(nn.y)); o[4] = __float_as_uint(phi);
            o[5] = __float_as_uint(fmodf((phi + PI_F) / (2.0f * PI_F) + A.h_offset, 1.0f));
        } else if (A.stage == STAGE_SKY) {
            const f3 rd = in ? mk(e.x, e.y, e.z) : stage_dir(k);
            const float miss[3] = {0.f, 0.f, 0.f};
            const f3 c = miss_colour(sky, A.img_w, A.img_h, miss, rd);
            const f3 d = normalized(rd);
            o[0] = __float_as_uint(c.x); o[1] = __float_as_uint(c.y); o[2] = __float_as_uint(c.z);
            o[3] = __float_as_uint(acosf(d.y)); o[4] = __float_as_uint(atan2f(d.z, d.x));
        }
        for (uint32_t w = 0; w < W; ++w) out[i * W + w] = o[w];
    }
}

// atan2f's closed-form answers on the structured sets (each rounded to f32): atan2(+-0, x) = +-0 for x > 0 or x = +0, +-pi for x < 0 or
// x = -0; atan2(z, +-0) = +-pi/2 for z != 0; |z| = |x| != 0: +-pi/4 for x > 0, +-3pi/4 for x < 0 -- the sign is z's.
DI float stage_atan2_expected(float z, float x) {
    if (z == 0.0f) return copysignf(signbit(x) ? PI_F : 0.0f, z);
    if (x == 0.0f) return copysignf(__uint_as_float(0x3FC90FDBu), z);
    return copysignf(x > 0.0f ? __uint_as_float(0x3F490FDBu) : __uint_as_float(0x4016CBE4u), z);
}
// Set 0 / 1: z = +0 / -0, x = bits(k); 2 / 3: x = +0 / -0, z = bits(k); 4..7: |z| = |x| = bits(k) (k < 2^31), z negative in 6, 7, x in 5, 7.
DI void stage_atan2_input(uint32_t set, uint64_t k, float& z, float& x) {
    const float v = __uint_as_float((uint32_t)k);
    if (set == 0u) { z = 0.0f; x = v; }
    else if (set == 1u) { z = -0.0f; x = v; }
    else if (set == 2u) { x = 0.0f; z = v; }
    else if (set == 3u) { x = -0.0f; z = v; }
    else { const float m = fabsf(v); z = (set & 2u) ? -m : m; x = (set & 1u) ? -m : m; }
}
__global__ void __launch_bounds__(256) k_debug_stages_exact(const StageArgs A, uint32_t* __restrict__ out, uint64_t n) {
    uint32_t bad = 0u, which = 0xFFFFFFFFu, near = 0u;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t k = A.first + i * A.stride;
        float got, want;
        if (A.stage == STAGE_ATAN2_EXACT) {
            float z, x;
            stage_atan2_input(A.set, k, z, x);
            if (!isfinite(z) || !isfinite(x)) continue;
            got = atan2f(z, x); want = stage_atan2_expected(z, x);
        } else {                                                                         // FMOD_EXACT: u = bits(k) in [0, 1]
            const float a = __uint_as_float((uint32_t)k) + A.h_offset;
            got = fmodf(a, 1.0f); want = a - floorf(a);
        }
        const uint32_t g = __float_as_uint(got), w = __float_as_uint(want);
        if (g == w) continue;
        if (A.stage == STAGE_ATAN2_EXACT && A.set >= 4u && (g ^ w) < 0x80000000u && (g > w ? g - w : w - g) == 1u) { ++near; continue; }   // the diagonal: 1 step
        ++bad; which = min(which, (uint32_t)k);
    }
    if (bad) { atomicAdd(&out[0], bad); atomicMin(&out[1], which); }
    if (near) atomicAdd(&out[2], near);
}

}  // namespace mi355rt

using namespace mi355rt;

// Not in the public header; the reference build's diagnostic entry.  Host pointers: args = one StageArgs; in4 = 4 floats per element or
// null; mat = one mi355rt_material (HALF); tex_rgba = img_w * img_h texels (TEX); sky = img_w * img_h * 3 floats (SKY); out = stage_words()
// words per element, or 3 words for the exact stages (mismatches; the smallest mismatching index, 0xFFFFFFFF if none; one-step results).  Synchronous; every buffer is freed before it returns.
extern "C" int mi355rt_debug_stages(const void* args, uint64_t n, const float* in4, const void* mat, const uint32_t* tex_rgba, const float* sky,
                                    uint32_t* out, int device) {
    return guard([&]() -> int {
    if (!args || !out) return fail(MI355RT_ERR_INVALID, "debug_stages: null");
    const StageArgs a = *static_cast<const StageArgs*>(args);
    if (a.stage >= STAGE_COUNT || a.stride == 0) return fail(MI355RT_ERR_INVALID, "debug_stages: stage / stride");
    if (a.stage == STAGE_HALF && (!mat || (!in4 && (a.first + (n ? n - 1 : 0) * a.stride >= (1ull << 24)))))
        return fail(MI355RT_ERR_INVALID, "debug_stages: HALF needs a material and lattice indices < 2^24");
    if (a.stage == STAGE_HALF && !(a.fixed_u >= 0.0f && a.fixed_u < 1.0f && (float)(uint32_t)(a.fixed_u * 16777216.0f) == a.fixed_u * 16777216.0f))
        return fail(MI355RT_ERR_INVALID, "debug_stages: fixed_u must be k * 2^-24");
    if ((a.stage == STAGE_TEX && (!tex_rgba || !a.img_w || !a.img_h || a.img_w > 256u || a.img_h > 256u)) ||
        (a.stage == STAGE_SKY && (!sky || !a.img_w || !a.img_h)))
        return fail(MI355RT_ERR_INVALID, "debug_stages: image");
    HIP_TRY(hipSetDevice(device));
    const uint32_t W = stage_words(a.stage);
    const size_t out_words = W ? (size_t)n * W : 3u;
    const size_t texels = (size_t)a.img_w * a.img_h;
    DevBuf<uint32_t> d_out; DevBuf<float> d_in, d_sky; DevBuf<DevMat> d_mat; DevBuf<uint32_t> d_texels; DevBuf<DevTexture> d_tex;
    int rc = d_out.ensure(out_words ? out_words : 1u);
    if (!rc && in4 && W) rc = d_in.ensure((size_t)n * 4u);
    if (!rc && a.stage == STAGE_HALF) rc = d_mat.ensure(1);
    if (!rc && a.stage == STAGE_TEX) { rc = d_texels.ensure(texels); if (!rc) rc = d_tex.ensure(1); }
    if (!rc && a.stage == STAGE_SKY) rc = d_sky.ensure(texels * 3u);
    hipError_t e = hipSuccess;
    if (!rc && d_in.p) e = hipMemcpy(d_in.p, in4, (size_t)n * 16u, hipMemcpyHostToDevice);
    if (!rc && e == hipSuccess && d_mat.p) e = hipMemcpy(d_mat.p, mat, sizeof(DevMat), hipMemcpyHostToDevice);
    if (!rc && e == hipSuccess && d_texels.p) {
        e = hipMemcpy(d_texels.p, tex_rgba, texels * 4u, hipMemcpyHostToDevice);
        const DevTexture t{d_texels.p, a.img_w, a.img_h};
        if (e == hipSuccess) e = hipMemcpy(d_tex.p, &t, sizeof t, hipMemcpyHostToDevice);
    }
    if (!rc && e == hipSuccess && d_sky.p) e = hipMemcpy(d_sky.p, sky, texels * 12u, hipMemcpyHostToDevice);
    if (!rc && e == hipSuccess && !W) { const uint32_t init[3] = {0u, 0xFFFFFFFFu, 0u}; e = hipMemcpy(d_out.p, init, 12, hipMemcpyHostToDevice); }
    if (!rc && e == hipSuccess && n) {
        const uint64_t blocks = (n + 255u) / 256u < 16384u ? (n + 255u) / 256u : 16384u;
        if (W) hipLaunchKernelGGL(k_debug_stages, dim3((uint32_t)blocks), dim3(256), 0, nullptr, a, d_in.p, d_mat.p, d_tex.p, d_sky.p, d_out.p, n);
        else hipLaunchKernelGGL(k_debug_stages_exact, dim3((uint32_t)blocks), dim3(256), 0, nullptr, a, d_out.p, n);
        e = hipGetLastError();
    }
    if (!rc && e == hipSuccess) e = hipMemcpy(out, d_out.p, out_words * 4u, hipMemcpyDeviceToHost);
    if (!rc && e != hipSuccess) rc = fail(MI355RT_ERR_HIP, std::string("debug_stages: ") + hipGetErrorString(e));
    d_out.release(); d_in.release(); d_sky.release(); d_mat.release(); d_texels.release(); d_tex.release();
    return rc;
    });
}
