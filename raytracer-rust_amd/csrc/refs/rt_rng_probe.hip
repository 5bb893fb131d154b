// rt_rng_probe.hip -- one block of the counter-mode generator per lane, through both forms of the draw address (rt_rng.h: RngCtrT<false>, the plain
// words, and RngCtrT<true>, the LCG-stepped words), at a caller-chosen (key, x, sample, ray, try).
// Compiled into the tests' reference build only (build.build_device_variant("refs"), -DMI355RT_REFS): the product library and its kernel
// hash do not contain it.
//
// The product's debug entry mi355rt_debug_scatter reaches a path's blocks only through a scatter event (block 0, and the tries a rejection
// happens to need); this entry exposes the try number j, so that tests/test_gpu_rng_stepped.py can put j and the ray number where the linear
// form (W_3 + j * A, W_2 + r * A mod 2^32) could go wrong -- around 2^6 (the cooperative rejection's 24-bit multiply stays below it), 2^24 and
// 2^32 -- and compare both forms with the oracle's generator word for word.  Nothing is restated: the kernel calls start / set_ray / block and,
// for the running form of unit_ball_cooperative, walks a word from try j0 = j & ~63 to try j in steps of A and A << lg as an owner and its worker would.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../device/rt_device.h"
#include "../device/rt_host.h"
#include "../device/rt_math.h"
#include "../device/rt_rng.h"

namespace mi355rt {

struct RngProbeIn { uint32_t k0, k1, x, s, ray, j; };          // 24 B; tests/test_gpu_rng_stepped.py packs the same six words
constexpr uint32_t RNG_PROBE_WORDS = 12;                         // per record: the block by the plain form, by the stepped form, by the stepped form's running word

__global__ void __launch_bounds__(64) k_debug_rng_block(const RngProbeIn* __restrict__ in, uint32_t* __restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const RngProbeIn r = in[i];
    uint32_t* o = out + (size_t)RNG_PROBE_WORDS * i;
    uint32_t b[4];
    RngCtrT<false> plain; plain.start(r.k0, r.k1, r.x, r.s); plain.set_ray(r.ray);
    RngCtrT<false>::block(plain.w, r.j, b);
    o[0] = b[0]; o[1] = b[1]; o[2] = b[2]; o[3] = b[3];
    if constexpr (RngCtrT<true>::STEPPED) {
        RngCtrT<true> st; st.start(r.k0, r.k1, r.x, r.s);
        // the ray number as the kernels reach it: set_ray for the first half of it, next_event one by one for up to 3 more (the two must agree)
        const uint32_t walk = r.ray & 3u;
        st.set_ray(r.ray - walk);
        for (uint32_t k = 0; k < walk; ++k) st.next_event();
        RngCtrT<true>::block(st.w, r.j, b);
        o[4] = b[0]; o[5] = b[1]; o[6] = b[2]; o[7] = b[3];
        // unit_ball_cooperative's form: the owner's running word starts at try 1 (W_3 + A), is advanced by A << lg per failed round, and a worker adds
        // sub * A with a 24-bit multiply, sub < 64.  Reach try j >= 1 that way: rounds of 64 tries (lg = 6) up to j's round, then sub = (j - 1) & 63.
        uint32_t wnext = st.w[3] + LCG_A;
        const uint32_t rounds = r.j == 0u ? 0u : (r.j - 1u) >> 6, sub = r.j == 0u ? 0u : (r.j - 1u) & 63u;
        // (rounds can be 2^26: the advance is linear, so it is taken in one multiply here -- the per-round addition is what the render tests run)
        wnext += rounds * (LCG_A << 6);
        if (r.j == 0u) RngCtrT<true>::block(st.w, 0u, b);
        else RngCtrT<true>::block_at(st.w[0], st.w[1], st.w[2], wnext + __umul24(sub, LCG_A), b);
        o[8] = b[0]; o[9] = b[1]; o[10] = b[2]; o[11] = b[3];
    } else {
        for (int k = 4; k < 12; ++k) o[k] = o[k & 3];          // (the Philox builds have one form)
    }
}

}  // namespace mi355rt

using namespace mi355rt;

// Not in the public header; the reference build's diagnostic entry.  Host pointers: records = n * 6 words (k0, k1, x, sample, ray, try),
// out = n * 12 words.  Synchronous; both device buffers are freed before it returns.
extern "C" int mi355rt_debug_rng_block(const uint32_t* records, uint32_t n, uint32_t* out, int device) {
    return guard([&]() -> int {
    if (!records || !out || !n) return fail(MI355RT_ERR_INVALID, "debug_rng_block: null / empty");
    if (n > (1u << 24)) return fail(MI355RT_ERR_INVALID, "debug_rng_block: at most 2^24 records");
    HIP_TRY(hipSetDevice(device));
    DevBuf<RngProbeIn> d_in; DevBuf<uint32_t> d_out;
    int rc = d_in.ensure(n);
    if (!rc) rc = d_out.ensure((size_t)n * RNG_PROBE_WORDS);
    hipError_t e = hipSuccess;
    if (!rc) e = hipMemcpy(d_in.p, records, (size_t)n * sizeof(RngProbeIn), hipMemcpyHostToDevice);
    if (!rc && e == hipSuccess) {
        hipLaunchKernelGGL(k_debug_rng_block, dim3((n + 63u) / 64u), dim3(64), 0, nullptr, d_in.p, d_out.p, n);
        e = hipGetLastError();
    }
    if (!rc && e == hipSuccess) e = hipMemcpy(out, d_out.p, (size_t)n * RNG_PROBE_WORDS * 4u, hipMemcpyDeviceToHost);
    if (!rc && e != hipSuccess) rc = fail(MI355RT_ERR_HIP, std::string("debug_rng_block: ") + hipGetErrorString(e));
    d_in.release(); d_out.release();
    return rc;
    });
}
