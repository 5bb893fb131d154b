// rt_radiance_paths.h -- the device code the radiance queries (rt_radiance.hip) and the views (rt_view.hip) share: the refilling path loop with the
// ray source as a template argument, and the ordered sum with the optional pack.  Device code only: included by those two translation units, behind
// rt_math.h, rt_rng.h, rt_intersect.h and rt_materials.h; each instantiates its own kernels from it (nothing here is a kernel).
#pragma once
#include "rt_radiance.h"

#include "rt_math.h"
#include "rt_rng.h"
#include "rt_intersect.h"
#include "rt_materials.h"

namespace mi355rt {

struct Rad3 { float x, y, z; };                                                             // 12 bytes: one global_store_dwordx3

// The ray source of the radiance queries: ray i is LOADED -- two 16-byte loads, the direction normalised once (Ray::new), the stream address from the
// record's two pad words.  A source's start() leaves the ray in ro / rd and the generator standing at ray 0 of sample s, its block 0 not drawn by the loop.
struct PathStart { f3 ro, rd; uint64_t ykey; uint32_t x; };                               // what a source hands the loop: the ray and its stream address (ykey = row + seed)
struct LoadedRays {
    struct Arg {};                                                                          // nothing beside RadianceParams
    const float4* __restrict__ rays;
    DI LoadedRays(const RadianceParams& P, const Arg&) : rays(reinterpret_cast<const float4*>(P.rays)) {}
    DI PathStart start(uint32_t i, uint32_t, uint64_t seed) const {
        const float4 r0 = rays[2u * (size_t)i], r1 = rays[2u * (size_t)i + 1u];
        PathStart a;
        a.ro = mk(r0.x, r0.y, r0.z);
        a.rd = normalized(mk(r1.x, r1.y, r1.z));                                            // Ray::new, ray.rs:12-17: once
        a.ykey = (uint64_t)__float_as_uint(r1.w) + seed; a.x = __float_as_uint(r0.w);
        return a;
    }
};

template <bool HAS_MESH, class Source>
DI void radiance_paths(const RadianceParams& P, const typename Source::Arg& arg) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = (uint64_t)blockIdx.x * (RADIANCE_BLOCK_THREADS / 64u) + (threadIdx.x >> 6);
    const uint64_t first = wave * (64u * (uint64_t)P.items_per_lane);                       // the wave's block of items: [first, first + count)
    if (first >= (uint64_t)P.n_items) return;                                               // (64 bit: the last workgroup's blocks may start past 2^32)
    const uint32_t first32 = (uint32_t)first;
    const uint32_t count = min(64u * P.items_per_lane, P.n_items - first32);                // <= 4096; first32 + count <= n_items: no index below wraps
    cprim_t prims = (cprim_t)P.prims;
    const Source src(P, arg);                                                               // what the source reads of its launch, set up behind the early return
    Rad3* __restrict__ out = reinterpret_cast<Rad3*>(P.scratch);
    const uint64_t seed = ((uint64_t)P.seed_hi << 32) | (uint64_t)P.seed_lo;
    uint32_t next = lane;                                                                   // offset of the lane's next item within the block
    bool live = false;
    uint32_t item = 0u, depth = 0u;
    f3 ro = mk(0.f, 0.f, 0.f), rd = mk(0.f, 0.f, 1.f), thr = mk(1.f, 1.f, 1.f);
    RngCtrT<true> rng; rng.clear();
    for (;;) {
        if (!live) {
            if (next >= count) break;
            item = first32 + next; next += 64u;
            const uint32_t i = item / P.samples, s = P.sample_begin + (item - i * P.samples);  // one division per path (items reach 2^32 - 1: no magic pair)
            const PathStart a = src.start(i, s, seed);
            ro = a.ro; rd = a.rd;
            rng.start((uint32_t)a.ykey, (uint32_t)(a.ykey >> 32), a.x, s);                   // the path stands at ray 0
            thr = mk(1.f, 1.f, 1.f); depth = 0u; live = true;
            if (P.max_depth == 0u) { out[item] = Rad3{0.f, 0.f, 0.f}; live = false; continue; }   // depth == 0 -> 1 * BLACK (renderer.rs:19-21)
        }
        // one segment: renderer.rs:24-36
        f3 term; bool fin = false;
        Hit h;
        if (!hit_scene<HAS_MESH>(prims, P.n_prims, P.nodes, P.tris, ro, rd, h)) { term = miss_colour(P.sky, P.sky_w, P.sky_h, P.miss, rd); fin = true; }
        else {
            float4 q0;
            if constexpr (HAS_MESH) q0 = reinterpret_cast<const float4*>(P.mats + (h.mat_ff & 0x7FFFFFFFu))[0];
            else q0 = h.q0;                                                                 // (the mesh-free finish_hit read it with the hit record)
            rng.next_event(); rng.load_block0();                                            // the event after ray r draws from ray r + 1
            f3 no, nd, atten, emitted;
            if (!surface_scatter(P.mats, P.textures, q0, h, rd, rng, no, nd, atten, emitted)) { term = emitted; fin = true; }
            else {
                thr = thr * atten; ro = no; rd = nd; ++depth;                               // scattered rays as surface_scatter returns them
                if (depth == P.max_depth) { term = mk(0.f, 0.f, 0.f); fin = true; }         // next level has depth == 0 (renderer.rs:20-22): throughput * BLACK
            }
        }
        if (fin) { const f3 L = thr * term; out[item] = Rad3{L.x, L.y, L.z}; live = false; }
    }
}

// The row chain of k_resolve (rt_kernels.hip): T = row_shr:1(T) + x, fifteen times.  Lane k's value is final after step k and every later step
// recomputes exactly the same sum, so no select is needed; lane 0 reads 0 from outside the row (bound_ctrl) and 0 + (acc + x0) is exact.  Samples
// past the chunk enter as +0, which leaves a sum unchanged -- unless the sum is -0: a running sum that started at +0 never is, and a stored sum
// that is -0 (only a caller could have put it there) becomes +0, which compares equal.
// PACK (the views): lane 0 of the row also writes color_to_u32(sqrt3(mean)) where out_packed is given, as k_resolve packs a pixel (renderer.rs:112-120).
DI float radiance_row_shr1_zero(float v) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x111, 0xF, 0xF, true)); }
DI float radiance_row_ror1(float v) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x121, 0xF, 0xF, true)); }
template <bool PACK>
DI void radiance_sum(const RadianceSum& S, uint32_t* __restrict__ out_packed) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = ((uint64_t)blockIdx.x * RADIANCE_BLOCK_THREADS + threadIdx.x) >> 6;
    const uint32_t s = lane & 15u;
    const uint64_t ray = wave * 4u + (lane >> 4);                                           // this row's ray
    const bool valid = ray < (uint64_t)S.n_rays;
    const float* __restrict__ rad = S.scratch + 3u * (size_t)(valid ? ray : 0u) * S.samples;   // 3 floats per sample, a ray's samples back to back
    float4* __restrict__ accum = reinterpret_cast<float4*>(S.accum);
    f3 acc = mk(0.f, 0.f, 0.f);                                                             // meaningful in lane 0 of the row
    if (S.accum_load && valid) { const float4 a = accum[ray]; acc = mk(a.x, a.y, a.z); }
    for (uint32_t c = 0; c < S.samples; c += 16u) {
        f3 x = mk(0.f, 0.f, 0.f);
        if (valid && s < S.samples - c) {
            const float* q = rad + 3u * (size_t)(c + s);
            x = mk(__builtin_nontemporal_load(q), __builtin_nontemporal_load(q + 1), __builtin_nontemporal_load(q + 2));
        }
        if (s == 0u) x = acc + x;                                                           // renderer.rs:100 goes on where the previous 16 samples stopped
        f3 t = x;
#pragma unroll
        for (int k = 0; k < 15; ++k) t = mk(radiance_row_shr1_zero(t.x) + x.x, radiance_row_shr1_zero(t.y) + x.y, radiance_row_shr1_zero(t.z) + x.z);
        acc = mk(radiance_row_ror1(t.x), radiance_row_ror1(t.y), radiance_row_ror1(t.z));   // lane 0 <- lane 15: the sum so far
    }
    if (!valid || s != 0u) return;
    accum[ray] = make_float4(acc.x, acc.y, acc.z, 0.0f);
    if constexpr (PACK) {
        const f3 mean = acc * S.inv_total;                                                  // renderer.rs:103
        if (S.out_linear) reinterpret_cast<Rad3*>(S.out_linear)[ray] = Rad3{mean.x, mean.y, mean.z};
        if (out_packed) out_packed[ray] = color_to_u32(sqrt3(mean));
    } else {
        if (S.out_linear) { const f3 mean = acc * S.inv_total; reinterpret_cast<Rad3*>(S.out_linear)[ray] = Rad3{mean.x, mean.y, mean.z}; }   // renderer.rs:103
    }
}

}  // namespace mi355rt
