// svgf_kernels.hip -- the kernels of mi355rt_svgf_accumulate and mi355rt_svgf_filter (defined in include/mi355rt_svgf.h), part of
// libmi355rt_svgf.so.
//
// Kernels (gfx950, wave64; one pixel per lane in tiles of 32 x 8 pixels -- a wave is two rows of 32 pixels --, 256-thread workgroups, a workgroup takes
// tiles blockIdx.x, blockIdx.x + gridDim.x, ...; the prepass and the copy run one pixel per lane over a plain grid)
//   k_svgf_accumulate   the reprojection's gather (csrc/post/post_reproject.hip: colour, hit record, projection, four taps of two record words, the
//                       primitive word and the 16-byte history word) plus the 8-byte moments word per tap.  A tap outside the previous frame reads
//                       pixel 0 and is dropped by its predicate, so the four taps' loads are requested together.  Writes the history, the moments and,
//                       for a TEMPORAL pixel, the variance; every other pixel gets SPATIAL_MARK (-1.0f: no variance is negative) in its place.
//   k_svgf_spatial      a launch of its own behind the first (it reads the neighbours' moments_out: the kernel boundary orders it behind all of the
//                       first kernel's stores): a lane whose variance word is the mark gathers its 7 x 7 neighbourhood -- two record words, the
//                       primitive word and the moments word per tap -- and writes the estimate; every other lane does nothing.
//   k_svgf_prepass      the 48-byte hit record becomes the denoiser's two 16-byte guide words, {history rgb, variance} the 16-byte pixel of image A.
//   k_svgf_level / k_svgf_last        a level as gathers from the scratch: 9 variance words at step 1, then 25 taps of three 16-byte words.
//   k_svgf_level_staged{1,2} / k_svgf_last_staged{1,2}   the levels with step 1 and 2: the tile and its halo of 2 s pixels -- pixel and both guide
//                       words, 48 bytes a cell: 20.3 / 30 KiB -- staged in LDS first, two workgroup barriers per tile, reached by every lane; the 3 x 3
//                       variance window lies inside the halo.  MI355RT_SVGF_GATHERS_ONLY runs those levels through the gathers: the same bytes.
//   k_svgf_copy         levels == 0: the history's rgb to the outputs.
// The camera and the params arrive as by-value kernel arguments: scalar loads.  No atomics and no polling waits; every loop is bounded by the tiles,
// 4 / 49 / 9 / 25 taps and normal_squarings <= 8.  The arithmetic is the header's, operation for operation: -ffp-contract=off keeps a*b+c two
// roundings, the divisions are the compiler's correctly rounded ones, and a tap is dropped by a select on its predicate, so a NaN weight adds nothing.
// The packing is the render's (csrc/device/rt_math.h: color_to_u32, sqrt3), included, not copied.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "svgf_plan.h"
#include "../device/rt_math.h"

namespace mi355rt_svgf {

using mi355rt::color_to_u32;
using mi355rt::f3;
using mi355rt::mk;
using mi355rt::sqrt3;

static_assert(sizeof(mi355rt_hit) == 48, "a hit record is read as three 16-byte words: {position, t}, {normal, front_face}, {primitive, material, pads}");

DI bool finite_f(float v) { return fabsf(v) < __builtin_inff(); }
DI float lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// The geometry weight G(p, q) of the header: np = {normal, miss word}, pp = {position, t} of the centre, spt = sigma_plane * t_p.
DI float geometry_weight(float4 np, float4 pp, bool miss_p, float spt, float4 nq, float4 pq, bool miss_q, uint32_t normal_squarings) {
    const float nd = (np.x * nq.x + np.y * nq.y) + np.z * nq.z;
    float wn = nd > 0.0f ? nd : 0.0f;
    for (uint32_t j = 0; j < normal_squarings; ++j) wn = wn * wn;
    const float Dx = pq.x - pp.x, Dy = pq.y - pp.y, Dz = pq.z - pp.z;
    const float d = fabsf((np.x * Dx + np.y * Dy) + np.z * Dz);
    const float e = 1.0f - d / spt;
    const float wp = e > 0.0f ? e : 0.0f;
    float G = wn * wp;
    if (miss_p) G = miss_q ? 1.0f : 0.0f; else if (miss_q) G = 0.0f;
    return G;
}

// ---- accumulate ------------------------------------------------------------------------------------------------------------------------------
// hits_* / hist_prev / moments_prev / color_cur are only read, the three outputs belong to this call alone: __restrict__.
__global__ void __launch_bounds__(BLOCK_THREADS) k_svgf_accumulate(const AccumulateConsts K, const uint4* __restrict__ hits_cur, const float* __restrict__ color_cur,
                                                                   const uint4* __restrict__ hits_prev, const float4* __restrict__ hist_prev, const float2* __restrict__ moments_prev,
                                                                   float4* __restrict__ hist_out, float2* __restrict__ moments_out, uint32_t* __restrict__ variance_out) {
    const uint32_t W = K.width, H = K.height, Wp = K.prev_width, Hp = K.prev_height;
    for (uint32_t tile = blockIdx.x; tile < K.n_tiles; tile += gridDim.x) {
        const uint32_t tile_y = tile / K.tiles_x, tile_x = tile - tile_y * K.tiles_x;
        const uint32_t x = tile_x * TILE_W + (threadIdx.x & (TILE_W - 1u)), y = tile_y * TILE_H + threadIdx.x / TILE_W;
        if (x >= W || y >= H) continue;
        const uint32_t ip = y * W + x;                                // (< 2^31: plan_accumulate)
        const float* c = color_cur + 3u * (size_t)ip;
        const float cr = c[0], cg = c[1], cb = c[2];
        const uint4* g = hits_cur + 3u * (size_t)ip;
        const uint4 g0 = g[0], g1 = g[1], g2 = g[2];
        const uint32_t prim = g2.x;
        const float l = lum(cr, cg, cb);
        float o_r = cr, o_g = cg, o_b = cb, o_w = 1.0f;               // no history
        float m1 = l, m2 = l * l;
        bool temporal = false;
        if (K.has_prev != 0u && prim != MI355RT_NO_HIT) {
            const float Px = __uint_as_float(g0.x), Py = __uint_as_float(g0.y), Pz = __uint_as_float(g0.z), t = __uint_as_float(g0.w);
            const float Nx = __uint_as_float(g1.x), Ny = __uint_as_float(g1.y), Nz = __uint_as_float(g1.z);
            // 1. projection into the previous view
            const float Dx = Px - K.position[0], Dy = Py - K.position[1], Dz = Pz - K.position[2];
            const float z = (Dx * K.forward[0] + Dy * K.forward[1]) + Dz * K.forward[2];
            const float a = (Dx * K.right[0] + Dy * K.right[1]) + Dz * K.right[2];
            const float b = (Dx * K.true_up[0] + Dy * K.true_up[1]) + Dz * K.true_up[2];
            if (z > 0.0f) {
                const float sx = a / (z * K.half_width), sy = b / (z * K.half_height);
                const float u = (sx + 1.0f) * 0.5f, v = (1.0f - sy) * 0.5f;
                const float fx = u * K.prev_width_f - 0.5f, fy = v * K.prev_height_f - 0.5f;
                if (fx > -1.0f && fx < K.prev_width_f && fy > -1.0f && fy < K.prev_height_f) {     // (a NaN fails)
                    const float flx = floorf(fx), fly = floorf(fy);   // in [-1, 2^31): the casts are exact
                    const int x0 = (int)flx, y0 = (int)fly;
                    const float tx = fx - flx, ty = fy - fly;
                    const float tol = K.plane_tolerance * t;
                    // 2. the four taps
                    float ar = 0.0f, ag = 0.0f, ab = 0.0f, a1 = 0.0f, a2 = 0.0f, ws = 0.0f, L = __builtin_inff();
#pragma unroll
                    for (int dy = 0; dy < 2; ++dy) {
#pragma unroll
                        for (int dx = 0; dx < 2; ++dx) {
                            const uint32_t qx = (uint32_t)(x0 + dx), qy = (uint32_t)(y0 + dy);     // -1 wraps to a value no frame has
                            const bool in = qx < Wp && qy < Hp;
                            const uint32_t iq = in ? qy * Wp + qx : 0u;                            // (< 2^31: plan_accumulate)
                            const uint4* h = hits_prev + 3u * (size_t)iq;
                            const uint4 h0 = h[0], h1 = h[1];
                            const uint32_t hprim = reinterpret_cast<const uint32_t*>(h + 2)[0];
                            const float4 m = hist_prev[iq];
                            const float2 mm = moments_prev[iq];
                            const float nd = (Nx * __uint_as_float(h1.x) + Ny * __uint_as_float(h1.y)) + Nz * __uint_as_float(h1.z);
                            const float Ex = __uint_as_float(h0.x) - Px, Ey = __uint_as_float(h0.y) - Py, Ez = __uint_as_float(h0.z) - Pz;
                            const float d = fabsf((Nx * Ex + Ny * Ey) + Nz * Ez);
                            const bool valid = in && hprim == prim && nd >= K.normal_min && d <= tol && m.w >= 1.0f && finite_f(m.x) && finite_f(m.y) && finite_f(m.z);
                            const float w = (dx ? tx : 1.0f - tx) * (dy ? ty : 1.0f - ty);
                            if (valid && w > 0.0f) { ar += m.x * w; ag += m.y * w; ab += m.z * w; a1 += mm.x * w; a2 += mm.y * w; ws += w; L = fminf(L, m.w); }
                        }
                    }
                    // 3. blend, 2'. moments
                    if (ws > 0.0f) {
                        const float hr = ar / ws, hg = ag / ws, hb = ab / ws;
                        const float n = fminf(L + 1.0f, K.max_history_f);
                        const float alpha = 1.0f / n;
                        o_r = hr + (cr - hr) * alpha; o_g = hg + (cg - hg) * alpha; o_b = hb + (cb - hb) * alpha; o_w = n;
                        const float h1m = a1 / ws, h2m = a2 / ws;
                        if (finite_f(h1m) && finite_f(h2m)) {
                            m1 = h1m + (l - h1m) * alpha; m2 = h2m + (l * l - h2m) * alpha;
                            temporal = n >= K.min_temporal_f;
                        }
                    }
                }
            }
        }
        // outputs: every word of every record; 3'. the variance of a TEMPORAL pixel, the mark for k_svgf_spatial otherwise
        hist_out[ip] = make_float4(o_r, o_g, o_b, o_w);
        moments_out[ip] = make_float2(m1, m2);
        const float v = m2 - m1 * m1;
        variance_out[ip] = temporal ? __float_as_uint(v > 0.0f ? v : 0.0f) : SPATIAL_MARK;
    }
}

// variance is read and written by its own lane only; the neighbours' moments, records and this pixel's length are only read.
__global__ void __launch_bounds__(BLOCK_THREADS) k_svgf_spatial(const AccumulateConsts K, const uint4* __restrict__ hits_cur, const float4* __restrict__ hist_out,
                                                                const float2* __restrict__ moments_out, uint32_t* __restrict__ variance_out) {
    const uint32_t W = K.width, H = K.height;
    for (uint32_t tile = blockIdx.x; tile < K.n_tiles; tile += gridDim.x) {
        const uint32_t tile_y = tile / K.tiles_x, tile_x = tile - tile_y * K.tiles_x;
        const uint32_t x = tile_x * TILE_W + (threadIdx.x & (TILE_W - 1u)), y = tile_y * TILE_H + threadIdx.x / TILE_W;
        if (x >= W || y >= H) continue;
        const uint32_t ip = y * W + x;
        if (variance_out[ip] != SPATIAL_MARK) continue;
        const uint4* g = hits_cur + 3u * (size_t)ip;
        const uint4 g0 = g[0], g1 = g[1];
        const bool miss_p = reinterpret_cast<const uint32_t*>(g + 2)[0] == MI355RT_NO_HIT;
        const float4 pp = make_float4(__uint_as_float(g0.x), __uint_as_float(g0.y), __uint_as_float(g0.z), __uint_as_float(g0.w));
        const float4 np = make_float4(__uint_as_float(g1.x), __uint_as_float(g1.y), __uint_as_float(g1.z), 0.0f);
        const float spt = K.sigma_plane * pp.w;
        const float n = hist_out[ip].w;
        float a1 = 0.0f, a2 = 0.0f, ws2 = 0.0f;
        for (int dy = -3; dy <= 3; ++dy) {
            const uint32_t qy = y + (uint32_t)dy;                     // below 0 it wraps to a value no frame has
            for (int dx = -3; dx <= 3; ++dx) {
                const uint32_t qx = x + (uint32_t)dx;
                const bool in = qx < W && qy < H;
                const uint32_t iq = in ? qy * W + qx : ip;
                const uint4* h = hits_cur + 3u * (size_t)iq;
                const uint4 h0 = h[0], h1 = h[1];
                const bool miss_q = reinterpret_cast<const uint32_t*>(h + 2)[0] == MI355RT_NO_HIT;
                const float2 mq = moments_out[iq];
                const float4 pq = make_float4(__uint_as_float(h0.x), __uint_as_float(h0.y), __uint_as_float(h0.z), __uint_as_float(h0.w));
                const float4 nq = make_float4(__uint_as_float(h1.x), __uint_as_float(h1.y), __uint_as_float(h1.z), 0.0f);
                const float G = geometry_weight(np, pp, miss_p, spt, nq, pq, miss_q, K.normal_squarings);
                if (in && G > 0.0f && finite_f(mq.x) && finite_f(mq.y)) { a1 += mq.x * G; a2 += mq.y * G; ws2 += G; }
            }
        }
        float var = 0.0f;
        if (ws2 > 0.0f) {
            const float M1 = a1 / ws2, M2 = a2 / ws2;
            const float v = M2 - M1 * M1;
            const float b = n < K.min_temporal_f ? K.min_temporal_f / n : 1.0f;
            var = (v > 0.0f ? v : 0.0f) * b;
        }
        variance_out[ip] = __float_as_uint(var);
    }
}

int launch_accumulate(const AccumulatePlan& plan, const AccumulateBuffers& b, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_svgf_accumulate, dim3(plan.grid), dim3(BLOCK_THREADS), 0, s, plan.k,
                       reinterpret_cast<const uint4*>(b.hits_cur), reinterpret_cast<const float*>(b.color_cur),
                       reinterpret_cast<const uint4*>(b.hits_prev), reinterpret_cast<const float4*>(b.hist_prev), reinterpret_cast<const float2*>(b.moments_prev),
                       reinterpret_cast<float4*>(b.hist_out), reinterpret_cast<float2*>(b.moments_out), reinterpret_cast<uint32_t*>(b.variance_out));
    if (hipError_t e = hipGetLastError()) return (int)e;
    hipLaunchKernelGGL(k_svgf_spatial, dim3(plan.grid), dim3(BLOCK_THREADS), 0, s, plan.k,
                       reinterpret_cast<const uint4*>(b.hits_cur), reinterpret_cast<const float4*>(b.hist_out), reinterpret_cast<const float2*>(b.moments_out),
                       reinterpret_cast<uint32_t*>(b.variance_out));
    return (int)hipGetLastError();
}

// ---- filter ----------------------------------------------------------------------------------------------------------------------------------
struct FilterLevel {
    const float4* guides;        // 2 per pixel
    const float4* src;           // {r, g, b, v} image read
    float4* dst;                 // image written (k_svgf_level*)
    float* out_linear;           // k_svgf_last*: may be null
    uint32_t* out_packed;        // k_svgf_last*: may be null
    uint32_t width, height, tiles_x, n_tiles;
    uint32_t step, normal_squarings;
    float sigma_plane, sl2;
};

struct FilterPrepass {
    const float4* hist; const float* variance; const uint4* hits;
    float4* guides; float4* img;
    float* out_linear; uint32_t* out_packed;     // k_svgf_copy
    uint32_t n;
};

DI void store_pixel(float* out_linear, uint32_t* out_packed, uint32_t i, f3 c) {
    if (out_linear) { float* o = out_linear + 3u * (size_t)i; o[0] = c.x; o[1] = c.y; o[2] = c.z; }
    if (out_packed) out_packed[i] = color_to_u32(sqrt3(c));
}

__global__ void __launch_bounds__(BLOCK_THREADS) k_svgf_prepass(const FilterPrepass P) {
    const uint32_t i = blockIdx.x * BLOCK_THREADS + threadIdx.x;
    if (i >= P.n) return;
    const uint4* __restrict__ h = P.hits + 3u * (size_t)i;
    const uint4 h0 = h[0], h1 = h[1], h2 = h[2];                      // {position, t}, {normal, front_face}, {primitive, material, pads}
    const float4 c = P.hist[i];
    P.img[i] = make_float4(c.x, c.y, c.z, P.variance[i]);
    P.guides[2u * (size_t)i] = make_float4(__uint_as_float(h1.x), __uint_as_float(h1.y), __uint_as_float(h1.z), __uint_as_float(h2.x == MI355RT_NO_HIT ? 1u : 0u));
    P.guides[2u * (size_t)i + 1u] = make_float4(__uint_as_float(h0.x), __uint_as_float(h0.y), __uint_as_float(h0.z), __uint_as_float(h0.w));
}

__global__ void __launch_bounds__(BLOCK_THREADS) k_svgf_copy(const FilterPrepass P) {
    const uint32_t i = blockIdx.x * BLOCK_THREADS + threadIdx.x;
    if (i >= P.n) return;
    const float4 c = P.hist[i];                                       // (no pass through the scratch here: the outputs must not overlap the history, whose pixels are 16 bytes against 12 and 4 -- the header says so, plan_filter refuses the equal pointers)
    store_pixel(P.out_linear, P.out_packed, i, mk(c.x, c.y, c.z));
}

// One pixel's state over its taps, and one tap: the header's weights, operation for operation.
struct FilterPixel {
    float4 cp, np, pp;           // the centre: {r, g, b, v}, {normal, miss word}, {position, t}
    bool miss_p; float spt, lp, a;
    float num, den;              // the centre variance's sums
    float ar, ag, ab, av, ws;
};
DI void pixel_begin(FilterPixel& a, float4 cp, float4 np, float4 pp, float sigma_plane) {
    a.cp = cp; a.np = np; a.pp = pp;
    a.miss_p = __float_as_uint(np.w) != 0u; a.spt = sigma_plane * pp.w;
    a.lp = lum(cp.x, cp.y, cp.z);
    a.num = a.den = 0.0f;
    a.ar = a.ag = a.ab = a.av = a.ws = 0.0f;
}
DI float window_weight(int ex, int ey) { return (ex == 0 && ey == 0) ? 0.25f : (ex == 0 || ey == 0) ? 0.125f : 0.0625f; }     // g = {1/4, 1/8, 1/16}
DI void window_tap(FilterPixel& a, bool in, float g, float vr) {
    if (in) { a.num += g * vr; a.den += g; }
}
DI void window_end(FilterPixel& a, float sl2) {
    const float gv = a.num / a.den;                                   // (den >= 1/4: the centre is in the frame)
    const float e = sl2 * (gv > 0.0f ? gv : 0.0f) + 1e-8f;
    a.a = 1.0f / e;
}
DI void tap(FilterPixel& a, bool in, float h, float4 cq, float4 nq, float4 pq, uint32_t normal_squarings) {
    const float G = geometry_weight(a.np, a.pp, a.miss_p, a.spt, nq, pq, __float_as_uint(nq.w) != 0u, normal_squarings);
    const float dl = lum(cq.x, cq.y, cq.z) - a.lp;
    const float wl = 1.0f / (1.0f + (dl * dl) * a.a);
    const float w = (h * G) * wl;
    if (in && w > 0.0f) { a.ar += cq.x * w; a.ag += cq.y * w; a.ab += cq.z * w; a.av += cq.w * (w * w); a.ws += w; }
}
template <bool LAST>
DI void pixel_end(const FilterPixel& a, const FilterLevel& L, uint32_t ip) {
    const bool any = a.ws > 0.0f;
    const f3 out = mk(any ? a.ar / a.ws : a.cp.x, any ? a.ag / a.ws : a.cp.y, any ? a.ab / a.ws : a.cp.z);
    if constexpr (LAST) store_pixel(L.out_linear, L.out_packed, ip, out);
    else L.dst[ip] = make_float4(out.x, out.y, out.z, any ? a.av / (a.ws * a.ws) : a.cp.w);
}
DI float tap_kernel(int d) { return d == 0 ? 0.375f : (d == 1 || d == -1) ? 0.25f : 0.0625f; }     // K = {3/8, 1/4, 1/16}

template <bool LAST>
DI void filter_level(const FilterLevel& L) {
    const uint32_t W = L.width, R = L.height, s = L.step;
    for (uint32_t tile = blockIdx.x; tile < L.n_tiles; tile += gridDim.x) {
        const uint32_t ty = tile / L.tiles_x, tx = tile - ty * L.tiles_x;
        const uint32_t x = tx * TILE_W + (threadIdx.x & (TILE_W - 1u)), y = ty * TILE_H + threadIdx.x / TILE_W;
        if (x >= W || y >= R) continue;
        const uint32_t ip = y * W + x;                                // (< 2^31: plan_filter)
        FilterPixel a;
        pixel_begin(a, L.src[ip], L.guides[2u * (size_t)ip], L.guides[2u * (size_t)ip + 1u], L.sigma_plane);
#pragma unroll
        for (int ey = -1; ey <= 1; ++ey) {
            const uint32_t ry = y + (uint32_t)ey;                     // below 0 it wraps to a value no frame has
#pragma unroll
            for (int ex = -1; ex <= 1; ++ex) {
                const uint32_t rx = x + (uint32_t)ex;
                const bool in = rx < W && ry < R;
                const uint32_t ir = in ? ry * W + rx : ip;
                window_tap(a, in, window_weight(ex, ey), L.src[ir].w);
            }
        }
        window_end(a, L.sl2);
        for (int dy = -2; dy <= 2; ++dy) {
            const uint32_t qy = y + (uint32_t)(dy * (int)s);
#pragma unroll
            for (int dx = -2; dx <= 2; ++dx) {
                const uint32_t qx = x + (uint32_t)(dx * (int)s);
                const bool in = qx < W && qy < R;
                const uint32_t iq = in ? qy * W + qx : ip;
                tap(a, in, tap_kernel(dy) * tap_kernel(dx), L.src[iq], L.guides[2u * (size_t)iq], L.guides[2u * (size_t)iq + 1u], L.normal_squarings);
            }
        }
        pixel_end<LAST>(a, L, ip);
    }
}

// The staged form of the levels with step S = 1 and 2: the tile and its halo of 2 S pixels -- pixel and both guide words -- go through LDS
// ((32 + 4 S) x (8 + 4 S) cells of 48 bytes: 20.3 / 30 KiB), the taps and the 3 x 3 window read LDS.  Cells of the halo outside the frame are
// left as they are: no tap reads them (a tap outside the frame reads the centre's cell).
template <bool LAST, uint32_t S>
DI void filter_level_staged(const FilterLevel& L) {
    constexpr uint32_t HALO = 2u * S, LW = TILE_W + 2u * HALO, LH = TILE_H + 2u * HALO;
    __shared__ float4 t_c[LW * LH], t_n[LW * LH], t_p[LW * LH];
    const uint32_t W = L.width, R = L.height;
    for (uint32_t tile = blockIdx.x; tile < L.n_tiles; tile += gridDim.x) {
        const uint32_t ty = tile / L.tiles_x, tx = tile - ty * L.tiles_x;
        const uint32_t x0 = tx * TILE_W, y0 = ty * TILE_H;
        for (uint32_t i = threadIdx.x; i < LW * LH; i += BLOCK_THREADS) {
            const uint32_t ly = i / LW, lx = i - ly * LW;
            const uint32_t gx = x0 + lx - HALO, gy = y0 + ly - HALO;  // left of / above the frame they wrap to a value no frame has
            if (gx < W && gy < R) {
                const uint32_t g = gy * W + gx;
                t_c[i] = L.src[g]; t_n[i] = L.guides[2u * (size_t)g]; t_p[i] = L.guides[2u * (size_t)g + 1u];
            }
        }
        __syncthreads();
        const uint32_t lx = threadIdx.x & (TILE_W - 1u), ly = threadIdx.x / TILE_W;
        const uint32_t x = x0 + lx, y = y0 + ly;
        if (x < W && y < R) {
            const uint32_t ip = y * W + x, lp = (ly + HALO) * LW + lx + HALO;
            FilterPixel a;
            pixel_begin(a, t_c[lp], t_n[lp], t_p[lp], L.sigma_plane);
#pragma unroll
            for (int ey = -1; ey <= 1; ++ey) {
                const uint32_t ry = y + (uint32_t)ey;
#pragma unroll
                for (int ex = -1; ex <= 1; ++ex) {
                    const uint32_t rx = x + (uint32_t)ex;
                    const bool in = rx < W && ry < R;
                    const uint32_t lr = in ? (uint32_t)((int)lp + ey * (int)LW + ex) : lp;
                    window_tap(a, in, window_weight(ex, ey), t_c[lr].w);
                }
            }
            window_end(a, L.sl2);
            for (int dy = -2; dy <= 2; ++dy) {
                const uint32_t qy = y + (uint32_t)(dy * (int)S);
#pragma unroll
                for (int dx = -2; dx <= 2; ++dx) {
                    const uint32_t qx = x + (uint32_t)(dx * (int)S);
                    const bool in = qx < W && qy < R;
                    const uint32_t lq = in ? (uint32_t)((int)lp + dy * (int)(S * LW) + dx * (int)S) : lp;
                    tap(a, in, tap_kernel(dy) * tap_kernel(dx), t_c[lq], t_n[lq], t_p[lq], L.normal_squarings);
                }
            }
            pixel_end<LAST>(a, L, ip);
        }
        __syncthreads();                                              // the next tile's staging overwrites what this one's taps read
    }
}

__global__ void __launch_bounds__(BLOCK_THREADS) k_svgf_level(const FilterLevel L) { filter_level<false>(L); }
__global__ void __launch_bounds__(BLOCK_THREADS) k_svgf_last(const FilterLevel L) { filter_level<true>(L); }
__global__ void __launch_bounds__(BLOCK_THREADS) k_svgf_level_staged1(const FilterLevel L) { filter_level_staged<false, 1>(L); }
__global__ void __launch_bounds__(BLOCK_THREADS) k_svgf_level_staged2(const FilterLevel L) { filter_level_staged<false, 2>(L); }
__global__ void __launch_bounds__(BLOCK_THREADS) k_svgf_last_staged1(const FilterLevel L) { filter_level_staged<true, 1>(L); }
__global__ void __launch_bounds__(BLOCK_THREADS) k_svgf_last_staged2(const FilterLevel L) { filter_level_staged<true, 2>(L); }

int launch_filter(const FilterPlan& plan, const FilterBuffers& b, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    const uint32_t n = plan.width * plan.height;                      // (< 2^31: plan_filter)
    const dim3 block(BLOCK_THREADS), grid_px(plan.grid_px), grid(plan.grid);
    float4* const guides = reinterpret_cast<float4*>(b.scratch);
    float4* const img[2] = {guides + 2u * (size_t)n, guides + 3u * (size_t)n};
    FilterPrepass p{};
    p.hist = reinterpret_cast<const float4*>(b.hist_in); p.variance = reinterpret_cast<const float*>(b.variance_in); p.hits = reinterpret_cast<const uint4*>(b.hits);
    p.guides = guides; p.img = img[0];
    p.out_linear = reinterpret_cast<float*>(b.out_linear); p.out_packed = reinterpret_cast<uint32_t*>(b.out_packed); p.n = n;
    if (plan.levels == 0) {
        hipLaunchKernelGGL(k_svgf_copy, grid_px, block, 0, s, p);
        return (int)hipGetLastError();
    }
    hipLaunchKernelGGL(k_svgf_prepass, grid_px, block, 0, s, p);
    if (hipError_t e = hipGetLastError()) return (int)e;
    FilterLevel L{};
    L.guides = guides; L.out_linear = p.out_linear; L.out_packed = p.out_packed;
    L.width = plan.width; L.height = plan.height; L.tiles_x = plan.tiles_x; L.n_tiles = plan.n_tiles;
    L.normal_squarings = plan.normal_squarings; L.sigma_plane = plan.sigma_plane; L.sl2 = plan.sl2;
    for (uint32_t k = 0; k < plan.levels; ++k) {
        L.src = img[k & 1u]; L.dst = img[(k & 1u) ^ 1u];
        L.step = 1u << k;
        const bool last = k + 1u == plan.levels;
        if (plan.staged && k == 0) { if (last) hipLaunchKernelGGL(k_svgf_last_staged1, grid, block, 0, s, L); else hipLaunchKernelGGL(k_svgf_level_staged1, grid, block, 0, s, L); }
        else if (plan.staged && k == 1) { if (last) hipLaunchKernelGGL(k_svgf_last_staged2, grid, block, 0, s, L); else hipLaunchKernelGGL(k_svgf_level_staged2, grid, block, 0, s, L); }
        else if (last) hipLaunchKernelGGL(k_svgf_last, grid, block, 0, s, L);
        else hipLaunchKernelGGL(k_svgf_level, grid, block, 0, s, L);
        if (hipError_t e = hipGetLastError()) return (int)e;
    }
    return 0;
}

}  // namespace mi355rt_svgf
