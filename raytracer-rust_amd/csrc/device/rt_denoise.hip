// rt_denoise.hip -- the edge-avoiding a-trous filter of mi355rt_context_denoise / mi355rt_denoise (defined in include/mi355rt.h).
//
// Kernels (gfx950, wave64; a translation unit of its own: no other kernel is recompiled differently for it)
//   k_denoise_prepass   one pixel per lane over a plain grid: the 12-byte input pixel becomes a 16-byte one in the scratch's colour image A, and
//                       what the taps read of the 48-byte hit record -- normal, miss word, position, t -- becomes two 16-byte guide words.
//   k_denoise_level_staged{1,2}   the levels with step 1 and 2: 25 taps per pixel from one colour image of the scratch into the other, the
//                       tile and its halo of 2 s pixels -- colour and both guide words -- staged in LDS first (measured 20 - 30 % faster
//                       than gathering).
//   k_denoise_level     the levels with step 4 and more: the same taps as gathers from global memory (a halo of 2 s pixels no longer fits).
//   k_denoise_last[_staged{1,2}]  the last level: the same taps, the result leaves as the 12-byte linear pixel and / or the packed word.
//   k_denoise_copy      levels == 0: the input to the outputs.
// The diagnostic knob "denoise_staged" = 0 runs the steps 1 and 2 through k_denoise_level / k_denoise_last as well: the other side of the A/B.
// The level kernels work on tiles of 32 x 8 pixels, one pixel per lane (a wave is two rows of 32 pixels: a tap of a wave reads two runs of 512
// contiguous bytes per 16-byte word, and the 25 taps of neighbouring lanes share their cache lines), a workgroup takes tiles blockIdx.x,
// blockIdx.x + gridDim.x, ... (one tile unless the window has more tiles than DENOISE_MAX_BLOCKS).  A tap is three 16-byte reads (colour, two
// guide words), from LDS in the staged forms, from the scratch otherwise; a tap outside the window reads the centre instead and is dropped by its
// predicate.  No atomics and no polling waits (the staged forms: two workgroup barriers per tile, reached by every lane of the workgroup);
// every loop is bounded by the window, 25 taps and normal_squarings <= 8.
// The arithmetic is the header's, operation for operation: -ffp-contract=off keeps a*b+c two roundings, divisions are the compiler's
// correctly rounded ones, and a tap is dropped by a select on (in window && w > 0), so a NaN weight adds nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rt_device.h"
#include "rt_denoise.h"

#include "rt_math.h"

namespace mi355rt {

constexpr uint32_t DENOISE_MAX_BLOCKS = 1u << 20;

struct DenoiseLevel {
    const float4* guides;        // 2 per pixel
    const float4* src;           // colour image read
    float4* dst;                 // colour image written (k_denoise_level)
    float* out_linear;           // k_denoise_last: may be null
    uint32_t* out_packed;        // k_denoise_last: may be null
    uint32_t width, rows, tiles_x, n_tiles;
    uint32_t step, normal_squarings;
    float sigma_plane, inv_sigma2;
};

struct DenoisePrepass {
    const float* in; const uint4* hits;
    float4* guides; float4* col;
    float* out_linear; uint32_t* out_packed;     // k_denoise_copy
    uint32_t n;
};

DI void store_pixel(float* out_linear, uint32_t* out_packed, uint32_t i, f3 c) {
    if (out_linear) { float* o = out_linear + 3u * (size_t)i; o[0] = c.x; o[1] = c.y; o[2] = c.z; }
    if (out_packed) out_packed[i] = color_to_u32(sqrt3(c));
}

__global__ void __launch_bounds__(DENOISE_BLOCK_THREADS) k_denoise_prepass(const DenoisePrepass P) {
    const uint32_t i = blockIdx.x * DENOISE_BLOCK_THREADS + threadIdx.x;
    if (i >= P.n) return;
    const float* __restrict__ c = P.in + 3u * (size_t)i;
    const uint4* __restrict__ h = P.hits + 3u * (size_t)i;
    const uint4 h0 = h[0], h1 = h[1], h2 = h[2];                      // {position, t}, {normal, front_face}, {primitive, material, pads}
    P.col[i] = make_float4(c[0], c[1], c[2], 0.0f);
    P.guides[2u * (size_t)i] = make_float4(__uint_as_float(h1.x), __uint_as_float(h1.y), __uint_as_float(h1.z), __uint_as_float(h2.x == MI355RT_NO_HIT ? 1u : 0u));
    P.guides[2u * (size_t)i + 1u] = make_float4(__uint_as_float(h0.x), __uint_as_float(h0.y), __uint_as_float(h0.z), __uint_as_float(h0.w));
}

__global__ void __launch_bounds__(DENOISE_BLOCK_THREADS) k_denoise_copy(const DenoisePrepass P) {
    const uint32_t i = blockIdx.x * DENOISE_BLOCK_THREADS + threadIdx.x;
    if (i >= P.n) return;
    const float* __restrict__ c = P.in + 3u * (size_t)i;
    const f3 v = mk(c[0], c[1], c[2]);                                // (out_linear may be `in`: a lane reads its pixel before it writes it)
    store_pixel(P.out_linear, P.out_packed, i, v);
}

// One pixel's state over its 25 taps, and one tap: the header's weights, operation for operation.
struct DenoisePixel {
    float4 cp, np, pp;           // the centre: colour, {normal, miss word}, {position, t}
    bool miss_p; float spt;      // sigma_plane * t_p
    float ar, ag, ab, ws;
};
DI void pixel_begin(DenoisePixel& a, float4 cp, float4 np, float4 pp, float sigma_plane) {
    a.cp = cp; a.np = np; a.pp = pp;
    a.miss_p = __float_as_uint(np.w) != 0u; a.spt = sigma_plane * pp.w;
    a.ar = a.ag = a.ab = a.ws = 0.0f;
}
DI void tap(DenoisePixel& a, bool in, float h, float4 cq, float4 nq, float4 pq, uint32_t normal_squarings, float inv_sigma2) {
    const bool miss_q = __float_as_uint(nq.w) != 0u;
    const float nd = (a.np.x * nq.x + a.np.y * nq.y) + a.np.z * nq.z;
    float wn = nd > 0.0f ? nd : 0.0f;
    for (uint32_t j = 0; j < normal_squarings; ++j) wn = wn * wn;
    const float Dx = pq.x - a.pp.x, Dy = pq.y - a.pp.y, Dz = pq.z - a.pp.z;
    const float d = fabsf((a.np.x * Dx + a.np.y * Dy) + a.np.z * Dz);
    const float e = 1.0f - d / a.spt;
    const float wp = e > 0.0f ? e : 0.0f;
    float G = wn * wp;
    if (a.miss_p) G = miss_q ? 1.0f : 0.0f; else if (miss_q) G = 0.0f;
    const float dr = cq.x - a.cp.x, dg = cq.y - a.cp.y, db = cq.z - a.cp.z;
    const float d2 = (dr * dr + dg * dg) + db * db;
    const float wc = 1.0f / (1.0f + d2 * inv_sigma2);
    const float w = (h * G) * wc;
    if (in && w > 0.0f) { a.ar += cq.x * w; a.ag += cq.y * w; a.ab += cq.z * w; a.ws += w; }
}
template <bool LAST>
DI void pixel_end(const DenoisePixel& a, const DenoiseLevel& L, uint32_t ip) {
    const bool any = a.ws > 0.0f;
    const f3 out = mk(any ? a.ar / a.ws : a.cp.x, any ? a.ag / a.ws : a.cp.y, any ? a.ab / a.ws : a.cp.z);
    if constexpr (LAST) store_pixel(L.out_linear, L.out_packed, ip, out);
    else L.dst[ip] = make_float4(out.x, out.y, out.z, 0.0f);
}
DI float tap_kernel(int d) { return d == 0 ? 0.375f : (d == 1 || d == -1) ? 0.25f : 0.0625f; }     // K = {3/8, 1/4, 1/16}

template <bool LAST>
DI void denoise_level(const DenoiseLevel& L) {
    const uint32_t W = L.width, R = L.rows, s = L.step;
    for (uint32_t tile = blockIdx.x; tile < L.n_tiles; tile += gridDim.x) {
        const uint32_t ty = tile / L.tiles_x, tx = tile - ty * L.tiles_x;
        const uint32_t x = tx * DENOISE_TILE_W + (threadIdx.x & (DENOISE_TILE_W - 1u)), y = ty * DENOISE_TILE_H + threadIdx.x / DENOISE_TILE_W;
        if (x >= W || y >= R) continue;
        const uint32_t ip = y * W + x;                                // (< 2^31: plan_denoise)
        DenoisePixel a;
        pixel_begin(a, L.src[ip], L.guides[2u * (size_t)ip], L.guides[2u * (size_t)ip + 1u], L.sigma_plane);
        for (int dy = -2; dy <= 2; ++dy) {
            const uint32_t qy = y + (uint32_t)(dy * (int)s);          // below 0 it wraps to a value no window has
#pragma unroll
            for (int dx = -2; dx <= 2; ++dx) {
                const uint32_t qx = x + (uint32_t)(dx * (int)s);
                const bool in = qx < W && qy < R;
                const uint32_t iq = in ? qy * W + qx : ip;
                tap(a, in, tap_kernel(dy) * tap_kernel(dx), L.src[iq], L.guides[2u * (size_t)iq], L.guides[2u * (size_t)iq + 1u], L.normal_squarings, L.inv_sigma2);
            }
        }
        pixel_end<LAST>(a, L, ip);
    }
}

// The staged form of the levels with step S = 1 and 2: the tile and its halo of 2 S pixels -- colour and both guide words -- go through LDS
// ((32 + 4 S) x (8 + 4 S) pixels of 48 bytes: 20.3 / 30 KiB), the taps read LDS.  Cells of the halo outside the window are left as they are: no tap reads them.
template <bool LAST, uint32_t S>
DI void denoise_level_staged(const DenoiseLevel& L) {
    constexpr uint32_t HALO = 2u * S, LW = DENOISE_TILE_W + 2u * HALO, LH = DENOISE_TILE_H + 2u * HALO;
    __shared__ float4 t_c[LW * LH], t_n[LW * LH], t_p[LW * LH];
    const uint32_t W = L.width, R = L.rows;
    for (uint32_t tile = blockIdx.x; tile < L.n_tiles; tile += gridDim.x) {
        const uint32_t ty = tile / L.tiles_x, tx = tile - ty * L.tiles_x;
        const uint32_t x0 = tx * DENOISE_TILE_W, y0 = ty * DENOISE_TILE_H;
        for (uint32_t i = threadIdx.x; i < LW * LH; i += DENOISE_BLOCK_THREADS) {
            const uint32_t ly = i / LW, lx = i - ly * LW;
            const uint32_t gx = x0 + lx - HALO, gy = y0 + ly - HALO;  // left of / above the window they wrap to a value no window has
            if (gx < W && gy < R) {
                const uint32_t g = gy * W + gx;
                t_c[i] = L.src[g]; t_n[i] = L.guides[2u * (size_t)g]; t_p[i] = L.guides[2u * (size_t)g + 1u];
            }
        }
        __syncthreads();
        const uint32_t lx = threadIdx.x & (DENOISE_TILE_W - 1u), ly = threadIdx.x / DENOISE_TILE_W;
        const uint32_t x = x0 + lx, y = y0 + ly;
        if (x < W && y < R) {
            const uint32_t ip = y * W + x, lp = (ly + HALO) * LW + lx + HALO;
            DenoisePixel a;
            pixel_begin(a, t_c[lp], t_n[lp], t_p[lp], L.sigma_plane);
            for (int dy = -2; dy <= 2; ++dy) {
                const uint32_t qy = y + (uint32_t)(dy * (int)S);
#pragma unroll
                for (int dx = -2; dx <= 2; ++dx) {
                    const uint32_t qx = x + (uint32_t)(dx * (int)S);
                    const bool in = qx < W && qy < R;
                    const uint32_t lq = in ? (uint32_t)((int)lp + dy * (int)(S * LW) + dx * (int)S) : lp;
                    tap(a, in, tap_kernel(dy) * tap_kernel(dx), t_c[lq], t_n[lq], t_p[lq], L.normal_squarings, L.inv_sigma2);
                }
            }
            pixel_end<LAST>(a, L, ip);
        }
        __syncthreads();                                              // the next tile's staging overwrites what this one's taps read
    }
}

__global__ void __launch_bounds__(DENOISE_BLOCK_THREADS) k_denoise_level(const DenoiseLevel L) { denoise_level<false>(L); }
__global__ void __launch_bounds__(DENOISE_BLOCK_THREADS) k_denoise_last(const DenoiseLevel L) { denoise_level<true>(L); }
__global__ void __launch_bounds__(DENOISE_BLOCK_THREADS) k_denoise_level_staged1(const DenoiseLevel L) { denoise_level_staged<false, 1>(L); }
__global__ void __launch_bounds__(DENOISE_BLOCK_THREADS) k_denoise_level_staged2(const DenoiseLevel L) { denoise_level_staged<false, 2>(L); }
__global__ void __launch_bounds__(DENOISE_BLOCK_THREADS) k_denoise_last_staged1(const DenoiseLevel L) { denoise_level_staged<true, 1>(L); }
__global__ void __launch_bounds__(DENOISE_BLOCK_THREADS) k_denoise_last_staged2(const DenoiseLevel L) { denoise_level_staged<true, 2>(L); }

int launch_denoise(const DenoiseLaunch& d, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    const uint32_t n = d.width * d.rows;                              // (< 2^31: plan_denoise)
    const dim3 block(DENOISE_BLOCK_THREADS), grid_px((n + DENOISE_BLOCK_THREADS - 1u) / DENOISE_BLOCK_THREADS);
    float4* const guides = reinterpret_cast<float4*>(d.scratch);
    float4* const col[2] = {guides + 2u * (size_t)n, guides + 3u * (size_t)n};
    DenoisePrepass p{};
    p.in = d.in; p.hits = reinterpret_cast<const uint4*>(d.hits); p.guides = guides; p.col = col[0];
    p.out_linear = d.out_linear; p.out_packed = d.out_packed; p.n = n;
    if (d.plan.levels == 0) {
        hipLaunchKernelGGL(k_denoise_copy, grid_px, block, 0, s, p);
        return (int)hipGetLastError();
    }
    hipLaunchKernelGGL(k_denoise_prepass, grid_px, block, 0, s, p);
    if (hipError_t e = hipGetLastError()) return (int)e;
    DenoiseLevel L{};
    L.guides = guides; L.out_linear = d.out_linear; L.out_packed = d.out_packed;
    L.width = d.width; L.rows = d.rows;
    L.tiles_x = (d.width + DENOISE_TILE_W - 1u) / DENOISE_TILE_W;
    const uint64_t n_tiles = (uint64_t)L.tiles_x * ((d.rows + DENOISE_TILE_H - 1u) / DENOISE_TILE_H);   // (< 2^29: width * rows < 2^31)
    L.n_tiles = (uint32_t)n_tiles;
    L.normal_squarings = d.plan.normal_squarings; L.sigma_plane = d.plan.sigma_plane;
    const dim3 grid(L.n_tiles < DENOISE_MAX_BLOCKS ? L.n_tiles : DENOISE_MAX_BLOCKS);
    for (uint32_t k = 0; k < d.plan.levels; ++k) {
        L.src = col[k & 1u]; L.dst = col[(k & 1u) ^ 1u];
        L.step = 1u << k; L.inv_sigma2 = d.plan.inv_sigma2[k];
        const bool last = k + 1u == d.plan.levels;
        if (d.staged && k == 0) { if (last) hipLaunchKernelGGL(k_denoise_last_staged1, grid, block, 0, s, L); else hipLaunchKernelGGL(k_denoise_level_staged1, grid, block, 0, s, L); }
        else if (d.staged && k == 1) { if (last) hipLaunchKernelGGL(k_denoise_last_staged2, grid, block, 0, s, L); else hipLaunchKernelGGL(k_denoise_level_staged2, grid, block, 0, s, L); }
        else if (last) hipLaunchKernelGGL(k_denoise_last, grid, block, 0, s, L);
        else hipLaunchKernelGGL(k_denoise_level, grid, block, 0, s, L);
        if (hipError_t e = hipGetLastError()) return (int)e;
    }
    return 0;
}

}  // namespace mi355rt
