// post_reproject.hip -- the kernel of mi355rt_post_reproject (defined in include/mi355rt_post.h), part of libmi355rt_post.so.
//
// k_post_reproject (gfx950, wave64): one pixel per lane in tiles of 32 x 8 pixels, as the denoiser's level kernels (a wave is two rows of 32
// pixels, so its taps fall in a few rows of the previous frame); a workgroup takes tiles blockIdx.x, blockIdx.x + gridDim.x, ...  A lane reads
// its colour (12 bytes) and its hit record (three 16-byte words), projects the hit into the previous view, and gathers its four taps: per tap
// two 16-byte words of the previous record ({position, t}, {normal, front_face}), the primitive word, and the 16-byte history word.  A tap
// outside the previous frame reads pixel 0 instead and is dropped by its predicate, so the four taps' loads are issued together.  The camera and
// the params arrive as a by-value kernel argument: scalar loads.  No LDS, no atomics, no waits; every loop is bounded by the tiles and 4 taps.
// The arithmetic is the header's, operation for operation: -ffp-contract=off keeps a*b+c two roundings, the divisions are the compiler's
// correctly rounded ones.  The packing is the render's (csrc/device/rt_math.h: color_to_u32, sqrt3), included, not copied.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "post_plan.h"
#include "../device/rt_math.h"

namespace mi355rt_post {

using mi355rt::color_to_u32;
using mi355rt::mk;
using mi355rt::sqrt3;

static_assert(sizeof(mi355rt_hit) == 48, "a hit record is read as three 16-byte words: {position, t}, {normal, front_face}, {primitive, material, pads}");

DI bool finite_f(float v) { return fabsf(v) < __builtin_inff(); }

// hits_cur / hits_prev and hist_prev are only read, hist_out and out_packed belong to this call alone: __restrict__.  out_linear may be
// color_cur (a lane reads its colour before it writes its pixel), so neither of those two is.
__global__ void __launch_bounds__(REPROJECT_BLOCK_THREADS) k_post_reproject(const ReprojectConsts K, const uint4* __restrict__ hits_cur, const float* color_cur,
                                                                            const uint4* __restrict__ hits_prev, const float4* __restrict__ hist_prev,
                                                                            float4* __restrict__ hist_out, float* out_linear, uint32_t* __restrict__ out_packed) {
    const uint32_t W = K.width, H = K.height, Wp = K.prev_width, Hp = K.prev_height;
    for (uint32_t tile = blockIdx.x; tile < K.n_tiles; tile += gridDim.x) {
        const uint32_t tile_y = tile / K.tiles_x, tile_x = tile - tile_y * K.tiles_x;
        const uint32_t x = tile_x * REPROJECT_TILE_W + (threadIdx.x & (REPROJECT_TILE_W - 1u)), y = tile_y * REPROJECT_TILE_H + threadIdx.x / REPROJECT_TILE_W;
        if (x >= W || y >= H) continue;
        const uint32_t ip = y * W + x;                                // (< 2^31: plan_reproject)
        const float* c = color_cur + 3u * (size_t)ip;
        const float cr = c[0], cg = c[1], cb = c[2];
        const uint4* g = hits_cur + 3u * (size_t)ip;
        const uint4 g0 = g[0], g1 = g[1], g2 = g[2];
        const uint32_t prim = g2.x;
        float o_r = cr, o_g = cg, o_b = cb, o_w = 1.0f;               // no history
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
                    float ar = 0.0f, ag = 0.0f, ab = 0.0f, ws = 0.0f, L = __builtin_inff();
#pragma unroll
                    for (int dy = 0; dy < 2; ++dy) {
#pragma unroll
                        for (int dx = 0; dx < 2; ++dx) {
                            const uint32_t qx = (uint32_t)(x0 + dx), qy = (uint32_t)(y0 + dy);     // -1 wraps to a value no frame has
                            const bool in = qx < Wp && qy < Hp;
                            const uint32_t iq = in ? qy * Wp + qx : 0u;                            // (< 2^31: plan_reproject)
                            const uint4* h = hits_prev + 3u * (size_t)iq;
                            const uint4 h0 = h[0], h1 = h[1];
                            const uint32_t hprim = reinterpret_cast<const uint32_t*>(h + 2)[0];
                            const float4 m = hist_prev[iq];
                            const float nd = (Nx * __uint_as_float(h1.x) + Ny * __uint_as_float(h1.y)) + Nz * __uint_as_float(h1.z);
                            const float Ex = __uint_as_float(h0.x) - Px, Ey = __uint_as_float(h0.y) - Py, Ez = __uint_as_float(h0.z) - Pz;
                            const float d = fabsf((Nx * Ex + Ny * Ey) + Nz * Ez);
                            const bool valid = in && hprim == prim && nd >= K.normal_min && d <= tol && m.w >= 1.0f && finite_f(m.x) && finite_f(m.y) && finite_f(m.z);
                            const float w = (dx ? tx : 1.0f - tx) * (dy ? ty : 1.0f - ty);
                            if (valid && w > 0.0f) { ar += m.x * w; ag += m.y * w; ab += m.z * w; ws += w; L = fminf(L, m.w); }
                        }
                    }
                    // 3. blend
                    if (ws > 0.0f) {
                        const float hr = ar / ws, hg = ag / ws, hb = ab / ws;
                        const float n = fminf(L + 1.0f, K.max_history_f);
                        const float alpha = 1.0f / n;
                        o_r = hr + (cr - hr) * alpha; o_g = hg + (cg - hg) * alpha; o_b = hb + (cb - hb) * alpha; o_w = n;
                    }
                }
            }
        }
        // 4. outputs: every word of every record
        hist_out[ip] = make_float4(o_r, o_g, o_b, o_w);
        if (out_linear) { float* o = out_linear + 3u * (size_t)ip; o[0] = o_r; o[1] = o_g; o[2] = o_b; }
        if (out_packed) out_packed[ip] = color_to_u32(sqrt3(mk(o_r, o_g, o_b)));
    }
}

int launch_reproject(const ReprojectPlan& plan, const ReprojectBuffers& b, void* stream) {
    hipLaunchKernelGGL(k_post_reproject, dim3(plan.grid), dim3(REPROJECT_BLOCK_THREADS), 0, (hipStream_t)stream, plan.k,
                       reinterpret_cast<const uint4*>(b.hits_cur), reinterpret_cast<const float*>(b.color_cur),
                       reinterpret_cast<const uint4*>(b.hits_prev), reinterpret_cast<const float4*>(b.hist_prev),
                       reinterpret_cast<float4*>(b.hist_out), reinterpret_cast<float*>(b.out_linear), reinterpret_cast<uint32_t*>(b.out_packed));
    return (int)hipGetLastError();
}

}  // namespace mi355rt_post
