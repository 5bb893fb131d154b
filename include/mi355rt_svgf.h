/* mi355rt_svgf.h -- a variance-guided temporal filter on device buffers: libmi355rt_svgf.so.
 *
 * A library of its own beside libmi355rt.so and libmi355rt_post.so: a stage here needs no scene and no context, only a device and a stream.  It
 * shares the records of mi355rt.h (mi355rt_view, mi355rt_hit, the error codes) and nothing else: a host may link any of the three without the
 * others.  Nothing aborts and nothing throws across this ABI; a call that fails returns a negative MI355RT_ERR_* code and leaves a text in
 * mi355rt_svgf_last_error().  Not part of the reference; an independent restatement of the definitions below in float32 is bit-identical to the
 * kernels (the library is built without FMA contraction).
 *
 * The two calls close the real-time route: mi355rt_context_render_view -> first hits (view_rays(MI355RT_VIEW_CENTRE) + trace_rays) ->
 * mi355rt_svgf_accumulate -> mi355rt_svgf_filter.  ACCUMULATE is mi355rt_post_reproject with a history of the luminance moments beside the colour
 * history and a per-pixel VARIANCE made from it; FILTER is the a-trous filter of mi355rt_context_denoise with its colour weight scaled by that
 * variance: a pixel whose history has converged is no longer blurred, a pixel disoccluded this frame is.
 *
 * ARITHMETIC of both definitions: float32 throughout, one rounding per operation, in the order written, IEEE division.  No transcendental
 * anywhere: the stage is + - * / and compares (the packed output's square root is the render's own packing).
 *   lum(c) = (0.2126f*c.r + 0.7152f*c.g) + 0.0722f*c.b.
 *   G(p, q), the GEOMETRY WEIGHT of a tap q seen from the centre p, is mi355rt_context_denoise's, with the call's normal_squarings and sigma_plane:
 *     a pixel is a MISS when its record's primitive == MI355RT_NO_HIT.  p a miss: G = 1 if q is a miss, else 0.  p a hit, q a miss: G = 0.  Otherwise
 *       nd = (n_p.x*n_q.x + n_p.y*n_q.y) + n_p.z*n_q.z;   wn = nd > 0 ? nd : 0, then wn = wn*wn repeated normal_squarings times;
 *       D = P_q - P_p;   d = |(n_p.x*D.x + n_p.y*D.y) + n_p.z*D.z|;   e = 1 - d / (sigma_plane * t_p);   wp = e > 0 ? e : 0;   G = wn * wp.
 *
 * ---- mi355rt_svgf_accumulate --------------------------------------------------------------------------------------------------------------
 * W x H is cur's size, W' x H' prev's; pixel (x, y) is pixel i = y * W + x.  g = hits_cur[i], c = color_cur[i], l = lum(c).
 *   Steps 1 (PROJECTION) and 2 (TAPS: the four taps, their validity, weights and order) are mi355rt_post_reproject's (mi355rt_post.h), word for
 *   word, with this call's max_history, normal_min and plane_tolerance; so are its cases of NO HISTORY and its step 3 (BLEND).  d_hist_out is
 *   therefore bit for bit what mi355rt_post_reproject writes for the same inputs: out = {r, g, b, n}.
 *   A COUNTED tap q additionally adds its moments: macc.k += mm.k * w (k = m1, m2) with mm = moments_prev[q], macc = {0, 0} before the taps.
 *   2'. MOMENTS.  n = out.w and alpha = 1.0f / n as in step 3.
 *      With history (ws > 0): hm.k = macc.k / ws.
 *        hm.m1 and hm.m2 both finite:   mo.m1 = hm.m1 + (l - hm.m1) * alpha,   mo.m2 = hm.m2 + (l*l - hm.m2) * alpha,
 *                                       and the pixel is TEMPORAL iff n >= (float)min_temporal.
 *        otherwise the moments RESTART: mo = {l, l*l}, and the pixel is not TEMPORAL (the colour history goes on: out is step 3's).
 *      Without history:                 mo = {l, l*l}, and the pixel is not TEMPORAL.
 *      d_moments_out[i] = mo.
 *   3'. VARIANCE.  A TEMPORAL pixel:  v = mo.m2 - mo.m1*mo.m1,  var = v > 0 ? v : 0.
 *      Every other pixel p takes a SPATIAL estimate over this frame's moments_out (of all pixels, TEMPORAL or not): a1 = a2 = ws2 = 0; for
 *      dy = -3 .. 3 (outer loop) and dx = -3 .. 3 (inner loop), q = (x + dx, y + dy); a tap outside [0, W) x [0, H) is skipped; a tap with !(G(p, q) > 0),
 *      or with a moments_out[q].m1 or .m2 that is not finite, is skipped; otherwise, with {m1_q, m2_q} = moments_out[q],
 *        a1 += m1_q * G,   a2 += m2_q * G,   ws2 += G.
 *      ws2 > 0:  M1 = a1 / ws2,  M2 = a2 / ws2,  v = M2 - M1*M1,  var = (v > 0 ? v : 0) * b  with
 *                b = n < (float)min_temporal ? (float)min_temporal / n : 1.0f   (a short history's estimate is widened).
 *      ws2 == 0: var = 0.
 *      d_variance_out[i] = var.
 *   Every word of the three outputs is written, and nothing is written past pixel W * H - 1.
 * CONSEQUENCES.  A variance is never NaN and never negative (a NaN v is not > 0).  A non-finite colour gives non-finite moments this frame; the
 *   next frame's taps find them, restart the moments and go on with the colour history (which dropped that colour itself): poisoned moments
 *   heal in one frame.  A constant colour whose pixels land exactly ON previous pixels (one counted tap of weight 1) has variance exactly 0 once
 *   TEMPORAL: hm = mo = {l, l*l} to the bit; elsewhere the rounding of the bilinear weights leaves a variance of the order of 2^-23 l*l, or 0.
 *   A pixel that keeps its history becomes TEMPORAL in the frame in which its length reaches min_temporal (min_temporal <= max_history).
 * BUFFERS.  As mi355rt_post_reproject's, and: d_moments_prev W'*H' float2 {m1, m2}, d_moments_out W*H float2, both 8-byte aligned; d_variance_out
 *   W*H float, 4-byte aligned.  d_hist_out must not be d_hist_prev and d_moments_out must not be d_moments_prev: the taps gather neighbours.  Any
 *   other overlap is the caller's business.  d_hist_out is what mi355rt_svgf_filter takes as d_hist_in, d_variance_out as d_variance_in.
 *
 * ---- mi355rt_svgf_filter ------------------------------------------------------------------------------------------------------------------
 * The image is {r, g, b, v} per pixel; level 0 reads {d_hist_in[i].rgb, d_variance_in[i]} (d_hist_in[i].w is ignored).  p = (x, y) is the centre,
 * c_p its colour, v_p its variance in the image of the previous level.  sl2 = sigma_luminance * sigma_luminance, computed on the host in f32.
 *   Per level k = 0 .. levels-1: step s = 1 << k.  Taps: dy = -2 .. 2 (outer loop), dx = -2 .. 2 (inner loop); q = (x + dx*s, y + dy*s); a tap outside
 *   [0, width) x [0, height) is skipped.  h = K[|dy|] * K[|dx|], K = {3/8, 1/4, 1/16}.  (Taps, their order, K, G and the skip rule are the denoiser's.)
 *   CENTRE VARIANCE.  num = den = 0; for ey = -1 .. 1 (outer loop), ex = -1 .. 1 (inner loop), r = (x + ex, y + ey) AT STEP 1 whatever the level; a tap
 *     outside the frame is skipped; g = 1/4 (ex == 0 && ey == 0), 1/8 (one of them 0), 1/16 (neither);   num += g * v_r,   den += g.
 *     gv = num / den;   e = sl2 * (gv > 0 ? gv : 0) + 1e-8f;   a = 1.0f / e.
 *   COLOUR WEIGHT.  dl = lum(c_q) - lum(c_p);   wl = 1.0f / (1.0f + (dl*dl) * a)     (rational, as the denoiser's: no exp).
 *   ACCUMULATION.  w = (h * G(p, q)) * wl.  A tap with !(w > 0) is SKIPPED.  Otherwise acc.ch += c_q.ch * w (r, g, b), accv += v_q * (w*w), ws += w.
 *   RESULT of the level: ws > 0 ? {acc.ch / ws, accv / (ws*ws)} : {c_p, v_p}.
 *   The last level's rgb goes to d_out_linear and / or, as color_to_u32(sqrt(.)) -- the packing of every render call -- to d_out_packed.
 *   levels == 0 copies d_hist_in's rgb to the outputs (and packs it).
 * CONSEQUENCES.  A pixel with a NaN colour passes through unchanged and contaminates nobody (its weights are NaN, as a tap and as a centre).  A
 *   pixel of variance 0 in a neighbourhood of variance 0 keeps itself, apart from neighbours of equal luminance (a = 1e8).  A non-finite VARIANCE
 *   under a finite colour is the caller's business: it spreads into the variances of the pixels that count it (mi355rt_svgf_accumulate writes none
 *   that is NaN).  Feeding the filtered image back as history is NOT part of this stage: the next frame's accumulate takes the plain d_hist_out.
 * BUFFERS.  d_hist_in width*height float4 (16-byte aligned), d_variance_in width*height float, d_hits width*height mi355rt_hit (16-byte aligned): this
 *   frame's records; d_scratch mi355rt_svgf_scratch_bytes(width, height) bytes, 16-byte aligned (two {r, g, b, v} images and the two 16-byte guide
 *   words per pixel; what it holds afterwards is unspecified); d_out_linear width*height*3 float, d_out_packed width*height uint32, at least one.
 *   With levels >= 1 the first kernel copies the inputs into the scratch and nothing reads them afterwards: an output may be an input.  With
 *   levels == 0 there is no such pass and the outputs' pixels have other sizes than d_hist_in's: an output must not overlap d_hist_in (the
 *   equal pointers are refused; any other overlap is the caller's business).
 *
 * THE CALLS only enqueue on hip_stream (NULL: the default stream of hip_device) and return; they allocate nothing, keep no state, read no
 *   environment variable.  hip_device becomes the calling thread's current device.  The kernels cannot fail: no atomics, no waits, bounded loops.
 * REFUSALS, all decided before any HIP call, MI355RT_ERR_INVALID with a text that names the argument.  accumulate: what mi355rt_post_reproject refuses
 *   of its views, params and buffers, and: min_temporal outside 1 .. max_history, normal_squarings > 8, sigma_plane not finite or not > 0, reserved
 *   != 0; a null or misaligned d_moments_out or d_variance_out; prev given without all three of d_hits_prev, d_hist_prev, d_moments_prev (or one of
 *   them misaligned), or one of those given without prev; d_hist_out == d_hist_prev; d_moments_out == d_moments_prev.  filter: width or height 0,
 *   width * height >= 2^31; levels > 8, normal_squarings > 8, sigma_luminance or sigma_plane not finite or not > 0, or a sigma_luminance whose
 *   square is 0 or infinite; flags with a bit other than MI355RT_SVGF_GATHERS_ONLY, reserved != 0; a null or misaligned d_hist_in, d_variance_in,
 *   d_hits or d_scratch; both outputs null, or one misaligned; with levels == 0, d_out_linear or d_out_packed == d_hist_in.  Both: a negative hip_device.  After the argument checks: MI355RT_ERR_NO_DEVICE when no
 *   HIP device is visible or hip_device is out of range (there is no CPU path).
 *
 * NOT BUILT: a flag of the rt_render tool; feeding a filtered level back as history; reprojecting misses by direction; motion of objects; a
 *   multi-GPU form; any change to mi355rt_context_denoise.
 */
#ifndef MI355RT_SVGF_H
#define MI355RT_SVGF_H

#include "mi355rt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MI355RT_SVGF_ABI_VERSION 1u

typedef struct mi355rt_svgf_accumulate_params {   /* 32 bytes */
    uint32_t max_history;       /* 1 .. 65535: the running means' length is clamped here (alpha >= 1/max_history) */
    uint32_t flags;             /* must be 0 */
    float    normal_min;        /* finite, in [-1, 1]: a tap needs n_cur . n_prev >= normal_min */
    float    plane_tolerance;   /* > 0, finite: a tap needs |n_cur . (P_prev - P_cur)| <= plane_tolerance * t_cur */
    uint32_t min_temporal;      /* 1 .. max_history: a history at least this long gives its own variance */
    uint32_t normal_squarings;  /* 0 .. 8: of the spatial estimate's geometry weight */
    float    sigma_plane;       /* > 0, finite: of the spatial estimate's geometry weight */
    uint32_t reserved;          /* must be 0 */
} mi355rt_svgf_accumulate_params;                 /* params_or_null == NULL: {32, 0, 0.9f, 0.05f, 4, 5, 0.05f, 0} */

#define MI355RT_SVGF_GATHERS_ONLY 1u              /* filter flags: the levels with step 1 and 2 gather from global memory like the later ones (the other side of an A/B; the same bytes) */

typedef struct mi355rt_svgf_filter_params {       /* 24 bytes */
    uint32_t levels;            /* a-trous passes, step 1, 2, 4, ...; 0 .. 8; 0 = copy (and pack) */
    uint32_t normal_squarings;  /* 0 .. 8 */
    float    sigma_luminance;   /* > 0, finite: the colour weight's width in standard deviations of the centre's luminance */
    float    sigma_plane;       /* > 0, finite */
    uint32_t flags;             /* 0 or MI355RT_SVGF_GATHERS_ONLY */
    uint32_t reserved;          /* must be 0 */
} mi355rt_svgf_filter_params;                     /* params_or_null == NULL: {5, 5, 1.0f, 0.05f, 0, 0} */

const char* mi355rt_svgf_last_error(void);   /* thread-local, as mi355rt_last_error */
uint32_t    mi355rt_svgf_abi_version(void);  /* MI355RT_SVGF_ABI_VERSION */
/* Bytes of mi355rt_svgf_filter's d_scratch for a frame of width x height pixels (64 per pixel; the layout is the library's own). */
int mi355rt_svgf_scratch_bytes(uint32_t width, uint32_t height, uint64_t* out_bytes);
int mi355rt_svgf_accumulate(int hip_device,
        const mi355rt_view* cur, const mi355rt_view* prev_or_null, const mi355rt_svgf_accumulate_params* params_or_null,
        const void* d_hits_cur, const void* d_color_cur,
        const void* d_hits_prev_or_null, const void* d_hist_prev_or_null, const void* d_moments_prev_or_null,
        void* d_hist_out, void* d_moments_out, void* d_variance_out,
        void* hip_stream);
int mi355rt_svgf_filter(int hip_device, uint32_t width, uint32_t height, const mi355rt_svgf_filter_params* params_or_null,
        const void* d_hist_in, const void* d_variance_in, const void* d_hits, void* d_scratch,
        void* d_out_linear_or_null, void* d_out_packed_or_null,
        void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* MI355RT_SVGF_H */
