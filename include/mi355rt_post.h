/* mi355rt_post.h -- image-space post stages on device buffers: libmi355rt_post.so.
 *
 * A library of its own beside libmi355rt.so: a stage here needs no scene and no context, only a device and a stream.  It shares the records of
 * mi355rt.h (mi355rt_view, mi355rt_hit, the error codes) and nothing else: a host may link either library without the other.  Nothing aborts and
 * nothing throws across this ABI; a call that fails returns a negative MI355RT_ERR_* code and leaves a text in mi355rt_post_last_error().
 *
 * ---- temporal reprojection: reuse of the previous frame's history ------------------------------------------------------------------------
 * A host that moves a camera at a few samples per frame keeps, per pixel, a HISTORY {r, g, b, length}: the running mean of the colour seen at
 * that surface point and the number of frames in it.  mi355rt_post_reproject makes this frame's history from this frame's colour and the
 * previous frame's history, found by projecting each pixel's first hit into the previous view.  The first-hit records are those of
 * mi355rt_context_view_rays(MI355RT_VIEW_CENTRE) + mi355rt_context_trace_rays, the colour is mi355rt_context_render_view's d_out_linear, and
 * the result is what mi355rt_context_denoise takes as its input, guided by the current records.
 *
 * DEFINITION.  All arithmetic is float32, one rounding per operation, in the order written, with IEEE division.  W x H is cur's size, W' x H'
 *   is prev's; cam' is prev->camera, USED AS GIVEN: an orthonormal basis is the caller's business (as a probe's normal is).  Of a view only
 *   camera, width and height are read (model must be a known one: the guides of both models are the pinhole rays through `position`, so one
 *   projection serves both).  Pixel (x, y) is pixel i = y * W + x (row-major, row 0 = top).  Let g = hits_cur[i] and c = color_cur[i].
 *
 *   There is NO HISTORY when prev_or_null is NULL, when g.primitive == MI355RT_NO_HIT, when the projection (1) fails, or when no tap of (2) is
 *   counted (ws == 0).  With no history out = {c.r, c.g, c.b, 1.0f}.  Otherwise:
 *
 *   1. PROJECTION.  D = g.position - cam'.position (per component).  With f = cam'.forward:  z = (D.x*f.x + D.y*f.y) + D.z*f.z;  a is the same
 *      with cam'.right, b the same with cam'.true_up.  The projection fails unless z > 0.
 *        sx = a / (z * half_width'),   sy = b / (z * half_height'),
 *        u = (sx + 1) * 0.5,           v = (1 - sy) * 0.5,
 *        fx = u * (float)W' - 0.5,     fy = v * (float)H' - 0.5.
 *      The projection fails unless fx > -1 && fx < (float)W' && fy > -1 && fy < (float)H' (a NaN fails here too).
 *        x0 = floor(fx), y0 = floor(fy) (integers),   tx = fx - (float)x0,   ty = fy - (float)y0.
 *   2. TAPS.  acc = {0, 0, 0}, ws = 0, L = +inf.  For dy = 0, 1 (outer loop) and dx = 0, 1 (inner loop), q = (x0 + dx, y0 + dy).  A tap outside
 *      [0, W') x [0, H') is skipped.  Let h = hits_prev[q] and m = hist_prev[q] = {r, g, b, w}.  The tap is VALID iff all of
 *        h.primitive == g.primitive;
 *        nd = (g.n.x*h.n.x + g.n.y*h.n.y) + g.n.z*h.n.z >= normal_min                                    (n = normal);
 *        d = |(g.n.x*E.x + g.n.y*E.y) + g.n.z*E.z| <= plane_tolerance * g.t   with E = h.position - g.position;
 *        m.w >= 1.0f;
 *        m.r, m.g and m.b are all finite.
 *      An invalid tap is skipped.  Its weight is w = (dx ? tx : 1 - tx) * (dy ? ty : 1 - ty); a tap with !(w > 0) is skipped.  Otherwise
 *        acc.ch += m.ch * w  (ch = r, g, b),   ws += w,   L = min(L, m.w).
 *   3. BLEND.  If ws > 0:   hc.ch = acc.ch / ws;   n = min(L + 1.0f, (float)max_history);   alpha = 1.0f / n;
 *        out.ch = hc.ch + (c.ch - hc.ch) * alpha;   out.w = n.
 *   4. OUTPUTS.  d_hist_out[i] = out.  d_out_linear, if given, receives out.rgb; d_out_packed, if given, color_to_u32(sqrt(out.rgb)): the word
 *      0x00RRGGBB every render call packs (sqrt, clamp to [0, 1], * 255, truncate: src/color.rs:87-93).  Every word of every output record is
 *      written, and nothing is written past pixel W * H - 1.
 *
 * CONSEQUENCES.
 *   A non-finite c shows in this frame's output and is dropped as history by the next frame (its tap is invalid): the history heals.
 *   A disoccluded pixel -- another primitive, another plane, a turned normal, out of prev's frame, behind prev's camera -- restarts at length 1.
 *   The length of a pixel that keeps its history grows by one per frame up to max_history and stays there: alpha >= 1 / max_history.
 *   A static camera is NOT bitwise the running mean: fx only rounds near x, so a pixel takes a little of its neighbours (of the order of
 *   2^-22 W' of their weight).
 *
 * BUFFERS.  DEVICE pointers of hip_device.  d_hits_cur: W*H mi355rt_hit; d_color_cur: W*H*3 float; d_hits_prev: W'*H' mi355rt_hit;
 *   d_hist_prev: W'*H' float4; d_hist_out: W*H float4; d_out_linear: W*H*3 float; d_out_packed: W*H uint32.  Hit records and float4 buffers
 *   must be 16-byte aligned, float and packed buffers 4-byte aligned.  d_out_linear MAY be d_color_cur (a pixel's colour is read before its
 *   output is written, and no other pixel reads it).  d_hist_out must not be d_hist_prev: the taps gather neighbours.  Any other overlap of
 *   an output with an input or another output is the caller's business: the call does not look for it.
 *
 * THE CALL only enqueues on hip_stream (NULL: the default stream of hip_device) and returns; it allocates nothing, keeps no state, reads no
 *   environment variable.  hip_device becomes the calling thread's current device, as with the context calls of mi355rt.h.  The kernel cannot
 *   fail: no atomics, no waits, bounded work.
 *
 * REFUSALS, all decided before any HIP call, MI355RT_ERR_INVALID with a text that names the argument: a null cur; an unknown model, a zero
 *   width or height or a camera field that is not finite, in either view; W * H or W' * H' >= 2^31; max_history outside 1 .. 65535, flags != 0,
 *   normal_min not finite or outside [-1, 1], plane_tolerance not finite or not > 0; a null or misaligned d_hits_cur, d_color_cur or
 *   d_hist_out; a misaligned d_out_linear or d_out_packed; prev given with a null or misaligned d_hits_prev or d_hist_prev, or one of those
 *   given without prev; d_hist_out == d_hist_prev; a negative hip_device.  After the argument checks: MI355RT_ERR_NO_DEVICE when no HIP
 *   device is visible or hip_device is out of range (there is no CPU path).
 *
 * NOT BUILT: reprojecting misses by direction (a sky), motion of objects, a multi-GPU form.  (Moment buffers and variance-guided filtering are
 * built beside this library, on the same steps 1 to 3: mi355rt_svgf.h.)
 */
#ifndef MI355RT_POST_H
#define MI355RT_POST_H

#include "mi355rt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MI355RT_POST_ABI_VERSION 1u

typedef struct mi355rt_reproject_params {   /* 16 bytes */
    uint32_t max_history;      /* 1 .. 65535: the running mean's length is clamped here (alpha >= 1/max_history) */
    uint32_t flags;            /* must be 0 */
    float    normal_min;       /* finite, in [-1, 1]: a tap needs n_cur . n_prev >= normal_min */
    float    plane_tolerance;  /* > 0, finite: a tap needs |n_cur . (P_prev - P_cur)| <= plane_tolerance * t_cur */
} mi355rt_reproject_params;     /* params_or_null == NULL: {32, 0, 0.9f, 0.05f} */

const char* mi355rt_post_last_error(void);   /* thread-local, as mi355rt_last_error */
uint32_t    mi355rt_post_abi_version(void);  /* MI355RT_POST_ABI_VERSION */
int mi355rt_post_reproject(int hip_device,
        const mi355rt_view* cur, const mi355rt_view* prev_or_null, const mi355rt_reproject_params* params_or_null,
        const void* d_hits_cur, const void* d_color_cur,
        const void* d_hits_prev_or_null, const void* d_hist_prev_or_null,
        void* d_hist_out,
        void* d_out_linear_or_null, void* d_out_packed_or_null,
        void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* MI355RT_POST_H */
