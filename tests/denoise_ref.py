"""The denoiser of include/mi355rt.h (mi355rt_context_denoise), restated in numpy float32 from the header's definition -- not from the kernels.

One rounding per operation, in the order the header writes them, IEEE division: with the library built without FMA contraction the kernels'
result is this one bit for bit.  Vectorised per tap: for tap (dy, dx) at step s, every pixel p whose tap q = p + (dx*s, dy*s) lies inside the
window is handled at once, as two shifted views of the same arrays; the taps come in the header's order (dy outer, dx inner), so every
pixel's sums receive their terms in the kernel's order."""
import numpy as np

F = np.float32
NO_HIT = 0xFFFFFFFF
K = (F(0.375), F(0.25), F(0.0625))                                       # 3/8, 1/4, 1/16
DEFAULTS = dict(levels=5, normal_squarings=5, sigma_color=2.0, sigma_plane=0.05)


def level_constants(sigma_color, k):
    """(step, a_k): sigma_k = sigma_color * 2^-k, a_k = 1 / (sigma_k * sigma_k), in f32."""
    sigma = F(sigma_color) * F(2.0 ** -k)
    with np.errstate(all="ignore"):
        a = F(1.0) / (sigma * sigma)
    assert isinstance(a, np.float32)
    return 1 << k, a


def denoise(linear, hits, levels=5, normal_squarings=5, sigma_color=2.0, sigma_plane=0.05):
    """linear: float32 [rows, W, 3]; hits: HIT_DTYPE records (position, t, normal, primitive) of the same window, any shape of rows * W.
    Returns float32 [rows, W, 3]."""
    c = np.array(linear, dtype=F, copy=True)
    assert c.ndim == 3 and c.shape[2] == 3 and linear.dtype == F
    R, W = c.shape[:2]
    hits = hits.reshape(R, W)
    n, P, t = hits["normal"].astype(F, copy=False), hits["position"].astype(F, copy=False), hits["t"].astype(F, copy=False)
    miss = hits["primitive"] == NO_HIT
    sp = F(sigma_plane)
    with np.errstate(all="ignore"):
        for k in range(levels):
            s, a = level_constants(sigma_color, k)
            acc, ws = np.zeros((R, W, 3), F), np.zeros((R, W), F)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    oy, ox = dy * s, dx * s
                    y0, y1, x0, x1 = max(0, -oy), min(R, R - oy), max(0, -ox), min(W, W - ox)
                    if y0 >= y1 or x0 >= x1:
                        continue                                         # the tap is outside the window for every pixel
                    p = (slice(y0, y1), slice(x0, x1))
                    q = (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
                    h = K[abs(dy)] * K[abs(dx)]
                    npx, npy, npz = n[p][..., 0], n[p][..., 1], n[p][..., 2]
                    nd = (npx * n[q][..., 0] + npy * n[q][..., 1]) + npz * n[q][..., 2]
                    wn = np.where(nd > 0, nd, F(0))
                    for _ in range(normal_squarings):
                        wn = wn * wn
                    D = P[q] - P[p]
                    d = np.abs((npx * D[..., 0] + npy * D[..., 1]) + npz * D[..., 2])
                    e = F(1) - d / (sp * t[p])
                    wp = np.where(e > 0, e, F(0))
                    G = wn * wp
                    G = np.where(miss[p], np.where(miss[q], F(1), F(0)), np.where(miss[q], F(0), G))
                    dc = c[q] - c[p]
                    d2 = (dc[..., 0] * dc[..., 0] + dc[..., 1] * dc[..., 1]) + dc[..., 2] * dc[..., 2]
                    wc = F(1) / (F(1) + d2 * a)
                    w = (h * G) * wc
                    assert w.dtype == F and G.dtype == F and wc.dtype == F
                    take = w > 0                                         # a NaN weight is not > 0: the tap is skipped
                    acc[p] = np.where(take[..., None], acc[p] + c[q] * w[..., None], acc[p])
                    ws[p] = np.where(take, ws[p] + w, ws[p])
            out = np.where((ws > 0)[..., None], acc / ws[..., None], c)
            assert out.dtype == F and acc.dtype == F and ws.dtype == F
            c = out
    return c


def rmse(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))
