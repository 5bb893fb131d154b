"""The variance-guided temporal filter of include/mi355rt_svgf.h restated in numpy float32 (not a test, not a conftest): written from the DEFINITIONS
there, formula by formula, one rounding per operation in the order written -- every numpy operation below is one float32 operation on float32
operands, and numpy fuses nothing.  The tests compare the bytes of mi355rt_svgf_accumulate and mi355rt_svgf_filter with it and check its properties
without a GPU.  Steps 1 and 2 of accumulate are restated here from mi355rt_post.h (the header says they are the reprojection's, word for word);
tests/test_svgf_cpu.py holds this restatement's hist_out against tests/reproject_ref.py bit for bit."""
import numpy as np

from device_buffers import packed_of  # noqa: F401  -- re-exported: out_packed is packed_of(out_linear)
from reproject_ref import project

F = np.float32
NO_HIT = 0xFFFFFFFF
K = (F(0.375), F(0.25), F(0.0625))                                       # 3/8, 1/4, 1/16
ACCUMULATE_DEFAULTS = (32, 0, 0.9, 0.05, 4, 5, 0.05, 0)                  # max_history, flags, normal_min, plane_tolerance, min_temporal, normal_squarings, sigma_plane, reserved
FILTER_DEFAULTS = dict(levels=5, normal_squarings=5, sigma_luminance=1.0, sigma_plane=0.05)
# the ways out of accumulate, per pixel (`way` of accumulate's result)
TEMPORAL, SPATIAL_SHORT, SPATIAL_RESTART, NO_HISTORY, MISS = 0, 1, 2, 3, 4


def lum(c):
    """(0.2126f*r + 0.7152f*g) + 0.0722f*b"""
    r = (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]
    assert r.dtype == F
    return r


def _dot3(ax, ay, az, bx, by, bz):
    r = (ax * bx + ay * by) + az * bz
    assert r.dtype == F
    return r


def geometry_weight(n, P, t, miss, p, q, normal_squarings, sigma_plane):
    """G(p, q) for the pixels of the index expression p (centres) and q (their taps), from [rows, W] arrays of the records."""
    npx, npy, npz = n[p][..., 0], n[p][..., 1], n[p][..., 2]
    nd = _dot3(npx, npy, npz, n[q][..., 0], n[q][..., 1], n[q][..., 2])
    wn = np.where(nd > 0, nd, F(0))
    for _ in range(normal_squarings):
        wn = wn * wn
    D = P[q] - P[p]
    d = np.abs(_dot3(npx, npy, npz, D[..., 0], D[..., 1], D[..., 2]))
    e = F(1) - d / (F(sigma_plane) * t[p])
    wp = np.where(e > 0, e, F(0))
    G = wn * wp
    G = np.where(miss[p], np.where(miss[q], F(1), F(0)), np.where(miss[q], F(0), G))
    assert G.dtype == F
    return G


def _shifted(R, W, oy, ox):
    """(p, q): the slices of the pixels whose tap at offset (oy, ox) lies in the frame, and of those taps; None where there is none."""
    y0, y1, x0, x1 = max(0, -oy), min(R, R - oy), max(0, -ox), min(W, W - ox)
    if y0 >= y1 or x0 >= x1:
        return None
    return (slice(y0, y1), slice(x0, x1)), (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))


def _params(params):
    if params is None:
        params = ACCUMULATE_DEFAULTS
    if not isinstance(params, tuple):
        params = (params.max_history, params.flags, params.normal_min, params.plane_tolerance, params.min_temporal, params.normal_squarings, params.sigma_plane, params.reserved)
    return params


def accumulate(cur, prev, hits_cur, color_cur, hits_prev=None, hist_prev=None, moments_prev=None, params=None):
    """(hist_out float32 [n, 4], moments_out float32 [n, 2], variance_out float32 [n], way uint8 [n]) for cur / prev: views (prev None: no previous
    frame); hits_*: abi.HIT_DTYPE records; color_cur float32 [n, 3]; hist_prev float32 [n', 4]; moments_prev float32 [n', 2]; params: the eight fields
    as a tuple, an abi.SvgfAccumulateParams, or None for the defaults.  `way` names how each pixel left (TEMPORAL ... MISS): for the tests' coverage."""
    max_history, _, normal_min, plane_tolerance, min_temporal, normal_squarings, sigma_plane, _ = _params(params)
    max_history, min_temporal, normal_squarings = int(max_history), int(min_temporal), int(normal_squarings)
    normal_min, plane_tolerance = F(normal_min), F(plane_tolerance)
    W, H = cur.width, cur.height
    n = W * H
    g = np.asarray(hits_cur).reshape(-1)
    c = np.ascontiguousarray(color_cur, F).reshape(-1, 3)
    assert len(g) == n and len(c) == n
    miss = g["primitive"] == NO_HIT
    with np.errstate(all="ignore"):
        l = lum(c)
        l2 = l * l
    hist = np.empty((n, 4), F)
    hist[:, :3], hist[:, 3] = c, F(1.0)
    mo = np.stack([l, l2], axis=1)
    temporal = np.zeros(n, bool)
    way = np.where(miss, MISS, NO_HISTORY).astype(np.uint8)
    if prev is not None:
        Wp, Hp = prev.width, prev.height
        hp = np.asarray(hits_prev).reshape(-1)
        mp = np.ascontiguousarray(hist_prev, F).reshape(-1, 4)
        mmp = np.ascontiguousarray(moments_prev, F).reshape(-1, 2)
        assert len(hp) == Wp * Hp and len(mp) == Wp * Hp and len(mmp) == Wp * Hp
        ok, fx, fy, _ = project(g["position"], prev)                     # step 1
        ok &= ~miss
        with np.errstate(all="ignore"):
            flx, fly = np.floor(np.where(ok, fx, F(0.0))), np.floor(np.where(ok, fy, F(0.0)))
            x0, y0 = flx.astype(np.int64), fly.astype(np.int64)
            tx, ty = fx - x0.astype(F), fy - y0.astype(F)
            gn, gp = g["normal"], g["position"]
            tol = plane_tolerance * g["t"]
            acc, macc, ws, L = np.zeros((n, 3), F), np.zeros((n, 2), F), np.zeros(n, F), np.full(n, np.inf, F)
            for dy in (0, 1):                                            # step 2
                for dx in (0, 1):
                    qx, qy = x0 + dx, y0 + dy
                    inside = ok & (qx >= 0) & (qx < Wp) & (qy >= 0) & (qy < Hp)
                    iq = np.where(inside, qy * Wp + qx, 0)
                    h, m, mm = hp[iq], mp[iq], mmp[iq]
                    hn, hpos = h["normal"], h["position"]
                    nd = _dot3(gn[:, 0], gn[:, 1], gn[:, 2], hn[:, 0], hn[:, 1], hn[:, 2])
                    Ex, Ey, Ez = hpos[:, 0] - gp[:, 0], hpos[:, 1] - gp[:, 1], hpos[:, 2] - gp[:, 2]
                    d = np.abs(_dot3(gn[:, 0], gn[:, 1], gn[:, 2], Ex, Ey, Ez))
                    valid = inside & (h["primitive"] == g["primitive"]) & (nd >= normal_min) & (d <= tol) & (m[:, 3] >= F(1.0)) & np.isfinite(m[:, :3]).all(axis=1)
                    w = (tx if dx else F(1.0) - tx) * (ty if dy else F(1.0) - ty)
                    assert w.dtype == F
                    use = valid & (w > F(0.0))
                    acc = np.where(use[:, None], acc + m[:, :3] * w[:, None], acc)
                    macc = np.where(use[:, None], macc + mm * w[:, None], macc)
                    ws = np.where(use, ws + w, ws)
                    L = np.where(use, np.minimum(L, m[:, 3]), L)
            assert acc.dtype == F and macc.dtype == F and ws.dtype == F and L.dtype == F
            hc = acc / ws[:, None]                                       # step 3
            nlen = np.minimum(L + F(1.0), F(max_history))
            alpha = F(1.0) / nlen
            blended = hc + (c - hc) * alpha[:, None]
            hm = macc / ws[:, None]                                      # step 2'
            m1 = hm[:, 0] + (l - hm[:, 0]) * alpha
            m2 = hm[:, 1] + (l2 - hm[:, 1]) * alpha
            assert blended.dtype == F and m1.dtype == F and m2.dtype == F
        have = ws > F(0.0)
        hist[have, :3], hist[have, 3] = blended[have], nlen[have]
        sound = have & np.isfinite(hm).all(axis=1)
        mo[sound, 0], mo[sound, 1] = m1[sound], m2[sound]
        temporal = sound & (nlen >= F(min_temporal))
        way[have & ~sound] = SPATIAL_RESTART
        way[sound & ~temporal] = SPATIAL_SHORT
        way[temporal] = TEMPORAL
    # step 3'
    with np.errstate(all="ignore"):
        v = mo[:, 1] - mo[:, 0] * mo[:, 0]
        var_t = np.where(v > 0, v, F(0))
        gh = g.reshape(H, W)
        nrm, P, t, miss2 = gh["normal"].astype(F, copy=False), gh["position"].astype(F, copy=False), gh["t"].astype(F, copy=False), miss.reshape(H, W)
        M = mo.reshape(H, W, 2)
        a1, a2, ws2 = np.zeros((H, W), F), np.zeros((H, W), F), np.zeros((H, W), F)
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                pq = _shifted(H, W, dy, dx)
                if pq is None:
                    continue
                p, q = pq
                G = geometry_weight(nrm, P, t, miss2, p, q, normal_squarings, sigma_plane)
                take = (G > 0) & np.isfinite(M[q]).all(axis=-1)
                a1[p] = np.where(take, a1[p] + M[q][..., 0] * G, a1[p])
                a2[p] = np.where(take, a2[p] + M[q][..., 1] * G, a2[p])
                ws2[p] = np.where(take, ws2[p] + G, ws2[p])
        M1, M2 = a1 / ws2, a2 / ws2
        vs = M2 - M1 * M1
        nl = hist[:, 3].reshape(H, W)
        b = np.where(nl < F(min_temporal), F(min_temporal) / nl, F(1.0))
        var_s = np.where(ws2 > 0, np.where(vs > 0, vs, F(0)) * b, F(0)).reshape(-1)
        assert var_s.dtype == F and var_t.dtype == F and b.dtype == F
    var = np.where(temporal, var_t, var_s)
    return hist, mo, var, way


def filter(hist, variance, hits, width, height, levels=5, normal_squarings=5, sigma_luminance=1.0, sigma_plane=0.05):
    """float32 [height, width, 3]: d_out_linear (d_out_packed is packed_of(it)).  hist float32 [n, 4] (its .w is ignored), variance float32 [n],
    hits abi.HIT_DTYPE records of the frame.  The last level's variance is not an output of the call."""
    return filter_levels(hist, variance, hits, width, height, levels, normal_squarings, sigma_luminance, sigma_plane)[..., :3]


def filter_levels(hist, variance, hits, width, height, levels=5, normal_squarings=5, sigma_luminance=1.0, sigma_plane=0.05):
    """float32 [height, width, 4]: the {r, g, b, v} image after `levels` levels (what the scratch holds between two levels)."""
    R, W = height, width
    img = np.empty((R, W, 4), F)
    img[..., :3] = np.ascontiguousarray(hist, F).reshape(R, W, 4)[..., :3]
    img[..., 3] = np.ascontiguousarray(variance, F).reshape(R, W)
    hits = np.asarray(hits).reshape(R, W)
    n, P, t = hits["normal"].astype(F, copy=False), hits["position"].astype(F, copy=False), hits["t"].astype(F, copy=False)
    miss = hits["primitive"] == NO_HIT
    sl2 = F(sigma_luminance) * F(sigma_luminance)
    assert isinstance(sl2, np.float32)
    with np.errstate(all="ignore"):
        for k in range(levels):
            s = 1 << k
            c, v = img[..., :3], img[..., 3]
            num, den = np.zeros((R, W), F), np.zeros((R, W), F)          # the centre variance: 3 x 3 at step 1
            for ey in (-1, 0, 1):
                for ex in (-1, 0, 1):
                    pq = _shifted(R, W, ey, ex)
                    if pq is None:
                        continue
                    p, q = pq
                    g = F(0.25) if (ex == 0 and ey == 0) else F(0.125) if (ex == 0 or ey == 0) else F(0.0625)
                    num[p] = num[p] + g * v[q]
                    den[p] = den[p] + g
            gv = num / den
            e = sl2 * np.where(gv > 0, gv, F(0)) + F(1e-8)
            a = F(1.0) / e
            lp = lum(c)
            assert a.dtype == F and lp.dtype == F
            acc, accv, ws = np.zeros((R, W, 3), F), np.zeros((R, W), F), np.zeros((R, W), F)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    pq = _shifted(R, W, dy * s, dx * s)
                    if pq is None:
                        continue                                         # the tap is outside the frame for every pixel
                    p, q = pq
                    h = K[abs(dy)] * K[abs(dx)]
                    G = geometry_weight(n, P, t, miss, p, q, normal_squarings, sigma_plane)
                    dl = lp[q] - lp[p]
                    wl = F(1.0) / (F(1.0) + (dl * dl) * a[p])
                    w = (h * G) * wl
                    assert w.dtype == F and wl.dtype == F
                    take = w > 0                                         # a NaN weight is not > 0: the tap is skipped
                    acc[p] = np.where(take[..., None], acc[p] + c[q] * w[..., None], acc[p])
                    accv[p] = np.where(take, accv[p] + v[q] * (w * w), accv[p])
                    ws[p] = np.where(take, ws[p] + w, ws[p])
            out = np.empty((R, W, 4), F)
            any_ = ws > 0
            out[..., :3] = np.where(any_[..., None], acc / ws[..., None], c)
            out[..., 3] = np.where(any_, accv / (ws * ws), v)
            assert acc.dtype == F and accv.dtype == F and ws.dtype == F
            img = out
    return img


def rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64).reshape(-1, 3) - np.asarray(b, np.float64).reshape(-1, 3)) ** 2)))
