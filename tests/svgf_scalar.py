"""A scalar anchor for tests/svgf_ref.py (not a test, not a conftest): the filter and the spatial estimate of step 3' of include/mi355rt_svgf.h
restated a second time, one pixel and one tap at a time -- Python loops over np.float32 scalars, every operation one float32 operation in the
header's order.  It shares no code with svgf_ref.py (lum's three constants are restated from the header): svgf_ref's vectorised slicing -- which
pixel pairs a shifted slice makes, which centre a tap's G belongs to -- is held against it bit for bit by tests/test_svgf_rough_cpu.py, on guides
where a wrong pairing changes G.  Slow by design; use it on small frames."""
import numpy as np

F = np.float32
NO_HIT = 0xFFFFFFFF
ZERO, ONE = F(0.0), F(1.0)
K = (F(0.375), F(0.25), F(0.0625))
WINDOW = {0: F(0.0625), 1: F(0.125), 2: F(0.25)}       # by the number of zero offsets among (ex, ey)
EPS = F(1e-8)


def lum(r, g, b):
    return (F(0.2126) * r + F(0.7152) * g) + F(0.0722) * b


class Guides:
    def __init__(self, hits, W, H):
        hits = np.asarray(hits).reshape(-1)
        assert len(hits) == W * H
        self.W, self.H = W, H
        self.n, self.P, self.t = hits["normal"].astype(F), hits["position"].astype(F), hits["t"].astype(F)
        self.miss = [int(p) == NO_HIT for p in hits["primitive"]]

    def G(self, p, q, normal_squarings, sigma_plane):
        """The header's G(p, q): p the centre, q the tap (pixel indices); sigma_plane an np.float32."""
        if self.miss[p]:
            return ONE if self.miss[q] else ZERO
        if self.miss[q]:
            return ZERO
        n_p, n_q, P_p, P_q = self.n[p], self.n[q], self.P[p], self.P[q]
        nd = (n_p[0] * n_q[0] + n_p[1] * n_q[1]) + n_p[2] * n_q[2]
        wn = nd if nd > 0 else ZERO
        for _ in range(normal_squarings):
            wn = wn * wn
        Dx, Dy, Dz = P_q[0] - P_p[0], P_q[1] - P_p[1], P_q[2] - P_p[2]
        d = abs((n_p[0] * Dx + n_p[1] * Dy) + n_p[2] * Dz)
        e = ONE - d / (sigma_plane * self.t[p])
        wp = e if e > 0 else ZERO
        G = wn * wp
        assert isinstance(G, np.float32)
        return G


def finite(v):
    return bool(np.isfinite(v))


def spatial_variance(hits, colour, W, H, min_temporal=4, normal_squarings=5, sigma_plane=0.05):
    """float32 [W * H]: d_variance_out of mi355rt_svgf_accumulate without a previous frame -- no pixel is TEMPORAL, every moments_out is {l, l*l}, every
    length is 1, so every pixel takes step 3''s SPATIAL estimate."""
    g = Guides(hits, W, H)
    c = np.ascontiguousarray(colour, F).reshape(-1, 3)
    sp, mt = F(sigma_plane), F(min_temporal)
    out = np.empty(W * H, F)
    with np.errstate(all="ignore"):
        m1 = [lum(c[i, 0], c[i, 1], c[i, 2]) for i in range(W * H)]
        m2 = [l * l for l in m1]
        for y in range(H):
            for x in range(W):
                p = y * W + x
                a1 = a2 = ws2 = ZERO
                for dy in range(-3, 4):
                    for dx in range(-3, 4):
                        qx, qy = x + dx, y + dy
                        if not (0 <= qx < W and 0 <= qy < H):
                            continue
                        q = qy * W + qx
                        G = g.G(p, q, normal_squarings, sp)
                        if not (G > 0) or not finite(m1[q]) or not finite(m2[q]):
                            continue
                        a1, a2, ws2 = a1 + m1[q] * G, a2 + m2[q] * G, ws2 + G
                if ws2 > 0:
                    M1, M2 = a1 / ws2, a2 / ws2
                    v = M2 - M1 * M1
                    n = ONE
                    b = mt / n if n < mt else ONE
                    var = (v if v > 0 else ZERO) * b
                else:
                    var = ZERO
                assert isinstance(var, np.float32)
                out[p] = var
    return out


def filter_levels(hist, variance, hits, W, H, levels=5, normal_squarings=5, sigma_luminance=1.0, sigma_plane=0.05):
    """[float32 [H * W, 4]] * (levels + 1): the {r, g, b, v} image before the first level and after each one."""
    g = Guides(hits, W, H)
    img = np.empty((W * H, 4), F)
    img[:, :3] = np.ascontiguousarray(hist, F).reshape(-1, 4)[:, :3]
    img[:, 3] = np.ascontiguousarray(variance, F).reshape(-1)
    sl2, sp = F(sigma_luminance) * F(sigma_luminance), F(sigma_plane)
    assert isinstance(sl2, np.float32)
    out = [img]
    with np.errstate(all="ignore"):
        for k in range(levels):
            s = 1 << k
            src, dst = out[-1], np.empty((W * H, 4), F)
            L = [lum(src[i, 0], src[i, 1], src[i, 2]) for i in range(W * H)]
            for y in range(H):
                for x in range(W):
                    p = y * W + x
                    num = den = ZERO
                    for ey in (-1, 0, 1):
                        for ex in (-1, 0, 1):
                            rx, ry = x + ex, y + ey
                            if not (0 <= rx < W and 0 <= ry < H):
                                continue
                            gw = WINDOW[(ex == 0) + (ey == 0)]
                            num, den = num + gw * src[ry * W + rx, 3], den + gw
                    gv = num / den
                    e = sl2 * (gv if gv > 0 else ZERO) + EPS
                    a = ONE / e
                    ar = ag = ab = av = ws = ZERO
                    for dy in range(-2, 3):
                        for dx in range(-2, 3):
                            qx, qy = x + dx * s, y + dy * s
                            if not (0 <= qx < W and 0 <= qy < H):
                                continue
                            q = qy * W + qx
                            h = K[abs(dy)] * K[abs(dx)]
                            dl = L[q] - L[p]
                            wl = ONE / (ONE + (dl * dl) * a)
                            w = (h * g.G(p, q, normal_squarings, sp)) * wl
                            if not (w > 0):
                                continue
                            cq = src[q]
                            ar, ag, ab, av, ws = ar + cq[0] * w, ag + cq[1] * w, ab + cq[2] * w, av + cq[3] * (w * w), ws + w
                    assert isinstance(ws, np.float32) and isinstance(a, np.float32)
                    dst[p] = (ar / ws, ag / ws, ab / ws, av / (ws * ws)) if ws > 0 else src[p]
            out.append(dst)
    return out
