"""The temporal reprojection of include/mi355rt_post.h restated in numpy float32 (not a test, not a conftest): written from the DEFINITION there,
formula by formula, one rounding per operation in the order written -- every numpy operation below is one float32 operation on float32 operands,
and numpy fuses nothing.  The tests compare mi355rt_post_reproject's bytes with it and check its properties without a GPU."""
import numpy as np

from device_buffers import packed_of  # noqa: F401  -- re-exported: out_packed is packed_of(out[:, :3]), and tests/test_reproject_cpu.py pins it here

F = np.float32
NO_HIT = 0xFFFFFFFF
DEFAULTS = (32, 0, 0.9, 0.05)                 # mi355rt_reproject_params for a null pointer: max_history, flags, normal_min, plane_tolerance


def _vec(a):
    return np.array(list(a), F)


def _dot3(ax, ay, az, bx, by, bz):
    """(a.x*b.x + a.y*b.y) + a.z*b.z"""
    r = (ax * bx + ay * by) + az * bz
    assert r.dtype == F
    return r


def project(positions, prev):
    """Step 1 of the definition for float32 positions [n, 3] and the view `prev` (camera, width, height): (ok, fx, fy, z) with ok = the
    projection did not fail."""
    P = np.ascontiguousarray(positions, F).reshape(-1, 3)
    cam = prev.camera
    pos, fwd, right, up = _vec(cam.position), _vec(cam.forward), _vec(cam.right), _vec(cam.true_up)
    with np.errstate(all="ignore"):
        Dx, Dy, Dz = P[:, 0] - pos[0], P[:, 1] - pos[1], P[:, 2] - pos[2]
        z = _dot3(Dx, Dy, Dz, fwd[0], fwd[1], fwd[2])
        a = _dot3(Dx, Dy, Dz, right[0], right[1], right[2])
        b = _dot3(Dx, Dy, Dz, up[0], up[1], up[2])
        sx = a / (z * F(cam.half_width))
        sy = b / (z * F(cam.half_height))
        u = (sx + F(1.0)) * F(0.5)
        v = (F(1.0) - sy) * F(0.5)
        Wf, Hf = F(prev.width), F(prev.height)
        fx = u * Wf - F(0.5)
        fy = v * Hf - F(0.5)
        assert fx.dtype == F and fy.dtype == F and z.dtype == F
        ok = (z > F(0.0)) & (fx > F(-1.0)) & (fx < Wf) & (fy > F(-1.0)) & (fy < Hf)
    return ok, fx, fy, z


def reproject(cur, prev, hits_cur, color_cur, hits_prev=None, hist_prev=None, params=None):
    """float32 [W*H, 4]: d_hist_out.  cur / prev: views (camera, width, height; prev None: no previous frame); hits_*: abi.HIT_DTYPE records;
    color_cur float32 [W*H, 3]; hist_prev float32 [W'*H', 4]; params: (max_history, flags, normal_min, plane_tolerance) or an
    abi.ReprojectParams or None for the defaults.  out_linear is out[:, :3], out_packed is packed_of(out[:, :3])."""
    if params is None:
        params = DEFAULTS
    if not isinstance(params, tuple):
        params = (params.max_history, params.flags, params.normal_min, params.plane_tolerance)
    max_history, _, normal_min, plane_tolerance = int(params[0]), params[1], F(params[2]), F(params[3])
    n = cur.width * cur.height
    g = np.asarray(hits_cur).reshape(-1)
    c = np.ascontiguousarray(color_cur, F).reshape(-1, 3)
    assert len(g) == n and len(c) == n
    out = np.empty((n, 4), F)
    out[:, :3], out[:, 3] = c, F(1.0)
    if prev is None:
        return out
    Wp, Hp = prev.width, prev.height
    hp = np.asarray(hits_prev).reshape(-1)
    mp = np.ascontiguousarray(hist_prev, F).reshape(-1, 4)
    assert len(hp) == Wp * Hp and len(mp) == Wp * Hp
    ok, fx, fy, _ = project(g["position"], prev)
    ok &= g["primitive"] != NO_HIT
    with np.errstate(all="ignore"):
        flx, fly = np.floor(np.where(ok, fx, F(0.0))), np.floor(np.where(ok, fy, F(0.0)))
        x0, y0 = flx.astype(np.int64), fly.astype(np.int64)
        tx, ty = fx - x0.astype(F), fy - y0.astype(F)
        gn, gp = g["normal"], g["position"]
        tol = plane_tolerance * g["t"]
        acc, ws, L = np.zeros((n, 3), F), np.zeros(n, F), np.full(n, np.inf, F)
        for dy in (0, 1):
            for dx in (0, 1):
                qx, qy = x0 + dx, y0 + dy
                inside = ok & (qx >= 0) & (qx < Wp) & (qy >= 0) & (qy < Hp)
                iq = np.where(inside, qy * Wp + qx, 0)
                h, m = hp[iq], mp[iq]
                hn, hpos = h["normal"], h["position"]
                nd = _dot3(gn[:, 0], gn[:, 1], gn[:, 2], hn[:, 0], hn[:, 1], hn[:, 2])
                Ex, Ey, Ez = hpos[:, 0] - gp[:, 0], hpos[:, 1] - gp[:, 1], hpos[:, 2] - gp[:, 2]
                d = np.abs(_dot3(gn[:, 0], gn[:, 1], gn[:, 2], Ex, Ey, Ez))
                valid = inside & (h["primitive"] == g["primitive"]) & (nd >= normal_min) & (d <= tol) & (m[:, 3] >= F(1.0)) & np.isfinite(m[:, :3]).all(axis=1)
                w = (tx if dx else F(1.0) - tx) * (ty if dy else F(1.0) - ty)
                assert w.dtype == F and d.dtype == F and tol.dtype == F
                use = valid & (w > F(0.0))
                acc = np.where(use[:, None], acc + m[:, :3] * w[:, None], acc)
                ws = np.where(use, ws + w, ws)
                L = np.where(use, np.minimum(L, m[:, 3]), L)
        assert acc.dtype == F and ws.dtype == F and L.dtype == F
        hc = acc / ws[:, None]
        nlen = np.minimum(L + F(1.0), F(max_history))
        alpha = F(1.0) / nlen
        blended = hc + (c - hc) * alpha[:, None]
        assert blended.dtype == F and nlen.dtype == F
    have = ws > F(0.0)
    out[have, :3], out[have, 3] = blended[have], nlen[have]
    return out
