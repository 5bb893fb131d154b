"""Cases of the camera views (mi355rt_context_view_rays, mi355rt_context_render_view; not a test, not a conftest): the two ray makers of
include/mi355rt.h in numpy float32, written from the definition there, one rounding per operation in the order written.

They extend tests/radiance_cases.py: the words of (ray 0, block j) come from oracle.ctr_block, u01 and normalized_rows are that module's.  A maker
returns abi.PATH_RAY_DTYPE [H * W], row-major, direction normalised once, x = column, row = y -- what mi355rt_context_view_rays writes."""
import numpy as np

import radiance_cases as RC

F = np.float32
LENS_TRIES = 64

SIZES = [(24, 16), (13, 7)]                  # W * H * S is no multiple of 64 for any S below
SAMPLES = [1, 5, 17]                         # 17 crosses the sum's 16-sample trip
SEEDS = [0, (1 << 32) - 3]                   # the second carries the key into its high word from row 3 on
DEPTH = 6
SCENES = ["cornell", "teapot"]
CAMERAS = ["own", "moved", "inside"]

_words = {}


def block_words(oracle_mod, W, H, s, seed, j=0):
    """uint32 [H * W, 4]: the words of (ray 0, block j) of sample s of every pixel, row-major; ykey = y + seed.  Computed once, read-only."""
    key = (W, H, s, seed, j)
    if key not in _words:
        out = np.zeros((H * W, 4), np.uint32)
        for y in range(H):
            ykey = (y + seed) & 0xFFFFFFFFFFFFFFFF
            k0, k1 = ykey & 0xFFFFFFFF, ykey >> 32
            for x in range(W):
                out[y * W + x] = oracle_mod.ctr_block(k0, k1, x, s, 0, j)
        out.setflags(write=False)
        _words[key] = out
    return _words[key]


def pixel_xy(W, H):
    return np.tile(np.arange(W, dtype=np.uint32), H), np.repeat(np.arange(H, dtype=np.uint32), W)


def uv(oracle_mod, W, H, s, seed, centre):
    x, y = pixel_xy(W, H)
    if centre:
        ju = jv = np.full(H * W, F(0.5))
    else:
        w = block_words(oracle_mod, W, H, s, seed)
        ju, jv = RC.u01(w[:, 0]), RC.u01(w[:, 1])
    u = (x.astype(F) + ju) / F(W)
    v = (y.astype(F) + jv) / F(H)
    assert u.dtype == F and v.dtype == F
    return u, v


def cam_vectors(cam):
    return tuple(np.array(list(a), F) for a in (cam.position, cam.forward, cam.right, cam.true_up))


def camera_raw(cam, u, v):
    """camera.rs:33-42 before its normalisations: forward + (right * ((2u - 1) * half_width) + true_up * ((1 - 2v) * half_height))."""
    _, fwd, right, up = cam_vectors(cam)
    ax = (F(2.0) * u - F(1.0)) * F(cam.half_width)
    ay = (F(1.0) - F(2.0) * v) * F(cam.half_height)
    raw = fwd[None, :] + (right[None, :] * ax[:, None] + up[None, :] * ay[:, None])
    assert raw.dtype == F
    return raw


def _records(abi, W, H, origin, direction):
    rays = np.zeros(H * W, abi.PATH_RAY_DTYPE)
    rays["origin"], rays["direction"] = origin, direction
    rays["x"], rays["row"] = pixel_xy(W, H)
    return rays


def pinhole_rays(oracle_mod, abi, cam, W, H, s, seed=0, centre=False):
    u, v = uv(oracle_mod, W, H, s, seed, centre)
    return _records(abi, W, H, cam_vectors(cam)[0][None, :], RC.normalized_rows(camera_raw(cam, u, v)))


def lens_points(n, block_source, tries=LENS_TRIES):
    """(a, b float32 [n], try number int [n]): rejection in the unit disk.  block_source(j) -> uint32 [n, 4], the words of (ray 0, block j); try j takes
    a = 2 f(w2) - 1, b = 2 f(w3) - 1 and is accepted on a*a + b*b < 1; after `tries` rejected tries (a, b) = (0, 0) and the try number is `tries`."""
    a, b = np.zeros(n, F), np.zeros(n, F)
    tried = np.full(n, tries, np.int64)
    open_ = np.ones(n, bool)
    for j in range(tries):
        if not open_.any():
            break
        w = np.asarray(block_source(j), np.uint32)
        aj = F(2.0) * RC.u01(w[:, 2]) - F(1.0)
        bj = F(2.0) * RC.u01(w[:, 3]) - F(1.0)
        assert aj.dtype == F
        ok = open_ & (aj * aj + bj * bj < F(1.0))
        a[ok], b[ok], tried[ok] = aj[ok], bj[ok], j
        open_ &= ~ok
    return a, b, tried


def thin_lens_rays(oracle_mod, abi, cam, W, H, s, lens_radius, focus_distance, seed=0, centre=False, block_source=None, want_tries=False):
    u, v = uv(oracle_mod, W, H, s, seed, centre)
    n = H * W
    if centre:
        a, b, tried = np.zeros(n, F), np.zeros(n, F), np.zeros(n, np.int64)
    else:
        a, b, tried = lens_points(n, block_source or (lambda j: block_words(oracle_mod, W, H, s, seed, j)))
    pos, _, right, up = cam_vectors(cam)
    off = right[None, :] * (F(lens_radius) * a)[:, None] + up[None, :] * (F(lens_radius) * b)[:, None]
    raw = camera_raw(cam, u, v) * F(focus_distance) - off
    assert off.dtype == F and raw.dtype == F
    rays = _records(abi, W, H, pos[None, :] + off, RC.normalized_rows(raw))
    return (rays, a, b, tried) if want_tries else rays


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------
def camera(name, sc):
    """own: the scene's camera.  moved: off to the side and above, looking where the scene's camera looks, another field of view.  inside: nine tenths of the way to
    that point (in cornell: inside the box), turned to the left and up -- towards a wall."""
    if name == "own":
        return sc.camera
    from oracle import scene_loader as L
    pos, fwd, right, up = (a.astype(np.float64) for a in cam_vectors(sc.camera))
    dist = float(np.linalg.norm(pos)) or 1.0
    target = pos + fwd * dist
    f = lambda a: tuple(float(F(v)) for v in a)
    if name == "moved":
        return L.camera_new(f(pos + right * 0.35 * dist + up * 0.2 * dist), f(target), (0.0, 1.0, 0.0), F(50.0), F(1.5))
    if name == "inside":
        eye = pos + fwd * 0.9 * dist
        return L.camera_new(f(eye), f(eye - right * dist + up * 0.3 * dist + fwd * 0.2 * dist), (0.0, 1.0, 0.0), F(75.0), F(13.0 / 7.0))
    raise KeyError(name)


def lens_of(cam):
    """A lens for `cam`: radius and focus distance scaled to the camera's distance from the origin."""
    dist = float(np.linalg.norm(cam_vectors(cam)[0])) or 1.0
    return float(F(0.02 * dist)), float(F(0.8 * dist))


def make_view(abi, cam, W, H, model, centre=False, lens=None):
    r, d = lens if lens is not None else ((lens_of(cam)) if model == abi.VIEW_THIN_LENS else (0.0, 0.0))
    return abi.View.make(cam, W, H, model, abi.VIEW_CENTRE if centre else 0, r, d)
