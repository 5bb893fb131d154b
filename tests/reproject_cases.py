"""Cases of the temporal reprojection (mi355rt_post_reproject; not a test, not a conftest): synthetic first-hit records of a plane seen by two
cameras, and records crafted to sit on the decision boundaries of include/mi355rt_post.h.

THE CANONICAL PREVIOUS CAMERA stands at (0, 0, -1) and looks along +z with right = +x, true_up = +y and half_width = half_height = 1.  For a
current record at P = (a, b, 0) every step of the projection up to sx = a, sy = b is exact (D = (a, b, 1), z = 1), so a crafted record lands
where its a and b say, and E = h.position - P is exact for a previous record on the same axis: d = |E.z| to the bit."""
import numpy as np

import reproject_ref as RR

F = np.float32
NO_HIT = 0xFFFFFFFF
PRIM = 7                                        # the plane's primitive index in the synthetic records

# (cur size, prev size): 1 x 1; no multiple of the 32 x 8 tile; across a tile in both directions; more than two tiles a row; two frames of different sizes
SIZES = [((1, 1), (1, 1)), ((5, 3), (5, 3)), ((33, 9), (33, 9)), ((70, 17), (70, 17)), ((33, 9), (20, 7)), ((20, 7), (33, 9)), ((33, 9), (16, 8))]
EDGE_SIZES = ((33, 9), (16, 8))                 # fx == -1 and fx == W' have no float32 landing in a frame 20 or 33 across, a power of two has one: the pair on which every crafted item fits
MAX_HISTORY = [1, 2, 65535]
NORMAL_MIN, PLANE_TOLERANCE = 0.5, 0.05        # of the crafted cases: 0.5 is exact, the records' t is 2, so the bound is 2 * F(0.05) exactly


def camera(abi, position, forward, right, true_up, half_width, half_height):
    cam = abi.Camera()
    for name, val in (("position", position), ("forward", forward), ("right", right), ("true_up", true_up)):
        for i in range(3):
            getattr(cam, name)[i] = float(F(val[i]))
    cam.half_width, cam.half_height = float(F(half_width)), float(F(half_height))
    return cam


def look_at(abi, eye, target, vfov_deg=60.0, aspect=4.0 / 3.0, up=(0.0, 1.0, 0.0)):
    """A camera as src/camera.rs builds one, in float64 and rounded once: an orthonormal basis, half_height = tan(vfov / 2)."""
    eye, target, up = (np.asarray(v, np.float64) for v in (eye, target, up))
    fwd = target - eye
    fwd /= np.linalg.norm(fwd)
    right = np.cross(fwd, up)
    right /= np.linalg.norm(right)
    true_up = np.cross(right, fwd)
    hh = np.tan(np.radians(vfov_deg) / 2.0)
    return camera(abi, eye, fwd, right, true_up, hh * aspect, hh)


def canonical(abi):
    return camera(abi, (0, 0, -1), (0, 0, 1), (1, 0, 0), (0, 1, 0), 1.0, 1.0)


def view(abi, cam, W, H):
    return abi.View.make(cam, W, H, abi.VIEW_PINHOLE, abi.VIEW_CENTRE)


def plane_hits(abi, cam, W, H, prim=PRIM):
    """abi.HIT_DTYPE [H * W]: the plane z = 0 (normal (0, 0, -1)) through the centre of every pixel of a pinhole at `cam`; a miss where the ray
    does not meet it in front of the camera.  Inputs of the stage, not a reference of anything: float64, rounded once."""
    pos, fwd, right, up = (np.array(list(a), np.float64) for a in (cam.position, cam.forward, cam.right, cam.true_up))
    x, y = np.tile(np.arange(W), H), np.repeat(np.arange(H), W)
    ax = (2.0 * (x + 0.5) / W - 1.0) * cam.half_width
    ay = (1.0 - 2.0 * (y + 0.5) / H) * cam.half_height
    d = fwd[None, :] + right[None, :] * ax[:, None] + up[None, :] * ay[:, None]
    d /= np.linalg.norm(d, axis=1)[:, None]
    with np.errstate(all="ignore"):
        t = -pos[2] / d[:, 2]
    hit = np.isfinite(t) & (t > 1e-4)
    out = np.zeros(H * W, abi.HIT_DTYPE)
    out["primitive"], out["material"], out["t"] = NO_HIT, NO_HIT, np.inf
    p = pos[None, :] + d * np.where(hit, t, 0.0)[:, None]
    p[:, 2] = 0.0
    out["position"][hit], out["t"][hit] = p[hit].astype(F), t[hit].astype(F)
    out["normal"][hit] = (0.0, 0.0, -1.0)
    out["front_face"][hit], out["primitive"][hit], out["material"][hit] = 1, prim, 1
    return out


def random_history(rng, n, max_length=40):
    h = np.empty((n, 4), F)
    h[:, :3] = rng.random((n, 3), dtype=F)
    h[:, 3] = rng.integers(1, max_length + 1, n).astype(F)
    return h


def next_f32(v, up=True):
    return np.nextafter(F(v), F(np.inf) if up else F(-np.inf))


def coord_x(a, size):
    """fx of a record at (a, ., 0) through the canonical camera into a frame `size` across: sx = a exactly."""
    return ((F(a) + F(1.0)) * F(0.5)) * F(size) - F(0.5)


def coord_y(b, size):
    """fy of a record at (., b, 0): sy = b exactly, v = (1 - b) * 0.5 -- it FALLS as b rises."""
    return ((F(1.0) - F(b)) * F(0.5)) * F(size) - F(0.5)


def landing(k, size, coord=coord_x):
    """The float32 a (coord_y: b) whose record projects to coordinate == k exactly, or None where no float32 near the real solution does.  k may be -1
    or `size`, the two edges of the projection's test: those need (k + 0.5) / size to be hit to the bit, which a width of 20 or 33 does not allow and a power of two does."""
    real = 2.0 * (k + 0.5) / size - 1.0
    a = F(real if coord is coord_x else -real)
    for _ in range(64):
        a = next_f32(a, up=False)
    for _ in range(129):
        if coord(a, size) == F(k):
            return a
        a = next_f32(a)
    return None


def landing_b(k, size):
    return landing(k, size, coord_y)


# ---- the crafted records ------------------------------------------------------------------------------------------------------------------
# Each item: (name, what the current record is, what the previous record / history at its landing pixel is, does it keep its history).
# The current record is at (a, b, 0) with normal (0, 0, 1), t = 2 and primitive PRIM unless stated; it lands exactly ON previous pixel q (tx = ty =
# 0: one counted tap), whose record is at (a, b, 0) with the same normal and primitive and whose history is {0.25, 0.5, 0.75, 3} unless stated.
def items(max_history):
    tol = F(PLANE_TOLERANCE) * F(2.0)
    half_below = next_f32(0.5, up=False)
    return [
        ("plain", {}, {}, True),
        ("nd == normal_min", {}, {"normal": (0.0, 0.75, 0.5)}, True),
        ("nd one ulp below normal_min", {}, {"normal": (0.0, 0.75, half_below)}, False),
        ("d == plane_tolerance * t", {}, {"dz": tol}, True),
        ("d one ulp above", {}, {"dz": next_f32(tol)}, False),
        ("d one ulp below, behind the plane", {}, {"dz": -next_f32(tol, up=False)}, True),
        ("primitive mismatch", {}, {"primitive": PRIM + 1}, False),
        ("miss in the previous frame", {}, {"primitive": NO_HIT}, False),
        ("miss in the current frame", {"primitive": NO_HIT}, {"primitive": NO_HIT}, False),
        ("length 0", {}, {"length": 0.0}, False),
        ("length 0.5", {}, {"length": 0.5}, False),
        ("length 1", {}, {"length": 1.0}, True),
        ("length max_history", {}, {"length": float(max_history)}, True),
        ("length inf", {}, {"length": np.inf}, True),
        ("length NaN", {}, {"length": np.nan}, False),
        ("history r NaN", {}, {"rgb": (np.nan, 0.5, 0.75)}, False),
        ("history g +inf", {}, {"rgb": (0.25, np.inf, 0.75)}, False),
        ("history b -inf", {}, {"rgb": (0.25, 0.5, -np.inf)}, False),
        ("z == 0", {"z": -1.0}, {}, False),                             # the canonical camera is at z = -1: a record there has depth 0, one at -3 is behind it
        ("z < 0", {"z": -3.0}, {}, False),
        ("NaN position", {"z": np.nan}, {}, False),
        ("t NaN", {"t": np.nan}, {}, False),
        ("colour NaN", {"color": (np.nan, 0.5, np.inf)}, {}, True),
    ]


def edge_landings(size, coord=coord_x, axis="fx", dim="W'"):
    """[(name, a)] for the edges of the projection's test on one axis: coordinate == -1 (fails), the nearest float32 inside (counts the tap at 0 with
    a weight near 1e-7), coordinate == size (fails), the nearest inside (counts the tap at size - 1).  Empty where the edge has no exact landing."""
    lo, hi = landing(-1, size, coord), landing(size, size, coord)
    if lo is None or hi is None:
        return []
    inward = lambda a, up: next(v for v in _walk(a, up) if F(-1.0) < coord(v, size) < F(size))
    rises = coord is coord_x                                          # fx rises with a, fy falls with b
    return [(f"{axis} == -1", lo), (f"{axis} just inside -1", inward(lo, rises)), (f"{axis} == {dim}", hi), (f"{axis} just inside {dim}", inward(hi, not rises))]


def _walk(a, up):
    for _ in range(64):
        a = next_f32(a, up)
        yield a


def build(abi, cur_size, prev_size, max_history=32, seed=0, crafted=True):
    """One synthetic frame pair: a dict with the two views, hits_cur, color_cur, hits_prev, hist_prev, params, and `placed`: for every crafted item
    that fitted [(name, current pixel, previous pixel or None, keeps its history?)].
    The base content is the plane seen by the canonical camera (previous) and by a camera moved and turned a little (current), a random history with
    lengths 1 .. 40, and a sprinkle of mismatching primitives and non-finite history; the crafted items then overwrite current pixel j = 0, 1, ... and
    the previous pixel each lands on, as long as both frames have pixels left; the edges of the projection's test follow where they can be landed on."""
    (W, H), (Wp, Hp) = cur_size, prev_size
    rng = np.random.default_rng(1000 * W + 10 * Wp + seed)
    prev_cam = canonical(abi)
    cur_cam = look_at(abi, (0.07, -0.04, -1.05), (0.02, 0.01, 0.0), vfov_deg=90.0, aspect=1.0)
    cur, prev = view(abi, cur_cam, W, H), view(abi, prev_cam, Wp, Hp)
    hits_cur, hits_prev = plane_hits(abi, cur_cam, W, H), plane_hits(abi, prev_cam, Wp, Hp)
    color = rng.random((W * H, 3), dtype=F)
    hist = random_history(rng, Wp * Hp)
    odd = rng.random(Wp * Hp)
    hits_prev["primitive"][odd < 0.05] = PRIM + 2
    hist[(odd > 0.05) & (odd < 0.08), 1] = np.nan
    hist[(odd > 0.08) & (odd < 0.10), 3] = 0.0
    placed = []
    free = list(range(Wp * Hp))                                        # previous pixels not yet given to an item, in order
    j = 0
    for name, cur_over, prev_over, keeps in items(max_history) if crafted else []:
        if j >= W * H:
            break
        q = None
        for cand in free:
            a, b = landing(cand % Wp, Wp), landing_b(cand // Wp, Hp)
            if a is not None and b is not None:
                q = cand
                break
        if q is None:
            break
        free.remove(q)
        g = hits_cur[j:j + 1]
        g["position"], g["t"], g["normal"], g["front_face"], g["primitive"], g["material"] = (a, b, cur_over.get("z", 0.0)), cur_over.get("t", 2.0), (0, 0, 1), 1, cur_over.get("primitive", PRIM), 1
        if "color" in cur_over:
            color[j] = cur_over["color"]
        h = hits_prev[q:q + 1]
        h["position"], h["t"], h["normal"], h["front_face"], h["primitive"], h["material"] = (a, b, prev_over.get("dz", 0.0)), 1.0, prev_over.get("normal", (0, 0, 1)), 1, prev_over.get("primitive", PRIM), 1
        hist[q, :3], hist[q, 3] = prev_over.get("rgb", (0.25, 0.5, 0.75)), prev_over.get("length", 3.0)
        placed.append((name, j, q, keeps))
        j += 1
    if crafted:                                                        # the edges: the other coordinate lands on pixel 0
        a0, b0 = landing(0, Wp), landing_b(0, Hp)
        edges = [(name, a, b0) for name, a in edge_landings(Wp)] + [(name, a0, b) for name, b in edge_landings(Hp, coord_y, "fy", "H'")]
        for name, a, b in edges if a0 is not None and b0 is not None else []:
            if j >= W * H:
                break
            g = hits_cur[j:j + 1]
            g["position"], g["t"], g["normal"], g["front_face"], g["primitive"], g["material"] = (a, b, 0.0), 2.0, (0, 0, 1), 1, PRIM, 1
            placed.append((name, j, None, None))
            j += 1
    params = abi.ReprojectParams.make(max_history, NORMAL_MIN, PLANE_TOLERANCE)
    return dict(cur=cur, prev=prev, hits_cur=hits_cur, color_cur=color, hits_prev=hits_prev, hist_prev=hist, params=params, placed=placed)


def reference(case):
    return RR.reproject(case["cur"], case["prev"], case["hits_cur"], case["color_cur"], case["hits_prev"], case["hist_prev"], case["params"])


# ---- the orbit of the quality case and of tools/reproject_bench.py ---------------------------------------------------------------------------
def orbit_camera(scene_camera, frame, step_deg, oracle_loader, fov_deg, aspect):
    """The scene's camera swung about the point it looks at (its distance from the origin ahead of it), `frame` steps of step_deg about the y axis."""
    pos, fwd = (np.array(list(a), np.float64) for a in (scene_camera.position, scene_camera.forward))
    dist = float(np.linalg.norm(pos)) or 1.0
    target = pos + fwd * dist
    ang = np.radians(step_deg * frame)
    rel = pos - target
    rot = np.array([rel[0] * np.cos(ang) + rel[2] * np.sin(ang), rel[1], -rel[0] * np.sin(ang) + rel[2] * np.cos(ang)])
    f = lambda a: tuple(float(F(v)) for v in a)
    return oracle_loader.camera_new(f(target + rot), f(target), (0.0, 1.0, 0.0), F(fov_deg), F(aspect))
