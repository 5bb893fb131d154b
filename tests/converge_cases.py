"""Scenes and helpers of test_gpu_converge_cli.py.  A plain module, imported like parity.py.

rt_render reads Tungsten JSON files only, so the scenes the converging loop is tested on are written as such files (with an OBJ beside them
where a mesh is wanted): the shipped cornell box, a scene in the manner of fuzz_scenes.random_scene with all five primitive kinds and a mesh,
and one in the manner of nonfinite_cases' "emissive_inf" -- Lambert quads and cubes around an emitter whose colour overflows float32 to +inf
in the loader (the JSON number 1e39)."""
import json
import math
import re

import numpy as np

NOISE_LINE = re.compile(r"^noise: samples=(\d+) chunks=(\d+) rendered=(\d+) above=(\d+) nonfinite=(\d+) max=(\S+) mean=(\S+) converged=([01]) "
                        r"wall_ms=(\S+) kernel_ms=(\S+)$", re.M)


def parse_noise_line(stdout):
    m = NOISE_LINE.findall(stdout)
    assert len(m) == 1, stdout
    s, k, r, a, f, mx, mean, conv, wall, kern = m[0]
    return dict(samples=int(s), chunks=int(k), rendered=int(r), above=int(a), nonfinite=int(f), max=float(mx), mean=float(mean), converged=int(conv),
                wall_ms=float(wall), kernel_ms=float(kern))


def read_pfm(path):
    """float32 [H, W, 3], row 0 = top (the file stores the rows bottom-up, little-endian)."""
    raw = open(path, "rb").read()
    m = re.match(rb"PF\n(\d+) (\d+)\n-1.0\n", raw)
    w, h = int(m.group(1)), int(m.group(2))
    return np.frombuffer(raw[m.end():], "<f4").reshape(h, w, 3)[::-1].copy()


def five_kinds_scene(tmp_path, seed=7):
    """Sphere, plane, quad, cube and a mesh (an OBJ of random triangles with a coplanar patch), Lambert, checker, plastic, glass and an
    emitter; drawn from a seeded generator."""
    rng = np.random.default_rng(seed)
    r = lambda lo, hi, n=3: [round(float(v), 3) for v in rng.uniform(lo, hi, n)]
    nt = 40
    v = rng.uniform(-1, 1, (nt, 3, 3))
    v[: nt // 4, :, 2] = 0.25
    lines = [f"v {a:.4f} {b:.4f} {c:.4f}" for a, b, c in v.reshape(-1, 3)] + [f"f {3 * i + 1} {3 * i + 2} {3 * i + 3}" for i in range(nt)]
    (tmp_path / "soup.obj").write_text("\n".join(lines) + "\n")
    bsdfs = [{"name": "a", "type": "lambert", "albedo": r(0.2, 0.9)}, {"name": "b", "type": "lambert", "albedo": {"on_color": r(0.5, 0.9), "off_color": r(0.1, 0.4), "res_u": 2.0}},
             {"name": "c", "type": "plastic", "albedo": r(0.2, 0.9), "ior": 1.5}, {"name": "d", "type": "dielectric", "ior": 1.6},
             {"name": "e", "type": "lambert", "albedo": 0.7}]
    tr = lambda: {"position": r(-2.5, 2.5), "scale": r(0.6, 1.8), "rotation": r(-180, 180)}
    prims = [{"type": "sphere", "bsdf": "c", "transform": {"position": r(-2, 2)}, "radius": 0.9},
             {"type": "plane", "point": [0, -2.5, 0], "normal": [0, 1, 0], "material": {"Lambertian": {"albedo": [0.6, 0.6, 0.5]}}},
             {"type": "quad", "bsdf": "a", "transform": tr()},
             {"type": "cube", "bsdf": "b", "transform": tr()},
             {"type": "mesh", "file": "soup.obj", "bsdf": "e", "transform": {"position": [0.5, 0.2, 0.5], "scale": [1.6, 1.6, 1.6], "rotation": r(-180, 180)}},
             {"type": "sphere", "bsdf": "d", "transform": {"position": r(-2, 2)}, "radius": 0.7},
             {"type": "quad", "bsdf": "a", "emission": [4.0, 3.5, 3.0], "transform": {"position": [0, 4.5, 0], "scale": [3, 1, 3], "rotation": [180, 0, 0]}},
             {"type": "cube", "bsdf": "e", "transform": tr()}]
    cam = {"transform": {"position": [0, 1, 9], "look_at": [0, 0, 0], "up": [0, 1, 0]}, "fov": 50}
    p = tmp_path / "five_kinds.json"
    p.write_text(json.dumps({"camera": cam, "primitives": prims, "bsdfs": bsdfs}))
    return str(p)


def infinite_emitter_scene(tmp_path):
    """Lambert quads and cubes around a quad whose emission is +inf in float32: pixels that reach it are +inf, others stay finite."""
    bsdfs = [{"name": "floor", "type": "lambert", "albedo": [0.7, 0.7, 0.6]}, {"name": "red", "type": "lambert", "albedo": [0.8, 0.2, 0.2]},
             {"name": "white", "type": "lambert", "albedo": 0.8}]
    prims = [{"type": "quad", "bsdf": "floor", "transform": {"position": [0, -1, 0], "scale": [30, 1, 30]}},
             {"type": "cube", "bsdf": "red", "transform": {"position": [-1.2, -0.3, -1.0], "scale": [1.4, 1.4, 1.4], "rotation": [0, 25, 0]}},
             {"type": "cube", "bsdf": "white", "transform": {"position": [1.3, 0.0, -2.0], "scale": [1.2, 2.0, 1.2], "rotation": [0, -20, 0]}},
             {"type": "quad", "bsdf": "white", "emission": [1e39, 1e39, 1e39], "transform": {"position": [2.5, 1.2, -3.0], "scale": [0.5, 1, 0.5], "rotation": [90, 0, 0]}}]
    cam = {"transform": {"position": [0, 1.5, 6], "look_at": [0, 0.3, -1], "up": [0, 1, 0]}, "fov": 40}
    p = tmp_path / "infinite_emitter.json"
    p.write_text(json.dumps({"camera": cam, "primitives": prims, "bsdfs": bsdfs}))
    return str(p)


def pick_threshold(maps, k_stop, fractions=(0.1, 0.2, 0.05, 0.3, 0.02)):
    """maps: {k: error map after chunk k} for k = 2 .. k_stop.  Returns (threshold, fraction, allowed_above) such that, with min_chunks = 2,
    `above <= allowed_above` holds at chunk k_stop and at no earlier chunk.  above(T) <= A exactly when T >= the (A + 1)-th largest error, so
    the threshold lies between that value at k_stop and the smallest of the earlier ones."""
    n = maps[k_stop].size
    for frac in fractions:
        allowed = int(math.floor(frac * n))
        edge = {}
        for k, m in maps.items():
            e = np.sort(m.reshape(-1).astype(np.float64)[~np.isnan(m.reshape(-1))])[::-1]
            edge[k] = e[allowed] if allowed < e.size else 0.0
        earlier = min(edge[k] for k in maps if k < k_stop)
        if np.isfinite(earlier) and edge[k_stop] < earlier:
            t = 0.5 * (edge[k_stop] + earlier)
            if edge[k_stop] <= t < earlier and t > 0:
                return float(t), frac, allowed
    raise AssertionError(f"no threshold separates chunk {k_stop} from the earlier ones")
