"""Inputs shared by the denoiser's tests (tests/test_denoise_reference_cpu.py, tests/test_gpu_denoise.py): the cornell-box frame of the quality
gate, the oracle's guides for it, and seeded synthetic images and guide records with the values a filter gets wrong.  Everything is computed
once per process and handed out read-only."""
import numpy as np

from conftest import SCENES
from parity import oracle_threads

F = np.float32
NO_HIT = 0xFFFFFFFF
GATE_W, GATE_H, GATE_DEPTH, GATE_SPP, GATE_REF_SPP = 96, 72, 8, 4, 1024
GATE_LIMIT = 0.60                                                     # RMSE(denoised, ref) / RMSE(noisy, ref): 0.476 measured with the defaults, plus 25 %

_cache = {}


def _once(key, make):
    if key not in _cache:
        v = make()
        for a in (v if isinstance(v, tuple) else (v,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[key] = v
    return _cache[key]


def gate_scene(host):
    return _once("scene", lambda: host.LoadedScene(SCENES["cornell"], GATE_W, GATE_H, GATE_SPP, GATE_DEPTH))


def gate_oracle_image(oracle_mod, abi, host, spp):
    """The oracle's linear image of the gate's frame at `spp` samples (counter mode: it does not depend on the thread count)."""
    sc = gate_scene(host)
    return _once(("oracle", spp), lambda: oracle_mod.render(sc, sc.camera, abi.Settings(GATE_W, GATE_H, spp, GATE_DEPTH), abi.Options.make(rng_mode=abi.RNG_CTR),
                                                            threads=oracle_threads())[1])


def gate_oracle_guides(oracle_mod, abi, host):
    """mi355rt_hit records of the gate's frame from oracle.scene_hit at the pixel centres.  `primitive` holds the material the oracle reports
    (the filter only asks whether it is NO_HIT)."""
    from test_gpu_ray_queries import camera_dirs
    sc = gate_scene(host)

    def make():
        dirs = camera_dirs(sc.camera, GATE_W, GATE_H).reshape(-1, 3)
        origin = np.array(list(sc.camera.position), F)
        out = np.zeros(GATE_W * GATE_H, abi.HIT_DTYPE)
        for i, d in enumerate(dirs):
            hit, r = oracle_mod.scene_hit(sc, origin, d)
            if hit:
                out[i]["position"], out[i]["normal"], out[i]["t"] = r[0:3], r[3:6], r[6]
                out[i]["primitive"] = out[i]["material"] = int(r[7])
                out[i]["front_face"] = int(r[8])
            else:
                out[i]["t"], out[i]["primitive"], out[i]["material"] = F(np.inf), NO_HIT, NO_HIT
        return out
    return _once("guides", make)


def synthetic(abi, W, H, seed):
    """A seeded image and guide records of H x W pixels with, at pixels chosen by the seed: negative, denormal, +inf, -inf and NaN colours; runs of
    misses, NaN normals, t = 0 / NaN / +inf on "hits", and coincident positions.  Returns (linear f32 [H, W, 3], hits HIT_DTYPE [H * W])."""
    def make():
        rng = np.random.default_rng(seed)
        n = W * H
        lin = rng.uniform(0.0, 1.5, (H, W, 3)).astype(F)
        # two flat regions with noise, so that colour weights are neither all 1 nor all 0
        lin[:, : W // 2] = (lin[:, : W // 2] * F(0.1) + F(0.6)).astype(F)
        hits = np.zeros(n, abi.HIT_DTYPE)
        yy, xx = np.divmod(np.arange(n), W)
        # a floor (normal +y) on the left, a wall (normal +z) on the right, positions on a jittered lattice, t = distance from (0, 1, 5)
        pos = np.stack([xx * 0.1, np.zeros(n), yy * 0.1], 1) + rng.normal(0, 0.002, (n, 3))
        nrm = np.tile(np.array([0.0, 1.0, 0.0]), (n, 1))
        right = xx >= (2 * W) // 3
        nrm[right] = [0.0, 0.0, 1.0]
        tilt = rng.random(n) < 0.3                                      # some normals in between: dot products strictly inside (0, 1)
        nrm[tilt] = nrm[tilt] + rng.normal(0, 0.3, (int(tilt.sum()), 3))
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        hits["position"], hits["normal"] = pos.astype(F), nrm.astype(F)
        hits["t"] = np.linalg.norm(pos - np.array([0.0, 1.0, 5.0]), axis=1).astype(F)
        hits["front_face"] = 1
        hits["primitive"] = rng.integers(0, 7, n)
        hits["material"] = hits["primitive"]
        flat = lin.reshape(n, 3)

        def pick(k):
            return rng.choice(n, size=min(k, n), replace=False)
        if n >= 4:
            i = pick(max(n // 40, 1)); flat[i] = -flat[i]                                      # negative colours
            i = pick(max(n // 40, 1)); flat[i] = (flat[i] * F(1e-40)).astype(F)                # denormals
            i = pick(max(n // 60, 1)); flat[i, rng.integers(0, 3, len(i))] = F(np.inf)
            i = pick(max(n // 60, 1)); flat[i, rng.integers(0, 3, len(i))] = F(-np.inf)
            i = pick(max(n // 60, 1)); flat[i, rng.integers(0, 3, len(i))] = F(np.nan)
            i = pick(max(n // 50, 1)); hits["normal"][i, rng.integers(0, 3, len(i))] = F(np.nan)
            i = pick(max(n // 50, 1)); hits["t"][i] = F(0.0)
            i = pick(max(n // 50, 1)); hits["t"][i] = F(np.nan)
            i = pick(max(n // 50, 1)); hits["t"][i] = F(np.inf)
            i = pick(max(n // 30, 1)); hits["position"][i] = hits["position"][(i + 1) % n]     # coincident positions
            for start in pick(max(n // 100, 1)):                                               # runs of misses, in the ray queries' miss record
                run = slice(int(start), min(int(start) + int(rng.integers(1, 2 * W + 2)), n))
                hits[run] = np.zeros((), abi.HIT_DTYPE)
                hits["t"][run], hits["primitive"][run], hits["material"][run] = F(np.inf), NO_HIT, NO_HIT
        else:
            flat[0, 1] = F(-0.25)
        return lin, hits
    return _once(("synthetic", W, H, seed), make)
