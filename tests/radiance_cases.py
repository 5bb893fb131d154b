"""Cases of the radiance queries (mi355rt_context_trace_radiance; not a test, not a conftest): the rays a pinhole camera would make, built on the
host in numpy float32, so that oracle.render -- whose every ray is a camera ray -- is the exact reference for a query along caller-supplied rays.

A case is a camera with any position, orientation and field of view at a small W x H.  For sample s the ray of pixel (x, y) is made as the render
makes it: the jitter from the words 0 / 1 of oracle.ctr_block(k0, k1, x, s, 0, 0) with ykey = y + seed, u = (x + j) / W, camera.rs:33-42 with ONE
normalisation (the query's Ray::new is the second), row = y, x = x.  The query is then called once per sample with [s, s + 1), carrying d_accum;
after the last call out_linear is the oracle's linear image."""
import numpy as np

F = np.float32
EPS = F(1e-4)


def u01(w):
    """rand's StandardUniform<f32> of a generator word (rt_rng.h u32_to_f01): the 24 high bits times 2^-24, exact."""
    return (np.asarray(w, np.uint32) >> np.uint32(8)).astype(F) * F(1.0 / 16777216.0)


def normalized_rows(a):
    """vec3.rs:37-44 on every row of a float32 [n, 3]: the length as sqrt((x*x + y*y) + z*z), a row shorter than 1e-4 left alone, else a * (1 / l)."""
    a = np.ascontiguousarray(a, F)
    l = np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])
    assert l.dtype == F
    inv = F(1.0) / np.where(l < EPS, F(1.0), l)
    return np.where((l < EPS)[:, None], a, a * inv[:, None]).astype(F)


def jitter(oracle_mod, W, H, s, seed=0):
    """(ju, jv) float32 [H * W]: words 0 / 1 of (ray 0, block 0) of sample s of every pixel, row-major."""
    ju, jv = np.zeros(H * W, F), np.zeros(H * W, F)
    for y in range(H):
        ykey = (y + seed) & 0xFFFFFFFFFFFFFFFF
        k0, k1 = ykey & 0xFFFFFFFF, ykey >> 32
        for x in range(W):
            w = oracle_mod.ctr_block(k0, k1, x, s, 0, 0)
            ju[y * W + x], jv[y * W + x] = u01(w[0]), u01(w[1])
    return ju, jv


def camera_rays(oracle_mod, abi, cam, W, H, s, seed=0):
    """abi.PATH_RAY_DTYPE [H * W]: the camera rays of sample s (renderer.rs:96-99, camera.rs:33-42), normalised once."""
    ju, jv = jitter(oracle_mod, W, H, s, seed)
    x = np.tile(np.arange(W, dtype=np.uint32), H)
    y = np.repeat(np.arange(H, dtype=np.uint32), W)
    u = (x.astype(F) + ju) / F(W)
    v = (y.astype(F) + jv) / F(H)
    ax = (F(2.0) * u - F(1.0)) * F(cam.half_width)
    ay = (F(1.0) - F(2.0) * v) * F(cam.half_height)
    right, up, fwd = (np.array(list(a), F) for a in (cam.right, cam.true_up, cam.forward))
    raw = fwd[None, :] + (right[None, :] * ax[:, None] + up[None, :] * ay[:, None])
    assert raw.dtype == F
    rays = np.zeros(H * W, abi.PATH_RAY_DTYPE)
    rays["origin"] = np.array(list(cam.position), F)[None, :]
    rays["direction"] = normalized_rows(raw)
    rays["x"], rays["row"] = x, y
    return rays


def walk(oracle_mod, sc, rays, s, seed, max_depth):
    """The query's definition as a Python loop over the oracle's per-ray hooks, float32 [n, 3]: sample s of every ray.  The scatter event after
    ray r is addressed at ray r + 1, the radiance is folded front to back.  oracle.scene_hit normalises whatever it is given, so a scattered
    direction is normalised once more than the query normalises it: this pins the addressing and the fold, not last-bit direction arithmetic."""
    out = np.zeros((len(rays), 3), F)
    miss = np.array(list(sc.c.miss_color), F)
    for i, r in enumerate(rays):
        ykey = (int(r["row"]) + seed) & 0xFFFFFFFFFFFFFFFF
        k0, k1, x = ykey & 0xFFFFFFFF, ykey >> 32, int(r["x"])
        o, d = r["origin"].copy(), r["direction"].copy()
        thr, ray = np.ones(3, F), 0
        for left in range(max_depth, -1, -1):
            if left == 0:
                out[i] = thr * F(0.0); break
            hit, h = oracle_mod.scene_hit(sc, o, d)
            if not hit:
                out[i] = thr * miss; break
            ray += 1
            rec = np.zeros(16, np.uint32)
            rec[0], rec[1] = int(h[7]), int(h[8])
            rec[2:5], rec[5:8], rec[8:11] = d.view(np.uint32), h[0:3].view(np.uint32), h[3:6].view(np.uint32)
            rec[11:16] = [k0, k1, x, s, ray]
            f = oracle_mod.scatter_ctr_batch(sc._mats, rec)[0].view(F)
            if f[0] == 0:
                out[i] = thr * f[10:13]; break
            thr = (thr * f[7:10]).astype(F)
            o, d = f[1:4].copy(), f[4:7].copy()
    return out


def fixed_rays(abi, n=300, seed=7):
    """n rays from inside the cornell box in every direction (un-normalised on purpose), with scattered stream addresses: the fixed set of
    the chunking and refill tests."""
    rng = np.random.default_rng(seed)
    rays = np.zeros(n, abi.PATH_RAY_DTYPE)
    rays["origin"] = (rng.uniform(-0.6, 0.6, (n, 3)) + np.array([0.0, 1.0, 0.0])).astype(F)
    rays["direction"] = (rng.normal(size=(n, 3)) * rng.uniform(0.5, 3.0, (n, 1))).astype(F)
    rays["x"] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    rays["row"] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    return rays
