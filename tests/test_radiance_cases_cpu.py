"""The case builder of the radiance-query tests (tests/radiance_cases.py) is sane, without a GPU: the camera rays it makes, walked by a Python
loop over the oracle's per-ray hooks, reproduce oracle.render."""
import numpy as np

import radiance_cases as RC
from conftest import load_for_both

F = np.float32


def test_camera_rays_walked_on_the_oracle_reproduce_its_render(native, oracle_mod, abi):
    """Cornell 16 x 12 x 8 at depth 8: the rays of radiance_cases.camera_rays, walked by radiance_cases.walk (oracle.scene_hit, then
    oracle.scatter_ctr_batch for the event after ray r at ray r + 1, the throughput folded front to back), summed in sample order and scaled
    by 1 / spp, are oracle.render's linear image bit for bit.
    This pins the ADDRESSING (key, x, sample, ray number) and the FOLD of the definition the GPU tests hold the kernels to -- not last-bit
    direction arithmetic: oracle.scene_hit normalises every direction it is given, a scattered one for the second time, and cornell's pixel
    values depend only on which materials a path meets."""
    host, _ = native
    W, H, S, D = 16, 12, 8, 8
    sc = load_for_both("cornell", oracle_mod, host, width=W, height=H, spp=S, max_depth=D)
    _, linear, _ = oracle_mod.render(sc, sc.camera, sc.settings, abi.Options.make(), threads=2)
    acc = np.zeros((W * H, 3), F)
    for s in range(S):
        rays = RC.camera_rays(oracle_mod, abi, sc.camera, W, H, s)
        assert rays.dtype == abi.PATH_RAY_DTYPE and rays.shape == (W * H,)
        assert (rays["x"].reshape(H, W) == np.arange(W)[None, :]).all() and (rays["row"].reshape(H, W) == np.arange(H)[:, None]).all()
        l2 = (rays["direction"].astype(np.float64) ** 2).sum(-1)
        assert np.abs(l2 - 1.0).max() < 1e-6                                       # normalised (once)
        acc = (acc + RC.walk(oracle_mod, sc, rays, s, 0, D)).astype(F)
    got = (acc * (F(1.0) / F(S))).reshape(H, W, 3)
    bad = (got.view(np.uint32) != linear.view(np.uint32)).any(-1)
    assert not bad.any(), f"{int(bad.sum())} of {W * H} pixels differ from oracle.render"
    assert float(linear.mean()) > 0.01                                             # (the image is not black: paths reach the light)


def test_jitter_depends_on_the_seed_and_the_high_key_word(oracle_mod, abi):
    """ykey = row + seed in 64 bits: a seed of 2^32 - 1 carries into the high word from row 1 on, and the builder follows it."""
    a = RC.jitter(oracle_mod, 3, 2, 0, seed=0)
    b = RC.jitter(oracle_mod, 3, 2, 0, seed=0xFFFFFFFF)
    assert not np.array_equal(a[0], b[0])
    w = oracle_mod.ctr_block(0, 1, 2, 0, 0, 0)                                      # row 1 + 0xFFFFFFFF = 2^32: k0 = 0, k1 = 1
    assert b[0][1 * 3 + 2] == RC.u01(w[0]) and b[1][1 * 3 + 2] == RC.u01(w[1])


def test_fixed_rays_are_fixed(abi):
    a, b = RC.fixed_rays(abi), RC.fixed_rays(abi)
    assert a.tobytes() == b.tobytes() and len(a) == 300 and a.dtype == abi.PATH_RAY_DTYPE
    assert len(np.unique(a["x"])) > 290 and len(np.unique(a["row"])) > 290
