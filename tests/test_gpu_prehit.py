"""k_render_ctr_simple_qc stocks the FIRST HITS of its camera rays (HitStock, rt_kernels.hip): a refill pass walks the camera rays of the next samples of
the wave's run, finishes there the paths whose camera ray misses or hits the light, and stocks the others as ready-to-scatter entries.  These cases
make every part of that happen: a camera in the box's opening with a wide field so that the image border sees the sky (a non-black miss colour)
and the ceiling light is in view, fewer than 64 samples per pixel (one refill spans pixels), an odd sample count (the last run ends in a partial refill), and
max_depth 1 (every path ends at its camera ray or right after the first scatter of a dealt entry).  Radiance, pixels and ray counts must be the
oracle's, bit for bit."""
import numpy as np
import pytest

from conftest import load_for_both
from parity import assert_parity

pytestmark = pytest.mark.gpu


def _scene(oracle_mod, host, W, H, spp, depth):
    from oracle import scene_loader
    sc = load_for_both("cornell", oracle_mod, host, width=W, height=H, spp=spp, max_depth=depth)
    sc.c.miss_color[:] = [0.25, 0.5, 0.75]
    sc.camera = scene_loader.camera_new((0.2, 1.0, 3.0), (0.0, 1.0, 0.0), (0.0, 1.0, 0.0), np.float32(45.0), np.float32(W / H))
    return sc


@pytest.mark.parametrize("W,H,spp,depth", [(37, 29, 7, 1), (37, 29, 7, 6), (53, 41, 3, 30)])
def test_stocked_first_hits_match_oracle(W, H, spp, depth, native, oracle_mod, abi):
    host, device = native
    sc = _scene(oracle_mod, host, W, H, spp, depth)
    ctx = device.Context(0)
    try:
        ctx.set_scene(sc, sc.camera, sc.settings)
        assert ctx.kernel_variant() == 14                              # k_render_ctr_simple_qc: the kernel with the stock of first hits
    finally:
        ctx.close()
    assert (W * H * spp) % 2 == 1
    opt = abi.Options.make(rng_mode=abi.RNG_CTR)
    gp, gl, st = device.render(sc, sc.camera, sc.settings, opt)
    op, ol, cnt = oracle_mod.render(sc, sc.camera, sc.settings, opt)
    if depth == 1:                                                     # the refill pass really finished paths: sky at the border, the light in view
        sky = np.abs(ol - np.float32([0.25, 0.5, 0.75])).max(axis=-1) < 1e-6
        assert sky[:, 0].any() and sky[:, -1].any() and sky.mean() < 0.2
        assert (ol.max(axis=-1) > 1.0).any()                           # emitter radiance above 1
    assert st.samples == cnt.samples == W * H * spp
    assert_parity(gp, gl, op, ol, exact=True, gpu_rays=st.rays, oracle_rays=cnt.rays)
