"""The LCG-stepped draw address on the device (rt_rng.h RngCtrT<true>, unit_ball_cooperative's running word) against the oracle, which addresses
draws by (x, sample, key, ray, try) and knows nothing of how the device keeps its words.

  * the generator itself, word for word: the reference build's probe (csrc/refs/rt_rng_probe.hip) returns the block at a chosen (key, x, sample,
    ray, try) through the plain form, the stepped form (set_ray + next_event, the full multiply) and the running word with the 24-bit multiply, at the
    rays and tries where r * A, base.z + r, j * A or base.w + j wrap, for keys and pixels of all-ones and zero words;
  * the product's debug entry (k_debug_scatter: start, set_ray, block 0, then tries by number) returns what the independent restatement gives
    at the same rays;
  * renders, bit-identical radiance and ray counts: 16x8 pixels at 4 and at 67 spp (runs that end mid-stock), depth 30 and depth 1, on a
    Lambert-only list of quads and cubes (kernel variant 14, whose draw address is stepped), a mesh-free list with metal (the general lockstep
    kernel) and a small mesh scene (the wavefront kernel), and on the cornell box, whose paths are long; and two of the fuzz generator's exact quad / cube scenes of 8 primitives."""
import numpy as np
import pytest

import kat_f32 as K
import scene_shapes as S
import test_gpu_scene_shapes as G
import test_kat_functions as T
from conftest import SCENES as CONFTEST_SCENES
from fuzz_scenes import random_scene

pytestmark = pytest.mark.gpu

RAYS = [0, 1, 2, 29, 30, 31, 2 ** 16, 2 ** 32 - 1]
TRIES = [0, 1, 2, 3, 63, 64, 65, 2 ** 24 - 1, 2 ** 24, 2 ** 32 - 1]
ONES = 0xFFFFFFFF
PATHS = [(0, 0, 0, 0), (ONES, ONES, ONES, ONES), (ONES, ONES, 0, 0), (0, 0, ONES, ONES), (0, ONES, 799, 255), (0x9E3779B9, 0x7F4A7C15, 0, ONES)]   # (key lo, key hi, x, sample)


def test_blocks_of_both_forms_equal_the_oracles(native, oracle_mod):
    host, device = native
    recs = [(k0, k1, x, s, r, j) for k0, k1, x, s in PATHS for r in RAYS for j in TRIES]
    got = device.debug_rng_block(np.array(recs, np.uint64).astype(np.uint32))
    assert got.shape == (len(recs), 3, 4)
    want = np.array([oracle_mod.ctr_block(*rec, gen=2) for rec in recs], np.uint32)
    for form, name in enumerate(("plain", "stepped", "running word")):
        bad = (got[:, form] != want).any(-1)
        assert not bad.any(), f"{name} form: {int(bad.sum())} of {len(recs)} blocks differ; first (k0, k1, x, s, ray, try): {recs[int(np.argmax(bad))]}"


def test_debug_scatter_at_wrapping_rays(native, abi):
    """A Lambert bounce at each edge ray: block 0 and the rejection's tries through set_ray on the stepped words."""
    host, device = native
    albedo = (0.7, 0.6, 0.5)
    mats = (abi.Material * 1)(T.material(abi, abi.MAT_LAMBERT_SOLID, albedo))
    n, p = T.unit((0.3, -0.8, 0.52)), K.V(0.5, -1.0, 2.0)
    rd = K.normalized(-n + K.V(0.1, 0.05, -0.02))
    recs, wants = [], []
    for k0, k1, x, s in PATHS:
        for r in RAYS:
            recs.append((0, True, rd, p, n, (k0, k1, x, s, r)))
            wants.append(K.scatter_lambert(K.V(*albedo), rd, p, n, K.CtrDraws(k0, k1, x, s, r)))
    for rec, want, g in zip(recs, wants, device.debug_scatter(mats, recs)):
        T.check_scatter(f"lambert at {rec[5]}", want, g, False)


SCENES = ("qc", "cornell", "metal", "mesh")


def _scene(abi, host, which):
    if which == "cornell":
        return host.LoadedScene(CONFTEST_SCENES["cornell"], 16, 8, 1, 1)  # the closed box: long paths, most events need a second or third try
    if which == "qc":
        return S.camera_scene(abi, host, "qc")                            # Lambert only, quads and cubes: k_render_ctr_simple_qc
    if which == "metal":
        return S.list_scene(abi, host, "meshfree", 33)                    # every material: the general lockstep kernel
    return S.list_scene(abi, host, "mesh", 33)                            # meshes of 8 triangles: the wavefront kernel


@pytest.mark.parametrize("depth", [30, 1])
@pytest.mark.parametrize("spp", [4, 67])
@pytest.mark.parametrize("which", SCENES)
def test_small_renders_equal_the_oracle(which, spp, depth, native, oracle_mod, abi):
    host, device = native
    sc = _scene(abi, host, which)
    st = abi.Settings(16, 8, spp, depth)
    got, chosen = G.render(device, abi, sc, sc.camera, st)
    if which in ("qc", "cornell"):
        assert chosen == 14
    elif which == "metal":
        assert chosen == 0                                                # KERNEL_LOCKSTEP (rt_device.h)
    else:
        assert chosen in (7, 10, 12, 13)                                  # a wavefront form
    ora = G.oracle_frame(oracle_mod, ("stepped", which, spp, depth), sc, sc.camera, st)
    G.against_oracle(got, ora, f"{which} 16x8x{spp} depth {depth}, variant {chosen}")


@pytest.mark.parametrize("seed", [101, 106])
def test_fuzz_quad_cube_scenes_equal_the_oracle(seed, native, oracle_mod, abi):
    host, device = native
    sc = random_scene(abi, host, seed, exact_only=True, n_prims=8, only_kinds=[abi.PRIM_QUAD, abi.PRIM_CUBE], lambert_only=True)
    for spp in (4, 67):
        st = abi.Settings(16, 8, spp, 30)
        got, chosen = G.render(device, abi, sc, sc.camera, st)
        assert chosen == 14
        G.against_oracle(got, G.oracle_frame(oracle_mod, ("stepped fuzz", seed, spp), sc, sc.camera, st), f"fuzz scene {seed} at {spp} spp")
