"""Committed golden vectors (tests/golden/oracle_*.npz, made by tools/make_golden_fixtures.py).

CPU: the oracle must still reproduce them bit-for-bit (guards the checker against drift).
GPU: the HIP path, through the C ABI, must reproduce them with the parity tolerances of DESIGN.md --
     bit-identical where the path uses only + - * / sqrt and everywhere in the reference-stream mode, the tolerant contract of
     tests/parity.py for the counter-mode renders of scenes with rough conductors (native float ln / atan / sin / cos on the device).
"""
import os

import numpy as np
import pytest

from conftest import ROOT, load_for_both
from parity import assert_parity

CASES = {"cornell": True, "teapot": True, "veach": False, "semesterbild": False}     # name -> exact on GPU


def _fixture(name):
    z = np.load(os.path.join(ROOT, "tests/golden", f"oracle_{name}.npz"))
    W, H, spp, depth = (int(v) for v in z["meta"])
    return z, W, H, spp, depth


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_reproduces_fixtures(name, native, oracle_mod, abi):
    host, _ = native
    z, W, H, spp, depth = _fixture(name)
    sc = load_for_both(name, oracle_mod, host, width=W, height=H, spp=spp, max_depth=depth)
    for mode, tag in ((abi.RNG_CTR, "ctr"), (abi.RNG_REF, "ref")):
        packed, linear, cnt = oracle_mod.render(sc, sc.camera, sc.settings, abi.Options.make(rng_mode=mode))
        assert np.array_equal(linear.view(np.uint32), z[f"{tag}_linear"].view(np.uint32)), (name, tag)
        assert np.array_equal(packed, z[f"{tag}_packed"])
        assert cnt.rays == int(z[f"{tag}_rays"][0])


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("tag", ["ctr", "ref"])
def test_hip_path_reproduces_fixtures(name, tag, native, abi):
    host, device = native
    z, W, H, spp, depth = _fixture(name)
    sc = host.LoadedScene(os.path.join(ROOT, {"cornell": "data/scenes/tungsten/cornell-box/scene.json",
                                              "veach": "data/scenes/tungsten/veach-mis/scene.json",
                                              "teapot": "data/scenes/tungsten/teapot/scene.json",
                                              "semesterbild": "data/scenes/semesterbild.json"}[name]),
                          W, H, spp, depth, skip_unknown_primitives=(name == "teapot"))      # PRODUCT loader end to end
    mode = abi.RNG_CTR if tag == "ctr" else abi.RNG_REF
    packed, linear, st = device.render(sc, sc.camera, sc.settings, abi.Options.make(rng_mode=mode))
    want_l, want_p = z[f"{tag}_linear"], z[f"{tag}_packed"]
    if CASES[name] or tag == "ref":        # the reference-stream mode rounds its ln / atan / sin / cos once from double on both sides: exact everywhere
        assert np.array_equal(linear.view(np.uint32), want_l.view(np.uint32))
        assert np.array_equal(packed, want_p)
        assert st.rays == int(z[f"{tag}_rays"][0])
    else:
        assert_parity(packed, linear, want_p, want_l, exact=False)
