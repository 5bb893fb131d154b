"""The conditions under which a pass of test_gpu_nonfinite_radiance.py means something, on the oracle alone (no GPU).

Every poisoned scene (tests/nonfinite_cases.py) must show what it was poisoned for -- each class its case names in at least 2 % of the
pixels, beside at least 5 % finite, non-zero pixels, so that a kernel that blackens or whitens everything cannot pass -- and must walk the
clean scene's control flow: the same rays and the same paths that run out of depth.  Colour never decides a branch in the reference
(src/renderer.rs), so no case declares another ray count; the GPU then walks what the existing tests already walk, with other numbers.
"""
import hashlib

import numpy as np
import pytest

import nonfinite_cases as nc
from fuzz_scenes import POISONS, random_scene

_clean = {}


def clean_of(oracle_mod, abi, host, base, opt, key="counter"):
    """The oracle's render of a base's clean scene, once per base and mode: (linear, counters)."""
    if (base, key) not in _clean:
        sc = nc.scene(abi, host, base)
        _, linear, cnt = oracle_mod.render(sc, sc.camera, nc.settings(abi), opt)
        _clean[(base, key)] = (linear, cnt)
    return _clean[(base, key)]


def test_poison_off_leaves_the_scene_of_a_seed_unchanged(native, abi):
    """A digest of one seed's arrays, taken before random_scene had the option."""
    host, _ = native
    sc = random_scene(abi, host, 1, exact_only=True, every_material=True)
    h = hashlib.sha256()
    for a in (bytes(sc._mats), bytes(sc._prims), sc.triangles.tobytes(), bytes(sc.c.miss_color)):
        h.update(a)
    assert h.hexdigest()[:16] == "1adc8055c8e820a2"
    assert random_scene.__defaults__[-1] is None                     # poison is off by default


def test_every_poison_family_is_planned_on_every_variant_that_can_take_it(native, abi):
    """Per family (emitter, miss colour, sky map, Lambert / metal albedo, checker colour): the variants its cases render with are all the
    variants whose materials hold the poisoned kind, the fixed-AABB forms included.  Rough conductors are outside this plan (counter mode
    compares only state machine and wavefront there, nonfinite_cases.FAMILY_KIND)."""
    import test_gpu_variant_matrix as vm
    host, _ = native
    assert {p for p, _, _ in nc.CASES} == set(POISONS)
    assert {what for what, _ in POISONS.values()} == set(nc.FAMILY_KIND) | {"rough"}
    plan = nc.family_plan(abi, host)
    for fam, planned in plan.items():
        assert planned == nc.takers(fam), (fam, sorted(nc.takers(fam) - planned))
    assert nc.takers("miss") == nc.takers("sky") == nc.takers("emissive") == set(vm.CAPABILITY) | set(vm.FLAG_FORMS)
    assert set(nc.variants_of(abi, host, "rough")) == set(vm.FLAG_FORMS)
    for fam in ("emissive", "miss"):                                 # the four colours of each
        assert {p for p, _, _ in nc.CASES if p.startswith(fam + "_")} == {f"{fam}_{k}" for k in ("inf", "mixed", "overflow", "signed")}
    for base in ("qc", "ident"):                                     # both paths carry two cases through bands, rows, chunks and devices
        assert sum(1 for _, b in nc.PATH_CASES if b == base) >= 2
    assert 14 in nc.variants_of(abi, host, "qc") and 7 in nc.variants_of(abi, host, "ident")        # lockstep and wavefront
    assert nc.SPP_PATHS > 1 + 5                                       # progressive chunks 1, 5, rest: the rest is not empty
    assert len(nc.REF_CASES) >= 2


@pytest.mark.parametrize("poison,base,classes", nc.CASES, ids=[f"{p}-{b}" for p, b, _ in nc.CASES])
def test_poisoned_scene_shows_its_classes_and_walks_the_clean_control_flow(poison, base, classes, native, oracle_mod, abi):
    host, _ = native
    st, opt = nc.settings(abi), nc.options(abi, base)
    clean_linear, clean = clean_of(oracle_mod, abi, host, base, opt)
    sc = nc.scene(abi, host, base, poison)
    _, linear, cnt = oracle_mod.render(sc, sc.camera, st, opt)
    assert (cnt.rays, cnt.depth_exhausted, cnt.samples) == (clean.rays, clean.depth_exhausted, clean.samples), (poison, base)
    shares = nc.class_shares(linear)
    print(poison, base, {k: round(v, 4) for k, v in shares.items()})
    for c in classes:
        assert shares[c] >= 0.02, (poison, base, c, shares)
    assert shares["finite"] >= 0.05, (poison, base, shares)
    if not classes:                                                  # in-range poisons (albedo 0, > 1): the image must at least differ from the clean one
        assert (linear != clean_linear).any(-1).mean() >= 0.02


@pytest.mark.parametrize("poison,base", nc.REF_CASES, ids=[f"{p}-{b}" for p, b in nc.REF_CASES])
def test_reference_stream_cases_show_their_classes(poison, base, native, oracle_mod, abi):
    host, _ = native
    st, opt = nc.settings(abi), abi.Options.make(rng_mode=abi.RNG_REF)      # (the flag of the fixed-AABB bases needs counter mode)
    _, clean = clean_of(oracle_mod, abi, host, base, opt, key="reference stream")
    sc = nc.scene(abi, host, base, poison)
    _, linear, cnt = oracle_mod.render(sc, sc.camera, st, opt)
    assert (cnt.rays, cnt.depth_exhausted) == (clean.rays, clean.depth_exhausted)
    shares = nc.class_shares(linear)
    want = next(c for p, b, c in nc.CASES if (p, b) == (poison, base))
    assert all(shares[c] >= 0.02 for c in want) and shares["finite"] >= 0.05, shares
