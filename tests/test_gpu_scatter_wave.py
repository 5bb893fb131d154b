"""The bounce's shipped pieces -- scatter_pre, unit_ball_cooperative, ball_finish, scatter_origin, ray_direction -- on whole waves whose lanes
the test chooses, through every form the library launches (the reference build's probe, csrc/refs/rt_scatter_wave_probe.h), against the
oracle's sequential Material::scatter.  Everything is exact: every output word of every lane equals the oracle's, the sign of zero and the
scattered flag included (a NaN matches any NaN), and the accepted unit-ball point equals the one the address search found.

  * waves of Lambert lanes with 0 .. 64 owners (lanes that still need a try behind the tries of their own lane), placed low, high, strided
    and shuffled, beside lanes accepted at once, idle lanes with garbage generator words, or both; owners shallow, all at try 8 or later (lg
    stays 0 for many rounds), one to four at try 16 or later (the last rounds run with one owner and 64 workers), half at try 12 or later;
  * the same with diffuse, fuzzed-metal and ball-free lanes in one wave, for the forms that have those kinds;
  * records at the edges: 2^12 per exact kind and face over every parameter value of tests/scatter_wave_cases.py (IOR 1, below 1, 0, inf,
    NaN; fuzz up to 1 and beyond; checker cells at the saturation limits), the critical angle +- 64 steps, glancing mirrors, fuzz 1 at the
    surface, near_zero taken and just missed, rough conductors whose sampled angle is 0 or the fallback, non-finite inputs -- also through the
    product's per-record hook (mi355rt_debug_scatter: the sequential form that k_render_ref ships).

The deepest first accepted try over all waves is 23 (the all-ones key at ray 30; 21 and 20 in the other two settings): 24 tries, where a
frame of a fuzz scene practically never shows a lane past try 12.  tests/test_scatter_wave_cpu.py holds the oracle's side: the pools'
conditions, the pin to kat_f32 and the branch census.  tools/scatter_wave_report.py writes profiles/scatter_wave_probe.txt from the same run.
"""
import numpy as np
import pytest

import scatter_wave_cases as W

pytestmark = pytest.mark.gpu
u32 = np.uint32
WORDS = ("scattered", "origin", "origin", "origin", "direction", "direction", "direction", "attenuation", "attenuation", "attenuation",
         "emitted", "emitted", "emitted", "ball point", "ball point", "ball point")


def distinct_forms(device):
    """The probe's forms grouped by the template arguments they resolve to: [(form number, form, [kernels])], every kernel in one group."""
    groups = {}
    for i, f in enumerate(device.scatter_wave_forms()):
        key = tuple(f[k] for k in ("mats", "wide", "fastn", "try1", "terminal_done", "stepped", "in_place"))
        groups.setdefault(key, (i, f, []))[2].append(f["kernel"])
    return list(groups.values())


@pytest.fixture(scope="module")
def setup(native, oracle_mod, abi):
    host, device = native
    mats_c = W.materials_ctypes(abi)
    forms = distinct_forms(device)
    assert sum(len(k) for _, _, k in forms) == 13 and len(forms) >= 7
    return device, oracle_mod, mats_c, forms


_refs = {}


def reference_of(key, oracle_mod, mats_c, records):
    """The oracle's side of a record set, computed once and shared by every form."""
    if key not in _refs:
        _refs[key] = W.reference(oracle_mod, mats_c, records)
        for a in _refs[key]:
            a.flags.writeable = False
    return _refs[key]


def describe(kernels, got, want, bad, names=None, n_words=16):
    i = int(np.argmax(bad))
    words = sorted({WORDS[c] for c in range(n_words) if not _same(got[i, c], want[i, c])})
    where = f"wave {i // 64} ({names[i // 64]}), lane {i % 64}" if names is not None else f"record {i}"
    return f"{'/'.join(kernels)}: {int(bad.sum())} of {bad.size} records differ; first: {where}: {', '.join(words)}; got {got[i].view(np.float32)}, want {want[i].view(np.float32)}"


def _same(g, w):
    return g == w or (np.isnan(np.array(g, u32).view(np.float32)) and np.isnan(np.array(w, u32).view(np.float32)))


def run_lambert_waves(device, oracle_mod, mats_c, form_no, form, kernels):
    recs, names = W.lambert_waves(form["try1"])
    want, tries, _ = reference_of(("lambert", form["try1"]), oracle_mod, mats_c, recs)
    got = device.debug_scatter_wave(form_no, mats_c, recs)
    bad = W.differing(got, want)
    return recs, names, want, tries, got, bad


def test_lambert_waves_through_every_form(setup):
    device, oracle_mod, mats_c, forms = setup
    failures = []
    for form_no, form, kernels in forms:
        recs, names, want, tries, got, bad = run_lambert_waves(device, oracle_mod, mats_c, form_no, form, kernels)
        live = (recs[:, 1] & W.LIVE) != 0
        assert not want[~live].any() and (tries[live] >= 1).all() and tries.max() >= 17
        print(f"{'/'.join(kernels)}: {len(names)} waves, {int(live.sum())} live lanes, {int(bad.sum())} differ")
        if bad.any():
            failures.append(describe(kernels, got, want, bad, names))
    assert not failures, "\n".join(failures)


def test_mixed_material_waves(setup):
    device, oracle_mod, mats_c, forms = setup
    failures, ran = [], 0
    for form_no, form, kernels in forms:
        kinds = tuple(k for k in range(10) if (form["mats"] >> k) & 1)
        if W.CHECKER not in kinds:
            continue                                                # (the Lambert-only forms have one scattering kind)
        recs, names = W.mixed_waves(kinds)
        want, tries, _ = reference_of(("mixed", kinds), oracle_mod, mats_c, recs)
        got = device.debug_scatter_wave(form_no, mats_c, recs)
        bad = W.differing(got, want)
        scattered = want[:, 0] != 0
        live = (recs[:, 1] & W.LIVE) != 0
        assert (live & (tries == 0)).sum() > 100 and (tries > 8).sum() > 100          # ball-free lanes and deep owners share the waves
        if W.METAL in kinds:
            assert (live & ~scattered & (tries > 8)).sum() >= 8                          # fuzzed reflections absorbed after a deep try
        print(f"{'/'.join(kernels)}: {len(names)} mixed waves, {int(bad.sum())} differ")
        ran += 1
        if bad.any():
            failures.append(describe(kernels, got, want, bad, names))
    assert ran >= 4
    assert not failures, "\n".join(failures)


def test_edge_records_through_every_form(setup):
    device, oracle_mod, mats_c, forms = setup
    recs, cls, names = W.edge_records()
    want, tries, _ = reference_of("edge", oracle_mod, mats_c, recs)
    failures = []
    for form_no, form, kernels in forms:
        ok = W.for_form(form, recs)
        got = device.debug_scatter_wave(form_no, mats_c, recs[ok])
        bad = W.differing(got, want[ok])
        print(f"{'/'.join(kernels)}: {int(ok.sum())} edge records, {int(bad.sum())} differ")
        if bad.any():
            per_class = {names[c]: int(((cls[ok] == c) & bad).sum()) for c in np.unique(cls[ok][bad])}
            failures.append(describe(kernels, got, want[ok], bad) + f"; by class {per_class}")
    assert not failures, "\n".join(failures)


def test_edge_records_through_the_products_hook(setup):
    """mi355rt_debug_scatter: scatter_pre<MATS_ALL> with the sequential rejection loop, one record per lane in the same seeded shuffle (ball and
    ball-free lanes share waves).  Its record has no ball point; the other 13 words are compared.  Where the hook itself says that nothing was
    scattered its ray and attenuation words are whatever scatter_pre left there (Material::scatter returned None: there is no ray; the oracle's
    record holds +0): the flag and the emitted colour are compared, as device.debug_scatter's callers always have."""
    device, oracle_mod, mats_c, forms = setup
    recs, cls, names = W.edge_records()
    want, tries, _ = reference_of("edge", oracle_mod, mats_c, recs)
    got = products_hook(device, mats_c, recs)
    assert not got[:, 13:].any()
    bad = W.differing(got, want, 13)
    per_class = {names[c]: int(((cls == c) & bad).sum()) for c in np.unique(cls[bad])}
    assert not bad.any(), describe(["k_debug_scatter"], got, want, bad, n_words=13) + f"; by class {per_class}"


def products_hook(device, mats_c, recs):
    rin = recs.copy()
    rin[:, 1] &= 1                                                  # (the hook's second word is the front face alone)
    got = device.debug_scatter_records(mats_c, rin)
    got[got[:, 0] == 0, 1:10] = 0
    return got
