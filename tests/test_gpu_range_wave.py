"""k_render_ctr_simple_qc's range arithmetic on waves whose lanes the test chooses (the reference build's probe, csrc/refs/rt_range_wave_probe.h).

Each range form (rt_math.h "Range arithmetic") ballots its operands over the wave's active lanes and sends the WHOLE wave to the guarded form, out of
line, when one lane is outside the range.  The probe runs the shipped normalized_ranged, ray_direction, hit_quad and hit_cube -- the functions themselves,
as walk_list and the bounce call them -- on three kinds of waves:
  * all 64 lanes ordinary (the straight line);
  * one odd lane among 63 ordinary ones, at a lane that moves, cycling through a zero vector, a vector below 1e-4, NaN, infinity, a denormal component,
    a direction whose object-space x is zero, and a direction with denom below EPS against the quad (and an origin beyond 2^60: a wide wave) -- so the wave
    takes an out-of-line path while 63 lanes hold ordinary values;
  * half the lanes inactive (a partial exec mask under the ballots), with and without an odd lane among the active ones, and with poison in inactive lanes.
Every word of every lane with the RANGE bits the library ships (selector 1) and with all four steps (selector 2) equals the guarded forms' (selector 0),
and every direction equals the numpy restatement of normalized(normalized(raw)) (vec3.rs:37-44 twice, numpy's correctly rounded sqrt and division)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F = np.float32
EPS = F(1e-4)

QUAD = np.array([0, 0, 1, 0,  -1, -1, 0,  2, 0, 0,  0, 2, 0,  0.25, 0.25, 0], F)          # n, d, base, e0, e1, 1 / |e0|^2, 1 / |e1|^2: the square [-1, 1]^2 in z = 0
CUBE = np.array([1, 0, 0,  0, 1, 0,  0, 0, 1,  0, 0, 2,  0, 0, 0,  0,                      # w2o columns, zd, pad: the unit cube centred at (0, 0, -2)
                 1, 0, 0,  0, 1, 0,  0, 0, 1,  0, 0, -2], F)                                 # o2w columns
FLAT = CUBE.copy(); FLAT[0] = 0                                                             # ... with zero scale on x: every object-space direction has x == 0

ODD = {
    "zero vector": ((0, 0, 0), None),
    "below 1e-4": ((3e-5, -2e-5, 1e-5), None),
    "NaN": ((np.nan, 0.3, -1), None),
    "infinity": ((np.inf, 0.3, -1), None),
    "denormal component": ((1e-40, 0.6, -0.8), None),
    "zero object-space component": ((0, 0.1, -1), None),
    "denom below EPS": ((1, 0.2, -5e-5), None),
    "origin beyond 2^60 (a wide wave)": ((0.1, 0.1, -1), (0, 0, 2.0 ** 61)),
}


def _ordinary(rng, n):
    rec = np.zeros((n, 16), np.uint32)
    v = np.concatenate([rng.uniform(-0.25, 0.25, (n, 2)), -np.ones((n, 1))], axis=1) * rng.uniform(0.1, 3.0, (n, 1))
    ro = np.concatenate([rng.uniform(-0.4, 0.4, (n, 2)), np.full((n, 1), 3.0)], axis=1)
    rec[:, 0:3] = F(v).view(np.uint32); rec[:, 3:6] = F(ro).view(np.uint32); rec[:, 6] = 1
    return rec


def _put(rec, lane, v, ro):
    rec[lane, 0:3] = np.array(v, F).view(np.uint32)
    if ro is not None:
        rec[lane, 3:6] = np.array(ro, F).view(np.uint32)


def _waves():
    rng = np.random.default_rng(11)
    waves, names = [_ordinary(rng, 64)], ["all lanes ordinary"]
    for k, (name, (v, ro)) in enumerate(ODD.items()):
        w = _ordinary(rng, 64); _put(w, (7 * k + 3) % 64, v, ro)
        waves.append(w); names.append(f"one odd lane: {name}")
    w = _ordinary(rng, 64); w[1::2, 6] = 0
    waves.append(w); names.append("odd lanes inactive")
    w = _ordinary(rng, 64); w[:32, 6] = 0
    for lane in range(0, 32, 4):                                                            # poison where no lane runs: it must not reach a ballot
        _put(w, lane, (np.nan, np.inf, 0), (np.nan, 0, 2.0 ** 90))
    waves.append(w); names.append("lower half inactive and poisoned")
    for k, (name, (v, ro)) in enumerate(ODD.items()):
        w = _ordinary(rng, 64); w[0::2, 6] = 0; _put(w, 2 * ((5 * k) % 32) + 1, v, ro)
        waves.append(w); names.append(f"even lanes inactive, one odd active lane: {name}")
    return np.concatenate(waves), names


def _normalized(v):
    with np.errstate(all="ignore"):
        l = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2], dtype=F)
        r = F(1) / l
        return np.where((l < EPS)[:, None], v, v * r[:, None]).astype(F)


def _same(a, b):
    """Bit for bit; two NaNs count as the same value (the guarded forms return the hardware's NaN, whatever the operand's payload was)."""
    fa, fb = a.view(F), b.view(F)
    return (a == b) | (np.isnan(fa) & np.isnan(fb))


@pytest.mark.parametrize("cube", ["unit", "flat"])
def test_range_forms_on_chosen_waves(cube, native):
    host, device = native
    rec, names = _waves()
    cube_d = CUBE if cube == "unit" else FLAT
    ref, bits0 = device.debug_range_wave(0, QUAD, cube_d, rec)
    shipped, bits1 = device.debug_range_wave(1, QUAD, cube_d, rec)
    every, bits2 = device.debug_range_wave(2, QUAD, cube_d, rec)
    assert bits0 == 0 and bits2 == 15 and bits1 & 1                                        # the closed-form second normalisation is among what ships
    active = rec[:, 6] == 1
    assert not ref[~active].any() and not shipped[~active].any() and not every[~active].any()
    for got, what in ((shipped, f"RANGE {bits1}"), (every, "RANGE 15")):
        bad = ~_same(got, ref).all(axis=1)
        assert not bad.any(), (what, [(names[i // 64], i % 64, got[i].tolist(), ref[i].tolist()) for i in np.flatnonzero(bad)[:3]])
    # the guarded forms themselves against numpy: both normalisations
    raw = rec[:, 0:3].view(F)
    once = _normalized(raw)
    want = _normalized(once)
    assert _same(ref[active, 0:3], once[active].view(np.uint32)).all()
    assert _same(ref[active, 3:6], want[active].view(np.uint32)).all()
    # the waves do what they are for: ordinary lanes hit the quad, some the cube behind it; the odd lanes are rejected or passed through
    ordinary = ref[:64]
    assert (ordinary[:, 6].view(F) == 1).sum() >= 48 and (ordinary[:, 7].view(F) > 1).all()
    assert (ordinary[:, 8].view(F) == 1).sum() >= 4                                        # (the flat cube's x slab is (-inf, +inf): y and z decide)
    lane = {n: 64 * (1 + k) + (7 * k + 3) % 64 for k, n in enumerate(ODD)}
    assert np.array_equal(ref[lane["zero vector"], 3:6], np.zeros(3, np.uint32))
    assert np.array_equal(ref[lane["below 1e-4"], 3:6], rec[lane["below 1e-4"], 0:3])       # passed through twice
    assert np.isnan(ref[lane["NaN"], 3:6].view(F)).all() and np.isnan(ref[lane["infinity"], 3:6].view(F)).any()
    assert ref[lane["denom below EPS"], 6] == 0 and ref[lane["origin beyond 2^60 (a wide wave)"], 6] == 0
