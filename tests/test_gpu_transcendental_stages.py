"""The device's transcendental stages against the oracle's libm, over enumerated inputs rather than sample frames.

Seven call sites of the device code evaluate acosf / atan2f / fmodf (texture_lookup, miss_colour) and ln / atan / sin / cos (the rough
conductor's half-vector sampling, scatter_pre).  Scenes that reach them get the tolerant contract of tests/parity.py; these tests check what
that tolerance is said to cover, input by input.  The device side is mi355rt_debug_stages of the reference build (csrc/refs/rt_stages.hip),
which runs the shipped device functions; the oracle side is oracle_debug_stages (oracle/rt_oracle.cpp), which runs the oracle's render-path
functions on the same inputs, rounds a float64 evaluation of every transcendental once, and counts differences in C++ chunk by chunk.

Domains: u = every value of u32_to_f01 (k * 2^-24); roughness: veach-mis's Beckmann values, semesterbild's GGX 0.1, and both kinds at
2^-20, 0.02, 0.5, 1.0; HALF (the whole rough-conductor branch): u1 over the lattice at 4 fixed u2 and u2 over the lattice at 4 fixed u1, on three
normals (+z; |n.z| >= 0.999, which switches to_world's up vector; a generic one) at normal and 89.9 degree incidence, every lattice value
for the scenes' roughness and every 64th for the rest (_half_cases); ACOS: every
f32 with |y| <= 1 + 2^-20; ATAN2: the structured sets on the device against their closed forms, 2^28 pseudo-random directions against the
oracle; TEX / SKY: image sizes down to 1 x 1; FMOD: every f32 u in [0, 1] for each h_offset.

The counter-mode bounds below (in f32 steps from the float64 value rounded once) are the measured maxima; profiles/transcendental_stages.txt
holds the counts (tools/transcendental_stages.py writes it from record())."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, pkg

sys.path.insert(0, os.path.join(ROOT, "tests"))
from parity import oracle_threads  # noqa: E402

LATTICE = 1 << 24
CHUNK = 1 << 22
PI_F = np.float32(np.pi)
ROUGH = ([("beckmann", r) for r in (0.01, 0.05, 0.1, 0.25)] + [("ggx", 0.1)] +
         [(kind, r) for kind in ("beckmann", "ggx") for r in (2.0 ** -20, 0.02, 0.5, 1.0)])
SCENE_ROUGH = ROUGH[:5]                                   # veach-mis's and semesterbild's values
FIXED_U2 = (0.0, 2.0 ** -24, 0.5, 1.0 - 2.0 ** -24)       # lattice values, the ends of the draws among them
# u1: the two ends (0 clamps to 1e-6, where ln already differs: attribution cannot bite there) and two lattice values near 0.25 / 0.5 where
# every transcendental of u1 agrees with the oracle, chosen per roughness (_agreeing_u1), so that on those lines a differing output must
# come from phi's sin / cos
FIXED_U1_ENDS = (0.0, 1.0 - 2.0 ** -24)
FULL_STRIDE, OTHER_STRIDE = 1, 64
NORMALS = {"+z": (0.0, 0.0, 1.0), "near_z": (0.0, 0.04471018, 0.9990000), "generic": (0.48, -0.6, 0.64)}
INCIDENCE = {"normal": 0.0, "grazing_89.9": np.radians(89.9)}
H_OFFSETS = (0.0, 0.3, 0.999999, 1.0 - 2.0 ** -24, 0.13218, 0.47706, 0.61534, 0.88243)   # the last four in the range the fuzz scenes draw, U(0.1, 0.9)
TEX_SIZES = (1, 2, 3, 5, 8, 16, 255, 256)
SKY_SIZES = [(w, h) for w in TEX_SIZES for h in TEX_SIZES] + [(1024, 512), (2048, 1024)]

# Counter mode: the device's largest distance from the float64 value, per function, in f32 steps (measured over the domains above)
# (glibc's maxima over the same inputs, in the record: 1 for every function)
BOUND_CTR = {"ln": 2, "atan": 2, "sin_theta": 1, "cos_theta": 1, "sin_phi": 1, "cos_phi": 2, "acos": 1, "atan2": 3}
WORDS_LATTICE = {"ln": 0, "atan": 2, "sin_theta": 3, "cos_theta": 4, "sin_phi": 5, "cos_phi": 6}

_RECORD = []                                              # (stage, domain, form, n, per-word differences, device / glibc ulp maxima, unattributed)


def record():
    return list(_RECORD)


def _mods():
    import oracle
    return pkg("device"), pkg("abi"), oracle


def _args(stage, form=0, first=0, stride=1, **kw):
    device = pkg("device")
    a = device.StageArgs()
    a.stage, a.form, a.first, a.stride = device.STAGES[stage], form, first, stride
    for k, v in kw.items():
        if k in ("n", "rd"):
            getattr(a, k)[:3] = v
        else:
            setattr(a, k, v)
    return a


def _run(stage, n, args, domain, in4=None, mat=None, tex=None, tex_rgba=None, sky=None, chunk=CHUNK):
    """Device, then oracle, chunk by chunk; returns the summed res (oracle_debug_stages' layout) and the device's words of the last chunk."""
    device, _, oracle = _mods()
    total = np.zeros(64)
    total[[4 * w + 3 for w in range(8)] + [33]] = -1
    words = None
    for c0 in range(0, n, chunk):
        m = min(chunk, n - c0)
        a = type(args).from_buffer_copy(args)
        a.first = args.first + c0 * args.stride
        sub = None if in4 is None else in4[c0:c0 + m]
        words = device.debug_stages(a, m, sub, mat, tex_rgba, sky)
        res, _ = oracle.debug_stages(a, m, sub, mat, tex, sky, dev=words, threads=oracle_threads())
        for w in range(8):
            total[4 * w] += res[4 * w]
            total[4 * w + 1] = max(total[4 * w + 1], res[4 * w + 1])
            total[4 * w + 2] = max(total[4 * w + 2], res[4 * w + 2])
            if total[4 * w + 3] < 0 <= res[4 * w + 3]:
                total[4 * w + 3] = c0 + res[4 * w + 3]
        total[32] += res[32]
        total[34] += res[34]
        if total[33] < 0 <= res[33]:
            total[33] = c0 + res[33]
    total[35] = n
    _RECORD.append((stage, domain, args.form, n, total.copy()))
    return total, words


def _diffs(res):
    return [int(res[4 * w]) for w in range(8)]


def _material(abi, ggx, rough):
    m = abi.Material()
    m.kind = abi.MAT_ROUGH_GGX if ggx else abi.MAT_ROUGH_BECKMANN
    m.albedo[:] = (0.9, 0.8, 0.7); m.p0 = rough; m.eta[:] = (0.2, 1.09, 1.42); m.k[:] = (3.91, 2.57, 2.30)
    return m


def _incoming(normal, angle):
    """A unit direction arriving at `angle` from the normal (f32, as a hit hands it to scatter)."""
    n = np.asarray(normal, np.float64); n /= np.linalg.norm(n)
    t = np.cross(n, [1.0, 0.0, 0.0] if abs(n[0]) < 0.9 else [0.0, 1.0, 0.0]); t /= np.linalg.norm(t)
    return tuple(np.float32(-(np.cos(angle) * n + np.sin(angle) * t)))


# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind,rough", ROUGH, ids=[f"{k}-{r:g}" for k, r in ROUGH])
def test_microfacet_transcendentals_over_every_u(kind, rough):
    """ln(u1), atan(sqrt(theta_arg)), sin / cos of theta and of phi = 2 pi u for every u the generators can draw.  REF form: the device equals
    the oracle bit for bit.  CTR form: every function within BOUND_CTR of the float64 value; theta_arg (plain f32 arithmetic on ln) differs
    only where ln does."""
    ggx = kind == "ggx"
    for form in (1, 0):
        res, _ = _run("lattice", LATTICE, _args("lattice", form, ggx=int(ggx), rough=rough), f"{kind} {rough:g}")
        if form == 1:
            assert _diffs(res) == [0] * 8, ("REF form differs from the oracle", _diffs(res), res[3::4][:8])
            continue
        for name, w in WORDS_LATTICE.items():
            assert res[4 * w + 1] <= BOUND_CTR[name], (name, res[4 * w + 1], "glibc", res[4 * w + 2])
        assert res[32] == 0, ("theta_arg differs where ln does not", res[33])


def _half_cases():
    """Every lattice value on both axes for the scene roughness values on +z at normal incidence and for veach-mis's 0.1 and semesterbild's
    GGX 0.1 on every normal and incidence; every 64th elsewhere (the whole product does not fit the module's time budget: the oracle's
    side of one lattice line costs about 0.3 s on 16 CPUs)."""
    for kind, rough in ROUGH:
        for nname in NORMALS:
            for iname in INCIDENCE:
                full = ((kind, rough) in SCENE_ROUGH and nname == "+z" and iname == "normal") or (kind, rough) in (("beckmann", 0.1), ("ggx", 0.1))
                yield kind, rough, nname, iname, full


def _agreeing_u1(kind, rough, near):
    """The first lattice value at or above `near` whose ln, theta_arg, theta, sin and cos theta the device computes as the oracle does."""
    device, _, oracle = _mods()
    k0 = int(near * LATTICE)
    a = _args("lattice", 0, first=k0, ggx=int(kind == "ggx"), rough=rough)
    dev = device.debug_stages(a, 4096)
    _, ora = oracle.debug_stages(a, 4096, dev=dev, want_words=True, threads=oracle_threads())
    same = np.nonzero((dev[:, :5] == ora[:, :5]).all(axis=1))[0]
    assert len(same), (kind, rough, near)
    return (k0 + int(same[0])) / LATTICE


@pytest.mark.gpu
@pytest.mark.parametrize("form", (1, 0), ids=("ref", "ctr"))
def test_rough_conductor_branch_over_the_lattice(form):
    """The shipped rough-conductor branch of scatter_pre<MATS_ALL> (direction, attenuation, absorbed or not) with the draws (u1, u2): u1 over
    the lattice at 4 fixed u2 and u2 over the lattice at 4 fixed u1, for every roughness, normal and incidence (the domain: _half_cases).
    REF form: bit for bit.  CTR form: an output differs only where a transcendental of the same draws differs, and on the u2 lines at a u1
    whose transcendentals agree that check is not vacuous (some draws have every transcendental equal)."""
    _, abi, _ = _mods()
    unattributed, differ, n_all = 0, 0, 0
    for kind, rough, nname, iname, full in _half_cases():
        ggx = kind == "ggx"
        mat = _material(abi, ggx, rough)
        rd = _incoming(NORMALS[nname], INCIDENCE[iname])
        stride = FULL_STRIDE if full else OTHER_STRIDE
        n = (LATTICE + stride - 1) // stride
        agreeing = tuple(_agreeing_u1(kind, rough, near) for near in (0.25, 0.5)) if form == 0 else (0.25, 0.5)
        for axis, fixed_values in ((0, FIXED_U2), (1, FIXED_U1_ENDS + agreeing)):
            for fixed in fixed_values:
                a = _args("half", form, stride=stride, ggx=int(ggx), rough=rough, axis=axis, fixed_u=fixed, n=NORMALS[nname], rd=rd)
                res, _ = _run("half", n, a, f"{kind} {rough:g} n={nname} {iname} axis={axis} fixed={fixed:.9g}", mat=mat)
                n_all += n
                if form == 1:
                    assert _diffs(res)[:7] == [0] * 7, (kind, rough, nname, iname, axis, fixed, _diffs(res), res[3::4][:8])
                elif axis == 1 and fixed in agreeing:
                    assert res[28] < n, (kind, rough, nname, iname, fixed, "every signature differs: attribution would be vacuous")
                unattributed += int(res[32]); differ += int(res[34])
    assert unattributed == 0, (unattributed, differ)
    assert n_all >= 15 * 8 * LATTICE


@pytest.mark.gpu
def test_acos_over_every_f32_up_to_one_and_a_bit():
    """acosf over every f32 with |y| <= 1 + 2^-20: within BOUND_CTR of the float64 value; the poles exact; beyond 1 NaN on both sides."""
    n = 2 * 0x3F800009
    res, _ = _run("acos", n, _args("acos"), "|y| <= 1 + 2^-20", chunk=1 << 26)
    assert res[1] <= BOUND_CTR["acos"], (res[1], "glibc", res[2])
    special = np.zeros((8, 4), np.float32)
    special[:, 0] = [1.0, -1.0, np.nextafter(np.float32(1), np.float32(2)), -np.nextafter(np.float32(1), np.float32(2)), np.nan, np.inf, -np.inf, 0.0]
    device, _, oracle = _mods()
    words = device.debug_stages(_args("acos"), 8, special)[:, 0].view(np.float32)
    assert words[0] == 0.0 and words[1] == PI_F and np.isnan(words[2:7]).all() and words[7] == np.float32(np.pi / 2)
    res, _ = oracle.debug_stages(_args("acos"), 8, special, dev=words.view(np.uint32).reshape(8, 1), threads=oracle_threads())
    assert res[0] == 0


@pytest.mark.gpu
def test_atan2_structured_sets_have_their_closed_forms():
    """z = +-0 with every finite x, x = +-0 with every finite z, |z| = |x| for every finite magnitude in the four sign combinations: the device
    returns +-0, +-pi/2 and +-pi rounded to f32 exactly, with the sign of zero honoured (the texture and sky seam).  On the diagonal it
    returns +-pi/4 / +-3pi/4 or their neighbour one f32 step away -- for about a quarter of all magnitudes (the counts are in
    profiles/transcendental_stages.txt) -- and never anything further off."""
    device, _, _ = _mods()
    for s in range(8):
        n = 1 << 32 if s < 4 else 1 << 31
        bad = device.debug_stages(_args("atan2_exact", set=s), n)
        _RECORD.append(("atan2x", f"set {s}: " + ("z = +-0, every finite x" if s < 2 else "x = +-0, every finite z" if s < 4 else "|z| = |x|, every finite")
                        + ("" if s < 4 else f"; one f32 step off: {int(bad[2])}"), 0, n, np.array([bad[0]] + [0] * 63, np.float64)))
        assert bad[0] == 0, (s, int(bad[0]), hex(int(bad[1])))
        if s < 4:
            assert bad[2] == 0


def _special_dirs():
    inf, nan = np.inf, np.nan
    d = [(-1, 0.3, 0.0), (-1, 0.3, -0.0), (-1, -0.0, 0.0), (-1, 0.0, -0.0), (1, 0.3, 0.0), (1, 0.3, -0.0),
         (0, 1, 0), (0, -1, 0), (0.0, 1.0, -0.0), (-0.0, -1.0, 0.0), (1e-30, 1, 0), (0, 0, 0), (-0.0, -0.0, -0.0),
         (nan, 0, 0), (0, nan, 0), (0, 0, nan), (inf, 0, 0), (-inf, 0, 0), (0, inf, 0), (0, 0, inf), (0, 0, -inf), (inf, 0, inf), (-inf, 0, -inf),
         (inf, inf, inf), (-1, 0, 1e-45), (-1, 0, -1e-45), (3.4e38, 0, -3.4e38), (1e-38, 1e-38, 1e-38)]
    out = np.zeros((len(d), 4), np.float32)
    out[:, :3] = np.array(d, np.float32)
    return out


@pytest.mark.gpu
def test_atan2_random_directions_and_special_values():
    """atan2f on 2^28 pseudo-random directions within BOUND_CTR of the float64 value, and on +-Inf, NaN, zero and seam inputs equal to glibc."""
    res, _ = _run("atan2", 1 << 28, _args("atan2"), "2^28 directions", chunk=1 << 26)
    assert res[1] <= BOUND_CTR["atan2"], (res[1], "glibc", res[2])
    sp = _special_dirs()
    res, _ = _run("atan2", len(sp), _args("atan2"), "special", in4=sp)
    assert res[0] == 0, res[3]


def _texture(w, h):
    _, abi, _ = _mods()
    import ctypes as C
    texels = (np.arange(w, dtype=np.uint32)[None, :] | (np.arange(h, dtype=np.uint32)[:, None] << 8)).astype(np.uint32)
    texels = np.ascontiguousarray(texels)
    tex = abi.Texture(texels.ctypes.data_as(C.POINTER(C.c_uint8)), w, h)
    return texels, tex


@pytest.mark.gpu
def test_texture_lookup_every_size_and_offset():
    """texture_lookup on textures whose texels encode their own (x, y), every size and h_offset: a texel differs from the oracle's only where
    acosf / atan2f / fmodf of the same normal differ; on the seam, poles, NaN / Inf / zero normals and 1-texel maps it is the oracle's exactly."""
    unattributed, n_special = 0, 0
    sp = _special_dirs()
    for w in TEX_SIZES:
        for h in TEX_SIZES:
            texels, tex = _texture(w, h)
            for hoff in H_OFFSETS:
                a = _args("tex", img_w=w, img_h=h, h_offset=hoff)
                res, _ = _run("tex", 1 << 14, a, f"{w}x{h} h={hoff:.9g}", tex=tex, tex_rgba=texels)
                unattributed += int(res[32])
                res, words = _run("tex", len(sp), a, f"{w}x{h} h={hoff:.9g} special", in4=sp, tex=tex, tex_rgba=texels)
                assert _diffs(res)[:3] == [0, 0, 0], (w, h, hoff, res[3::4][:3])
                if w == 1 and h == 1:
                    assert (words[:, :3].view(np.float32) == 0).all()
                n_special += len(sp)
    assert unattributed == 0


@pytest.mark.gpu
def test_sky_lookup_every_size_and_the_seam():
    """miss_colour on skies whose floats are their own index: every size up to 2048 x 1024; a texel differs from the oracle's only where acosf /
    atan2f differ; the seam picks column W-1 for z = +0 and column 0 for z = -0 (x < 0), the poles rows 0 and H-1, exactly as the oracle."""
    unattributed = 0
    sp = _special_dirs()
    for w, h in SKY_SIZES:
        sky = np.arange(w * h * 3, dtype=np.float32).reshape(h, w, 3)
        a = _args("sky", img_w=w, img_h=h)
        res, _ = _run("sky", 1 << 16, a, f"{w}x{h}", sky=sky)
        unattributed += int(res[32])
        res, words = _run("sky", len(sp), a, f"{w}x{h} special", in4=sp, sky=sky)
        assert _diffs(res)[:3] == [0, 0, 0], (w, h, res[3::4][:3])
        idx = words[:, 0].view(np.float32) / 3
        col, row = idx % w, idx // w
        assert col[0] == w - 1 and col[1] == 0, (w, h, col[:2])                   # (-1, 0.3, +0) / (-1, 0.3, -0)
        assert row[6] == 0 and row[7] == h - 1, (w, h, row[6:8])                  # the poles
    assert unattributed == 0


@pytest.mark.gpu
@pytest.mark.parametrize("hoff", H_OFFSETS)
def test_fmod_is_exact_for_every_u(hoff):
    """fmodf(u + h, 1) equals a - floorf(a) for every f32 u in [0, 1] on the device; the oracle's std::fmod does too (on the same inputs)."""
    device, _, oracle = _mods()
    n = 0x3F800001
    bad = device.debug_stages(_args("fmod_exact", h_offset=hoff), n)
    assert bad[0] == 0, (hoff, int(bad[0]), hex(int(bad[1])))
    res, _ = oracle.debug_stages(_args("fmod_exact", h_offset=hoff), n, threads=oracle_threads())
    assert res[0] == 0, (hoff, res[1])
    _RECORD.append(("fmod", f"every u in [0, 1], h={hoff:.9g}", 0, n, np.array([bad[0]] + [0] * 63, np.float64)))
