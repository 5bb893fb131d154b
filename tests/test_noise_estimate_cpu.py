"""mi355rt_noise_* (libmi355rt_host.so, pure CPU): the library against the numpy float64 restatement of the header's definition
(tests/noise_ref.py) bit for bit, the two structs against the C compiler, every refusal with its text, and two calibrations -- on synthetic
sums with a known variance, and on independent renders of the CPU oracle against a long reference render."""
import ctypes as C
import json
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from conftest import ROOT
from noise_ref import DEFAULTS, NoiseRef

NEW = ("mi355rt_noise_create", "mi355rt_noise_free", "mi355rt_noise_reset", "mi355rt_noise_update", "mi355rt_noise_evaluate")
SUMMARY_FIELDS = ("chunks", "samples", "pixels", "above", "nonfinite", "max_error", "mean_error", "converged", "_pad")
PARAM_FIELDS = ("threshold", "floor", "min_chunks", "_pad", "allowed_above")


def _bits64(v):
    return np.array([v], np.float64).view(np.uint64)[0]


def _same(host, abi, sums, totals, width, rows, **params):
    """Feeds the same running sums to the library and to the restatement; asserts the map and every summary field bit for bit after every
    chunk from the second on.  Returns the last (map, summary dict)."""
    st, ref = host.NoiseState(width, rows), NoiseRef(width, rows)
    got = None
    kw = dict(DEFAULTS, **params)
    for k, (a, n) in enumerate(zip(sums, totals), 1):
        st.update(a, n)
        ref.update(a, n)
        if k < 2:
            continue
        err, s = st.evaluate(abi.NoiseParams.make(**kw))
        want_err, want = ref.evaluate(**kw)
        assert np.array_equal(err.view(np.uint32), want_err.view(np.uint32)), f"error map after chunk {k}"
        for f in SUMMARY_FIELDS:
            g, w = getattr(s, f), want[f]
            assert (_bits64(g) == _bits64(w)) if isinstance(w, float) else (g == w), (k, f, g, w)
        got = (err, want)
    st.close()
    return got


def _random_sums(rng, width, rows, sizes, scale=1.0, signed=False):
    """Running sums in float32 (what d_accum holds) and their sample totals: every chunk adds n draws' worth to every channel."""
    acc = np.zeros((rows * width, 4), np.float32)
    acc[:, 3] = np.float32(123.0)                                       # the fourth float is not read
    out, totals, total = [], [], 0
    for n in sizes:
        inc = (rng.gamma(2.0, 0.25, (rows * width, 3)) * n * scale).astype(np.float32)
        if signed:
            inc = inc * rng.choice(np.float32([-1.0, 1.0]), inc.shape)
        acc = acc.copy()
        acc[:, :3] = acc[:, :3] + inc
        total += n
        out.append(acc)
        totals.append(total)
    return out, totals


@pytest.mark.parametrize("width,rows,sizes", [(1, 1, (4, 4)), (1, 7, (3, 3, 3)), (9, 1, (1, 2, 5, 11)), (65, 3, (16,) * 5), (65, 3, (7, 1, 16, 2, 30, 4)),
                                              (24, 16, (4,) * 8)])
def test_library_equals_the_restatement_bit_for_bit(width, rows, sizes, native, abi):
    host, _ = native
    rng = np.random.default_rng([width, rows, len(sizes)])
    sums, totals = _random_sums(rng, width, rows, sizes)
    err, s = _same(host, abi, sums, totals, width, rows, threshold=0.05, min_chunks=2)
    assert s["nonfinite"] == 0 and 0 < s["mean_error"] <= s["max_error"] and np.isfinite(err).all()
    # another threshold, floor and allowance over the same sums
    _same(host, abi, sums, totals, width, rows, threshold=1e-3, floor=0.0, min_chunks=3, allowed_above=width * rows // 2)


def test_negative_denormal_and_huge_sums(native, abi):
    host, _ = native
    rng = np.random.default_rng(11)
    W, R = 13, 5
    sums, totals = _random_sums(rng, W, R, (5, 3, 8, 8), signed=True)
    tiny = np.float32(1e-41)                                             # denormal in float32
    for k, a in enumerate(sums):
        a[0:7, :3] = tiny * np.float32(k + 1) * np.arange(1, 8, dtype=np.float32)[:, None]   # denormal running sums: exact in double
        a[7, :3] = 0.0                                                   # a black pixel: err = 0 / floor = 0
        a[8, :3] = np.float32(3e38) * np.float32((k + 1) / 8)            # near FLT_MAX: T*T stays far inside double
        a[9, :3] = -np.float32(k + 1)                                    # a negative mean: the denominator is the floor alone
    err, s = _same(host, abi, sums, totals, W, R, min_chunks=2)
    assert s["nonfinite"] == 0 and err.reshape(-1)[7] == 0.0 and (err.reshape(-1)[:7] > 0).all()
    # floor 0: the black pixel is 0 / 0 -> NaN, counted as non-finite; the negative pixel divides by 0 -> +inf, counted above
    err, s = _same(host, abi, sums, totals, W, R, floor=0.0, min_chunks=2)
    flat = err.reshape(-1)
    assert np.isnan(flat[7]) and s["nonfinite"] == 1 and flat[9] == np.inf and s["max_error"] == np.inf and s["above"] >= 1


def test_a_nonfinite_pixel_changes_no_other_word_and_does_not_block(native, abi):
    host, _ = native
    rng = np.random.default_rng(5)
    W, R = 17, 4
    sums, totals = _random_sums(rng, W, R, (4,) * 6, scale=1e-3)
    clean, s0 = _same(host, abi, sums, totals, W, R, threshold=10.0, min_chunks=2)
    assert s0["converged"] == 1 and s0["nonfinite"] == 0
    poisoned = [a.copy() for a in sums]
    where = {3: np.inf, 20: -np.inf, 41: np.nan}
    for k, a in enumerate(poisoned):
        for p, v in where.items():
            if k >= 2:                                                   # the first chunks are finite: the state turns non-finite on the way
                a[p, 1] = v
        if k >= 4:
            a[50, :3] = [np.inf, -np.inf, 1.0]                           # inf - inf in the luminance
    err, s = _same(host, abi, poisoned, totals, W, R, threshold=10.0, min_chunks=2)
    bad = sorted(list(where) + [50])
    assert s["nonfinite"] == len(bad) and s["above"] == 0 and s["converged"] == 1       # reported, and they do not block convergence
    flat, flat0 = err.reshape(-1), clean.reshape(-1)
    assert np.isnan(flat[bad]).all() and (flat[bad].view(np.uint32) == 0x7FC00000).all()
    keep = np.setdiff1d(np.arange(W * R), bad)
    assert np.array_equal(flat[keep].view(np.uint32), flat0[keep].view(np.uint32))
    assert np.isfinite(s["mean_error"]) and np.isfinite(s["max_error"])   # the statistics are those of the other pixels


def test_reset_two_chunks_and_the_allowance_boundary(native, abi):
    host, _ = native
    rng = np.random.default_rng(3)
    W, R = 8, 6
    sums, totals = _random_sums(rng, W, R, (4, 4, 4))
    st = host.NoiseState(W, R)
    st.update(sums[0], totals[0])
    with pytest.raises(RuntimeError, match="at least 2 chunks"):
        st.evaluate()
    st.update(sums[1], totals[1])
    err2, s2 = st.evaluate(abi.NoiseParams.make(threshold=1e-6, min_chunks=2))       # K = 2: one degree of freedom
    ref = NoiseRef(W, R); ref.update(sums[0], totals[0]); ref.update(sums[1], totals[1])
    want, ws = ref.evaluate(threshold=1e-6, min_chunks=2)
    assert np.array_equal(err2.view(np.uint32), want.view(np.uint32)) and (s2.chunks, s2.samples, s2.pixels) == (2, 8, W * R)
    assert s2.above == ws["above"] > 0 and s2.converged == 0
    # the default min_chunks (4) holds the verdict back however generous the rest is; allowed_above decides at its boundary
    A = int(s2.above)
    for params, verdict in ((abi.NoiseParams.make(threshold=1e-6, min_chunks=2, allowed_above=A), 1),
                            (abi.NoiseParams.make(threshold=1e-6, min_chunks=2, allowed_above=A - 1), 0),
                            (abi.NoiseParams.make(threshold=1e-6, min_chunks=3, allowed_above=A), 0),
                            (abi.NoiseParams.make(threshold=1e30, allowed_above=W * R), 0)):
        _, s = st.evaluate(params, want_map=False)
        assert (s.converged, s.above) == (verdict, A if params.threshold < 1 else 0), (params.min_chunks, params.allowed_above)
    # a null params pointer is {0.02, 0.01, 4, 0, 0}
    st.update(sums[2], totals[2])
    e_null, s_null = st.evaluate(None)
    e_def, s_def = st.evaluate(abi.NoiseParams(*abi.NOISE_DEFAULTS))
    assert abi.NOISE_DEFAULTS == (0.02, 0.01, 4, 0, 0) and bytes(s_null) == bytes(s_def) and np.array_equal(e_null.view(np.uint32), e_def.view(np.uint32))
    assert bytes(abi.NoiseParams.make()) == bytes(abi.NoiseParams(*abi.NOISE_DEFAULTS))
    # reset: the same state fed again gives the same words as a fresh one; a smaller total is accepted again
    st.reset()
    with pytest.raises(RuntimeError, match="at least 2 chunks"):
        st.evaluate()
    st.update(sums[0], totals[0]); st.update(sums[1], totals[1])
    err_again, s_again = st.evaluate(abi.NoiseParams.make(threshold=1e-6, min_chunks=2))
    assert np.array_equal(err_again.view(np.uint32), err2.view(np.uint32)) and bytes(s_again) == bytes(s2)
    st.free()


LAYOUT_C = r"""
#include <stdio.h>
#include "mi355rt.h"
#define F(T, f) printf(#T "." #f " %zu %zu\n", offsetof(T, f), sizeof(((T*)0)->f))
int main(void) {
    printf("sizeof %zu %zu %zu %zu\n", sizeof(mi355rt_noise_params), _Alignof(mi355rt_noise_params), sizeof(mi355rt_noise_summary), _Alignof(mi355rt_noise_summary));
    F(mi355rt_noise_params, threshold); F(mi355rt_noise_params, floor); F(mi355rt_noise_params, min_chunks); F(mi355rt_noise_params, _pad);
    F(mi355rt_noise_params, allowed_above);
    F(mi355rt_noise_summary, chunks); F(mi355rt_noise_summary, samples); F(mi355rt_noise_summary, pixels); F(mi355rt_noise_summary, above);
    F(mi355rt_noise_summary, nonfinite); F(mi355rt_noise_summary, max_error); F(mi355rt_noise_summary, mean_error);
    F(mi355rt_noise_summary, converged); F(mi355rt_noise_summary, _pad);
    printf("abi %u\n", MI355RT_ABI_VERSION);
    return 0;
}
"""


def test_structs_are_laid_out_as_the_c_compiler_lays_out_the_header(tmp_path, abi):
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = subprocess.check_output([str(exe)], text=True).split("\n")
    assert out[0] == "sizeof 32 8 56 8"
    assert (C.sizeof(abi.NoiseParams), C.sizeof(abi.NoiseSummary)) == (32, 56)
    got = {line.split()[0]: tuple(int(v) for v in line.split()[1:]) for line in out[1:] if "." in line}
    want = {}
    for cname, T, fields in (("mi355rt_noise_params", abi.NoiseParams, PARAM_FIELDS), ("mi355rt_noise_summary", abi.NoiseSummary, SUMMARY_FIELDS)):
        assert tuple(n for n, _ in T._fields_) == fields
        for f in fields:
            d = getattr(T, f)
            want[f"{cname}.{f}"] = (d.offset, d.size)
    assert got == want
    assert "abi 5" in out and abi.ABI_VERSION == 5                        # the number did not move


def test_declared_in_the_header_and_exported_by_the_host_library(native, abi):
    from conftest import pkg
    header = open(os.path.join(ROOT, "include", "mi355rt.h")).read()
    so = C.CDLL(pkg("build").HOST_SO)
    for name in NEW:
        assert re.search(r"\b(?:int|void)\s+" + name + r"\s*\(", header), name
        assert hasattr(so, name), name
        assert name in header[header.index("#define MI355RT_ABI_VERSION"):header.index("/* ---- error codes")], name   # named in the version comment
    assert header.index("Host-side helpers") < header.index("int  mi355rt_noise_create")         # the host section
    src = open(os.path.join(ROOT, "raytracer-rust_amd/csrc/host/noise_estimate.cpp")).read()
    assert "hip" not in src.lower()                                                               # pure CPU


def test_every_refusal_names_its_argument(native, abi):
    host, _ = native
    L = host.lib()
    err = lambda: L.mi355rt_host_last_error().decode()
    h = C.c_void_p()
    for args, text in (((4, 4, None), "out is null"), ((0, 4, C.byref(h)), "width is 0"), ((4, 0, C.byref(h)), "rows is 0"),
                       ((1 << 16, 1 << 15, C.byref(h)), "width * rows must be below 2^31"), ((0xFFFFFFFF, 0xFFFFFFFF, C.byref(h)), "width * rows")):
        assert L.mi355rt_noise_create(*args) == abi.ERR_INVALID and text in err(), (args, err())
        assert not h.value
    assert L.mi355rt_noise_reset(None) == abi.ERR_INVALID and "state is null" in err()
    buf = np.zeros(4 * 4 * 4, np.float32)
    assert L.mi355rt_noise_update(None, buf.ctypes.data, 1) == abi.ERR_INVALID and "state is null" in err()
    s = abi.NoiseSummary()
    assert L.mi355rt_noise_evaluate(None, None, None, C.byref(s)) == abi.ERR_INVALID and "state is null" in err()
    L.mi355rt_noise_free(None)                                            # like free(): a null state is fine
    assert L.mi355rt_noise_create(4, 4, C.byref(h)) == 0 and h.value
    assert L.mi355rt_noise_update(h, None, 1) == abi.ERR_INVALID and "accum is null" in err()
    assert L.mi355rt_noise_update(h, buf.ctypes.data, 0) == abi.ERR_INVALID and "samples_total (0) must exceed the 0 samples already seen" in err()
    assert L.mi355rt_noise_update(h, buf.ctypes.data, 4) == 0
    assert L.mi355rt_noise_evaluate(h, None, None, C.byref(s)) == abi.ERR_INVALID and "at least 2 chunks" in err()
    assert L.mi355rt_noise_update(h, buf.ctypes.data, 4) == abi.ERR_INVALID and "samples_total (4) must exceed the 4 samples already seen" in err()
    assert L.mi355rt_noise_update(h, buf.ctypes.data, 3) == abi.ERR_INVALID and "samples_total (3)" in err()
    assert L.mi355rt_noise_update(h, buf.ctypes.data, 9) == 0
    assert L.mi355rt_noise_evaluate(h, None, None, None) == abi.ERR_INVALID and "out_summary is null" in err()
    inf, nan = float("inf"), float("nan")
    for kw, text in ((dict(threshold=0.0), "params.threshold"), (dict(threshold=-1.0), "params.threshold"), (dict(threshold=inf), "params.threshold"),
                     (dict(threshold=nan), "params.threshold"), (dict(floor=-1e-9), "params.floor"), (dict(floor=inf), "params.floor"),
                     (dict(floor=nan), "params.floor"), (dict(min_chunks=1), "params.min_chunks"), (dict(min_chunks=0), "params.min_chunks")):
        p = abi.NoiseParams.make(**kw)
        before = bytes(s)
        assert L.mi355rt_noise_evaluate(h, C.byref(p), None, C.byref(s)) == abi.ERR_INVALID and text in err(), (kw, err())
        assert bytes(s) == before                                        # a refused call writes nothing
    p = abi.NoiseParams.make(); p._pad = 1
    assert L.mi355rt_noise_evaluate(h, C.byref(p), None, C.byref(s)) == abi.ERR_INVALID and "params._pad" in err()
    assert L.mi355rt_noise_evaluate(h, None, None, C.byref(s)) == 0 and (s.chunks, s.samples, s.pixels, s.nonfinite, s._pad) == (2, 9, 16, 0, 0)
    L.mi355rt_noise_free(h)


OOM_CHILD = textwrap.dedent("""
    import ctypes as C, importlib, json, resource, sys
    sys.path.insert(0, sys.argv[1])
    build = importlib.import_module("raytracer-rust_amd.build")
    host = C.CDLL(build.HOST_SO)
    host.mi355rt_host_last_error.restype = C.c_char_p
    host.mi355rt_noise_create.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]
    h = C.c_void_p()
    vm = int([l for l in open("/proc/self/status") if l.startswith("VmSize")][0].split()[1]) * 1024
    resource.setrlimit(resource.RLIMIT_AS, (vm + (24 << 20), vm + (24 << 20)))
    rc = host.mi355rt_noise_create(8192, 8192, C.byref(h))                # 28 bytes a pixel: 1.9 GB
    print(json.dumps([rc, host.mi355rt_host_last_error().decode(), bool(h.value)]))
""")


def test_a_failed_allocation_is_an_error_code(native, tmp_path):
    script = tmp_path / "child.py"
    script.write_text(OOM_CHILD)
    out = subprocess.run([sys.executable, str(script), ROOT], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    rc, text, handle = json.loads(out.stdout.strip().splitlines()[-1])
    assert rc == -4 and "noise_create" in text and "allocation failed" in text and not handle      # MI355RT_ERR_OOM


def test_calibration_on_synthetic_sums(native, abi):
    """4096 grey pixels, K = 8 chunks of n = 4 samples of mean mu and deviation sigma: a chunk's sum is n*mu + sqrt(n)*sigma*z.  se^2 * N
    estimates sigma^2 per pixel with 7 degrees of freedom (relative deviation sqrt(2/7)); the mean over 4096 pixels has the relative
    deviation sqrt(2/7)/64 = 0.8 %, so the 5 % band is six deviations."""
    host, _ = native
    P, K, n, mu, sigma = 4096, 8, 4, 0.4, 0.15
    rng = np.random.default_rng(20240607)
    st, ref = host.NoiseState(64, 64), NoiseRef(64, 64)
    acc = np.zeros((P, 4), np.float64)
    for k in range(1, K + 1):
        acc[:, :3] += (n * mu + np.sqrt(n) * sigma * rng.standard_normal(P))[:, None]       # grey: r = g = b, the weights sum to 1
        st.update(acc.astype(np.float32), k * n)
        ref.update(acc.astype(np.float32), k * n)
    N = K * n
    est = float(np.mean(ref.standard_error() ** 2 * N))
    print(f"mean of se^2 * N = {est:.6f}, sigma^2 = {sigma * sigma:.6f}, ratio {est / sigma ** 2:.4f}")
    assert abs(est / sigma ** 2 - 1.0) < 0.05
    # ... and the library's map is that se over (mu-ish + floor): the same figure recovered from its output
    err, s = st.evaluate(abi.NoiseParams.make(floor=0.0, min_chunks=2))
    m = ref.T / N
    est_lib = float(np.mean((err.reshape(-1).astype(np.float64) * m) ** 2 * N))
    assert abs(est_lib / sigma ** 2 - 1.0) < 0.05 and s.nonfinite == 0


# ---- calibration on real renders: the CPU oracle on an exact scene of bounded radiance -----------------------------------------------------
CAL_W, CAL_H, CAL_CHUNKS, CAL_CHUNK_SPP, CAL_REF_SPP, CAL_DEPTH = 24, 16, 8, 16, 16384, 6
CAL_SEED = 1                                                              # base seeds 1, 2 and 3 were measured before this one was fixed: see the test


def _calibration_scene(tmp_path, host):
    """Lambert quads and cubes under the constant miss colour (0.5 grey), no emitter: every path's radiance lies in [0, 0.5]."""
    bsdfs = [{"name": "floor", "type": "lambert", "albedo": [0.7, 0.7, 0.6]}, {"name": "wall", "type": "lambert", "albedo": [0.3, 0.5, 0.8]},
             {"name": "red", "type": "lambert", "albedo": [0.8, 0.2, 0.2]}, {"name": "white", "type": "lambert", "albedo": 0.9}]
    prims = [{"type": "quad", "bsdf": "floor", "transform": {"position": [0, -1, 0], "scale": [30, 1, 30]}},
             {"type": "quad", "bsdf": "wall", "transform": {"position": [0, 4, -6], "scale": [30, 1, 30], "rotation": [90, 0, 0]}},
             {"type": "cube", "bsdf": "red", "transform": {"position": [-1.2, -0.3, -1.0], "scale": [1.4, 1.4, 1.4], "rotation": [0, 25, 0]}},
             {"type": "cube", "bsdf": "white", "transform": {"position": [1.3, 0.0, -2.0], "scale": [1.2, 2.0, 1.2], "rotation": [0, -20, 0]}},
             {"type": "quad", "bsdf": "red", "transform": {"position": [0.2, 1.6, -1.5], "scale": [2.5, 1, 1.5], "rotation": [20, 0, 10]}}]
    cam = {"transform": {"position": [0, 1.5, 6], "look_at": [0, 0.3, -1], "up": [0, 1, 0]}, "fov": 40, "resolution": [CAL_W, CAL_H]}
    p = tmp_path / "calibration.json"
    p.write_text(json.dumps({"camera": cam, "primitives": prims, "bsdfs": bsdfs, "renderer": {"spp": CAL_CHUNK_SPP}, "integrator": {"max_bounces": CAL_DEPTH}}))
    return host.LoadedScene(str(p))


def _calibration_figure(oracle_mod, abi, sc, base_seed, reference):
    ref = NoiseRef(CAL_W, CAL_H)
    acc = np.zeros((CAL_H * CAL_W, 4), np.float32)
    st = abi.Settings(CAL_W, CAL_H, CAL_CHUNK_SPP, CAL_DEPTH)
    for k in range(CAL_CHUNKS):                                           # independent chunks: another seed each, far apart (the row key is y + seed)
        _, lin, _ = oracle_mod.render(sc, sc.camera, st, abi.Options.make(seed=base_seed * 1000003 + 4096 * (k + 1)))
        acc = acc.copy()
        acc[:, :3] += lin.reshape(-1, 3) * np.float32(CAL_CHUNK_SPP)      # the chunk's sums: mean * 16, exact
        ref.update(acc, (k + 1) * CAL_CHUNK_SPP)
    w = np.float64([0.2126, 0.7152, 0.0722])
    lum_ref = reference.reshape(-1, 3).astype(np.float64) @ w
    mean = ref.T / ref.N
    se = ref.standard_error()
    live = se > 0                                                         # a pixel that sees nothing but the miss colour has no variance at all
    z = (mean[live] - lum_ref[live]) / se[live]
    return float(np.sqrt(np.mean(z * z))), int(live.sum()), ref, acc


def test_calibration_on_oracle_renders(native, oracle_mod, abi, tmp_path):
    """8 independent 16-spp renders of the oracle as chunks, a 16384-spp render as the truth: the RMS over pixels of (mean - truth) / se must
    lie in [0.5, 2.0].  With 7 degrees of freedom the figure is expected near sqrt(7/5) = 1.18; taking n, N or K for one another in the
    formula moves it by a factor of 2.8 or more.  Measured before the seed was fixed: 1.187, 1.181 and 1.220 for base seeds 1, 2 and 3
    (all 384 pixels have variance)."""
    host, _ = native
    sc = _calibration_scene(tmp_path, host)
    _, reference, _ = oracle_mod.render(sc, sc.camera, abi.Settings(CAL_W, CAL_H, CAL_REF_SPP, CAL_DEPTH), abi.Options.make(seed=77777))
    assert np.isfinite(reference).all() and reference.max() <= 0.5 and reference.min() >= 0.0           # bounded radiance
    rms, live, ref, acc = _calibration_figure(oracle_mod, abi, sc, CAL_SEED, reference)
    print(f"RMS of (mean - reference) / se over {live} pixels: {rms:.4f} (base seed {CAL_SEED})")
    assert live >= CAL_W * CAL_H * 3 // 4
    assert 0.5 <= rms <= 2.0
    # the library holds the same state: its map over the same sums is the restatement's
    st = host.NoiseState(CAL_W, CAL_H)
    half = acc.copy(); half[:, :3] *= np.float32(0.5)
    st.update(half, CAL_CHUNKS * CAL_CHUNK_SPP // 2); st.update(acc, CAL_CHUNKS * CAL_CHUNK_SPP)
    r2 = NoiseRef(CAL_W, CAL_H); r2.update(half, CAL_CHUNKS * CAL_CHUNK_SPP // 2); r2.update(acc, CAL_CHUNKS * CAL_CHUNK_SPP)
    assert np.array_equal(st.evaluate(abi.NoiseParams.make(min_chunks=2))[0].view(np.uint32), r2.evaluate(min_chunks=2)[0].view(np.uint32))
