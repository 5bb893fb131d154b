"""The surface probes (mi355rt_context_probe_rays, mi355rt_context_probe_radiance; added within ABI version 5) without a GPU: the numpy ray maker of
tests/probe_cases.py against the definition's edges, its distribution and the oracle's own Lambert bounce, the struct as the C compiler lays it out,
the exports, every refusal with its text reached before the device, the barrier in front of rt_probe.hip's entry points, and the register, LDS and
spill figures of the new kernels read off the built code object."""
import ctypes as C
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import probe_cases as PC
import radiance_cases as RC
from conftest import ROOT, load_for_both, pkg

sys.path.insert(0, os.path.join(ROOT, "tools"))

F = np.float32
NEW = ("mi355rt_context_probe_rays", "mi355rt_context_probe_radiance")
PROBE_FIELDS = ("position", "x", "normal", "row")


@pytest.fixture(scope="module")
def scenes(native, oracle_mod):
    host, _ = native
    return {n: load_for_both(n, oracle_mod, host, width=PC.W, height=PC.H, spp=1, max_depth=PC.DEPTH) for n in PC.SCENES}


@pytest.fixture(scope="module")
def sets(scenes, oracle_mod, abi):
    return {n: PC.probe_set(oracle_mod, abi, n, scenes[n]) for n in PC.SCENES}


# ---- the maker ------------------------------------------------------------------------------------------------------------------------------
def test_the_case_sets_hold_what_the_tests_need(sets, abi):
    for name, probes in sets.items():
        n_hits = len(probes) - 42
        assert probes.dtype == abi.PROBE_DTYPE and n_hits >= 100, (name, n_hits)            # first hits, 40 free-space probes, two odd normals
        lens = np.sqrt((probes["normal"].astype(np.float64) ** 2).sum(axis=1))
        assert np.abs(lens[:-2] - 1.0).max() < 1e-6 and lens[-2] == 2.0 and lens[-1] == 0.0
        assert (probes["row"][:n_hits] < PC.H).all() and (probes["x"][:n_hits] < PC.W).all()
        assert (probes["row"][n_hits:n_hits + 40] > 0xFFFF).all()                            # scattered 32-bit addresses
        for n in PC.counts(len(probes)):
            for S in PC.SAMPLES:
                assert (n * S) % 64 != 0 and n <= len(probes), (name, n, S)                  # the last wave of every call is a partial one
    assert all(len(p) - 42 < PC.W * PC.H for p in sets.values())                            # both views have misses: they are dropped


def test_rejected_tries_run_and_the_cap_is_far_away(sets, oracle_mod, abi):
    """A try is rejected with probability 1 - pi / 6 = 0.476.  The case set must hold probes whose first accepted try is 4 or later, so that rejected
    tries run on the device; 64 rejections in a row have probability 2e-21, so the fallback is not among the cases (the test below drives it)."""
    worst = 0
    for name, probes in sets.items():
        for seed in PC.SEEDS:
            for s in range(max(PC.SAMPLES)):
                rays, p, tried, nz = PC.probe_rays(oracle_mod, abi, probes, s, seed, want=True)
                assert ((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2] < F(1.0)).all() and p.dtype == F
                assert not nz.any()                                                          # only a cancelling normal reaches near_zero (the zero normal: d = normalized(p))
                worst = max(worst, int(tried.max()))
    print(f"largest first-accepted try over all case inputs: {worst} (cap {PC.TRIES})")
    assert 4 <= worst < PC.TRIES


def test_the_fallback_after_64_rejected_tries_gives_the_normal(sets, oracle_mod, abi):
    probes = sets["cornell"][-50:]
    n = len(probes)
    calls = []

    def corner(j, rows):                                                                    # p = (1 - 2^-22) * (1, 1, 1): outside the ball, every try
        calls.append((j, len(rows)))
        w = np.zeros((len(rows), 4), np.uint32); w[:, 1:] = 0xFFFFFFFF
        return w

    rays, p, tried, nz = PC.probe_rays(oracle_mod, abi, probes, 0, 0, block_source=corner, want=True)
    assert calls == [(j, n) for j in range(PC.TRIES)] and (tried == PC.TRIES).all()
    assert (p.view(np.uint32) == 0).all()                                                   # p = (0, 0, 0) ...
    assert rays["direction"].tobytes() == RC.normalized_rows(probes["normal"] + F(0.0)).tobytes()   # ... so d = N + 0 (a -0 of N becomes +0), normalised once
    assert (rays["direction"] == RC.normalized_rows(probes["normal"])).all()
    assert rays["origin"].tobytes() == (probes["position"] + probes["normal"] * F(1e-4)).astype(F).tobytes()
    assert rays["direction"][-2].tolist() == [0.0, 1.0, 0.0] and rays["direction"][-1].tolist() == [0.0, 0.0, 0.0]   # the length-2 normal, the zero normal
    assert nz.tolist() == [False] * (n - 1) + [True]                                        # 0 + 0: near_zero, d = N = 0

    def late(j, rows):                                                                      # accepted on the last try the cap allows
        w = corner(j, rows)
        if j == PC.TRIES - 1:
            w[:, 1:] = 0xC0000000                                                           # p = (0.5, 0.5, 0.5)
        return w

    _, p, tried, _ = PC.probe_rays(oracle_mod, abi, probes, 0, 0, block_source=late, want=True)
    assert (tried == PC.TRIES - 1).all() and (p == F(0.5)).all()
    p, tried = PC.ball_points(3, lambda j, rows: np.array([[9, 0x80000000, 0x80000000, 0x80000000], [9, 0xFFFFFFFF, 0x80000000, 0x80000000],
                                                           [9, 0, 0x80000000, 0x80000000]], np.uint32)[rows], tries=2)
    assert list(tried) == [0, 0, 2] and p[0].tolist() == [0, 0, 0] and p[1, 0] == F(1.0) - F(2.0 ** -22)   # |p| = 1 - 2^-22 is inside, p.x = -1 is not; word 0 is not read


def test_a_cancelling_normal_reaches_near_zero_and_leaves_along_the_normal(sets, oracle_mod, abi):
    base = sets["cornell"][:37]
    for seed in PC.SEEDS:
        probes = PC.cancelling_probes(oracle_mod, abi, base, seed)
        rays, p, tried, nz = PC.probe_rays(oracle_mod, abi, probes, 0, seed, want=True)
        assert nz.all()                                                                     # N + normalized(p) is exactly zero
        assert rays["direction"].tobytes() == RC.normalized_rows(probes["normal"]).tobytes()
        assert not PC.probe_rays(oracle_mod, abi, probes, 1, seed, want=True)[3].any()      # another sample, another p


def test_the_directions_are_cosine_weighted(oracle_mod, abi):
    """64 addresses x 256 samples about N = (0, 1, 0).  The share of directions inside the cone of half-angle asin(0.5) about N is the cosine-weighted
    form factor of the cone's cap, sin^2 = 0.25; a uniform hemisphere would give 1 - cos = 0.134.  A binomial share of 16384 draws has
    sigma = sqrt(0.25 * 0.75 / 16384) = 0.00338: accepted within 6 sigma = 0.0203."""
    rng = np.random.default_rng(3)
    probes = np.zeros(64, abi.PROBE_DTYPE)
    probes["normal"] = [0.0, 1.0, 0.0]
    probes["x"] = rng.integers(0, 1 << 32, 64, dtype=np.uint64).astype(np.uint32)
    probes["row"] = rng.integers(0, 1 << 32, 64, dtype=np.uint64).astype(np.uint32)
    d = np.concatenate([PC.probe_rays(oracle_mod, abi, probes, s, 0)["direction"] for s in range(256)]).astype(np.float64)
    assert d.shape == (16384, 3)
    cos = d[:, 1]
    assert (cos >= 0).all()                                                                 # every direction on the normal's side
    assert np.abs(np.sqrt((d * d).sum(axis=1)) - 1.0).max() < 1e-6
    share = float((cos > np.sqrt(0.75)).mean())                                             # inside the cone: cos(theta) > cos(asin(0.5))
    tol = 6.0 * np.sqrt(0.1875 / 16384)
    print(f"share inside the cone: {share:.4f} (cosine-weighted 0.25, uniform 0.134, tolerance {tol:.4f})")
    assert abs(share - 0.25) <= tol
    assert abs(float(cos.mean()) - 2.0 / 3.0) <= 6.0 * np.sqrt((0.5 - 4.0 / 9.0) / 16384)    # E[cos] = 2/3, Var = 1/2 - 4/9


def test_the_oracles_white_lambert_bounce_addressed_at_ray_0_is_the_probe_ray(sets, oracle_mod, abi):
    """oracle.scatter_ctr_batch takes the ray an event draws from as a record word, so `ray = 0` expresses the probe's addressing: a white
    LAMBERT_SOLID at (P, N) scatters into the maker's ray -- its origin, and its direction after one more normalisation (Ray::new)."""
    mats = (abi.Material * 1)()
    mats[0].kind = abi.MAT_LAMBERT_SOLID
    mats[0].albedo[:] = [1.0, 1.0, 1.0]
    for name, probes in sets.items():
        for seed, s in ((PC.SEEDS[0], 0), (PC.SEEDS[1], 16)):
            rays = PC.probe_rays(oracle_mod, abi, probes, s, seed)
            rec = np.zeros((len(probes), 16), np.uint32)
            rec[:, 1] = 1
            rec[:, 2:5] = np.array([0.0, -1.0, 0.0], F).view(np.uint32)
            rec[:, 5:8], rec[:, 8:11] = probes["position"].view(np.uint32), probes["normal"].view(np.uint32)
            ykey = (probes["row"].astype(np.uint64) + np.uint64(seed))
            rec[:, 11], rec[:, 12], rec[:, 13], rec[:, 14], rec[:, 15] = ykey & np.uint64(0xFFFFFFFF), ykey >> np.uint64(32), probes["x"], s, 0
            f = oracle_mod.scatter_ctr_batch(mats, rec).view(F)
            assert (f[:, 0] == 1).all() and (f[:, 7:10] == 1).all()
            assert f[:, 1:4].tobytes() == rays["origin"].tobytes(), (name, seed, s)
            assert f[:, 4:7].tobytes() == RC.normalized_rows(rays["direction"]).tobytes(), (name, seed, s)


def test_probes_from_hits_drops_the_misses_and_addresses_by_pixel(abi):
    hits = np.zeros(12, abi.HIT_DTYPE)
    hits["primitive"] = [0, abi.NO_HIT, 3, 3, abi.NO_HIT, 1, 0, 0, abi.NO_HIT, abi.NO_HIT, 2, 7]
    hits["position"] = np.arange(36, dtype=F).reshape(12, 3)
    hits["normal"] = -np.arange(36, dtype=F).reshape(12, 3)
    got = abi.probes_from_hits(hits, 5)
    keep = [0, 2, 3, 5, 6, 7, 10, 11]
    assert got.dtype == abi.PROBE_DTYPE and got.dtype.itemsize == 32 and len(got) == 8
    assert got["x"].tolist() == [i % 5 for i in keep] and got["row"].tolist() == [i // 5 for i in keep]
    assert got["position"].tobytes() == hits["position"][keep].tobytes() and got["normal"].tobytes() == hits["normal"][keep].tobytes()
    assert len(abi.probes_from_hits(hits.reshape(3, 4), 4)) == 8
    with pytest.raises(ValueError):
        abi.probes_from_hits(np.zeros(4, abi.RAY_DTYPE), 2)
    with pytest.raises(ValueError):
        abi.probes_from_hits(hits, 0)


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------------
LAYOUT_C = r"""
#include <stdio.h>
#include "mi355rt.h"
#define F(T, f) printf(#T "." #f " %zu %zu\n", offsetof(T, f), sizeof(((T*)0)->f))
int main(void) {
    printf("sizeof %zu %zu %zu\n", sizeof(mi355rt_probe), _Alignof(mi355rt_probe), sizeof(mi355rt_path_ray));
    F(mi355rt_probe, position); F(mi355rt_probe, x); F(mi355rt_probe, normal); F(mi355rt_probe, row);
    F(mi355rt_path_ray, origin); F(mi355rt_path_ray, x); F(mi355rt_path_ray, direction); F(mi355rt_path_ray, row);
    return 0;
}
"""


def test_the_probe_is_laid_out_as_the_c_compiler_lays_out_the_header_and_as_a_path_ray(tmp_path, abi):
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = subprocess.check_output([str(exe)], text=True).split("\n")
    assert out[0] == "sizeof 32 4 32" and C.sizeof(abi.Probe) == 32 == abi.PROBE_DTYPE.itemsize
    got = {line.split()[0]: tuple(int(v) for v in line.split()[1:]) for line in out[1:] if "." in line}
    assert tuple(n for n, _ in abi.Probe._fields_) == PROBE_FIELDS == abi.PROBE_DTYPE.names
    want = {f"mi355rt_probe.{f}": (getattr(abi.Probe, f).offset, getattr(abi.Probe, f).size) for f in PROBE_FIELDS}
    assert {k: v for k, v in got.items() if k.startswith("mi355rt_probe.")} == want
    assert [abi.PROBE_DTYPE.fields[f][1] for f in PROBE_FIELDS] == [want[f"mi355rt_probe.{f}"][0] for f in PROBE_FIELDS] == [0, 12, 16, 28]
    for pf, rf in zip(PROBE_FIELDS, ("origin", "x", "direction", "row")):
        assert got[f"mi355rt_probe.{pf}"] == got[f"mi355rt_path_ray.{rf}"]


def test_declared_and_exported_and_the_abi_number_did_not_move(native, abi):
    _, device = native
    header = open(os.path.join(ROOT, "include", "mi355rt.h")).read()
    so = C.CDLL(pkg("build").DEVICE_SO)
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert hasattr(so, name) and name in device.EXPORTS
        assert name in header.split("#define MI355RT_ABI_VERSION")[1].split("*/")[0], name       # the version comment names them
    assert device.lib().mi355rt_abi_version() == abi.ABI_VERSION == 5
    assert callable(device.Context.probe_rays) and callable(device.Context.probe_radiance) and callable(abi.probes_from_hits)
    assert "irradiance is pi" in header and "library does not multiply" in header


def test_every_entry_point_of_rt_probe_sits_behind_the_barrier():
    """The regular expression of tests/test_exception_barrier.py, applied to the two entry points: they stand in rt_queries.cpp, which sees the context
    struct, each defined once and opening with the guard, and no .hip file defines either."""
    dev_dir = os.path.join(ROOT, "raytracer-rust_amd/csrc/device")
    src = {n: open(os.path.join(dev_dir, n)).read() for n in sorted(os.listdir(dev_dir)) if n.endswith((".cpp", ".hip"))}
    text = src["rt_queries.cpp"]
    defs = [(n, first) for n, first in re.findall(r"\nint (mi355rt_\w+)\((?:[^()]|\([^()]*\))*\) \{\n(.*)\n", text[text.index('extern "C" {'):]) if n in NEW]
    assert sorted(n for n, _ in defs) == sorted(NEW) and len(defs) == 2
    bare = [n for n, first in defs if "return guard([&]() -> int {" not in first]
    assert not bare, bare
    for name, other in src.items():                                                             # ... defined there only, and in no .hip
        if name != "rt_queries.cpp":
            assert not re.search(r"\nint (?:" + "|".join(NEW) + r")\(", other), name
    prepare = src["rt_prepare.cpp"]
    for plan in ("int plan_probe(", "int plan_probe_rays("):
        assert plan in prepare and "hip" not in prepare.split(plan)[1].split("\n}\n")[0].lower()   # the plans hold no HIP call
    assert "#include <hip" not in prepare


def test_refusals_are_reached_before_the_device(native, abi):
    _, device = native
    L = device.lib()
    buf = (C.c_uint8 * 256)()
    p = (C.addressof(buf) + 15) & ~15
    err = lambda: L.mi355rt_last_error().decode()
    rays, rad = L.mi355rt_context_probe_rays, L.mi355rt_context_probe_radiance
    P = C.byref
    ok = abi.RadianceParams.make(0, 4, 8)
    # probe_rays: its two buffers, then the context
    assert rays(None, None, 1, 0, 0, p, None) == abi.ERR_INVALID and err() == "probe_rays: d_probes is null"
    assert rays(None, p, 1, 0, 0, None, None) == abi.ERR_INVALID and err() == "probe_rays: d_rays is null"
    assert rays(None, p + 8, 1, 0, 0, p, None) == abi.ERR_INVALID and err() == "probe_rays: d_probes must be 16-byte aligned"
    assert rays(None, p, 1, 0, 0, p + 4, None) == abi.ERR_INVALID and err() == "probe_rays: d_rays must be 16-byte aligned"
    assert rays(None, p, 0xFFFFFFFF, 0xFFFFFFFF, 2 ** 64 - 1, p, None) == abi.ERR_INVALID and err() == "probe_rays: ctx is null"   # any n, sample and seed
    assert rays(None, None, 0, 0, 0, None, None) == abi.ERR_INVALID and err() == "probe_rays: ctx is null"                       # n == 0: the pointers are not looked at
    # probe_radiance: plan_radiance's refusals, in its order, under the call's own name, d_probes in the place of d_rays
    assert rad(None, None, p, 1, p, None, p, None) == abi.ERR_INVALID and err() == "probe_radiance: params is null"
    bad = [(abi.RadianceParams(0, 4, 8, 1, 0, 0), "params.flags must be 0"), (abi.RadianceParams(0, 4, 8, 0, 0, 1), "params.reserved must be 0"),
           (abi.RadianceParams(4, 4, 8, 0, 0, 0), "params.sample_begin must be below params.sample_end"),
           (abi.RadianceParams(5, 4, 8, 0, 0, 0), "params.sample_begin must be below params.sample_end"),
           (abi.RadianceParams(0, 0, 8, 0, 0, 0), "params.sample_begin must be below params.sample_end")]
    for prm, text in bad:
        assert rad(None, P(prm), p, 1, p, None, p, None) == abi.ERR_INVALID and err() == "probe_radiance: " + text, (text, err())
        assert rad(None, P(prm), None, 0, None, None, None, None) == abi.ERR_INVALID and err() == "probe_radiance: " + text       # ... with n == 0 as well
    q = L.mi355rt_context_trace_radiance
    for args, text in (((None, 1, p, None, p), "{} is null"), ((p, 1, None, None, p), "d_accum is null"), ((p, 1, p, None, None), "d_scratch is null"),
                       ((p + 8, 1, p, None, p), "{} must be 16-byte aligned"), ((p, 1, p + 8, None, p), "d_accum must be 16-byte aligned"),
                       ((p, 1, p, None, p + 4), "d_scratch must be 16-byte aligned"), ((p, 1, p, p + 2, p), "d_out_linear must be 4-byte aligned"),
                       ((p, 1, p, p + 4, p), "ctx is null"), ((None, 0, None, None, None), "ctx is null")):
        assert rad(None, P(ok), *args, None) == abi.ERR_INVALID and err() == "probe_radiance: " + text.format("d_probes"), (text, err())
        assert q(None, P(ok), *args, None) == abi.ERR_INVALID and err() == "trace_radiance: " + text.format("d_rays"), (text, err())   # the query's own texts did not move
    big = abi.RadianceParams.make(0, 65536, 8)
    assert rad(None, P(big), p, 65536, p, None, p, None) == abi.ERR_INVALID and err() == "probe_radiance: n * samples must stay below 2^32 (split the call)"
    assert rad(None, P(big), p, 65535, p, None, p, None) == abi.ERR_INVALID and err() == "probe_radiance: ctx is null"           # 2^32 - 65536 items pass
    h = C.c_void_p()
    if L.mi355rt_context_create(0, C.byref(h)) == 0:                   # a GPU is visible here: a context that never saw a scene
        try:
            assert rays(h, p, 1, 0, 0, p, None) == abi.ERR_INVALID and "no scene" in err()
            assert rad(h, P(ok), p, 1, p, None, p, None) == abi.ERR_INVALID and "no scene" in err()
        finally:
            L.mi355rt_context_destroy(h)


# ---- the code object ---------------------------------------------------------------------------------------------------------------------
# kernel: (VGPRs allowed, code bytes).  Every new kernel: no spilled register of either kind, no private segment, no scratch instruction, no LDS.  The path
# kernels stay at 128 VGPRs or fewer (4 waves per SIMD, as k_radiance_paths: every material and the sky lookup are compiled in), the ray maker and the
# sum at 64 or fewer (8).  Code sizes: k_radiance_paths[_mesh]'s budgets plus 4 KB for the maker in the refill, as for the views.
PROBE_BUDGET = {"k_probe_paths": (128, 28 * 1024), "k_probe_paths_mesh": (128, 32 * 1024), "k_probe_rays": (64, 4 * 1024), "k_probe_sum": (64, 2 * 1024)}


def test_probe_kernels_are_built_and_stay_inside_their_budgets(native):
    isa_stats = importlib.import_module("isa_stats")
    build = pkg("build")
    stats = {isa_stats.short(k): v for k, v in isa_stats.kernel_stats(build.DEVICE_SO).items()}
    assert {k for k in stats if k.startswith("k_probe")} == set(PROBE_BUDGET)
    isa = {isa_stats.short(k): v for k, v in isa_stats.kernel_isa(build.DEVICE_SO).items()}
    for name, (vgprs, code) in PROBE_BUDGET.items():
        st = stats[name]
        print(name, st)
        assert st["vgpr_count"] <= vgprs, (name, st)
        assert st["vgpr_spill_count"] == 0 and st["sgpr_spill_count"] == 0, (name, st)
        assert st["private_segment_fixed_size"] == 0 and st.get("scratch_insts", 0) == 0, (name, st)
        assert st["group_segment_fixed_size"] == 0, (name, st)                                  # no LDS
        assert st["code_bytes"] <= code, (name, st)
        ops = [i.split()[0] for i in isa[name]]
        stores = [o for o in ops if "store" in o]
        assert stores and all(o.startswith("global_store_dword") for o in stores), (name, sorted(set(stores)))   # vector stores to global memory, nothing else
        assert not [o for o in ops if "atomic" in o or o.startswith(("ds_", "s_barrier", "s_sleep", "v_writelane", "v_readlane"))], name
    stores = lambda name: sorted(i.split()[0] for i in isa[name] if "store" in i.split()[0])
    loads = lambda name: sorted(i.split()[0] for i in isa[name] if i.startswith("global_load"))
    assert set(stores("k_probe_paths")) == set(stores("k_probe_paths_mesh")) == {"global_store_dwordx3"}     # a path's radiance leaves as one 12-byte store
    assert stores("k_probe_rays") == ["global_store_dwordx4"] * 2                                # the two float4 of a mi355rt_path_ray
    assert loads("k_probe_rays") == ["global_load_dwordx4"] * 2                                  # the two float4 of a mi355rt_probe
    for mesh in ("", "_mesh"):                                                                   # a probe is read as a ray is: the query's loads, no more
        assert loads("k_probe_paths" + mesh) == loads("k_radiance_paths" + mesh), mesh
    # the sum is the query's, instantiated again: instruction for instruction
    assert isa["k_probe_sum"] == isa["k_radiance_sum"]
    # the maker has no transcendental stage: + - * / sqrt and compares only (the path kernels carry the materials' and the sky lookup's, as the query's do)
    assert not [i for i in isa["k_probe_rays"] if i.split()[0].startswith(("v_sin", "v_cos", "v_exp", "v_log"))]
    srcs = [os.path.basename(s) for s in build.DEVICE_SRCS]
    assert srcs.count("rt_probe.hip") == 1                                                      # kernel_hash() covers the source and its header
    assert os.path.join(build.CSRC, "device", "rt_probe.h") in build.DEVICE_HEADERS
    assert srcs.index("rt_probe.hip") < srcs.index("rt_api.cpp") and srcs[0] == "rt_kernels.hip"   # (the reference build replaces the first source)
