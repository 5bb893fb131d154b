"""The noise estimate on the device (mi355rt_noise_device_*; added within ABI version 5) without a GPU: the five functions are declared at the
end of the header, named in the version comment and exported, every refusal that does not need a created object is reached before the
device, the entry points of rt_noise.hip sit behind the exception barrier, the k_noise_* kernels are in the built code object within the
figures DESIGN.md 4.11 quotes, and the reduction tree of mean_error (noise_device_ref.py) agrees with the host's sum in pixel order within the
header's bound."""
import ctypes as C
import importlib
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT, pkg
from noise_device_ref import TILE, mean_error, tree_sum

sys.path.insert(0, os.path.join(ROOT, "tools"))

NEW = ("mi355rt_noise_device_create", "mi355rt_noise_device_destroy", "mi355rt_noise_device_reset", "mi355rt_noise_device_update",
       "mi355rt_noise_device_evaluate")
# The pixel counts of tests/test_gpu_noise_device.py: around a wave, around the tile, 33 x 17, and more tiles than k_noise_finish has threads.
PIXEL_COUNTS = (1, 63, 64, 65, 255, 256, 257, 33 * 17, 257 * TILE, 258 * TILE + 1)


def test_declared_last_and_exported_and_the_abi_number_did_not_move(native, abi):
    _, device = native
    header = open(os.path.join(ROOT, "include", "mi355rt.h")).read()
    so = C.CDLL(pkg("build").DEVICE_SO)
    after = header.index("mi355rt_host_last_error(void);")
    for name in NEW:
        m = re.search(r"\b(?:int|void)\s+" + name + r"\s*\(", header)
        assert m and m.start() > after, name                                                     # a new section at the end: nothing existing moved
        assert hasattr(so, name) and name in device.EXPORTS
        assert name in header.split("#define MI355RT_ABI_VERSION")[1].split("*/")[0], name       # the version comment names them
    assert device.lib().mi355rt_abi_version() == abi.ABI_VERSION == 5
    assert "#define MI355RT_ABI_VERSION 5u" in header
    for name in ("update", "evaluate", "reset", "free"):
        assert callable(getattr(device.NoiseDevice, name))


def test_refusals_are_reached_before_the_device(native, abi):
    _, device = native
    L = device.lib()
    buf = (C.c_uint8 * 256)()
    p = (C.addressof(buf) + 15) & ~15
    err = lambda: L.mi355rt_last_error().decode()
    create, reset, update, evaluate = L.mi355rt_noise_device_create, L.mi355rt_noise_device_reset, L.mi355rt_noise_device_update, L.mi355rt_noise_device_evaluate
    h = C.c_void_p(0x1234)
    assert create(0, 4, 4, None) == abi.ERR_INVALID and err() == "noise_device_create: out is null"
    for w, r, text in ((0, 4, "width is 0"), (4, 0, "rows is 0"), (1 << 16, 1 << 15, "width * rows must be below 2^31"), (0xFFFFFFFF, 0xFFFFFFFF, "below 2^31")):
        h.value = 0x1234
        assert create(0, w, r, C.byref(h)) == abi.ERR_INVALID and err().startswith("noise_device_create: ") and text in err(), (w, r, err())
        assert h.value is None                                                                   # *out is null after a refusal
    assert reset(None, None) == abi.ERR_INVALID and err() == "noise_device_reset: state is null"
    # update: the pointer first (it does not need the object), then the object
    assert update(None, None, 1, None) == abi.ERR_INVALID and err() == "noise_device_update: d_accum is null"
    for off in (4, 8, 12):
        assert update(None, p + off, 1, None) == abi.ERR_INVALID and err() == "noise_device_update: d_accum must be 16-byte aligned"
    assert update(None, p, 1, None) == abi.ERR_INVALID and err() == "noise_device_update: state is null"
    # evaluate: pointers, then the parameters, then the object
    assert evaluate(None, None, None, None, None) == abi.ERR_INVALID and err() == "noise_device_evaluate: d_out_summary is null"
    assert evaluate(None, None, None, p + 4, None) == abi.ERR_INVALID and err() == "noise_device_evaluate: d_out_summary must be 8-byte aligned"
    assert evaluate(None, None, p + 2, p + 8, None) == abi.ERR_INVALID and err() == "noise_device_evaluate: d_out_error must be 4-byte aligned"
    bad = [(abi.NoiseParams(0.0, 0.01, 4, 0, 0), "threshold"), (abi.NoiseParams(-1.0, 0.01, 4, 0, 0), "threshold"), (abi.NoiseParams(float("nan"), 0.01, 4, 0, 0), "threshold"),
           (abi.NoiseParams(float("inf"), 0.01, 4, 0, 0), "threshold"), (abi.NoiseParams(0.02, -1e-300, 4, 0, 0), "floor"), (abi.NoiseParams(0.02, float("nan"), 4, 0, 0), "floor"),
           (abi.NoiseParams(0.02, float("inf"), 4, 0, 0), "floor"), (abi.NoiseParams(0.02, 0.01, 1, 0, 0), "min_chunks"), (abi.NoiseParams(0.02, 0.01, 0, 0, 0), "min_chunks"),
           (abi.NoiseParams(0.02, 0.01, 4, 1, 0), "_pad")]
    for prm, word in bad:
        assert evaluate(None, C.byref(prm), p + 4, p + 8, None) == abi.ERR_INVALID and err().startswith("noise_device_evaluate: params." + word), (word, err())
    for prm in (None, abi.NoiseParams.make(), abi.NoiseParams(5e-324, 0.0, 2, 0, 1 << 40)):     # the defaults and the extremes pass
        assert evaluate(None, C.byref(prm) if prm is not None else None, p + 4, p + 8, None) == abi.ERR_INVALID and err() == "noise_device_evaluate: state is null"
    L.mi355rt_noise_device_destroy(None)                                                          # a null object is not an error
    # the texts mirror the host's, with the prefix noise_device_
    host_src = open(os.path.join(ROOT, "raytracer-rust_amd/csrc/host/noise_estimate.cpp")).read()
    dev_src = open(os.path.join(ROOT, "raytracer-rust_amd/csrc/device/rt_noise.hip")).read()
    for text in re.findall(r'refuse\("noise_(\w+: [^"]+)"\)', host_src):
        want = "noise_device_" + text.replace("accum is null", "d_accum is null").replace("out_summary is null", "d_out_summary is null").replace("mi355rt_noise_update", "mi355rt_noise_device_update")
        assert '"' + want + '"' in dev_src, want


def test_without_a_gpu_create_says_so(native, abi):
    _, device = native
    L = device.lib()
    h = C.c_void_p()
    rc = L.mi355rt_noise_device_create(0, 8, 8, C.byref(h))
    if rc == abi.OK:                                                  # a GPU is visible here: the object works, tests/test_gpu_noise_device.py has the rest
        L.mi355rt_noise_device_destroy(h)
        return
    assert rc == abi.ERR_NO_DEVICE and "no HIP device" in L.mi355rt_last_error().decode() and h.value is None
    with pytest.raises(device.RenderError) as e:
        device.NoiseDevice(8, 8)
    assert e.value.rc == abi.ERR_NO_DEVICE


def test_every_entry_point_of_rt_noise_sits_behind_the_barrier():
    """The regular expression of tests/test_exception_barrier.py, applied to rt_noise.hip: the entry points live beside their kernels."""
    text = open(os.path.join(ROOT, "raytracer-rust_amd/csrc/device/rt_noise.hip")).read()
    assert len(re.findall(r"\nint mi355rt_\w+\(", text)) == 4
    defs = re.findall(r"\nint (mi355rt_\w+)\((?:[^()]|\([^()]*\))*\) \{\n(.*)\n", text[text.index('extern "C" {'):])
    assert {n for n, _ in defs} == set(NEW) - {"mi355rt_noise_device_destroy"} and len(defs) == 4
    bare = [n for n, first in defs if "return guard([&]() -> int {" not in first]
    assert not bare, bare
    assert re.search(r"\nvoid mi355rt_noise_device_destroy\(", text)
    # ... and no entry point of the device library moved into the files the barrier test counts
    dev_dir = os.path.join(ROOT, "raytracer-rust_amd/csrc/device")
    for name in ("rt_api.cpp", "rt_queries.cpp", "rt_debug.cpp", "rt_multi.cpp", "rt_oneshot.cpp", "rt_prepare.cpp"):
        assert "mi355rt_noise_device" not in open(os.path.join(dev_dir, name)).read(), name


# kernel: (VGPRs allowed, code bytes allowed, LDS bytes).  DESIGN.md 4.11 quotes the measured build: 24 / 28 / 27 VGPRs and 372 / 2120 / 1776 bytes for
# k_noise_update / _evaluate / _finish; the budgets are those rounded up to the next 8 VGPRs and the next KB.  The LDS of the two reducing
# kernels is the four waves' records: 4 x (two doubles + two 64-bit counts).
NOISE_BUDGET = {"k_noise_update": (24, 1024, 0), "k_noise_evaluate": (32, 3 * 1024, 128), "k_noise_finish": (32, 2 * 1024, 128)}


def test_noise_kernels_are_built_and_stay_inside_their_budgets(native):
    isa_stats = importlib.import_module("isa_stats")
    build = pkg("build")
    raw = isa_stats.kernel_stats(build.DEVICE_SO)
    stats = {isa_stats.short(k): v for k, v in raw.items()}
    assert {k for k in stats if k.startswith("k_noise_")} == set(NOISE_BUDGET)
    assert "k_render_ctr_simple_qc" in stats and "k_denoise_last" in stats                      # the tool reads every code object of the library
    for name, (vgprs, code, lds) in NOISE_BUDGET.items():
        st = stats[name]
        assert st["vgpr_count"] <= vgprs, (name, st)
        assert st["vgpr_spill_count"] == 0 and st["sgpr_spill_count"] == 0, (name, st)
        assert st["private_segment_fixed_size"] == 0 and st.get("scratch_insts", 0) == 0, (name, st)
        assert st["code_bytes"] <= code, (name, st)
        assert st["group_segment_fixed_size"] == lds, (name, st)
    isa = {isa_stats.short(k): v for k, v in isa_stats.kernel_isa(build.DEVICE_SO).items()}
    for name in NOISE_BUDGET:
        ops = [i.split()[0] for i in isa[name]]
        assert not [o for o in ops if "atomic" in o or o.startswith("scratch_")], name            # no atomics of any kind, no scratch
        assert not [o for o in ops if o.startswith(("v_fma_f32", "v_fmac_f32", "v_pk_"))], name


def test_build_lists_cover_the_new_unit():
    build = pkg("build")
    srcs = [os.path.basename(s) for s in build.DEVICE_SRCS]
    assert srcs.count("rt_noise.hip") == 1 and os.path.join(build.CSRC, "device", "rt_noise.h") in build.DEVICE_HEADERS   # kernel_hash() covers both


def test_the_tree_is_the_headers_and_agrees_with_the_sum_in_pixel_order():
    """mean_error: the sequential sum errs by at most gamma_(n-1), the tree by gamma_depth with depth <= 16 + n_tiles / 256, relative to the sum
    itself because every term is >= 0 -- together below (pixels + 64) * 2^-53."""
    # the tree on inputs whose every partial sum is exact is the plain sum, and the order is the header's: powers of two placed so that a
    # different pairing would lose them
    assert tree_sum(np.arange(1, 1001, dtype=np.float64)) == 500500.0
    v = np.zeros(2 * TILE); v[0] = 1.0; v[32] = 2.0 ** -53; v[1] = 2.0 ** -53               # lane 0 meets lane 32 first: 1 + 2^-53 rounds to 1 (ties to even)
    assert tree_sum(v) == 1.0                                                                    # ... and then (1) + lane 16 ..., lane 1 comes last: 1 + 2^-53 = 1
    v = np.zeros(2 * TILE); v[1] = 2.0 ** -53; v[33] = 2.0 ** -53; v[0] = 1.0                # lanes 1 and 33 meet first: 2^-52 survives the later meeting with lane 0
    assert tree_sum(v) == 1.0 + 2.0 ** -52
    v = np.zeros(300 * TILE); v[0] = 1.0; v[TILE] = 2.0 ** -53; v[256 * TILE] = 2.0 ** -53  # tiles 0 and 256 are 256 apart: they meet before tile 1 does
    assert tree_sum(v) == 1.0
    v = np.zeros(300 * TILE); v[TILE] = 2.0 ** -53; v[257 * TILE] = 2.0 ** -53; v[0] = 1.0  # tiles 1 and 257 meet first
    assert tree_sum(v) == 1.0 + 2.0 ** -52
    rng = np.random.default_rng(11)
    for n in PIXEL_COUNTS:
        for scale in (1.0, 1e-300, 1e150):
            e = rng.random(n) ** 8 * scale
            e[rng.random(n) < 0.05] = np.nan
            good = e[~np.isnan(e)]
            seq = float(np.cumsum(good)[-1] / np.float64(good.size)) if good.size else 0.0
            got = mean_error(e)
            assert abs(got - seq) <= (n + 64) * 2.0 ** -53 * seq, (n, scale, got, seq)
    assert mean_error(np.full(70, np.nan)) == 0.0
    assert mean_error(np.array([np.inf, 1.0, np.nan])) == np.inf
