"""The radiance queries (mi355rt_radiance_scratch_bytes, mi355rt_context_trace_radiance, mi355rt_trace_radiance; added within ABI version 5)
without a GPU: the two records are laid out as the C compiler lays out the header's, the numpy dtype is the ctypes struct, the functions are
declared and exported, every refusal that does not need a resident scene is reached before the device, the scratch size is 12 bytes per
(ray, sample) pair rounded up to 16, the knob takes 0 .. 64, and the three k_radiance* kernels are in the built code object within the
register, spill and code-size figures DESIGN.md 4.12 quotes."""
import ctypes as C
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, pkg

sys.path.insert(0, os.path.join(ROOT, "tools"))

NEW = ("mi355rt_radiance_scratch_bytes", "mi355rt_context_trace_radiance", "mi355rt_trace_radiance")
RAY_FIELDS = ("origin", "x", "direction", "row")
PARAM_FIELDS = ("sample_begin", "sample_end", "max_depth", "flags", "seed", "reserved")

LAYOUT_C = r"""
#include <stdio.h>
#include "mi355rt.h"
#define F(T, f) printf(#T "." #f " %zu %zu\n", offsetof(T, f), sizeof(((T*)0)->f))
int main(void) {
    printf("sizeof %zu %zu %zu %zu\n", sizeof(mi355rt_path_ray), _Alignof(mi355rt_path_ray), sizeof(mi355rt_radiance_params), _Alignof(mi355rt_radiance_params));
    F(mi355rt_path_ray, origin); F(mi355rt_path_ray, x); F(mi355rt_path_ray, direction); F(mi355rt_path_ray, row);
    F(mi355rt_radiance_params, sample_begin); F(mi355rt_radiance_params, sample_end); F(mi355rt_radiance_params, max_depth);
    F(mi355rt_radiance_params, flags); F(mi355rt_radiance_params, seed); F(mi355rt_radiance_params, reserved);
    return 0;
}
"""


def test_structs_are_laid_out_as_the_c_compiler_lays_out_the_header(tmp_path, abi):
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = subprocess.check_output([str(exe)], text=True).split("\n")
    assert out[0] == "sizeof 32 4 32 8"
    assert (C.sizeof(abi.PathRay), C.sizeof(abi.RadianceParams)) == (32, 32)
    got = {line.split()[0]: tuple(int(v) for v in line.split()[1:]) for line in out[1:] if "." in line}
    want = {}
    for cname, T, fields in (("mi355rt_path_ray", abi.PathRay, RAY_FIELDS), ("mi355rt_radiance_params", abi.RadianceParams, PARAM_FIELDS)):
        assert tuple(n for n, _ in T._fields_) == fields
        for f in fields:
            d = getattr(T, f)
            want[f"{cname}.{f}"] = (d.offset, d.size)
    assert got == want
    assert abi.PathRay.x.offset == abi.Ray._pad0.offset and abi.PathRay.row.offset == abi.Ray._pad1.offset      # a mi355rt_ray whose pads are read
    p = abi.RadianceParams.make(3, 9, 30, seed=0x1_0000_0005)
    assert (p.sample_begin, p.sample_end, p.max_depth, p.flags, p.seed, p.reserved) == (3, 9, 30, 0, 0x1_0000_0005, 0)


def test_numpy_dtype_is_the_ctypes_struct(abi):
    T, dt = abi.PathRay, abi.PATH_RAY_DTYPE
    assert dt.itemsize == C.sizeof(T) and dt.names == RAY_FIELDS
    for f in RAY_FIELDS:
        sub, off = dt.fields[f][:2]
        d = getattr(T, f)
        assert (off, sub.itemsize) == (d.offset, d.size), f
        assert sub.base == np.dtype("<u4" if f in ("x", "row") else "<f4"), f
    r = abi.PathRay(); r.origin[:] = [1.0, 2.0, 3.0]; r.direction[:] = [0.0, -1.0, 0.0]; r.x, r.row = 7, 0xFFFFFFFE
    a = np.frombuffer(bytes(r), dt)[0]
    assert list(a["origin"]) == [1.0, 2.0, 3.0] and list(a["direction"]) == [0.0, -1.0, 0.0] and (a["x"], a["row"]) == (7, 0xFFFFFFFE)


def test_declared_and_exported_and_the_abi_number_did_not_move(native, abi):
    _, device = native
    header = open(os.path.join(ROOT, "include", "mi355rt.h")).read()
    so = C.CDLL(pkg("build").DEVICE_SO)
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert hasattr(so, name) and name in device.EXPORTS
        assert name in header.split("#define MI355RT_ABI_VERSION")[1].split("*/")[0], name       # the version comment names them
    assert device.lib().mi355rt_abi_version() == abi.ABI_VERSION == 5
    assert callable(device.Context.trace_radiance) and callable(device.trace_radiance) and callable(device.radiance_scratch_bytes)


def test_every_entry_point_of_rt_radiance_sits_behind_the_barrier():
    """The regular expression of tests/test_exception_barrier.py, applied to the three entry points: the two of the resident scene stand in rt_queries.cpp,
    which sees the context struct, and mi355rt_trace_radiance with the other calls with host buffers in rt_oneshot.cpp, on its query scaffold; each is
    defined once and opens with the guard, and no .hip file defines any of them."""
    dev_dir = os.path.join(ROOT, "raytracer-rust_amd/csrc/device")
    src = {n: open(os.path.join(dev_dir, n)).read() for n in sorted(os.listdir(dev_dir)) if n.endswith((".cpp", ".hip"))}
    defs = {n: re.findall(r"\nint (mi355rt_\w+)\((?:[^()]|\([^()]*\))*\) \{\n(.*)\n", text[text.index('extern "C" {'):]) for n, text in src.items() if 'extern "C" {' in text}
    where = {"mi355rt_radiance_scratch_bytes": "rt_queries.cpp", "mi355rt_context_trace_radiance": "rt_queries.cpp", "mi355rt_trace_radiance": "rt_oneshot.cpp"}
    assert set(where) == set(NEW)
    for name, home in where.items():
        assert [n for n, d in defs.items() for f, _ in d if f == name] == [home], name
        assert sum(len(re.findall(r"\nint " + name + r"\(", text)) for text in src.values()) == 1, name
    bare = [f for d in defs.values() for f, first in d if f in NEW and "return guard([&]() -> int {" not in first]
    assert not bare, bare
    for name, text in src.items():                                                              # ... and none of the three is defined in any .hip
        if name.endswith(".hip"):
            assert not re.search(r"\nint (?:" + "|".join(NEW) + r")\(", text), name
    prepare = src["rt_prepare.cpp"]
    assert "int plan_radiance(" in prepare and "hip" not in prepare.split("int plan_radiance(")[1].split("\n}\n")[0].lower()   # the plan holds no HIP call


def test_scratch_bytes(native, abi):
    _, device = native
    L = device.lib()
    for n, s in ((0, 1), (1, 1), (1, 4), (4, 1), (3, 5), (300, 17), (91, 8), (480000, 16), (0xFFFFFFFF, 1), (65536, 65535), (7, 0)):
        assert device.radiance_scratch_bytes(n, s) == (12 * n * s + 15) // 16 * 16, (n, s)
    out = C.c_uint64(77)
    for n, s in ((65536, 65536), (0xFFFFFFFF, 2), (0xFFFFFFFF, 0xFFFFFFFF), (2, 0x80000000)):      # n * samples >= 2^32
        assert L.mi355rt_radiance_scratch_bytes(n, s, C.byref(out)) == abi.ERR_INVALID and b"split the call" in L.mi355rt_last_error(), (n, s)
        assert out.value == 77
    assert L.mi355rt_radiance_scratch_bytes(1, 1, None) == abi.ERR_INVALID and b"out_bytes is null" in L.mi355rt_last_error()


def test_refusals_are_reached_before_the_device(native, abi):
    _, device = native
    L = device.lib()
    buf = (C.c_uint8 * 256)()
    p = (C.addressof(buf) + 15) & ~15
    err = lambda: L.mi355rt_last_error().decode()
    call = L.mi355rt_context_trace_radiance
    ok = abi.RadianceParams.make(0, 4, 8)
    P = C.byref
    # the parameters first, then the pointers (neither needs the context), each with a text that names the argument
    assert call(None, None, p, 1, p, None, p, None) == abi.ERR_INVALID and "params is null" in err()
    bad = [(abi.RadianceParams(0, 4, 8, 1, 0, 0), "params.flags"), (abi.RadianceParams(0, 4, 8, 0, 0, 1), "params.reserved"),
           (abi.RadianceParams(4, 4, 8, 0, 0, 0), "params.sample_begin"), (abi.RadianceParams(5, 4, 8, 0, 0, 0), "params.sample_begin"),
           (abi.RadianceParams(0, 0, 8, 0, 0, 0), "params.sample_begin")]
    for prm, word in bad:
        assert call(None, P(prm), p, 1, p, None, p, None) == abi.ERR_INVALID and word in err(), (word, err())
        assert call(None, P(prm), None, 0, None, None, None, None) == abi.ERR_INVALID and word in err(), (word, err())   # also with nothing to do
    assert call(None, P(ok), None, 1, p, None, p, None) == abi.ERR_INVALID and "d_rays is null" in err()
    assert call(None, P(ok), p, 1, None, None, p, None) == abi.ERR_INVALID and "d_accum is null" in err()
    assert call(None, P(ok), p, 1, p, None, None, None) == abi.ERR_INVALID and "d_scratch is null" in err()
    assert call(None, P(ok), p + 8, 1, p, None, p, None) == abi.ERR_INVALID and "d_rays must be 16-byte aligned" in err()
    assert call(None, P(ok), p, 1, p + 8, None, p, None) == abi.ERR_INVALID and "d_accum must be 16-byte aligned" in err()
    assert call(None, P(ok), p, 1, p, None, p + 4, None) == abi.ERR_INVALID and "d_scratch must be 16-byte aligned" in err()
    assert call(None, P(ok), p, 1, p, p + 2, p, None) == abi.ERR_INVALID and "d_out_linear must be 4-byte aligned" in err()
    big = abi.RadianceParams.make(0, 65536, 8)
    assert call(None, P(big), p, 65536, p, None, p, None) == abi.ERR_INVALID and "split the call" in err()
    big = abi.RadianceParams.make(1, 3, 8)
    assert call(None, P(big), p, 0x80000000, p, None, p, None) == abi.ERR_INVALID and "split the call" in err()
    assert call(None, P(big), p, 0x7FFFFFFF, p, p + 4, p, None) == abi.ERR_INVALID and "ctx is null" in err()    # 2^32 - 2 items pass; a 4-byte aligned mean is fine
    assert call(None, P(ok), p, 1, p, None, p, None) == abi.ERR_INVALID and "ctx is null" in err()
    assert call(None, P(ok), None, 0, None, None, None, None) == abi.ERR_INVALID and "ctx is null" in err()      # n == 0 skips the pointers, not the context
    # the one-shot: argument checks first, then the device (there is no CPU path)
    sc = abi.Scene(); sc.miss_color[:] = [0.5] * 3
    one = L.mi355rt_trace_radiance
    assert one(None, P(ok), p, 1, p, None) == abi.ERR_INVALID and "scene is null" in err()
    assert one(P(sc), None, p, 1, p, None) == abi.ERR_INVALID and "params is null" in err()
    for prm, word in bad:
        assert one(P(sc), P(prm), p, 1, p, None) == abi.ERR_INVALID and word in err(), (word, err())
    assert one(P(sc), P(ok), None, 1, p, None) == abi.ERR_INVALID and "rays is null" in err()
    assert one(P(sc), P(ok), p, 1, None, None) == abi.ERR_INVALID and "accum_in_out is null" in err()
    assert one(P(sc), P(ok), None, 0, None, None) == abi.OK
    h = C.c_void_p()
    if L.mi355rt_context_create(0, C.byref(h)) == 0:                   # a GPU is visible here: a context that never saw a scene
        try:
            assert call(h, P(ok), p, 1, p, None, p, None) == abi.ERR_INVALID and "no scene" in err()
            assert call(h, P(ok), None, 0, None, None, None, None) == abi.ERR_INVALID and "no scene" in err()
        finally:
            L.mi355rt_context_destroy(h)
        return
    assert one(P(sc), P(ok), p, 1, p, None) == abi.ERR_NO_DEVICE and "no CPU path" in err()
    with pytest.raises(device.RenderError) as e:
        device.trace_radiance(sc, np.zeros(2, abi.PATH_RAY_DTYPE), ok)
    assert e.value.rc == abi.ERR_NO_DEVICE


def test_the_items_knob_takes_0_to_64(native, abi):
    _, device = native
    L = device.lib()
    try:
        for v in (0, 1, 2, 4, 16, 63, 64):
            device.set_knob("radiance_items", v)
        for v in (-1, 65, 128, -64):
            assert L.mi355rt_debug_set_knob(None, b"radiance_items", v) == abi.ERR_INVALID and b"radiance_items" in L.mi355rt_last_error(), v
    finally:
        device.clear_knobs()


# kernel: (VGPRs allowed, spilled VGPRs, spilled SGPRs, private-segment bytes, code bytes, scratch_ instructions in the ISA).  DESIGN.md 4.12 quotes the
# measured build: 105 / 104 / 12 VGPRs, nothing spilled, no scratch, 18.6 / 22.0 / 0.8 KB.  Budgets in the style of tests/test_ray_query_abi.py, VGPRs
# rounded up to the next occupancy step: the path kernels stay at 128 or fewer (4 waves per SIMD: every material and the sky lookup are compiled in),
# the sum at 64 or fewer (8); nothing spills in either form.
RADIANCE_BUDGET = {
    "k_radiance_paths": (128, 0, 0, 0, 24 * 1024, 0),
    "k_radiance_paths_mesh": (128, 0, 0, 0, 28 * 1024, 0),
    "k_radiance_sum": (64, 0, 0, 0, 2 * 1024, 0),
}


def test_radiance_kernels_are_built_and_stay_inside_their_budgets(native):
    isa_stats = importlib.import_module("isa_stats")
    build = pkg("build")
    raw = isa_stats.kernel_stats(build.DEVICE_SO)
    stats = {isa_stats.short(k): v for k, v in raw.items()}
    assert {k for k in stats if k.startswith("k_radiance")} == set(RADIANCE_BUDGET)
    assert "k_render_ctr_simple_qc" in stats and "k_resolve" in stats and "k_query_rays" in stats   # the tool reads every code object of the library
    isa = {isa_stats.short(k): v for k, v in isa_stats.kernel_isa(build.DEVICE_SO).items()}
    for name, (vgprs, vspill, sspill, private, code, scratch) in RADIANCE_BUDGET.items():
        st = stats[name]
        assert st["vgpr_count"] <= vgprs, (name, st)
        assert st["vgpr_spill_count"] <= vspill and st["sgpr_spill_count"] <= sspill, (name, st)
        assert st["private_segment_fixed_size"] <= private and st.get("scratch_insts", 0) <= scratch, (name, st)
        assert st["code_bytes"] <= code, (name, st)
        assert st["group_segment_fixed_size"] == 0, (name, st)                                  # no LDS: nothing is shared between the paths
        ops = [i.split()[0] for i in isa[name]]
        stores = [o for o in ops if "store" in o]
        assert stores and all(o.startswith("global_store_dword") for o in stores), (name, sorted(set(stores)))   # vector stores to global memory, nothing else
        assert not [o for o in ops if "atomic" in o or o.startswith(("ds_", "s_barrier", "s_sleep"))], name
    stores = lambda name: [i.split()[0] for i in isa[name] if "store" in i.split()[0]]
    assert set(stores("k_radiance_paths")) == set(stores("k_radiance_paths_mesh")) == {"global_store_dwordx3"}  # a path's radiance leaves as one 12-byte store
    assert sorted(stores("k_radiance_sum")) == ["global_store_dwordx3", "global_store_dwordx4"]               # the float4 sum and the mean
    dpp = [i for i in isa["k_radiance_sum"] if "row_shr:1" in i]
    assert len(dpp) >= 45, len(dpp)                                                             # k_resolve's chain: 15 steps on three channels
    srcs = [os.path.basename(s) for s in build.DEVICE_SRCS]
    assert srcs.count("rt_radiance.hip") == 1 and os.path.join(build.CSRC, "device", "rt_radiance.h") in build.DEVICE_HEADERS   # kernel_hash() covers both
