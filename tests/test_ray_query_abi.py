"""The ray queries (mi355rt_context_trace_rays, mi355rt_context_first_hits, mi355rt_trace_rays; added within ABI version 5) without a GPU:
the two records are laid out as the C compiler lays out the header's, the numpy dtypes are the ctypes structs, the functions are declared and
exported, the context calls check their arguments before they look for a device, and the k_query_* kernels are in the built code object
within the register, spill and scratch figures DESIGN.md 4.6 quotes."""
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

NEW = ("mi355rt_context_trace_rays", "mi355rt_context_first_hits", "mi355rt_trace_rays")
RAY_FIELDS = ("origin", "_pad0", "direction", "_pad1")
HIT_FIELDS = ("position", "t", "normal", "front_face", "primitive", "material", "_pad")

LAYOUT_C = r"""
#include <stdio.h>
#include "mi355rt.h"
#define F(T, f) printf(#T "." #f " %zu %zu\n", offsetof(T, f), sizeof(((T*)0)->f))
int main(void) {
    printf("sizeof %zu %zu %zu %zu\n", sizeof(mi355rt_ray), _Alignof(mi355rt_ray), sizeof(mi355rt_hit), _Alignof(mi355rt_hit));
    F(mi355rt_ray, origin); F(mi355rt_ray, _pad0); F(mi355rt_ray, direction); F(mi355rt_ray, _pad1);
    F(mi355rt_hit, position); F(mi355rt_hit, t); F(mi355rt_hit, normal); F(mi355rt_hit, front_face);
    F(mi355rt_hit, primitive); F(mi355rt_hit, material); F(mi355rt_hit, _pad);
    printf("no_hit %u\n", MI355RT_NO_HIT);
    return 0;
}
"""


def test_records_are_laid_out_as_the_c_compiler_lays_out_the_header(tmp_path, abi):
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = subprocess.check_output([str(exe)], text=True).split("\n")
    assert out[0] == "sizeof 32 4 48 4"
    assert (C.sizeof(abi.Ray), C.sizeof(abi.Hit)) == (32, 48)
    got = {line.split()[0]: tuple(int(v) for v in line.split()[1:]) for line in out[1:] if "." in line}
    want = {}
    for cname, T, fields in (("mi355rt_ray", abi.Ray, RAY_FIELDS), ("mi355rt_hit", abi.Hit, HIT_FIELDS)):
        assert tuple(n for n, _ in T._fields_) == fields
        for f in fields:
            d = getattr(T, f)
            want[f"{cname}.{f}"] = (d.offset, d.size)
    assert got == want
    assert "no_hit 4294967295" in out and abi.NO_HIT == 0xFFFFFFFF


def test_numpy_dtypes_are_the_ctypes_structs(abi):
    for T, dt, fields in ((abi.Ray, abi.RAY_DTYPE, RAY_FIELDS), (abi.Hit, abi.HIT_DTYPE, HIT_FIELDS)):
        assert dt.itemsize == C.sizeof(T) and dt.names == fields
        for f in fields:
            sub, off = dt.fields[f][:2]
            d = getattr(T, f)
            assert (off, sub.itemsize) == (d.offset, d.size), f
            assert sub.base == (np.dtype("<f4") if dict(T._fields_)[f] in (C.c_float, C.c_float * 3) else np.dtype("<u4")), f
    # a record written through ctypes reads back through numpy
    h = abi.Hit(); h.position[:] = [1.0, 2.0, 3.0]; h.t = 4.0; h.normal[:] = [0.0, -1.0, 0.0]; h.front_face = 1; h.primitive = 7; h.material = 9
    a = np.frombuffer(bytes(h), abi.HIT_DTYPE)[0]
    assert list(a["position"]) == [1.0, 2.0, 3.0] and a["t"] == 4.0 and list(a["normal"]) == [0.0, -1.0, 0.0]
    assert (a["front_face"], a["primitive"], a["material"], list(a["_pad"])) == (1, 7, 9, [0, 0])


def test_declared_and_exported_and_the_abi_number_did_not_move(native, abi):
    _, device = native
    header = open(os.path.join(ROOT, "include", "mi355rt.h")).read()
    so = C.CDLL(pkg("build").DEVICE_SO)
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert hasattr(so, name) and name in device.EXPORTS
    assert device.lib().mi355rt_abi_version() == abi.ABI_VERSION == 5
    assert not re.search(r"mi355rt_debug_", re.sub(r"/\*.*?\*/", "", header, flags=re.S))       # the test hooks stay out of the public header


def test_context_calls_check_their_arguments_before_the_device(native, abi):
    _, device = native
    L = device.lib()
    buf = (C.c_uint8 * 256)()
    p = C.addressof(buf)
    assert L.mi355rt_context_trace_rays(None, p, 1, p, None) == abi.ERR_INVALID
    assert b"no scene" in L.mi355rt_last_error()
    assert L.mi355rt_context_trace_rays(None, None, 0, None, None) == abi.ERR_INVALID
    assert L.mi355rt_context_first_hits(None, None, p, None) == abi.ERR_INVALID
    assert b"no scene" in L.mi355rt_last_error()
    opt = abi.Options.make()
    assert L.mi355rt_context_first_hits(None, C.byref(opt), None, None) == abi.ERR_INVALID
    # the one-shot: argument checks first, then the device (there is no CPU path)
    sc = abi.Scene(); sc.miss_color[:] = [0.5] * 3
    assert L.mi355rt_trace_rays(None, p, 1, p) == abi.ERR_INVALID and b"scene is null" in L.mi355rt_last_error()
    assert L.mi355rt_trace_rays(C.byref(sc), None, 1, p) == abi.ERR_INVALID
    assert L.mi355rt_trace_rays(C.byref(sc), p, 1, None) == abi.ERR_INVALID
    assert L.mi355rt_trace_rays(C.byref(sc), None, 0, None) == abi.OK
    h = C.c_void_p()
    if L.mi355rt_context_create(0, C.byref(h)) == 0:
        L.mi355rt_context_destroy(h)
        return                                                          # a GPU is visible here: the rest is what its absence looks like
    assert L.mi355rt_trace_rays(C.byref(sc), p, 1, p) == abi.ERR_NO_DEVICE
    assert b"no CPU path" in L.mi355rt_last_error()
    with pytest.raises(device.RenderError) as e:
        device.trace_rays(sc, np.zeros(2, abi.RAY_DTYPE))
    assert e.value.rc == abi.ERR_NO_DEVICE


# kernel: (VGPRs allowed, spilled VGPRs, spilled SGPRs, private-segment bytes, code bytes, scratch_ instructions in the ISA).  DESIGN.md 4.6 quotes the
# measured build: 31 / 60 / 31 / 57 VGPRs, nothing spilled, no scratch, 4.3 / 7.7 / 4.9 / 8.4 KB.  Budgets in the style of tests/test_isa_budget.py: the
# mesh-free forms must not spill at all; every form stays at 64 VGPRs or fewer (8 waves per SIMD).
QUERY_BUDGET = {
    "k_query_rays": (40, 0, 0, 0, 6 * 1024, 0),
    "k_query_pixels": (40, 0, 0, 0, 6 * 1024, 0),
    "k_query_rays_mesh": (64, 0, 0, 0, 10 * 1024, 0),
    "k_query_pixels_mesh": (64, 0, 0, 0, 10 * 1024, 0),
}


def test_query_kernels_are_built_and_stay_inside_their_budgets(native):
    isa_stats = importlib.import_module("isa_stats")
    build = pkg("build")
    raw = isa_stats.kernel_stats(build.DEVICE_SO)
    stats = {isa_stats.short(k): v for k, v in raw.items()}
    queries = {k for k in stats if k.startswith("k_query")}
    assert queries == set(QUERY_BUDGET), queries
    assert not [k for k in raw if "k_query" in k and "k_render_ctr" in k]
    assert "k_render_ctr_simple_qc" in stats and "k_resolve" in stats                 # the tool reads every code object of the library, not only the queries'
    for name, (vgprs, vspill, sspill, private, code, scratch) in QUERY_BUDGET.items():
        st = stats[name]
        assert st["vgpr_count"] <= vgprs, (name, st)
        assert st["vgpr_spill_count"] <= vspill and st["sgpr_spill_count"] <= sspill, (name, st)
        assert st["private_segment_fixed_size"] <= private, (name, st)
        assert st["code_bytes"] <= code, (name, st)
        assert st.get("scratch_insts", 0) <= scratch, (name, st)
        assert st["group_segment_fixed_size"] == 0, (name, st)                      # no LDS: nothing is shared between the rays
    # a record leaves as three 16-byte vector stores per lane, and nothing else is stored
    isa = {isa_stats.short(k): v for k, v in isa_stats.kernel_isa(build.DEVICE_SO).items()}
    for name in QUERY_BUDGET:
        stores = [i.split()[0] for i in isa[name] if i.split()[0].startswith(("global_store", "flat_store"))]
        assert stores == ["global_store_dwordx4"] * 3, (name, stores)
        assert not [i for i in isa[name] if "atomic" in i.split()[0] or i.split()[0].startswith("ds_")], name
    assert build.DEVICE_SRCS.count(os.path.join(build.CSRC, "device", "rt_query.hip")) == 1    # kernel_hash() covers the new translation unit
