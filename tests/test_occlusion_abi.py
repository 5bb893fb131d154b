"""The occlusion queries (mi355rt_context_occluded, mi355rt_occluded, mi355rt_context_ambient_occlusion; added within ABI version 5) without a
GPU: the two structs are laid out as the C compiler lays out the header's, the numpy dtype is the ctypes struct, the functions are declared
and exported, every refusal that does not need a resident scene is reached before the device, and the k_occluded* / k_ao_* kernels are in the
built code object within the register, code-size and LDS figures DESIGN.md 4.8 quotes."""
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

NEW = ("mi355rt_context_occluded", "mi355rt_occluded", "mi355rt_context_ambient_occlusion")
SEGMENT_FIELDS = ("origin", "_pad0", "direction", "t_max")
AO_FIELDS = ("samples", "seed", "radius", "_pad")

LAYOUT_C = r"""
#include <stdio.h>
#include "mi355rt.h"
#define F(T, f) printf(#T "." #f " %zu %zu\n", offsetof(T, f), sizeof(((T*)0)->f))
int main(void) {
    printf("sizeof %zu %zu %zu %zu %zu\n", sizeof(mi355rt_segment), _Alignof(mi355rt_segment), sizeof(mi355rt_ao_params), _Alignof(mi355rt_ao_params), sizeof(mi355rt_ray));
    F(mi355rt_segment, origin); F(mi355rt_segment, _pad0); F(mi355rt_segment, direction); F(mi355rt_segment, t_max);
    F(mi355rt_ao_params, samples); F(mi355rt_ao_params, seed); F(mi355rt_ao_params, radius); F(mi355rt_ao_params, _pad);
    printf("ray_pad1 %zu\n", offsetof(mi355rt_ray, _pad1));
    return 0;
}
"""


def test_structs_are_laid_out_as_the_c_compiler_lays_out_the_header(tmp_path, abi):
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = subprocess.check_output([str(exe)], text=True).split("\n")
    assert out[0] == "sizeof 32 4 16 4 32"
    assert (C.sizeof(abi.Segment), C.sizeof(abi.AoParams)) == (32, 16)
    got = {line.split()[0]: tuple(int(v) for v in line.split()[1:]) for line in out[1:] if "." in line}
    want = {}
    for cname, T, fields in (("mi355rt_segment", abi.Segment, SEGMENT_FIELDS), ("mi355rt_ao_params", abi.AoParams, AO_FIELDS)):
        assert tuple(n for n, _ in T._fields_) == fields
        for f in fields:
            d = getattr(T, f)
            want[f"{cname}.{f}"] = (d.offset, d.size)
    assert got == want
    assert "ray_pad1 28" in out and abi.Segment.t_max.offset == 28 == abi.Ray._pad1.offset     # the layout of mi355rt_ray with the last pad read
    p = abi.AoParams.make()
    assert (p.samples, p.seed, p.radius, p._pad) == (16, 0, float("inf"), 0)                    # what a null pointer means


def test_numpy_dtype_is_the_ctypes_struct(abi):
    T, dt = abi.Segment, abi.SEGMENT_DTYPE
    assert dt.itemsize == C.sizeof(T) and dt.names == SEGMENT_FIELDS
    for f in SEGMENT_FIELDS:
        sub, off = dt.fields[f][:2]
        d = getattr(T, f)
        assert (off, sub.itemsize) == (d.offset, d.size) and sub.base == np.dtype("<f4"), f
    s = abi.Segment(); s.origin[:] = [1.0, 2.0, 3.0]; s.direction[:] = [0.0, -1.0, 0.0]; s.t_max = 4.5
    a = np.frombuffer(bytes(s), dt)[0]
    assert list(a["origin"]) == [1.0, 2.0, 3.0] and list(a["direction"]) == [0.0, -1.0, 0.0] and a["t_max"] == 4.5
    r = np.zeros(1, abi.RAY_DTYPE); r["origin"], r["direction"], r["_pad1"] = [1, 2, 3], [0, -1, 0], 4.5
    assert r.tobytes() == bytes(s)


def test_declared_and_exported_and_the_abi_number_did_not_move(native, abi):
    _, device = native
    header = open(os.path.join(ROOT, "include", "mi355rt.h")).read()
    so = C.CDLL(pkg("build").DEVICE_SO)
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert hasattr(so, name) and name in device.EXPORTS
        assert name in header.split("#define MI355RT_ABI_VERSION")[1].split("*/")[0], name       # the version comment names them
    assert device.lib().mi355rt_abi_version() == abi.ABI_VERSION == 5
    for name in ("occluded", "ambient_occlusion"):
        assert callable(getattr(device.Context, name))
    assert callable(device.occluded)


def test_refusals_are_reached_before_the_device(native, abi):
    _, device = native
    L = device.lib()
    buf = (C.c_uint8 * 256)()
    p = (C.addressof(buf) + 15) & ~15
    err = lambda: L.mi355rt_last_error().decode()
    occ = L.mi355rt_context_occluded
    # pointers first (they do not need the context), each with a text that names the argument
    assert occ(None, None, 1, p, None) == abi.ERR_INVALID and "d_segments is null" in err()
    assert occ(None, p, 1, None, None) == abi.ERR_INVALID and "d_out_u32 is null" in err()
    assert occ(None, p + 8, 1, p, None) == abi.ERR_INVALID and "d_segments must be 16-byte aligned" in err()
    assert occ(None, p, 1, p + 2, None) == abi.ERR_INVALID and "d_out_u32 must be 4-byte aligned" in err()
    assert occ(None, p, 1, p + 4, None) == abi.ERR_INVALID and "ctx is null" in err()             # a 4-byte aligned output is fine
    assert occ(None, None, 0, None, None) == abi.ERR_INVALID and "ctx is null" in err()           # n == 0 skips the pointers, not the context
    ao = L.mi355rt_context_ambient_occlusion
    bad_params = [(abi.AoParams(0, 0, 1.0, 0), "samples"), (abi.AoParams(3, 0, 1.0, 0), "samples"), (abi.AoParams(512, 0, 1.0, 0), "samples"),
                  (abi.AoParams(48, 0, 1.0, 0), "samples"), (abi.AoParams(16, 0, float("nan"), 0), "radius"), (abi.AoParams(16, 0, 0.0, 0), "radius"),
                  (abi.AoParams(16, 0, -1.0, 0), "radius"), (abi.AoParams(16, 0, float("-inf"), 0), "radius"), (abi.AoParams(16, 0, 1.0, 1), "_pad")]
    for prm, word in bad_params:
        assert ao(None, None, C.byref(prm), p, p, None) == abi.ERR_INVALID and ("params." + word) in err(), (word, err())
    for s in (1, 2, 4, 8, 16, 32, 64, 128, 256):
        for radius in (1e-30, 0.25, float("inf")):
            prm = abi.AoParams(s, 7, radius, 0)
            assert ao(None, None, C.byref(prm), p, p, None) == abi.ERR_INVALID and "ctx is null" in err(), (s, radius, err())
    assert ao(None, None, None, p, p, None) == abi.ERR_INVALID and "ctx is null" in err()         # null params: the defaults pass
    opt = abi.Options.make()
    opt.abi_version = 3
    assert ao(None, C.byref(opt), None, p, p, None) == abi.ERR_INVALID and "abi_version" in err()
    opt = abi.Options.make(flags=2)
    assert ao(None, C.byref(opt), None, p, p, None) == abi.ERR_INVALID and "flags" in err()
    opt = abi.Options.make(flags=abi.FLAG_FIXED_AABB)
    assert ao(None, C.byref(opt), None, p, p, None) == abi.ERR_INVALID and "ctx is null" in err()  # UNSUPPORTED is decided with the scene's rows, behind the context
    # the one-shot: argument checks first, then the device (there is no CPU path)
    sc = abi.Scene(); sc.miss_color[:] = [0.5] * 3
    one = L.mi355rt_occluded
    assert one(None, p, 1, p) == abi.ERR_INVALID and "scene is null" in err()
    assert one(C.byref(sc), None, 1, p) == abi.ERR_INVALID and "segments is null" in err()
    assert one(C.byref(sc), p, 1, None) == abi.ERR_INVALID and "out is null" in err()
    assert one(C.byref(sc), None, 0, None) == abi.OK
    h = C.c_void_p()
    if L.mi355rt_context_create(0, C.byref(h)) == 0:                   # a GPU is visible here: a context that never saw a scene
        try:
            assert occ(h, p, 1, p, None) == abi.ERR_INVALID and "no scene" in err()
            assert occ(h, None, 0, None, None) == abi.ERR_INVALID and "no scene" in err()
            assert ao(h, None, None, p, p, None) == abi.ERR_INVALID and "no scene" in err()
        finally:
            L.mi355rt_context_destroy(h)
        return
    assert one(C.byref(sc), p, 1, p) == abi.ERR_NO_DEVICE
    with pytest.raises(device.RenderError) as e:
        device.occluded(sc, np.zeros(2, abi.SEGMENT_DTYPE))
    assert e.value.rc == abi.ERR_NO_DEVICE


# kernel: (VGPRs allowed, code bytes).  DESIGN.md 4.8 quotes the measured build: 28 / 50 VGPRs and 3.2 / 4.8 KB for k_occluded / _mesh,
# 50 / 63 and 4.8 / 6.4 KB for k_ao_spread / _mesh, 46 / 60 and 4.6 / 6.3 KB for k_ao_lane / _mesh.  Budgets in the style of tests/test_ray_query_abi.py:
# every form stays at 64 VGPRs or fewer (8 waves per SIMD), the mesh-free forms well below; nothing spills, no private segment, no LDS.
OCCLUSION_BUDGET = {
    "k_occluded": (40, 5 * 1024), "k_occluded_mesh": (64, 7 * 1024),
    "k_ao_spread": (56, 7 * 1024), "k_ao_spread_mesh": (64, 9 * 1024),
    "k_ao_lane": (56, 7 * 1024), "k_ao_lane_mesh": (64, 9 * 1024),
}


def test_occlusion_kernels_are_built_and_stay_inside_their_budgets(native):
    isa_stats = importlib.import_module("isa_stats")
    build = pkg("build")
    raw = isa_stats.kernel_stats(build.DEVICE_SO)
    stats = {isa_stats.short(k): v for k, v in raw.items()}
    assert {k for k in stats if k.startswith(("k_occluded", "k_ao_"))} == set(OCCLUSION_BUDGET)
    assert "k_render_ctr_simple_qc" in stats and "k_query_rays" in stats                       # the tool reads every code object of the library
    isa = {isa_stats.short(k): v for k, v in isa_stats.kernel_isa(build.DEVICE_SO).items()}
    for name, (vgprs, code) in OCCLUSION_BUDGET.items():
        st = stats[name]
        assert st["vgpr_count"] <= vgprs, (name, st)
        assert st["vgpr_spill_count"] == 0 and st["sgpr_spill_count"] == 0, (name, st)
        assert st["private_segment_fixed_size"] == 0 and st.get("scratch_insts", 0) == 0, (name, st)
        assert st["code_bytes"] <= code, (name, st)
        assert st["group_segment_fixed_size"] == 0, (name, st)                                  # no LDS: whole pixels stay inside a wave
        ops = [i.split()[0] for i in isa[name]]
        stores = [o for o in ops if o.startswith(("global_store", "flat_store"))]
        assert stores == ["global_store_dword"], (name, stores)                                 # one 4-byte vector store per lane, nothing else
        assert not [o for o in ops if "atomic" in o or o.startswith(("ds_", "s_barrier", "s_sleep"))], name
    srcs = [os.path.basename(s) for s in build.DEVICE_SRCS]
    assert srcs.count("rt_occlusion.hip") == 1 and os.path.join(build.CSRC, "device", "rt_occlusion.h") in build.DEVICE_HEADERS   # kernel_hash() covers both
