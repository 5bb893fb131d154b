"""The denoiser (mi355rt_denoise_scratch_bytes, mi355rt_context_denoise, mi355rt_denoise; added within ABI version 5) without a GPU: the
parameter struct is laid out as the C compiler lays out the header's, the functions are declared and exported, the defaults are the header's,
every refusal of the header is decided before a device is looked for (and before the context is touched), the scratch size is monotone, and
the k_denoise* kernels are in the built code object within the register, spill and scratch figures DESIGN.md 4.7 quotes."""
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

NEW = ("mi355rt_denoise_scratch_bytes", "mi355rt_context_denoise", "mi355rt_denoise")
FIELDS = ("levels", "normal_squarings", "sigma_color", "sigma_plane")

LAYOUT_C = r"""
#include <stdio.h>
#include "mi355rt.h"
#define F(T, f) printf(#T "." #f " %zu %zu\n", offsetof(T, f), sizeof(((T*)0)->f))
int main(void) {
    printf("sizeof %zu %zu\n", sizeof(mi355rt_denoise_params), _Alignof(mi355rt_denoise_params));
    F(mi355rt_denoise_params, levels); F(mi355rt_denoise_params, normal_squarings); F(mi355rt_denoise_params, sigma_color); F(mi355rt_denoise_params, sigma_plane);
    return 0;
}
"""


def test_params_are_laid_out_as_the_c_compiler_lays_out_the_header(tmp_path, abi):
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = subprocess.check_output([str(exe)], text=True).split("\n")
    assert out[0] == "sizeof 16 4" and C.sizeof(abi.DenoiseParams) == 16
    assert tuple(n for n, _ in abi.DenoiseParams._fields_) == FIELDS
    got = {line.split()[0]: tuple(int(v) for v in line.split()[1:]) for line in out[1:] if "." in line}
    assert got == {f"mi355rt_denoise_params.{f}": (getattr(abi.DenoiseParams, f).offset, getattr(abi.DenoiseParams, f).size) for f in FIELDS}


def test_declared_and_exported_and_the_abi_number_did_not_move(native, abi):
    _, device = native
    header = open(os.path.join(ROOT, "include", "mi355rt.h")).read()
    so = C.CDLL(pkg("build").DEVICE_SO)
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert hasattr(so, name) and name in device.EXPORTS
    assert device.lib().mi355rt_abi_version() == abi.ABI_VERSION == 5
    assert hasattr(device.Context, "denoise") and callable(device.denoise) and callable(device.denoise_scratch_bytes)


def test_defaults_are_the_headers(abi):
    header = open(os.path.join(ROOT, "include", "mi355rt.h")).read()
    assert "params_or_null == NULL: {5, 5, 2.0f, 0.05f}" in header
    p = abi.DenoiseParams.make()
    assert (p.levels, p.normal_squarings, p.sigma_color, p.sigma_plane) == (5, 5, 2.0, np.float32(0.05)) and abi.DENOISE_DEFAULTS == (5, 5, 2.0, 0.05)
    prepare = open(os.path.join(ROOT, "raytracer-rust_amd", "csrc", "device", "rt_prepare.cpp")).read()
    assert "defaults = {5u, 5u, 2.0f, 0.05f}" in prepare


def test_every_refusal_comes_before_the_device_and_names_its_argument(native, abi):
    _, device = native
    L = device.lib()
    buf = (C.c_uint8 * 4096)()
    base = (C.addressof(buf) + 63) & ~63
    ctx = base + 2048             # never read: every refusal below is decided from the arguments alone
    a, h, s, ol, op = base, base + 256, base + 512, base + 768, base + 1024
    ok = abi.DenoiseParams.make()

    def call(c=ctx, w=4, r=4, p=ok, i=a, hits=h, scratch=s, lin=ol, packed=op):
        return L.mi355rt_context_denoise(c, w, r, C.byref(p) if p is not None else None, i, hits, scratch, lin, packed, None)

    refusals = [
        (dict(c=None), b"ctx"), (dict(i=None), b"d_linear_in"), (dict(hits=None), b"d_hits"), (dict(scratch=None), b"d_scratch"),
        (dict(lin=None, packed=None), b"both null"),
        (dict(hits=h + 8), b"d_hits must be 16-byte"), (dict(scratch=s + 4), b"d_scratch must be 16-byte"), (dict(i=a + 2), b"d_linear_in must be 4-byte"),
        (dict(lin=ol + 1), b"d_out_linear must be 4-byte"), (dict(packed=op + 2), b"d_out_packed must be 4-byte"),
        (dict(w=0), b"width"), (dict(r=0), b"rows"), (dict(w=1 << 16, r=1 << 15), b"2^31"), (dict(w=(1 << 31) - 1, r=2), b"2^31"),
        (dict(p=abi.DenoiseParams.make(levels=9)), b"levels"), (dict(p=abi.DenoiseParams.make(normal_squarings=9)), b"normal_squarings"),
        (dict(p=abi.DenoiseParams.make(sigma_color=0.0)), b"sigma_color"), (dict(p=abi.DenoiseParams.make(sigma_color=-1.0)), b"sigma_color"),
        (dict(p=abi.DenoiseParams.make(sigma_color=float("nan"))), b"sigma_color"), (dict(p=abi.DenoiseParams.make(sigma_color=float("inf"))), b"sigma_color"),
        (dict(p=abi.DenoiseParams.make(sigma_plane=0.0)), b"sigma_plane"), (dict(p=abi.DenoiseParams.make(sigma_plane=float("nan"))), b"sigma_plane"),
        (dict(p=abi.DenoiseParams.make(sigma_plane=float("inf"))), b"sigma_plane"), (dict(p=abi.DenoiseParams.make(sigma_plane=-0.5)), b"sigma_plane"),
    ]
    for kw, word in refusals:
        assert call(**kw) == abi.ERR_INVALID, kw
        assert word in L.mi355rt_last_error(), (kw, L.mi355rt_last_error())
    assert bytes(buf) == bytes(4096)
    # the one-shot: argument checks first, then the device (there is no CPU path)
    lin, hits = np.zeros((2, 2, 3), np.float32), np.zeros(4, abi.HIT_DTYPE)
    out, packed = np.zeros((2, 2, 3), np.float32), np.zeros((2, 2), np.uint32)
    one = lambda w=2, r=2, p=None, i=lin.ctypes.data, hh=hits.ctypes.data, o=out.ctypes.data, k=packed.ctypes.data: L.mi355rt_denoise(w, r, p, i, hh, o, k)
    for kw, word in ((dict(i=None), b"linear_in"), (dict(hh=None), b"hits"), (dict(o=None, k=None), b"both null"), (dict(w=0), b"width"), (dict(r=0), b"rows"),
                     (dict(w=1 << 20, r=1 << 11), b"2^31"), (dict(p=C.byref(abi.DenoiseParams.make(levels=9))), b"levels"),
                     (dict(p=C.byref(abi.DenoiseParams.make(sigma_color=float("nan")))), b"sigma_color")):
        assert one(**kw) == abi.ERR_INVALID, kw
        assert word in L.mi355rt_last_error(), (kw, L.mi355rt_last_error())
    hnd = C.c_void_p()
    if L.mi355rt_context_create(0, C.byref(hnd)) == 0:
        L.mi355rt_context_destroy(hnd)
        return                                                          # a GPU is visible here: the rest is what its absence looks like
    assert one() == abi.ERR_NO_DEVICE and b"no CPU path" in L.mi355rt_last_error()
    with pytest.raises(device.RenderError) as e:
        device.denoise(lin, hits)
    assert e.value.rc == abi.ERR_NO_DEVICE


def test_scratch_bytes_is_monotone_and_non_zero(native, abi):
    _, device = native
    L = device.lib()
    assert device.denoise_scratch_bytes(1, 1) > 0
    last = 0
    for w, r in ((1, 1), (1, 2), (2, 2), (3, 2), (37, 1), (64, 64), (131, 70), (800, 600), (1920, 1080), (1 << 15, (1 << 16) - 1)):
        b = device.denoise_scratch_bytes(w, r)
        assert b >= 48 * w * r and b % 16 == 0 and b > last, (w, r, b)   # at least two colour images and the guides a tap reads
        assert device.denoise_scratch_bytes(r, w) == b
        last = b
    n = C.c_uint64(7)
    for w, r in ((0, 1), (1, 0), (1 << 16, 1 << 15)):
        assert L.mi355rt_denoise_scratch_bytes(w, r, C.byref(n)) == abi.ERR_INVALID and n.value == 7
    assert L.mi355rt_denoise_scratch_bytes(4, 4, None) == abi.ERR_INVALID


# kernel: (VGPRs allowed, code bytes allowed, LDS bytes).  DESIGN.md 4.7 quotes the measured build: 18 / 10 / 43 / 44 VGPRs, 0.2 / 0.7 / 3.0 / 3.6 KB
# (the staged forms of the steps 1 and 2: 44 - 45 VGPRs, 3.3 - 3.9 KB), nothing spilled, no scratch.  Budgets in the style of
# tests/test_ray_query_abi.py: about a quarter above the build, and 64 VGPRs or fewer for the level kernels (8 waves per SIMD).  Only the
# staged forms use LDS -- tile plus halo, 48 bytes per pixel: 5 workgroups per CU at step 2 -- and a workgroup barrier.
DENOISE_BUDGET = {
    "k_denoise_prepass": (24, 512, 0),
    "k_denoise_copy": (16, 1024, 0),
    "k_denoise_level": (56, 4 * 1024, 0),
    "k_denoise_last": (56, 5 * 1024, 0),
    "k_denoise_level_staged1": (56, 4608, 36 * 12 * 48),
    "k_denoise_last_staged1": (56, 5 * 1024, 36 * 12 * 48),
    "k_denoise_level_staged2": (56, 4608, 40 * 16 * 48),
    "k_denoise_last_staged2": (56, 5 * 1024, 40 * 16 * 48),
}


def test_denoise_kernels_are_built_and_stay_inside_their_budgets(native):
    isa_stats = importlib.import_module("isa_stats")
    build = pkg("build")
    raw = isa_stats.kernel_stats(build.DEVICE_SO)
    stats = {isa_stats.short(k): v for k, v in raw.items()}
    assert {k for k in stats if k.startswith("k_denoise")} == set(DENOISE_BUDGET)
    assert not [k for k in raw if "k_denoise" in k and ("k_render_ctr" in k or isa_stats.short(k).startswith("k_query"))]
    isa = {isa_stats.short(k): v for k, v in isa_stats.kernel_isa(build.DEVICE_SO).items()}
    for name, (vgprs, code, lds) in DENOISE_BUDGET.items():
        st = stats[name]
        assert st["vgpr_count"] <= vgprs and st["code_bytes"] <= code, (name, st)
        assert st["vgpr_spill_count"] == 0 and st["sgpr_spill_count"] == 0, (name, st)
        assert st["private_segment_fixed_size"] == 0 and st.get("scratch_insts", 0) == 0, (name, st)
        assert st["group_segment_fixed_size"] == lds, (name, st)
        ops = [i.split()[0] for i in isa[name]]
        assert not [o for o in ops if "atomic" in o or o.startswith(("scratch_", "s_sleep"))], name
        assert lds or not [o for o in ops if o.startswith(("ds_", "s_barrier"))], name
    assert build.DEVICE_SRCS.count(os.path.join(build.CSRC, "device", "rt_denoise.hip")) == 1    # kernel_hash() covers the new translation unit
