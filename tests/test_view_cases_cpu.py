"""The camera views (mi355rt_view_scratch_bytes, mi355rt_context_view_rays, mi355rt_context_render_view; added within ABI version 5) without a GPU:
the numpy ray makers of tests/view_cases.py against each other and against tests/radiance_cases.py, the struct as the C compiler lays it out, the
exports, every refusal with its text reached before the device, the barrier in front of rt_view.hip's entry points, and the register, LDS and spill
figures of the new kernels read off the built code object."""
import ctypes as C
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import radiance_cases as RC
import view_cases as VC
from conftest import ROOT, load_for_both, pkg

sys.path.insert(0, os.path.join(ROOT, "tools"))

F = np.float32
NEW = ("mi355rt_view_scratch_bytes", "mi355rt_context_view_rays", "mi355rt_context_render_view")
VIEW_FIELDS = ("camera", "model", "width", "height", "flags", "lens_radius", "focus_distance", "reserved")


@pytest.fixture(scope="module")
def scenes(native, oracle_mod):
    host, _ = native
    return {n: load_for_both(n, oracle_mod, host, width=24, height=16, spp=1, max_depth=VC.DEPTH) for n in VC.SCENES}


def all_cases(scenes):
    for name in VC.SCENES:
        for cam in VC.CAMERAS:
            for W, H in VC.SIZES:
                for seed in VC.SEEDS:
                    yield name, cam, VC.camera(cam, scenes[name]), W, H, seed


# ---- the makers ---------------------------------------------------------------------------------------------------------------------------
def test_the_pinhole_maker_is_radiance_cases_camera_rays_bit_for_bit(scenes, oracle_mod, abi):
    for name, cname, cam, W, H, seed in all_cases(scenes):
        for s in (0, 4, 16):
            got = VC.pinhole_rays(oracle_mod, abi, cam, W, H, s, seed)
            want = RC.camera_rays(oracle_mod, abi, cam, W, H, s, seed)
            assert got.tobytes() == want.tobytes(), (name, cname, W, H, seed, s)


def test_the_thin_lens_with_radius_0_has_the_pinholes_origins_and_every_lens_point_is_inside_the_disk(scenes, oracle_mod, abi):
    worst = 0
    for name, cname, cam, W, H, seed in all_cases(scenes):
        radius, focus = VC.lens_of(cam)
        for s in range(max(VC.SAMPLES)):
            rays, a, b, tried = VC.thin_lens_rays(oracle_mod, abi, cam, W, H, s, radius, focus, seed, want_tries=True)
            assert (a * a + b * b < F(1.0)).all() and (a.dtype, b.dtype) == (F, F)
            worst = max(worst, int(tried.max()))
            if cname != "own" or s not in (0, 16):
                continue
            zero = VC.thin_lens_rays(oracle_mod, abi, cam, W, H, s, 0.0, focus, seed)
            pin = VC.pinhole_rays(oracle_mod, abi, cam, W, H, s, seed)
            assert zero["origin"].tobytes() == pin["origin"].tobytes(), (name, W, H, seed, s)
            assert not np.array_equal(rays["origin"], pin["origin"])                        # ... and with a radius they move
            assert (np.abs(rays["origin"] - pin["origin"]).max(axis=1) <= F(radius)).all()
    # a try is rejected with probability 1 - pi / 4 = 0.215: 64 rejections in a row have probability 1e-43.  The fallback is not among the cases.
    print(f"largest try number over all case inputs: {worst} (cap {VC.LENS_TRIES})")
    assert worst <= 16 < VC.LENS_TRIES


def test_the_thin_lens_fallback_after_64_rejected_tries(scenes, oracle_mod, abi):
    cam, W, H = scenes["cornell"].camera, 13, 7
    n = W * H
    calls = []

    def corner(j):                                                                          # a = b = 1 - 2^-23: outside the disk, every try
        calls.append(j)
        w = np.zeros((n, 4), np.uint32); w[:, 2:] = 0xFFFFFFFF
        return w

    rays, a, b, tried = VC.thin_lens_rays(oracle_mod, abi, cam, W, H, 0, 0.25, 3.0, block_source=corner, want_tries=True)
    assert calls == list(range(VC.LENS_TRIES)) and (tried == VC.LENS_TRIES).all()
    assert (a.view(np.uint32) == 0).all() and (b.view(np.uint32) == 0).all()
    zero = VC.thin_lens_rays(oracle_mod, abi, cam, W, H, 0, 0.0, 3.0)
    assert rays["origin"].tobytes() == zero["origin"].tobytes()

    def late(j):                                                                            # accepted on the last try the cap allows
        w = corner(j)
        if j == VC.LENS_TRIES - 1:
            w[:, 2:] = 0x80000000                                                           # a = b = 0
        return w

    _, a, b, tried = VC.thin_lens_rays(oracle_mod, abi, cam, W, H, 0, 0.25, 3.0, block_source=late, want_tries=True)
    assert (tried == VC.LENS_TRIES - 1).all() and (a == 0).all() and (b == 0).all()
    a, b, tried = VC.lens_points(3, lambda j: np.array([[0, 0, 0x80000000, 0x80000000], [0, 0, 0xFFFFFFFF, 0xFFFFFFFF], [0, 0, 0, 0xFFFFFFFF]], np.uint32), tries=2)
    assert list(tried) == [0, 2, 2] and list(a) == [0, 0, 0]                                 # (-1, 1 - 2^-23) is outside as well


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------------
LAYOUT_C = r"""
#include <stdio.h>
#include "mi355rt.h"
#define F(T, f) printf(#T "." #f " %zu %zu\n", offsetof(T, f), sizeof(((T*)0)->f))
int main(void) {
    printf("sizeof %zu %zu\n", sizeof(mi355rt_view), _Alignof(mi355rt_view));
    printf("constants %u %u %u\n", MI355RT_VIEW_PINHOLE, MI355RT_VIEW_THIN_LENS, MI355RT_VIEW_CENTRE);
    F(mi355rt_view, camera); F(mi355rt_view, model); F(mi355rt_view, width); F(mi355rt_view, height); F(mi355rt_view, flags);
    F(mi355rt_view, lens_radius); F(mi355rt_view, focus_distance); F(mi355rt_view, reserved);
    return 0;
}
"""


def test_the_view_is_laid_out_as_the_c_compiler_lays_out_the_header(tmp_path, abi):
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = subprocess.check_output([str(exe)], text=True).split("\n")
    assert out[0] == "sizeof 96 4" and C.sizeof(abi.View) == 96 and 96 % 16 == 0
    assert out[1] == f"constants {abi.VIEW_PINHOLE} {abi.VIEW_THIN_LENS} {abi.VIEW_CENTRE}" == "constants 0 1 1"
    got = {line.split()[0]: tuple(int(v) for v in line.split()[1:]) for line in out[2:] if "." in line}
    assert tuple(n for n, _ in abi.View._fields_) == VIEW_FIELDS
    want = {f"mi355rt_view.{f}": (getattr(abi.View, f).offset, getattr(abi.View, f).size) for f in VIEW_FIELDS}
    assert got == want and want["mi355rt_view.camera"] == (0, C.sizeof(abi.Camera))
    cam = abi.Camera(); cam.position[:] = [1.0, 2.0, 3.0]; cam.half_height = 0.25
    v = abi.View.make(cam, 24, 16, abi.VIEW_THIN_LENS, abi.VIEW_CENTRE, 0.5, 4.0)
    assert (list(v.camera.position), v.camera.half_height, v.model, v.width, v.height, v.flags, v.lens_radius, v.focus_distance, list(v.reserved)) == \
        ([1.0, 2.0, 3.0], 0.25, 1, 24, 16, 1, 0.5, 4.0, [0, 0, 0, 0])


def test_declared_and_exported_and_the_abi_number_did_not_move(native, abi):
    _, device = native
    header = open(os.path.join(ROOT, "include", "mi355rt.h")).read()
    so = C.CDLL(pkg("build").DEVICE_SO)
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert hasattr(so, name) and name in device.EXPORTS
        assert name in header.split("#define MI355RT_ABI_VERSION")[1].split("*/")[0], name       # the version comment names them
    assert device.lib().mi355rt_abi_version() == abi.ABI_VERSION == 5
    assert callable(device.Context.view_rays) and callable(device.Context.render_view) and callable(device.view_scratch_bytes)


def test_every_entry_point_of_rt_view_sits_behind_the_barrier():
    """The regular expression of tests/test_exception_barrier.py, applied to the three entry points: they stand in rt_queries.cpp, which sees the context
    struct, each defined once and opening with the guard, and no .hip file defines any of them."""
    dev_dir = os.path.join(ROOT, "raytracer-rust_amd/csrc/device")
    src = {n: open(os.path.join(dev_dir, n)).read() for n in sorted(os.listdir(dev_dir)) if n.endswith((".cpp", ".hip"))}
    text = src["rt_queries.cpp"]
    defs = [(n, first) for n, first in re.findall(r"\nint (mi355rt_\w+)\((?:[^()]|\([^()]*\))*\) \{\n(.*)\n", text[text.index('extern "C" {'):]) if n in NEW]
    assert sorted(n for n, _ in defs) == sorted(NEW) and len(defs) == 3
    bare = [n for n, first in defs if "return guard([&]() -> int {" not in first]
    assert not bare, bare
    for name, other in src.items():                                                             # ... defined there only, and in no .hip
        if name != "rt_queries.cpp":
            assert not re.search(r"\nint (?:" + "|".join(NEW) + r")\(", other), name
    prepare = src["rt_prepare.cpp"]
    assert "int plan_view(" in prepare and "hip" not in prepare.split("int plan_view(")[1].split("\n}\n")[0].lower()   # the plan holds no HIP call


def a_view(abi, model=None, W=4, H=3, **kw):
    cam = abi.Camera()
    cam.position[:] = [0.0, 1.0, 5.0]; cam.forward[:] = [0.0, 0.0, -1.0]; cam.right[:] = [1.0, 0.0, 0.0]; cam.true_up[:] = [0.0, 1.0, 0.0]
    cam.half_width, cam.half_height = 0.4, 0.3
    model = abi.VIEW_PINHOLE if model is None else model
    lens = (0.1, 2.0) if model == abi.VIEW_THIN_LENS else (0.0, 0.0)
    v = abi.View.make(cam, W, H, model, 0, *lens)
    for k, val in kw.items():
        setattr(v, k, val)
    return v


def bad_views(abi):
    """(view, the words its refusal names)."""
    inf, nan = float("inf"), float("nan")
    out = [(a_view(abi, model=2), "view.model"), (a_view(abi, model=3), "view.model"), (a_view(abi, model=0xFFFFFFFF), "view.model"), (a_view(abi, width=0), "view.width"),
           (a_view(abi, height=0), "view.height"), (a_view(abi, flags=2), "view.flags"), (a_view(abi, flags=0x80000001), "view.flags")]
    for k in range(4):
        v = a_view(abi); v.reserved[k] = 1
        out.append((v, "view.reserved"))
    for field in ("position", "forward", "right", "true_up"):
        for k, bad in ((0, nan), (1, inf), (2, -inf)):
            v = a_view(abi); getattr(v.camera, field)[k] = bad
            out.append((v, "view.camera"))
    for field in ("half_width", "half_height"):
        v = a_view(abi); setattr(v.camera, field, nan)
        out.append((v, "view.camera"))
    T = abi.VIEW_THIN_LENS
    out += [(a_view(abi, T, lens_radius=-0.5), "view.lens_radius"), (a_view(abi, T, lens_radius=nan), "view.lens_radius"), (a_view(abi, T, lens_radius=inf), "view.lens_radius"),
            (a_view(abi, T, focus_distance=0.0), "view.focus_distance"), (a_view(abi, T, focus_distance=-1.0), "view.focus_distance"),
            (a_view(abi, T, focus_distance=nan), "view.focus_distance"), (a_view(abi, T, focus_distance=inf), "view.focus_distance")]
    out += [(a_view(abi, lens_radius=0.1), "view.lens_radius"), (a_view(abi, focus_distance=1.0), "view.focus_distance"), (a_view(abi, lens_radius=nan), "view.lens_radius")]
    return out


def test_scratch_bytes(native, abi):
    _, device = native
    L = device.lib()
    for W, H, s in ((1, 1, 1), (4, 3, 5), (24, 16, 17), (13, 7, 1), (800, 600, 16), (65535, 65537, 1), (1, 1, 0xFFFFFFFF), (7, 3, 0)):
        assert device.view_scratch_bytes(a_view(abi, W=W, H=H), s) == (12 * W * H * s + 15) // 16 * 16, (W, H, s)
        assert device.view_scratch_bytes(a_view(abi, W=W, H=H), s) == device.radiance_scratch_bytes(W * H, s) if W * H < 2 ** 32 else True
    out = C.c_uint64(77)
    for W, H, s in ((65536, 65536, 1), (0xFFFFFFFF, 0xFFFFFFFF, 1), (65536, 1, 65536), (800, 600, 8948), (2, 1, 0x80000000)):   # W * H * samples >= 2^32
        assert L.mi355rt_view_scratch_bytes(C.byref(a_view(abi, W=W, H=H)), s, C.byref(out)) == abi.ERR_INVALID and b"split the call" in L.mi355rt_last_error(), (W, H, s)
        assert out.value == 77
    assert device.view_scratch_bytes(a_view(abi, W=800, H=600), 8947) == (12 * 480000 * 8947 + 15) // 16 * 16          # 2^32 - 407 040 items pass
    assert L.mi355rt_view_scratch_bytes(C.byref(a_view(abi)), 1, None) == abi.ERR_INVALID and b"out_bytes is null" in L.mi355rt_last_error()
    assert L.mi355rt_view_scratch_bytes(None, 1, C.byref(out)) == abi.ERR_INVALID and b"view is null" in L.mi355rt_last_error()
    for v, word in bad_views(abi):
        assert L.mi355rt_view_scratch_bytes(C.byref(v), 1, C.byref(out)) == abi.ERR_INVALID and word.encode() in L.mi355rt_last_error(), word


def test_refusals_are_reached_before_the_device(native, abi):
    _, device = native
    L = device.lib()
    buf = (C.c_uint8 * 256)()
    p = (C.addressof(buf) + 15) & ~15
    err = lambda: L.mi355rt_last_error().decode()
    rays, render = L.mi355rt_context_view_rays, L.mi355rt_context_render_view
    P = C.byref
    ok, view = abi.RadianceParams.make(0, 4, 8), a_view(abi)
    # the view first, in both calls, each with a text that names the field
    assert rays(None, None, 0, 0, p, None) == abi.ERR_INVALID and "view_rays: view is null" in err()
    assert render(None, None, P(ok), p, None, None, p, None) == abi.ERR_INVALID and "render_view: view is null" in err()
    for v, word in bad_views(abi):
        assert rays(None, P(v), 0, 0, p, None) == abi.ERR_INVALID and word in err() and err().startswith("view_rays: "), (word, err())
        assert render(None, P(v), P(ok), p, None, None, p, None) == abi.ERR_INVALID and word in err() and err().startswith("render_view: "), (word, err())
    for model in (abi.VIEW_PINHOLE, abi.VIEW_THIN_LENS):                     # ... and every model passes it, with and without CENTRE
        for flags in (0, abi.VIEW_CENTRE):
            assert rays(None, P(a_view(abi, model, flags=flags)), 0, 0, p, None) == abi.ERR_INVALID and "ctx is null" in err(), (model, flags, err())
            assert render(None, P(a_view(abi, model, flags=flags)), P(ok), p, p + 4, p + 8, p, None) == abi.ERR_INVALID and "ctx is null" in err(), (model, flags, err())
    v = a_view(abi, abi.VIEW_THIN_LENS, lens_radius=0.0)                                        # a lens of radius 0 is a thin lens
    assert rays(None, P(v), 0, 0, p, None) == abi.ERR_INVALID and "ctx is null" in err()
    # view_rays: its buffer and its size
    assert rays(None, P(view), 0, 0, None, None) == abi.ERR_INVALID and "d_rays is null" in err()
    assert rays(None, P(view), 0, 0, p + 8, None) == abi.ERR_INVALID and "d_rays must be 16-byte aligned" in err()
    assert rays(None, P(a_view(abi, W=65536, H=65536)), 0, 0, p, None) == abi.ERR_INVALID and "split the call" in err()
    assert rays(None, P(a_view(abi, W=65535, H=65537)), 0xFFFFFFFF, 2 ** 64 - 1, p, None) == abi.ERR_INVALID and "ctx is null" in err()   # 2^32 - 1 pixels, any sample and seed
    # render_view: everything the radiance query refuses about the params and the pointers
    assert render(None, P(view), None, p, None, None, p, None) == abi.ERR_INVALID and "params is null" in err()
    bad = [(abi.RadianceParams(0, 4, 8, 1, 0, 0), "params.flags"), (abi.RadianceParams(0, 4, 8, 0, 0, 1), "params.reserved"),
           (abi.RadianceParams(4, 4, 8, 0, 0, 0), "params.sample_begin"), (abi.RadianceParams(5, 4, 8, 0, 0, 0), "params.sample_begin"),
           (abi.RadianceParams(0, 0, 8, 0, 0, 0), "params.sample_begin")]
    for prm, word in bad:
        assert render(None, P(view), P(prm), p, None, None, p, None) == abi.ERR_INVALID and word in err() and err().startswith("render_view: "), (word, err())
    assert render(None, P(view), P(ok), None, None, None, p, None) == abi.ERR_INVALID and "d_accum is null" in err()
    assert render(None, P(view), P(ok), p, None, None, None, None) == abi.ERR_INVALID and "d_scratch is null" in err()
    assert render(None, P(view), P(ok), p + 8, None, None, p, None) == abi.ERR_INVALID and "d_accum must be 16-byte aligned" in err()
    assert render(None, P(view), P(ok), p, None, None, p + 4, None) == abi.ERR_INVALID and "d_scratch must be 16-byte aligned" in err()
    assert render(None, P(view), P(ok), p, p + 2, None, p, None) == abi.ERR_INVALID and "d_out_linear must be 4-byte aligned" in err()
    assert render(None, P(view), P(ok), p, None, p + 1, p, None) == abi.ERR_INVALID and "d_out_packed must be 4-byte aligned" in err()
    big = abi.RadianceParams.make(0, 8948, 8)
    assert render(None, P(a_view(abi, W=800, H=600)), P(big), p, None, None, p, None) == abi.ERR_INVALID and "split the call" in err() and "view.width * view.height * samples" in err()
    assert render(None, P(a_view(abi, W=65536, H=65536)), P(ok), p, None, None, p, None) == abi.ERR_INVALID and "split the call" in err()
    big = abi.RadianceParams.make(1, 8948, 8)
    assert render(None, P(a_view(abi, W=800, H=600)), P(big), p, None, None, p, None) == abi.ERR_INVALID and "ctx is null" in err()      # 8947 samples pass
    # the radiance query's own texts did not move
    q = L.mi355rt_context_trace_radiance
    assert q(None, P(ok), None, 1, p, None, p, None) == abi.ERR_INVALID and err() == "trace_radiance: d_rays is null"
    assert q(None, P(abi.RadianceParams.make(0, 65536, 8)), p, 65536, p, None, p, None) == abi.ERR_INVALID and err() == "trace_radiance: n_rays * samples must stay below 2^32 (split the call)"
    h = C.c_void_p()
    if L.mi355rt_context_create(0, C.byref(h)) == 0:                   # a GPU is visible here: a context that never saw a scene
        try:
            assert rays(h, P(view), 0, 0, p, None) == abi.ERR_INVALID and "no scene" in err()
            assert render(h, P(view), P(ok), p, None, None, p, None) == abi.ERR_INVALID and "no scene" in err()
        finally:
            L.mi355rt_context_destroy(h)


# ---- the code object ---------------------------------------------------------------------------------------------------------------------
MODELS = ("pinhole", "thin_lens")
# kernel: (VGPRs allowed, code bytes).  Every new kernel: no spilled register of either kind, no private segment, no scratch instruction, no LDS.  The path
# kernels stay at 128 VGPRs or fewer (4 waves per SIMD, as k_radiance_paths: every material and the sky lookup are compiled in), the ray makers and the
# sum at 64 or fewer (8).  Code sizes: k_radiance_paths[_mesh]'s budgets plus 4 KB for the maker in the refill.
VIEW_BUDGET = {f"k_view_paths_{m}": (128, 28 * 1024) for m in MODELS}
VIEW_BUDGET.update({f"k_view_paths_{m}_mesh": (128, 32 * 1024) for m in MODELS})
VIEW_BUDGET.update({f"k_view_rays_{m}": (64, 4 * 1024) for m in MODELS})
VIEW_BUDGET["k_view_sum"] = (64, 2 * 1024)


def test_view_kernels_are_built_and_stay_inside_their_budgets(native):
    isa_stats = importlib.import_module("isa_stats")
    build = pkg("build")
    stats = {isa_stats.short(k): v for k, v in isa_stats.kernel_stats(build.DEVICE_SO).items()}
    assert {k for k in stats if k.startswith("k_view")} == set(VIEW_BUDGET)
    isa = {isa_stats.short(k): v for k, v in isa_stats.kernel_isa(build.DEVICE_SO).items()}
    for name, (vgprs, code) in VIEW_BUDGET.items():
        st = stats[name]
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
    for m in MODELS:
        assert set(stores(f"k_view_paths_{m}")) == set(stores(f"k_view_paths_{m}_mesh")) == {"global_store_dwordx3"}    # a path's radiance leaves as one 12-byte store
        assert stores(f"k_view_rays_{m}") == ["global_store_dwordx4"] * 2                        # the two float4 of a mi355rt_path_ray
        # the paths kernels load NO ray: whatever they read from global memory, the scene, k_radiance_paths reads too -- minus its two 16-byte ray loads
        loads = lambda name: sorted(i.split()[0] for i in isa[name] if i.startswith("global_load"))
        for mesh in ("", "_mesh"):
            want = loads("k_radiance_paths" + mesh)
            for _ in range(2):
                want.remove("global_load_dwordx4")
            assert loads(f"k_view_paths_{m}{mesh}") == want, (m, mesh)
        assert not [i for i in isa[f"k_view_rays_{m}"] if i.startswith("global_load")], m        # the view arrives as kernel arguments
    assert stores("k_view_sum") == ["global_store_dword", "global_store_dwordx3", "global_store_dwordx4"]   # the packed pixel, the mean, the float4 sum
    assert len([i for i in isa["k_view_sum"] if "row_shr:1" in i]) >= 45                          # k_resolve's chain: 15 steps on three channels
    # a pinhole view does not pay for the rejection loop: it is the smaller of the two, and close to the query's kernel
    for mesh in ("", "_mesh"):
        pin, lens, query = (stats[n + mesh]["code_bytes"] for n in ("k_view_paths_pinhole", "k_view_paths_thin_lens", "k_radiance_paths"))
        assert pin < lens and pin - query < 2048, (mesh, pin, lens, query)
    srcs = [os.path.basename(s) for s in build.DEVICE_SRCS]
    assert srcs.count("rt_view.hip") == 1                                                       # kernel_hash() covers the source and the two new headers
    for h in ("rt_view.h", "rt_radiance_paths.h"):
        assert os.path.join(build.CSRC, "device", h) in build.DEVICE_HEADERS
