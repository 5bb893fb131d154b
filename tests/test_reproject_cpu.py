"""The temporal reprojection (mi355rt_post_reproject of include/mi355rt_post.h, libmi355rt_post.so) without a GPU: the params struct is laid out as
the C compiler lays out the header's, the header's functions are the library's exports, the library reads no environment, libmi355rt.so exports what
it exported, every refusal is decided before a device is looked for and names its argument, k_post_reproject is in the code object without spills
or scratch, the numpy restatement (tests/reproject_ref.py) has the properties the header states, and on the oracle's frames of a small orbit
the reprojected image is closer to the converged one than the raw frame."""
import ctypes as C
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import reproject_cases as RC
import reproject_ref as RR
from conftest import ROOT, SCENES, pkg
from parity import assert_same_bits_nan_folded, oracle_threads

sys.path.insert(0, os.path.join(ROOT, "tools"))

F = np.float32
FIELDS = ("max_history", "flags", "normal_min", "plane_tolerance")
DECLARED = ("mi355rt_post_abi_version", "mi355rt_post_last_error", "mi355rt_post_reproject")

LAYOUT_C = r"""
#include <stdio.h>
#include "mi355rt_post.h"
#define F(T, f) printf(#T "." #f " %zu %zu\n", offsetof(T, f), sizeof(((T*)0)->f))
int main(void) {
    printf("sizeof %zu %zu\n", sizeof(mi355rt_reproject_params), _Alignof(mi355rt_reproject_params));
    F(mi355rt_reproject_params, max_history); F(mi355rt_reproject_params, flags); F(mi355rt_reproject_params, normal_min); F(mi355rt_reproject_params, plane_tolerance);
    return 0;
}
"""


@pytest.fixture(scope="module")
def post():
    """Build (if stale) and return the binding of libmi355rt_post.so."""
    pkg("build").build_post()
    return pkg("post")


def header_text(name):
    return open(os.path.join(ROOT, "include", name)).read()


def declared_functions(name):
    text = re.sub(r"/\*.*?\*/", "", header_text(name), flags=re.S)
    return sorted(set(re.findall(r"\b(mi355rt_[a-z0-9_]+)\s*\(", text)))


def exported_functions(so):
    isa_stats = importlib.import_module("isa_stats")
    table = subprocess.check_output([os.path.join(isa_stats.LLVM, "llvm-readelf"), "--dyn-syms", "-W", so], text=True)
    return sorted(f[7] for f in (line.split() for line in table.splitlines()) if len(f) == 8 and f[3] == "FUNC" and f[6] != "UND" and f[7].startswith("mi355rt_"))


# ---- 1: the ABI ------------------------------------------------------------------------------------------------------------------------------
def test_params_are_laid_out_as_the_c_compiler_lays_out_the_header(tmp_path, abi):
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = subprocess.check_output([str(exe)], text=True).split("\n")
    assert out[0] == "sizeof 16 4" and C.sizeof(abi.ReprojectParams) == 16
    assert tuple(n for n, _ in abi.ReprojectParams._fields_) == FIELDS
    got = {line.split()[0]: tuple(int(v) for v in line.split()[1:]) for line in out[1:] if "." in line}
    assert got == {f"mi355rt_reproject_params.{f}": (getattr(abi.ReprojectParams, f).offset, getattr(abi.ReprojectParams, f).size) for f in FIELDS}


def test_the_headers_functions_are_exactly_the_librarys_exports(post, abi):
    build = pkg("build")
    assert tuple(declared_functions("mi355rt_post.h")) == DECLARED
    assert tuple(exported_functions(build.POST_SO)) == DECLARED and sorted(post.EXPORTS) == sorted(DECLARED)
    assert post.lib().mi355rt_post_abi_version() == abi.POST_ABI_VERSION == 1
    assert not [n for n in declared_functions("mi355rt.h") if n.startswith("mi355rt_post")]       # tests/test_abi.py looks for mi355rt.h's in the two old libraries
    undef = subprocess.run(["nm", "-D", "--undefined-only", build.POST_SO], capture_output=True, text=True, check=True).stdout
    assert "getenv" not in undef
    assert "mi355rt_last_error" not in subprocess.run(["nm", "-D", build.POST_SO], capture_output=True, text=True, check=True).stdout   # nothing of rt_prepare.cpp is linked in


def test_the_device_library_exports_what_its_header_declares(native, post):
    """libmi355rt.so did not grow: its mi355rt_* exports are functions mi355rt.h declares or debug hooks, none is a post stage, and every function the
    header declares is still an export of one of the two old libraries."""
    build = pkg("build")
    declared = set(declared_functions("mi355rt.h"))
    dev, host = set(exported_functions(build.DEVICE_SO)), set(exported_functions(build.HOST_SO))
    assert not [n for n in dev | host if n.startswith("mi355rt_post")]
    assert not [n for n in dev if n not in declared and not n.startswith("mi355rt_debug_")], sorted(dev - declared)
    assert declared <= dev | host, sorted(declared - dev - host)
    assert len(dev) == 58                                                       # the count tests/test_exception_barrier.py pins


def test_defaults_are_the_headers(post, abi):
    assert "params_or_null == NULL: {32, 0, 0.9f, 0.05f}" in header_text("mi355rt_post.h")
    p = abi.ReprojectParams.make()
    assert (p.max_history, p.flags, p.normal_min, p.plane_tolerance) == (32, 0, F(0.9), F(0.05)) and abi.REPROJECT_DEFAULTS == RR.DEFAULTS == (32, 0, 0.9, 0.05)
    plan = open(os.path.join(ROOT, "raytracer-rust_amd", "csrc", "post", "post_plan.cpp")).read()
    assert "defaults = {32u, 0u, 0.9f, 0.05f}" in plan
    assert not re.search(r"#include\s*<hip|\bhip[A-Z]\w*\(", plan)                  # the plan is the HIP-free half: no runtime header, no runtime call


# ---- 2: refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_comes_before_the_device_and_names_its_argument(native, post, abi):
    _, device = native
    L = post.lib()
    buf = (C.c_uint8 * 8192)()
    base = (C.addressof(buf) + 63) & ~63          # never read: every refusal below is decided from the arguments alone
    hc, cc, hp, mp, ho, ol, op = (base + 512 * i for i in range(7))
    cam = RC.canonical(abi)
    ok_view = lambda W=4, H=4: RC.view(abi, cam, W, H)
    ok = abi.ReprojectParams.make()

    def call(dev=0, cur=ok_view(), prev=ok_view(), p=ok, hits_cur=hc, color=cc, hits_prev=hp, hist_prev=mp, hist_out=ho, lin=ol, packed=op):
        ref = lambda s: C.byref(s) if s is not None else None
        v = lambda a: C.c_void_p(a) if a else None
        return L.mi355rt_post_reproject(dev, ref(cur), ref(prev), ref(p), v(hits_cur), v(color), v(hits_prev), v(hist_prev), v(hist_out), v(lin), v(packed), None)

    def changed(W=4, H=4, **fields):
        v = ok_view(W, H)
        for k, val in fields.items():
            if k == "forward1":
                v.camera.forward[1] = val
            elif k == "half_width":
                v.camera.half_width = val
            else:
                setattr(v, k, val)
        return v

    nan, inf = float("nan"), float("inf")
    refusals = [
        (dict(cur=None), b"cur is null"),
        (dict(cur=changed(model=2)), b"cur.model"), (dict(prev=changed(model=3)), b"prev.model"),
        (dict(cur=changed(W=0)), b"cur.width"), (dict(cur=changed(H=0)), b"cur.height"), (dict(prev=changed(W=0)), b"prev.width"), (dict(prev=changed(H=0)), b"prev.height"),
        (dict(cur=changed(forward1=nan)), b"cur.camera"), (dict(prev=changed(half_width=inf)), b"prev.camera"),
        (dict(cur=changed(W=1 << 16, H=1 << 15)), b"cur.width * cur.height must be below 2^31"), (dict(prev=changed(W=(1 << 31) - 1, H=2)), b"prev.width * prev.height must be below 2^31"),
        (dict(p=abi.ReprojectParams.make(max_history=0)), b"params.max_history"), (dict(p=abi.ReprojectParams.make(max_history=65536)), b"params.max_history"),
        (dict(p=abi.ReprojectParams.make(flags=1)), b"params.flags"),
        (dict(p=abi.ReprojectParams.make(normal_min=nan)), b"params.normal_min"), (dict(p=abi.ReprojectParams.make(normal_min=1.5)), b"params.normal_min"),
        (dict(p=abi.ReprojectParams.make(normal_min=-1.5)), b"params.normal_min"), (dict(p=abi.ReprojectParams.make(normal_min=-inf)), b"params.normal_min"),
        (dict(p=abi.ReprojectParams.make(plane_tolerance=0.0)), b"params.plane_tolerance"), (dict(p=abi.ReprojectParams.make(plane_tolerance=-1.0)), b"params.plane_tolerance"),
        (dict(p=abi.ReprojectParams.make(plane_tolerance=nan)), b"params.plane_tolerance"), (dict(p=abi.ReprojectParams.make(plane_tolerance=inf)), b"params.plane_tolerance"),
        (dict(hits_cur=None), b"d_hits_cur is null"), (dict(color=None), b"d_color_cur is null"), (dict(hist_out=None), b"d_hist_out is null"),
        (dict(hits_cur=hc + 8), b"d_hits_cur must be 16-byte"), (dict(color=cc + 2), b"d_color_cur must be 4-byte"), (dict(hist_out=ho + 4), b"d_hist_out must be 16-byte"),
        (dict(lin=ol + 1), b"d_out_linear must be 4-byte"), (dict(packed=op + 2), b"d_out_packed must be 4-byte"),
        (dict(hits_prev=None), b"d_hits_prev is null"), (dict(hist_prev=None), b"d_hist_prev is null"),
        (dict(hits_prev=hp + 4), b"d_hits_prev must be 16-byte"), (dict(hist_prev=mp + 8), b"d_hist_prev must be 16-byte"),
        (dict(prev=None), b"d_hits_prev is given without prev"), (dict(prev=None, hits_prev=None), b"d_hist_prev is given without prev"),
        (dict(hist_out=mp), b"d_hist_out must not be d_hist_prev"),
        (dict(dev=-1), b"hip_device"),
    ]
    for kw, word in refusals:
        assert call(**kw) == abi.ERR_INVALID, kw
        assert word in L.mi355rt_post_last_error(), (kw, L.mi355rt_post_last_error())
    assert bytes(buf) == bytes(8192)
    with pytest.raises(post.RenderError) as e:
        post.reproject(None, None, hc, cc, None, None, ho)
    assert e.value.rc == abi.ERR_INVALID and "cur is null" in str(e.value)
    hnd = C.c_void_p()
    if device.lib().mi355rt_context_create(0, C.byref(hnd)) == 0:
        device.lib().mi355rt_context_destroy(hnd)
        return                                                          # a GPU is visible here: the rest is what its absence looks like
    for kw in (dict(), dict(prev=None, hits_prev=None, hist_prev=None), dict(p=None), dict(lin=None, packed=None), dict(lin=cc)):
        assert call(**kw) == abi.ERR_NO_DEVICE and b"no CPU path" in L.mi355rt_post_last_error(), kw
    assert bytes(buf) == bytes(8192)


# ---- 3: the kernel in the code object ------------------------------------------------------------------------------------------------------------
def test_the_kernel_is_built_without_spills_or_scratch(post):
    """DESIGN.md 4.15 quotes the build: 41 VGPRs, 84 SGPRs, 3.1 KB.  The budget is 64 VGPRs (8 waves per SIMD) and a quarter more code."""
    isa_stats = importlib.import_module("isa_stats")
    build = pkg("build")
    stats = {isa_stats.short(k): v for k, v in isa_stats.kernel_stats(build.POST_SO).items()}
    assert set(stats) == {"k_post_reproject"}
    st = stats["k_post_reproject"]
    print("k_post_reproject:", st)
    assert st["vgpr_count"] <= 64 and st["sgpr_count"] <= 102 and st["code_bytes"] <= 4096, st
    assert st["vgpr_spill_count"] == 0 and st["sgpr_spill_count"] == 0, st
    assert st["private_segment_fixed_size"] == 0 and st.get("scratch_insts", 0) == 0 and st["group_segment_fixed_size"] == 0, st
    # the product library's kernels are not this library's business: kernel_hash() covers csrc/device only
    assert not [s for s in build.DEVICE_SRCS if os.sep + "post" + os.sep in s]


# ---- 4: properties of the reference ----------------------------------------------------------------------------------------------------------
STATIC_SIZE = (33, 9)
STATIC_FRAMES = 40
STATIC_MAX_HISTORY = 32


@pytest.fixture(scope="module")
def static_chain(abi):
    """The same camera and the same hits for STATIC_FRAMES frames of seeded colour: [(colour, history out)] -- computed once, read-only."""
    W, H = STATIC_SIZE
    cam = RC.look_at(abi, (0.3, 0.2, -1.4), (0.0, 0.0, 0.0), vfov_deg=70.0, aspect=W / H)
    v = RC.view(abi, cam, W, H)
    hits = RC.plane_hits(abi, cam, W, H)
    assert (hits["primitive"] != RC.NO_HIT).all()
    rng = np.random.default_rng(5)
    params = abi.ReprojectParams.make(STATIC_MAX_HISTORY)
    frames, hist = [], None
    for k in range(STATIC_FRAMES):
        c = rng.random((W * H, 3), dtype=F)
        hist = RR.reproject(v, v if k else None, hits, c, hits if k else None, hist, params)
        hist.setflags(write=False)
        frames.append((c, hist))
    return v, hits, frames


def test_static_camera_the_length_counts_up_to_max_history_and_stays(static_chain):
    _, _, frames = static_chain
    for k, (_, hist) in enumerate(frames):
        assert (hist[:, 3] == F(min(k + 1, STATIC_MAX_HISTORY))).all(), k


def test_static_camera_the_colour_is_the_running_mean_within_the_bilinear_rounding(static_chain):
    """fx is x only to rounding: sx, u and fx carry about 8 float32 roundings of values up to W', so |fx - x| <= e = 8 * 2^-24 * W' pixels, and a
    pixel gives at most 2 e of its weight (x and y) to neighbours whose colour differs by at most 1 (the colours are in [0, 1)).  The error is
    carried from frame to frame with weight below 1, so after N frames it is at most 2 e N, plus N roundings of the blend itself (2^-23 each):
    for W' = 33 and N = 40 that is 1.3e-3.  Measured on the reference: 7.0e-6 -- the margin is what the rounding
    argument allows, not what this plane happens to need."""
    (W, _), N = STATIC_SIZE, STATIC_FRAMES
    bound = 2.0 * (8 * 2.0 ** -24 * W) * N + N * 2.0 ** -23
    assert 1.2e-3 < bound < 1.4e-3
    _, _, frames = static_chain
    mean = np.zeros((len(frames[0][0]), 3), np.float64)
    worst = 0.0
    for k, (c, hist) in enumerate(frames):
        n = min(k + 1, STATIC_MAX_HISTORY)
        mean = mean + (c.astype(np.float64) - mean) / n                          # the running mean with the length clamped, in float64
        worst = max(worst, float(np.abs(hist[:, :3].astype(np.float64) - mean).max()))
    print("static camera: worst |history - running mean| =", worst, "bound", bound)
    assert worst <= bound


def test_mismatch_behind_outside_and_no_previous_frame_restart_at_length_one(abi):
    W, H = 33, 9
    case = RC.build(abi, (W, H), (W, H), crafted=False)                         # the plane seen by the two cameras, nothing crafted
    c = case["color_cur"]
    kept = RC.reference(case)
    assert (kept[:, 3] > 1).sum() > W * H // 2                                  # (as the case stands most pixels keep their history)
    restart = np.concatenate([c, np.ones((W * H, 1), F)], axis=1)
    # no previous frame: {c, 1} everywhere
    assert_same_bits_nan_folded(RR.reproject(case["cur"], None, case["hits_cur"], c), restart, "prev NULL")
    # every previous primitive another one
    other = case["hits_prev"].copy()
    other["primitive"] = np.where(other["primitive"] == RC.NO_HIT, RC.NO_HIT, other["primitive"] + 100)
    assert_same_bits_nan_folded(RR.reproject(case["cur"], case["prev"], case["hits_cur"], c, other, case["hist_prev"], case["params"]), restart, "primitive mismatch")
    # the previous camera turned away: every point is behind it
    away = RC.view(abi, RC.camera(abi, (0, 0, -1), (0, 0, -1), (-1, 0, 0), (0, 1, 0), 1.0, 1.0), W, H)
    ok, _, _, z = RR.project(case["hits_cur"]["position"], away)
    assert not ok.any() and (z[case["hits_cur"]["primitive"] != RC.NO_HIT] < 0).any()
    assert_same_bits_nan_folded(RR.reproject(case["cur"], away, case["hits_cur"], c, case["hits_prev"], case["hist_prev"], case["params"]), restart, "behind prev")
    # the previous camera looking past the plane's patch: every point one pixel and more outside its frame
    past = RC.view(abi, RC.camera(abi, (50, 0, -1), (0, 0, 1), (1, 0, 0), (0, 1, 0), 1.0, 1.0), W, H)
    ok, fx, _, z = RR.project(case["hits_cur"]["position"], past)
    hit = case["hits_cur"]["primitive"] != RC.NO_HIT
    assert not ok.any() and (z[hit] > 0).any() and (fx[hit & (z > 0)] <= -1).all()
    assert_same_bits_nan_folded(RR.reproject(case["cur"], past, case["hits_cur"], c, case["hits_prev"], case["hist_prev"], case["params"]), restart, "outside prev")


@pytest.mark.parametrize("max_history", RC.MAX_HISTORY)
def test_the_crafted_records_sit_on_their_boundaries(max_history, abi):
    (cur_size, (Wp, Hp)) = RC.EDGE_SIZES
    case = RC.build(abi, cur_size, (Wp, Hp), max_history)
    names = [p[0] for p in case["placed"]]
    edges = [f"{ax} {what}" for ax, dim in (("fx", "W'"), ("fy", "H'")) for what in ("== -1", "just inside -1", "== " + dim, "just inside " + dim)]
    assert names == [i[0] for i in RC.items(max_history)] + edges                # every crafted item fits this pair
    assert len(RC.build(abi, (33, 9), (20, 7), max_history)["placed"]) == len(RC.items(max_history))    # 1 / 20 is no float32: no edge to land on
    out = RC.reference(case)
    ok, fx, fy, _ = RR.project(case["hits_cur"]["position"], case["prev"])
    for name, j, q, keeps in case["placed"]:
        if q is not None:
            if name not in ("z == 0", "z < 0", "NaN position"):
                assert ok[j] and fx[j] == q % Wp and fy[j] == q // Wp, name     # exactly ON previous pixel q: one counted tap
            if max_history > 1:                                                 # (with max_history 1 every length is 1)
                assert (out[j, 3] != 1.0) == keeps, (name, out[j])
            if keeps and name == "length inf":
                assert out[j, 3] == max_history
            if keeps and name == "length 1":
                assert out[j, 3] == min(2, max_history)
            if not keeps:
                assert out[j].tobytes() == np.array([*case["color_cur"][j], 1.0], F).tobytes(), name
    by = {p[0]: p[1] for p in case["placed"]}
    for c, ax, dim, size in ((fx, "fx", "W'", Wp), (fy, "fy", "H'", Hp)):
        lo, lo_in, hi, hi_in = (by[f"{ax} {what}"] for what in ("== -1", "just inside -1", "== " + dim, "just inside " + dim))
        assert c[lo] == -1 and not ok[lo] and c[hi] == size and not ok[hi]
        assert ok[lo_in] and -1 < c[lo_in] < -0.9999 and ok[hi_in] and size - 0.0001 < c[hi_in] < size
    # a NaN colour is in this frame's output and is dropped by the next frame, which restarts from its own colour
    j = by["colour NaN"]
    assert np.isnan(out[j, 0]) and np.isinf(out[j, 2]) and np.isfinite(out[j, 1])
    again = RR.reproject(case["cur"], case["cur"], case["hits_cur"], np.full_like(case["color_cur"], 0.5), case["hits_cur"], out, case["params"])
    assert np.isfinite(again[:, :3]).all()
    assert again[j].tobytes() == np.array([0.5, 0.5, 0.5, 1.0], F).tobytes()


# ---- 5: quality on the oracle's frames -----------------------------------------------------------------------------------------------------------
Q_W, Q_H, Q_FRAMES, Q_DEPTH, Q_REF_SPP, Q_STEP_DEG = 64, 48, 8, 8, 256, 0.5


def oracle_hits(oracle_mod, abi, sc, cam, W, H):
    """mi355rt_hit records from oracle.scene_hit along the pixel centres' rays.  `primitive` holds the material index the oracle reports: coarser
    than the primitive index, and enough for a scene whose walls differ in material or in plane."""
    import view_cases as VC
    rays = VC.pinhole_rays(oracle_mod, abi, cam, W, H, 0, 0, centre=True)
    out = np.zeros(W * H, abi.HIT_DTYPE)
    out["t"], out["primitive"], out["material"] = np.inf, RC.NO_HIT, RC.NO_HIT
    origin = np.array(list(cam.position), F)
    for i, d in enumerate(rays["direction"]):
        hit, r = oracle_mod.scene_hit(sc, origin, d)
        if hit:
            out[i]["position"], out[i]["normal"], out[i]["t"] = r[0:3], r[3:6], r[6]
            out[i]["primitive"] = out[i]["material"] = int(r[7])
            out[i]["front_face"] = int(r[8])
    return out


def test_reprojected_frames_of_an_orbit_are_closer_to_the_converged_image_than_raw_ones(native, oracle_mod, abi):
    """cornell at 64 x 48, 8 frames of 1 spp (depth 8, seed = frame number) along an orbit of 0.5 degrees a frame, all on the CPU: the RMSE of the
    last reprojected frame against the oracle's 256-spp image of the last camera is below the last raw frame's.  Measured when the case was
    written: raw 0.705, reprojected 0.241 (the test prints both)."""
    from oracle import scene_loader
    host, _ = native
    sc = host.LoadedScene(SCENES["cornell"], Q_W, Q_H, 1, Q_DEPTH)
    fov = float(np.degrees(2.0 * np.arctan(sc.camera.half_height)))
    aspect = sc.camera.half_width / sc.camera.half_height
    hist = hits_prev = view_prev = None
    for k in range(Q_FRAMES):
        cam = RC.orbit_camera(sc.camera, k, Q_STEP_DEG, scene_loader, fov, aspect)
        v = abi.View.make(cam, Q_W, Q_H, abi.VIEW_PINHOLE, abi.VIEW_CENTRE)
        _, raw, _ = oracle_mod.render(sc, cam, abi.Settings(Q_W, Q_H, 1, Q_DEPTH), abi.Options.make(seed=k), threads=oracle_threads())
        hits = oracle_hits(oracle_mod, abi, sc, cam, Q_W, Q_H)
        hist = RR.reproject(v, view_prev, hits, raw.reshape(-1, 3), hits_prev, hist)
        hits_prev, view_prev = hits, v
    _, want, _ = oracle_mod.render(sc, cam, abi.Settings(Q_W, Q_H, Q_REF_SPP, Q_DEPTH), abi.Options.make(seed=1000), threads=oracle_threads())
    rmse = lambda a: float(np.sqrt(np.mean((np.asarray(a, np.float64).reshape(-1, 3) - want.reshape(-1, 3).astype(np.float64)) ** 2)))
    raw_rmse, rep_rmse = rmse(raw), rmse(hist[:, :3])
    print(f"orbit quality: raw {raw_rmse:.4f} reprojected {rep_rmse:.4f}; mean history length {float(hist[:, 3].mean()):.2f}")
    assert np.isfinite(raw_rmse) and np.isfinite(rep_rmse)
    assert rep_rmse < raw_rmse
    assert float(hist[:, 3].mean()) > 4.0                                         # most pixels kept their history over the 8 frames
