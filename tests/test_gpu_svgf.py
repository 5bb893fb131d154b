"""mi355rt_svgf_accumulate and mi355rt_svgf_filter (libmi355rt_svgf.so, include/mi355rt_svgf.h) on the GPU against tests/svgf_ref.py, the numpy
restatement of the header's definitions: every output bit for bit (NaNs folded), every buffer wrapped in guard bytes that keep their pattern, the
inputs unchanged.  Synthetic records on the decision boundaries (tests/svgf_cases.py), every size at which the tiling takes another path, the
clamps of the lengths, each level form of the filter, and a real chain: first hits and 2-spp colour of three cameras of an orbit made on the device,
three frames in ping-pong through accumulate and filter."""
import numpy as np
import pytest

import reproject_cases as RC
import svgf_cases as SC
import svgf_ref as SR
from conftest import load_for_both, pkg
from device_buffers import Guarded
from parity import assert_same_bits_nan_folded

pytestmark = pytest.mark.gpu

F = np.float32
CUR_SIZES = [(1, 1), (5, 3), (33, 9), (70, 17)]         # one pixel; no multiple of the 32 x 8 tile; one past the tile in each direction; several tiles with ragged edges
LEVELS = [0, 1, 2, 3, 5]                                # the copy, each staged step, the first gathered step, the default


@pytest.fixture(scope="module")
def svgf():
    pkg("build").build_svgf()
    return pkg("svgf")


@pytest.fixture(scope="module")
def post():
    pkg("build").build_post()
    return pkg("post")


# ---- device plumbing ------------------------------------------------------------------------------------------------------------------
class AccumulateBuffers:
    def __init__(self, case):
        n, n_prev = case["cur"].width * case["cur"].height, case["prev"].width * case["prev"].height
        self.case, self.n = case, n
        self.inputs = [("hits_cur", Guarded(n * 48, case["hits_cur"])), ("color_cur", Guarded(n * 12, case["color_cur"])),
                       ("hits_prev", Guarded(n_prev * 48, case["hits_prev"])), ("hist_prev", Guarded(n_prev * 16, case["hist_prev"])),
                       ("moments_prev", Guarded(n_prev * 8, case["moments_prev"]))]
        self.hist, self.moments, self.variance = Guarded(n * 16), Guarded(n * 8), Guarded(n * 4)

    def call(self, svgf, prev=True, stream=None):
        hc, cc, hp, mp, mmp = (b.ptr for _, b in self.inputs)
        if not prev:
            hp = mp = mmp = None
        svgf.accumulate(self.case["cur"], self.case["prev"] if prev else None, hc, cc, hp, mp, mmp, self.hist.ptr, self.moments.ptr, self.variance.ptr,
                        self.case["params"], 0, stream)

    def read(self):
        """(hist [n, 4], moments [n, 2], variance [n]) after checking every guard and that no input changed."""
        for name, b in self.inputs:
            assert b.read(np.uint8, name).tobytes() == np.ascontiguousarray(self.case[name]).tobytes(), f"{name} was written"
        return self.hist.read(F, "hist_out").reshape(-1, 4), self.moments.read(F, "moments_out").reshape(-1, 2), self.variance.read(F, "variance_out")


def run_accumulate(svgf, case, prev=True):
    import torch
    b = AccumulateBuffers(case)
    b.call(svgf, prev)
    torch.cuda.synchronize()
    return b.read()


def assert_is_accumulate(got, want, what):
    for g, w, name in zip(got, want[:3], ("hist_out", "moments_out", "variance_out")):
        assert_same_bits_nan_folded(g, w, f"{what}: {name}")


def run_filter(svgf, abi, W, H, hist, variance, hits, linear=True, packed=True, stream=None, **params):
    """(out_linear [H, W, 3] or None, out_packed [n] or None), the guards of the outputs, of the scratch and of the inputs checked."""
    import torch
    n = W * H
    d_hist, d_var, d_hits = Guarded(n * 16, hist), Guarded(n * 4, variance), Guarded(n * 48, hits)
    scratch, lin, pk = Guarded(svgf.scratch_bytes(W, H)), Guarded(n * 12), Guarded(n * 4)
    svgf.filter(W, H, d_hist.ptr, d_var.ptr, d_hits.ptr, scratch.ptr, lin.ptr if linear else None, pk.ptr if packed else None, abi.SvgfFilterParams.make(**params), 0, stream)
    torch.cuda.synchronize()
    scratch.read(np.uint8, "scratch")
    assert d_hist.read(np.uint8, "hist_in").tobytes() == np.ascontiguousarray(hist).tobytes() and d_var.read(np.uint8, "variance_in").tobytes() == np.ascontiguousarray(variance).tobytes()
    assert d_hits.read(np.uint8, "hits").tobytes() == hits.tobytes()
    if not linear:
        assert lin.untouched()
    if not packed:
        assert pk.untouched()
    return lin.read(F, "out_linear").reshape(H, W, 3) if linear else None, pk.read(np.uint32, "out_packed") if packed else None


def assert_is_filter(got, want, what):
    lin, pk = got
    if lin is not None:
        assert_same_bits_nan_folded(lin, want, f"{what}: out_linear")
    if pk is not None:
        assert pk.tobytes() == SR.packed_of(want.reshape(-1, 3)).tobytes(), f"{what}: out_packed"


_cases = {}


def synthetic(abi, cur_size, prev_size, max_history=32, min_temporal=4):
    """The case and its reference (with and without a previous frame): computed once, shared, read-only."""
    key = (cur_size, prev_size, max_history, min_temporal)
    if key not in _cases:
        case = SC.build(abi, cur_size, prev_size, max_history, min_temporal)
        want, restart = SC.reference(case), SC.reference(case, prev=False)
        for a in (case["hits_cur"], case["color_cur"], case["hits_prev"], case["hist_prev"], case["moments_prev"], *want, *restart):
            a.setflags(write=False)
        _cases[key] = (case, want, restart)
    return _cases[key]


_filtered = {}


def filtered(abi, cur_size, levels):
    """The reference's filter of the synthetic case's accumulate outputs at `levels`: computed once, shared, read-only."""
    key = (cur_size, levels)
    if key not in _filtered:
        case, want, _ = synthetic(abi, cur_size, cur_size)
        out = SR.filter(want[0], want[2], case["hits_cur"], *cur_size, levels=levels)
        out.setflags(write=False)
        _filtered[key] = out
    return _filtered[key]


# ---- 1: accumulate, synthetic records --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cur_size,prev_size", RC.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_accumulate_is_the_reference_bit_for_bit(cur_size, prev_size, native, svgf, abi):
    case, want, restart = synthetic(abi, cur_size, prev_size)
    assert_is_accumulate(run_accumulate(svgf, case), want, f"{cur_size} from {prev_size}")
    if cur_size[0] * cur_size[1] > 64:
        assert len(np.unique(want[3])) == 5                                       # every way out is taken
    assert_is_accumulate(run_accumulate(svgf, case, prev=False), restart, f"{cur_size} without prev")


@pytest.mark.parametrize("max_history,min_temporal", [(1, 1), (2, 1), (65535, 1), (65535, 4)])
def test_the_clamp_of_the_lengths_and_min_temporal(max_history, min_temporal, native, svgf, abi):
    """The pair on which every crafted record fits."""
    case, want, _ = synthetic(abi, *RC.EDGE_SIZES, max_history, min_temporal)
    assert len(case["added"]) == len(SC.items(min_temporal))
    assert want[0][:, 3].max() <= max_history and (min_temporal > 1 or not (want[3] == SR.SPATIAL_SHORT).any())
    assert_is_accumulate(run_accumulate(svgf, case), want, f"max_history {max_history} min_temporal {min_temporal}")


def test_hist_out_is_what_the_reprojection_writes_on_the_same_buffers(native, svgf, post, abi):
    import torch
    case, _, _ = synthetic(abi, (70, 17), (70, 17))
    b = AccumulateBuffers(case)
    b.call(svgf)
    hc, cc, hp, mp, _ = (buf.ptr for _, buf in b.inputs)
    rep = Guarded(b.n * 16)
    post.reproject(case["cur"], case["prev"], hc, cc, hp, mp, rep.ptr, None, None, case["reproject_params"])
    torch.cuda.synchronize()
    assert b.read()[0].tobytes() == rep.read(F, "reproject's hist_out").reshape(-1, 4).tobytes()


# ---- 2: filter -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", LEVELS)
@pytest.mark.parametrize("cur_size", CUR_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_filter_is_the_reference_bit_for_bit_in_both_forms(cur_size, levels, native, svgf, abi):
    case, want, _ = synthetic(abi, cur_size, cur_size)
    W, H = cur_size
    out = filtered(abi, cur_size, levels)
    assert_is_filter(run_filter(svgf, abi, W, H, want[0], want[2], case["hits_cur"], levels=levels), out, f"{cur_size} levels {levels}")
    assert_is_filter(run_filter(svgf, abi, W, H, want[0], want[2], case["hits_cur"], levels=levels, flags=abi.SVGF_GATHERS_ONLY), out, f"{cur_size} levels {levels}, gathers only")


def test_each_filter_output_alone_gives_the_same_bytes(native, svgf, abi):
    case, want, _ = synthetic(abi, (70, 17), (70, 17))
    for levels in (0, 2):
        out = filtered(abi, (70, 17), levels)
        assert_is_filter(run_filter(svgf, abi, 70, 17, want[0], want[2], case["hits_cur"], packed=False, levels=levels), out, f"linear alone, levels {levels}")
        assert_is_filter(run_filter(svgf, abi, 70, 17, want[0], want[2], case["hits_cur"], linear=False, levels=levels), out, f"packed alone, levels {levels}")


# ---- 3: the real chain ---------------------------------------------------------------------------------------------------------------------
CHAIN_W, CHAIN_H, CHAIN_SPP, CHAIN_DEPTH, CHAIN_STEP_DEG = 64, 48, 2, 6, 2.0


@pytest.mark.parametrize("name", ["cornell", "teapot"])
def test_three_frames_of_an_orbit_in_ping_pong_through_accumulate_and_filter(name, native, oracle_mod, svgf, abi):
    import torch
    from oracle import scene_loader
    host, device = native
    W, H, n = CHAIN_W, CHAIN_H, CHAIN_W * CHAIN_H
    sc = load_for_both(name, oracle_mod, host, width=W, height=H, spp=CHAIN_SPP, max_depth=CHAIN_DEPTH)
    fov = float(np.degrees(2.0 * np.arctan(sc.camera.half_height)))
    aspect = sc.camera.half_width / sc.camera.half_height
    ctx = device.Context(0)
    try:
        ctx.set_scene(sc, sc.camera, abi.Settings(W, H, CHAIN_SPP, CHAIN_DEPTH))
        hist, moments, hits = ([Guarded(n * size), Guarded(n * size)] for size in (16, 8, 48))     # the three buffers that ping-pong
        views = [None, None]
        want = want_hits = None
        temporal = 0
        params = abi.SvgfAccumulateParams.make(min_temporal=2)                    # three frames: a length of 2 is reached in the second
        for k in range(3):
            cam = RC.orbit_camera(sc.camera, k, CHAIN_STEP_DEG, scene_loader, fov, aspect)
            v = abi.View.make(cam, W, H, abi.VIEW_PINHOLE, abi.VIEW_CENTRE)
            me, other = k & 1, (k & 1) ^ 1
            views[me] = v
            rays, accum, colour = Guarded(n * 32), Guarded(n * 16), Guarded(n * 12)
            scratch = Guarded(device.view_scratch_bytes(v, CHAIN_SPP))
            ctx.view_rays(v, 0, rays.ptr)
            ctx.trace_rays(rays.ptr, n, hits[me].ptr)
            ctx.render_view(abi.View.make(cam, W, H, abi.VIEW_PINHOLE), abi.RadianceParams.make(0, CHAIN_SPP, CHAIN_DEPTH, seed=k), accum.ptr, scratch.ptr, colour.ptr)
            variance, out_lin, packed, f_scratch = Guarded(n * 4), Guarded(n * 12), Guarded(n * 4), Guarded(svgf.scratch_bytes(W, H))
            svgf.accumulate(v, views[other] if k else None, hits[me].ptr, colour.ptr, hits[other].ptr if k else None, hist[other].ptr if k else None,
                            moments[other].ptr if k else None, hist[me].ptr, moments[me].ptr, variance.ptr, params)
            svgf.filter(W, H, hist[me].ptr, variance.ptr, hits[me].ptr, f_scratch.ptr, out_lin.ptr, packed.ptr)
            torch.cuda.synchronize()
            ctx.check()
            got_hits, got_colour = hits[me].read(abi.HIT_DTYPE, "hits"), colour.read(F, "colour").reshape(-1, 3)
            assert (got_hits["primitive"] != abi.NO_HIT).any() and np.isfinite(got_colour).all()
            prev_out = want
            want = SR.accumulate(v, views[other] if k else None, got_hits, got_colour, want_hits, *(prev_out[:2] if k else (None, None)), params)   # the reference, fed the device-made inputs
            got = (hist[me].read(F, "hist_out").reshape(-1, 4), moments[me].read(F, "moments_out").reshape(-1, 2), variance.read(F, "variance_out"))
            assert_is_accumulate(got, want, f"{name} frame {k}")
            f_scratch.read(np.uint8, "filter scratch")
            assert_is_filter((out_lin.read(F, "out_linear").reshape(H, W, 3), packed.read(np.uint32, "out_packed")), SR.filter(want[0], want[2], got_hits, W, H), f"{name} frame {k}")
            temporal += int((want[3] == SR.TEMPORAL).sum())
            want_hits = got_hits
        assert temporal > n // 2 and want[0][:, 3].max() == 3                     # the orbit is small enough for most pixels to keep their history
    finally:
        ctx.close()


# ---- 4: beside other work --------------------------------------------------------------------------------------------------------------------
def test_on_a_second_stream_beside_a_render_view_of_another_context(native, oracle_mod, svgf, abi):
    import torch
    host, device = native
    case, want, _ = synthetic(abi, (70, 17), (70, 17))
    W, H = 64, 48
    sc = load_for_both("cornell", oracle_mod, host, width=W, height=H, spp=16, max_depth=8)
    ctx = device.Context(0)
    try:
        ctx.set_scene(sc, sc.camera, sc.settings)
        v = abi.View.make(sc.camera, W, H, abi.VIEW_PINHOLE)
        prm = abi.RadianceParams.make(0, 16, 8, seed=3)

        def render(stream):
            accum, lin, scratch = Guarded(W * H * 16), Guarded(W * H * 12), Guarded(device.view_scratch_bytes(v, 16))
            ctx.render_view(v, prm, accum.ptr, scratch.ptr, lin.ptr, None, stream)
            return accum, lin, scratch                                           # (kept alive until the synchronise)

        solo = render(None)
        torch.cuda.synchronize()
        want_lin = solo[1].read(F, "render_view")
        s_render, s_svgf = torch.cuda.Stream(), torch.cuda.Stream()
        b = AccumulateBuffers(case)
        f_scratch, f_lin = Guarded(svgf.scratch_bytes(70, 17)), Guarded(b.n * 12)
        torch.cuda.synchronize()
        beside = render(s_render.cuda_stream)
        b.call(svgf, stream=s_svgf.cuda_stream)
        svgf.filter(70, 17, b.hist.ptr, b.variance.ptr, b.inputs[0][1].ptr, f_scratch.ptr, f_lin.ptr, None, None, 0, s_svgf.cuda_stream)
        torch.cuda.synchronize()
        ctx.check()
        assert_is_accumulate(b.read(), want, "second stream")
        assert_is_filter((f_lin.read(F, "out_linear").reshape(17, 70, 3), None), filtered(abi, (70, 17), 5), "second stream")
        assert beside[1].read(F, "render_view").tobytes() == want_lin.tobytes()
    finally:
        ctx.close()


# ---- 5: refusals on a live device ------------------------------------------------------------------------------------------------------------
def test_refusals_on_a_live_device_leave_the_outputs_untouched(native, svgf, abi):
    import torch
    case, _, _ = synthetic(abi, (33, 9), (20, 7))
    b = AccumulateBuffers(case)
    hc, cc, hp, mp, mmp = (buf.ptr for _, buf in b.inputs)
    ok = dict(cur=case["cur"], prev=case["prev"], hc=hc, cc=cc, hp=hp, mp=mp, mmp=mmp, ho=b.hist.ptr, mo=b.moments.ptr, vo=b.variance.ptr, params=case["params"], dev=0)

    def refused(word, rc=abi.ERR_INVALID, **kw):
        a = {**ok, **kw}
        with pytest.raises(svgf.RenderError) as e:
            svgf.accumulate(a["cur"], a["prev"], a["hc"], a["cc"], a["hp"], a["mp"], a["mmp"], a["ho"], a["mo"], a["vo"], a["params"], a["dev"])
        assert e.value.rc == rc and word in str(e.value), (word, str(e.value))

    bad = RC.view(abi, RC.canonical(abi), 20, 7); bad.model = 2
    refused("prev.model", prev=bad)
    refused("cur is null", cur=None)
    refused("params.max_history", params=abi.SvgfAccumulateParams.make(0, min_temporal=1))
    refused("params.min_temporal", params=abi.SvgfAccumulateParams.make(2, min_temporal=3))
    refused("params.min_temporal", params=abi.SvgfAccumulateParams.make(min_temporal=0))
    refused("params.normal_squarings", params=abi.SvgfAccumulateParams.make(normal_squarings=9))
    refused("params.sigma_plane", params=abi.SvgfAccumulateParams.make(sigma_plane=0.0))
    refused("params.reserved", params=abi.SvgfAccumulateParams.make(reserved=1))
    refused("d_moments_out must be 8-byte", mo=b.moments.ptr + 4)
    refused("d_variance_out must be 4-byte", vo=b.variance.ptr + 2)
    refused("d_moments_prev is null", mmp=None)
    refused("given without prev", prev=None)
    refused("d_hist_out must not be d_hist_prev", ho=mp)
    refused("d_moments_out must not be d_moments_prev", mo=mmp)
    refused("hip_device", dev=-1)
    refused("out of range", rc=abi.ERR_NO_DEVICE, dev=1 << 20)
    n = 33 * 9
    scratch, lin = Guarded(svgf.scratch_bytes(33, 9)), Guarded(n * 12)

    def filter_refused(word, W=33, H=9, hist=b.hist.ptr, var=b.variance.ptr, hits=hc, scr=scratch.ptr, ol=lin.ptr, op=None, dev=0, **params):
        with pytest.raises(svgf.RenderError) as e:
            svgf.filter(W, H, hist, var, hits, scr, ol, op, abi.SvgfFilterParams.make(**params), dev)
        assert e.value.rc == abi.ERR_INVALID and word in str(e.value), (word, str(e.value))

    filter_refused("width is 0", W=0)
    filter_refused("params.levels", levels=9)
    filter_refused("params.sigma_luminance", sigma_luminance=float("nan"))
    filter_refused("params.flags", flags=2)
    filter_refused("both null", ol=None)
    filter_refused("d_scratch must be 16-byte", scr=scratch.ptr + 8)
    filter_refused("d_variance_in is null", var=None)
    filter_refused("d_out_linear must not be d_hist_in", ol=b.hist.ptr, levels=0)
    filter_refused("d_out_packed must not be d_hist_in", ol=None, op=b.hist.ptr, levels=0)
    filter_refused("hip_device", dev=-1)
    with pytest.raises(svgf.RenderError) as e:
        svgf.scratch_bytes(0, 4)
    assert e.value.rc == abi.ERR_INVALID and "width is 0" in str(e.value)
    assert svgf.scratch_bytes(33, 9) == 64 * n
    torch.cuda.synchronize()
    assert b.hist.untouched() and b.moments.untouched() and b.variance.untouched() and scratch.untouched() and lin.untouched()       # nothing was enqueued
    b.read()
