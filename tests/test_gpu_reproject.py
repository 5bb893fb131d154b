"""mi355rt_post_reproject (libmi355rt_post.so, include/mi355rt_post.h) on the GPU against tests/reproject_ref.py, the numpy restatement of the
header's definition: d_hist_out, d_out_linear and d_out_packed bit for bit (NaNs folded), every buffer wrapped in guard bytes that keep
their pattern.  Synthetic records on the decision boundaries (tests/reproject_cases.py), every size at which the tiling takes another path, the
lengths' clamp, and a real chain: first hits and 2-spp colour of three cameras of an orbit made on the device, three frames in ping-pong, then
the denoiser on the result."""
import numpy as np
import pytest

import denoise_ref
import reproject_cases as RC
import reproject_ref as RR
from conftest import load_for_both, pkg
from device_buffers import Guarded
from parity import assert_same_bits_nan_folded

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope="module")
def post():
    pkg("build").build_post()
    return pkg("post")


# ---- device plumbing ------------------------------------------------------------------------------------------------------------------
def run(post, case, linear=True, packed=True, alias=False, prev=True, stream=None, sync=True):
    """One call on the case's records.  (hist float32 [n, 4], linear float32 [n, 3] or None, packed uint32 [n] or None), the guards checked: of the
    outputs AND of the inputs (the call writes nothing but its outputs)."""
    import torch
    n, n_prev = case["cur"].width * case["cur"].height, case["prev"].width * case["prev"].height
    hits_cur, color = Guarded(n * 48, case["hits_cur"]), Guarded(n * 12, case["color_cur"])
    hits_prev, hist_prev = Guarded(n_prev * 48, case["hits_prev"]), Guarded(n_prev * 16, case["hist_prev"])
    hist_out, lin, pk = Guarded(n * 16), Guarded(n * 12), Guarded(n * 4)
    post.reproject(case["cur"], case["prev"] if prev else None, hits_cur.ptr, color.ptr, hits_prev.ptr if prev else None, hist_prev.ptr if prev else None, hist_out.ptr,
                   (color.ptr if alias else lin.ptr) if linear else None, pk.ptr if packed else None, case["params"], 0, stream)
    if sync:
        torch.cuda.synchronize()
    assert hits_cur.read(np.uint8, "hits_cur").tobytes() == case["hits_cur"].tobytes() and hits_prev.read(np.uint8, "hits_prev").tobytes() == case["hits_prev"].tobytes()
    assert hist_prev.read(np.uint8, "hist_prev").tobytes() == np.ascontiguousarray(case["hist_prev"]).tobytes()
    got_lin = (color if alias else lin).read(F, "out_linear").reshape(-1, 3) if linear else None
    if not alias:
        assert color.read(np.uint8, "color_cur").tobytes() == np.ascontiguousarray(case["color_cur"]).tobytes()
    if not linear or alias:
        assert lin.untouched()
    if not packed:
        assert pk.untouched()
    return hist_out.read(F, "hist_out").reshape(-1, 4), got_lin, pk.read(np.uint32, "out_packed") if packed else None


def assert_is_reference(got, want, what):
    hist, lin, pk = got
    assert_same_bits_nan_folded(hist, want, f"{what}: hist_out")
    if lin is not None:
        assert_same_bits_nan_folded(lin, want[:, :3], f"{what}: out_linear")
    if pk is not None:
        assert pk.tobytes() == RR.packed_of(want[:, :3]).tobytes(), f"{what}: out_packed"


_cases = {}


def synthetic(abi, cur_size, prev_size, max_history=32):
    """The case and its reference: computed once, shared, read-only."""
    key = (cur_size, prev_size, max_history)
    if key not in _cases:
        case = RC.build(abi, cur_size, prev_size, max_history)
        want = RC.reference(case)
        for a in (case["hits_cur"], case["color_cur"], case["hits_prev"], case["hist_prev"], want):
            a.setflags(write=False)
        _cases[key] = (case, want)
    return _cases[key]


# ---- 1: synthetic records, every size ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cur_size,prev_size", RC.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_synthetic_records_are_the_reference_bit_for_bit(cur_size, prev_size, native, post, abi):
    case, want = synthetic(abi, cur_size, prev_size)
    assert_is_reference(run(post, case), want, f"{cur_size} from {prev_size}")
    if cur_size[0] * cur_size[1] > 15:
        assert (want[:, 3] > 1).any() and (want[:, 3] == 1).any()                # both ways out are taken
    # no previous frame: {c, 1}
    restart = np.concatenate([case["color_cur"], np.ones((len(want), 1), F)], axis=1)
    assert_is_reference(run(post, case, prev=False), restart, f"{cur_size} without prev")


@pytest.mark.parametrize("max_history", RC.MAX_HISTORY)
def test_the_boundaries_and_the_lengths_clamp(max_history, native, post, abi):
    """The pair on which every crafted record fits (tests/test_reproject_cpu.py checks that each sits exactly on its boundary)."""
    case, want = synthetic(abi, *RC.EDGE_SIZES, max_history)
    assert len(case["placed"]) == len(RC.items(max_history)) + 8
    assert want[:, 3].max() <= max_history and (max_history == 1 or want[:, 3].max() > 1)
    assert_is_reference(run(post, case), want, f"max_history {max_history}")


# ---- 2: the outputs ------------------------------------------------------------------------------------------------------------------------
def test_aliasing_the_colour_and_each_output_alone_give_the_same_bytes(native, post, abi):
    case, want = synthetic(abi, (70, 17), (70, 17))
    assert_is_reference(run(post, case, alias=True), want, "d_out_linear == d_color_cur")
    assert_is_reference(run(post, case, linear=True, packed=False), want, "linear alone")
    assert_is_reference(run(post, case, linear=False, packed=True), want, "packed alone")
    assert_is_reference(run(post, case, linear=False, packed=False), want, "history alone")


# ---- 3: the real chain ---------------------------------------------------------------------------------------------------------------------
CHAIN_W, CHAIN_H, CHAIN_SPP, CHAIN_DEPTH, CHAIN_STEP_DEG = 64, 48, 2, 6, 2.0


@pytest.mark.parametrize("name", ["cornell", "teapot"])
def test_three_frames_of_an_orbit_in_ping_pong_then_the_denoiser(name, native, oracle_mod, post, abi):
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
        hist = [Guarded(n * 16), Guarded(n * 16)]
        hits = [Guarded(n * 48), Guarded(n * 48)]
        views = [None, None]
        want_hist = want_hits = None
        kept = 0
        for k in range(3):
            cam = RC.orbit_camera(sc.camera, k, CHAIN_STEP_DEG, scene_loader, fov, aspect)
            v = abi.View.make(cam, W, H, abi.VIEW_PINHOLE, abi.VIEW_CENTRE)
            me, other = k & 1, (k & 1) ^ 1
            views[me] = v
            rays, accum, colour, packed = Guarded(n * 32), Guarded(n * 16), Guarded(n * 12), Guarded(n * 4)
            scratch = Guarded(device.view_scratch_bytes(v, CHAIN_SPP))
            ctx.view_rays(v, 0, rays.ptr)
            ctx.trace_rays(rays.ptr, n, hits[me].ptr)
            jittered = abi.View.make(cam, W, H, abi.VIEW_PINHOLE)
            ctx.render_view(jittered, abi.RadianceParams.make(0, CHAIN_SPP, CHAIN_DEPTH, seed=k), accum.ptr, scratch.ptr, colour.ptr)
            out_lin = Guarded(n * 12)
            post.reproject(v, views[other] if k else None, hits[me].ptr, colour.ptr, hits[other].ptr if k else None, hist[other].ptr if k else None, hist[me].ptr,
                           out_lin.ptr, packed.ptr)
            torch.cuda.synchronize()
            ctx.check()
            got_hits, got_colour = hits[me].read(abi.HIT_DTYPE, "hits"), colour.read(F, "colour").reshape(-1, 3)
            assert (got_hits["primitive"] != abi.NO_HIT).any() and np.isfinite(got_colour).all()
            want = RR.reproject(v, views[other] if k else None, got_hits, got_colour, want_hits, want_hist)      # the reference, fed the device-made inputs
            assert_is_reference((hist[me].read(F, "hist_out").reshape(-1, 4), out_lin.read(F, "out_linear").reshape(-1, 3), packed.read(np.uint32, "out_packed")), want,
                                f"{name} frame {k}")
            kept += int((want[:, 3] > 1).sum())
            want_hist, want_hits = want, got_hits
        assert kept > n // 2 and want[:, 3].max() == 3                           # the orbit is small enough for most pixels to keep their history
        # ... and the denoiser on the result, guided by the current records: the header's filter of the reference's image
        params = abi.DenoiseParams.make(levels=2)
        dn_scratch, dn_out = Guarded(device.denoise_scratch_bytes(W, H)), Guarded(n * 12)
        ctx.denoise(W, H, out_lin.ptr, hits[me].ptr, dn_scratch.ptr, dn_out.ptr, None, params)
        torch.cuda.synchronize()
        ctx.check()
        filtered = denoise_ref.denoise(want[:, :3].reshape(H, W, 3), got_hits, levels=2)
        assert_same_bits_nan_folded(dn_out.read(F, "denoised").reshape(H, W, 3), filtered, f"{name}: denoised")
    finally:
        ctx.close()


# ---- 4: beside other work --------------------------------------------------------------------------------------------------------------------
def test_on_a_second_stream_beside_a_render_view_of_another_context(native, oracle_mod, post, abi):
    import torch
    host, device = native
    case, want = synthetic(abi, (70, 17), (70, 17))
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
        s_render, s_post = torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()
        beside = render(s_render.cuda_stream)
        n, n_prev = len(want), len(case["hist_prev"])
        bufs = [Guarded(n * 48, case["hits_cur"]), Guarded(n * 12, case["color_cur"]), Guarded(n_prev * 48, case["hits_prev"]), Guarded(n_prev * 16, case["hist_prev"]),
                Guarded(n * 16), Guarded(n * 12), Guarded(n * 4)]
        torch.cuda.synchronize()
        again = render(s_render.cuda_stream)
        post.reproject(case["cur"], case["prev"], *(b.ptr for b in bufs), case["params"], 0, s_post.cuda_stream)
        torch.cuda.synchronize()
        ctx.check()
        assert_is_reference((bufs[4].read(F, "hist_out").reshape(-1, 4), bufs[5].read(F, "out_linear").reshape(-1, 3), bufs[6].read(np.uint32, "out_packed")), want, "second stream")
        assert again[1].read(F, "render_view").tobytes() == want_lin.tobytes() and beside[1].read(F, "render_view").tobytes() == want_lin.tobytes()
    finally:
        ctx.close()


# ---- 5: refusals on a live device ------------------------------------------------------------------------------------------------------------
def test_refusals_on_a_live_device_leave_the_outputs_untouched(native, post, abi):
    import torch
    case, _ = synthetic(abi, (33, 9), (20, 7))
    n, n_prev = 33 * 9, 20 * 7
    hits_cur, color = Guarded(n * 48, case["hits_cur"]), Guarded(n * 12, case["color_cur"])
    hits_prev, hist_prev = Guarded(n_prev * 48, case["hits_prev"]), Guarded(n_prev * 16, case["hist_prev"])
    hist_out, lin, pk = Guarded(n * 16), Guarded(n * 12), Guarded(n * 4)

    def refused(word, cur=case["cur"], prev=case["prev"], params=case["params"], hc=hits_cur.ptr, cc=color.ptr, hp=hits_prev.ptr, mp=hist_prev.ptr, ho=hist_out.ptr,
                ol=lin.ptr, op=pk.ptr, dev=0):
        with pytest.raises(post.RenderError) as e:
            post.reproject(cur, prev, hc, cc, hp, mp, ho, ol, op, params, dev)
        assert e.value.rc == abi.ERR_INVALID and word in str(e.value), (word, str(e.value))

    bad = RC.view(abi, RC.canonical(abi), 20, 7); bad.model = 2
    refused("prev.model", prev=bad)
    bad = RC.view(abi, RC.canonical(abi), 33, 9); bad.camera.position[2] = float("inf")
    refused("cur.camera", cur=bad)
    refused("cur is null", cur=None)
    refused("params.max_history", params=abi.ReprojectParams.make(0))
    refused("params.flags", params=abi.ReprojectParams.make(flags=2))
    refused("params.normal_min", params=abi.ReprojectParams.make(normal_min=2.0))
    refused("params.plane_tolerance", params=abi.ReprojectParams.make(plane_tolerance=0.0))
    refused("d_hits_cur must be 16-byte", hc=hits_cur.ptr + 8)
    refused("d_hist_out must be 16-byte", ho=hist_out.ptr + 4)
    refused("d_out_linear must be 4-byte", ol=lin.ptr + 2)
    refused("d_out_packed must be 4-byte", op=pk.ptr + 1)
    refused("d_hist_prev is null", mp=None)
    refused("given without prev", prev=None)
    refused("d_hist_out must not be d_hist_prev", ho=hist_prev.ptr)
    refused("hip_device", dev=-1)
    with pytest.raises(post.RenderError) as e:
        post.reproject(case["cur"], case["prev"], hits_cur.ptr, color.ptr, hits_prev.ptr, hist_prev.ptr, hist_out.ptr, lin.ptr, pk.ptr, case["params"], 1 << 20)
    assert e.value.rc == abi.ERR_NO_DEVICE and "out of range" in str(e.value)
    torch.cuda.synchronize()
    assert hist_out.untouched() and lin.untouched() and pk.untouched()       # nothing was enqueued
    assert hist_prev.read(np.uint8, "hist_prev").tobytes() == np.ascontiguousarray(case["hist_prev"]).tobytes()
