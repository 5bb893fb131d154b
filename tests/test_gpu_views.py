"""Camera views on the resident scene (mi355rt_context_view_rays, mi355rt_context_render_view): the rays of a pinhole and a thin lens
made on the device, in front of the radiance queries' path loop.

The references are the numpy makers of tests/view_cases.py (bit for bit wherever a ray is + - * / sqrt), mi355rt_context_render and oracle.render
(a pinhole view IS the render), and mi355rt_context_trace_radiance called once per sample along a view's rays (render_view's definition)."""
import subprocess

import numpy as np
import pytest

import scene_shapes as SS
import view_cases as VC
from conftest import SCENES, load_for_both, pkg
from device_buffers import Guarded, RadianceBuffers, packed_of, scene_contexts
from parity import assert_same_bits_nan_folded

pytestmark = pytest.mark.gpu

F = np.float32


# ---- device plumbing ------------------------------------------------------------------------------------------------------------------
def buffers(device, view, samples=1, fill_nan=True):
    """The buffers of one view and up to `samples` samples per call, the packed words among them."""
    buf = RadianceBuffers("render_view", view.width * view.height, device.view_scratch_bytes(view, samples), packed=True, fill_nan=fill_nan)
    buf.view = view
    return buf


def render_view(ctx, abi, buf, begin, end, depth=VC.DEPTH, seed=0, stream=None, linear=True, packed=True):
    ctx.render_view(buf.view, abi.RadianceParams.make(begin, end, depth, seed), buf.accum.ptr, buf.scratch.ptr,
                    buf.linear.ptr if linear else None, buf.packed.ptr if packed else None, stream)


def one_call(device, abi, ctx, view, S, depth=VC.DEPTH, seed=0):
    import torch
    buf = buffers(device, view, S)
    render_view(ctx, abi, buf, 0, S, depth, seed)
    torch.cuda.synchronize()
    ctx.check()
    return buf.read()


@pytest.fixture(scope="module")
def scenes(native, oracle_mod, abi):
    host, _ = native
    out = {n: load_for_both(n, oracle_mod, host, width=24, height=16, spp=1, max_depth=VC.DEPTH) for n in VC.SCENES}
    out["mesh"] = SS.camera_scene(abi, host, "mesh")                      # a list with meshes and exact materials: k_view_paths_*_mesh against the oracle
    return out


@pytest.fixture(scope="module")
def contexts(native, abi, scenes):
    """One context per scene, with a view the calls never look at: a view needs no set_scene of its own."""
    yield from scene_contexts(native[1], abi, scenes)


CAM_CASES = [(n, c) for n in VC.SCENES for c in VC.CAMERAS]
ALL_SAMPLES = range(max(VC.SAMPLES))


def device_rays(device, abi, ctx, view, s, seed):
    import torch
    buf = buffers(device, view)
    ctx.view_rays(view, s, buf.rays.ptr, seed)
    torch.cuda.synchronize()
    return buf.read_rays(abi, "view_rays")


# ---- 1: pinhole rays ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cname", CAM_CASES)
def test_pinhole_rays_are_the_numpy_makers_word_for_word(name, cname, native, oracle_mod, abi, scenes, contexts):
    _, device = native
    cam = VC.camera(cname, scenes[name])
    for W, H in VC.SIZES:
        view = VC.make_view(abi, cam, W, H, abi.VIEW_PINHOLE)
        for seed in VC.SEEDS:
            for s in ALL_SAMPLES:
                got = device_rays(device, abi, contexts[name], view, s, seed)
                assert got.tobytes() == VC.pinhole_rays(oracle_mod, abi, cam, W, H, s, seed).tobytes(), (W, H, seed, s)
        centre = VC.make_view(abi, cam, W, H, abi.VIEW_PINHOLE, centre=True)
        got = device_rays(device, abi, contexts[name], centre, 3, VC.SEEDS[1])
        assert got.tobytes() == VC.pinhole_rays(oracle_mod, abi, cam, W, H, 0, 0, centre=True).tobytes(), (W, H, "centre")


# ---- 2: a pinhole view is the render ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "mesh"])
def test_the_scenes_own_camera_gives_the_render_and_a_moved_one_the_oracles(name, native, oracle_mod, abi, scenes):
    import torch
    _, device = native
    sc = scenes[name]
    depth = VC.DEPTH
    ctx = device.Context(0)
    try:
        for (W, H), S, seed in ((VC.SIZES[0], 17, VC.SEEDS[0]), (VC.SIZES[1], 5, VC.SEEDS[1]), (VC.SIZES[1], 1, VC.SEEDS[0])):
            st, opt = abi.Settings(W, H, S, depth), abi.Options.make(seed=seed)
            ctx.set_scene(sc, sc.camera, st)
            packed = torch.zeros((H, W), dtype=torch.int32, device="cuda")
            linear = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
            ctx.render(packed.data_ptr(), linear.data_ptr(), opt)
            torch.cuda.synchronize()
            ctx.check()
            _, got_linear, got_packed = one_call(device, abi, ctx, VC.make_view(abi, sc.camera, W, H, abi.VIEW_PINHOLE), S, depth, seed)
            assert got_packed.tobytes() == packed.cpu().numpy().view(np.uint32).tobytes(), (W, H, S, "packed against context_render")
            _, want, _ = oracle_mod.render(sc, sc.camera, st, opt, threads=4)
            assert_same_bits_nan_folded(got_linear.reshape(H, W, 3), want, f"{name} {W}x{H}x{S} own camera")
            assert got_packed.tobytes() == packed_of(got_linear).astype(np.uint32).tobytes()
            assert len(np.unique(got_linear, axis=0)) > 1                      # an image, not a constant
            for cname in VC.CAMERAS[1:]:                                       # the context keeps the scene's own camera: the view does not need it
                cam = VC.camera(cname, sc)
                _, got_linear, got_packed = one_call(device, abi, ctx, VC.make_view(abi, cam, W, H, abi.VIEW_PINHOLE), S, depth, seed)
                _, want, _ = oracle_mod.render(sc, cam, st, opt, threads=4)
                assert_same_bits_nan_folded(got_linear.reshape(H, W, 3), want, f"{name} {W}x{H}x{S} {cname}")
                assert got_packed.tobytes() == packed_of(got_linear).astype(np.uint32).tobytes()
    finally:
        ctx.close()


# ---- 3: the thin lens ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cname", CAM_CASES)
def test_thin_lens_rays_are_the_numpy_makers_word_for_word(name, cname, native, oracle_mod, abi, scenes, contexts):
    _, device = native
    cam = VC.camera(cname, scenes[name])
    lens = VC.lens_of(cam)
    for W, H in VC.SIZES:
        view = VC.make_view(abi, cam, W, H, abi.VIEW_THIN_LENS)
        for seed in VC.SEEDS:
            for s in ALL_SAMPLES:
                got = device_rays(device, abi, contexts[name], view, s, seed)
                assert got.tobytes() == VC.thin_lens_rays(oracle_mod, abi, cam, W, H, s, *lens, seed).tobytes(), (W, H, seed, s)
        centre = VC.make_view(abi, cam, W, H, abi.VIEW_THIN_LENS, centre=True)
        got = device_rays(device, abi, contexts[name], centre, 3, VC.SEEDS[1])
        assert got.tobytes() == VC.thin_lens_rays(oracle_mod, abi, cam, W, H, 0, *lens, centre=True).tobytes(), (W, H, "centre")
        assert got["origin"].tobytes() == VC.pinhole_rays(oracle_mod, abi, cam, W, H, 0, centre=True)["origin"].tobytes()      # no lens offset


@pytest.mark.parametrize("name,cname,size,S,seed", [("cornell", "inside", 1, 17, 0), ("cornell", "own", 0, 5, 1), ("teapot", "moved", 1, 17, 1), ("teapot", "own", 0, 1, 0)])
def test_a_thin_lens_view_is_the_radiance_query_along_the_numpy_rays(name, cname, size, S, seed, native, oracle_mod, abi, scenes, contexts):
    _, device = native
    (W, H), seed = VC.SIZES[size], VC.SEEDS[seed]
    cam = VC.camera(cname, scenes[name])
    lens = VC.lens_of(cam)
    view = VC.make_view(abi, cam, W, H, abi.VIEW_THIN_LENS)
    sums, means, packed = one_call(device, abi, contexts[name], view, S, VC.DEPTH, seed)
    want_sums, want_means = buffers(device, view).by_query(contexts[name], abi, S, lambda s: VC.thin_lens_rays(oracle_mod, abi, cam, W, H, s, *lens, seed), VC.DEPTH, seed)
    assert sums.tobytes() == want_sums.tobytes() and means.tobytes() == want_means.tobytes()
    assert packed.tobytes() == packed_of(means).astype(np.uint32).tobytes()
    assert np.isfinite(means).all() and len(np.unique(means, axis=0)) > 1


# ---- 5: chunking and K ----------------------------------------------------------------------------------------------------------------------
MODELS = ["pinhole", "thin_lens"]
_whole = {}


def model_view(abi, scenes, model, size=0):
    cam = VC.camera("inside", scenes["cornell"])
    return VC.make_view(abi, cam, *VC.SIZES[size], {"pinhole": abi.VIEW_PINHOLE, "thin_lens": abi.VIEW_THIN_LENS}[model])


def whole(device, abi, contexts, scenes, model):
    """[0, 17) of the model's 24 x 16 view inside the cornell box in one call with the default K: computed once, shared, read-only."""
    if model not in _whole:
        out = one_call(device, abi, contexts["cornell"], model_view(abi, scenes, model), 17, VC.DEPTH, VC.SEEDS[1])
        for a in out:
            a.setflags(write=False)
        _whole[model] = out
    return _whole[model]


@pytest.mark.parametrize("model", MODELS)
def test_any_chunking_gives_the_words_of_one_call(model, native, abi, scenes, contexts):
    import torch
    _, device = native
    sums, means, packed = whole(device, abi, contexts, scenes, model)
    assert np.isfinite(sums).all() and (sums[:, :3] > 0).any()             # the NaN the sums were pre-filled with was not read
    buf = buffers(device, model_view(abi, scenes, model), 11)              # the scratch is sized for the largest chunk
    for a, b in ((0, 5), (5, 16), (16, 17)):
        render_view(contexts["cornell"], abi, buf, a, b, VC.DEPTH, VC.SEEDS[1])
    torch.cuda.synchronize()
    got = buf.read()
    assert got[0].tobytes() == sums.tobytes() and got[1].tobytes() == means.tobytes() and got[2].tobytes() == packed.tobytes()


@pytest.mark.parametrize("K", [1, 2, 64])
@pytest.mark.parametrize("model", MODELS)
def test_items_per_lane_does_not_change_a_word(model, K, native, abi, scenes, contexts):
    _, device = native
    ctx = contexts["cornell"]
    want = whole(device, abi, contexts, scenes, model)                     # 384 * 17 = 6528 items: 102 waves at K = 1, 2 at K = 64
    try:
        ctx.set_knob("radiance_items", K)
        got = one_call(device, abi, ctx, model_view(abi, scenes, model), 17, VC.DEPTH, VC.SEEDS[1])
    finally:
        ctx.set_knob("radiance_items", 0)
    assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want))


# ---- 6: composition with the ray queries ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "teapot"])
def test_centre_rays_fed_to_trace_rays_are_first_hits(name, native, abi, scenes):
    import torch
    _, device = native
    sc = scenes[name]
    ctx = device.Context(0)
    try:
        for W, H in VC.SIZES:
            ctx.set_scene(sc, sc.camera, abi.Settings(W, H, 1, VC.DEPTH))
            want = torch.zeros(W * H * 48, dtype=torch.uint8, device="cuda")
            ctx.first_hits(want.data_ptr())
            view = VC.make_view(abi, sc.camera, W, H, abi.VIEW_PINHOLE, centre=True)
            buf = buffers(device, view)
            ctx.view_rays(view, 0, buf.rays.ptr)
            got = Guarded(W * H * 48)
            ctx.trace_rays(buf.rays.ptr, W * H, got.ptr)
            torch.cuda.synchronize()
            ctx.check()
            g, w = got.read(abi.HIT_DTYPE, "trace_rays: hits"), want.cpu().numpy().view(abi.HIT_DTYPE)
            assert g.tobytes() == w.tobytes(), (W, H)
            assert (w["primitive"] != abi.NO_HIT).any()
    finally:
        ctx.close()


# ---- 7: beside a render ------------------------------------------------------------------------------------------------------------------------
def test_beside_a_render_of_the_same_context(native, oracle_mod, abi, scenes):
    """A render_view enqueued on a second stream while a render of the same context is in flight: both results are those of their solo runs."""
    import torch
    host, device = native
    W, H = 64, 48
    sc = load_for_both("cornell", oracle_mod, host, width=W, height=H, spp=16, max_depth=8)
    ctx = device.Context(0)
    try:
        ctx.set_scene(sc, sc.camera, sc.settings)
        view = VC.make_view(abi, VC.camera("inside", sc), *VC.SIZES[0], abi.VIEW_THIN_LENS)
        want = one_call(device, abi, ctx, view, 17, VC.DEPTH, 5)
        want_packed = torch.zeros((H, W), dtype=torch.int32, device="cuda")
        ctx.render(want_packed.data_ptr())
        torch.cuda.synchronize()
        s_render, s_view = torch.cuda.Stream(), torch.cuda.Stream()
        packed = torch.zeros((H, W), dtype=torch.int32, device="cuda")
        buf = buffers(device, view, 17)
        torch.cuda.synchronize()
        ctx.render(packed.data_ptr(), None, None, s_render.cuda_stream)
        render_view(ctx, abi, buf, 0, 17, VC.DEPTH, 5, stream=s_view.cuda_stream)
        ctx.render(packed.data_ptr(), None, None, s_render.cuda_stream)
        torch.cuda.synchronize()
        ctx.check()
        got = buf.read()
        assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want))
        assert torch.equal(packed, want_packed)
    finally:
        ctx.close()


# ---- 8: refusals on a live context ------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_sums_untouched_and_one_pixel_works(native, oracle_mod, abi, scenes, contexts):
    import ctypes as C
    import torch
    _, device = native
    ctx, sc = contexts["cornell"], scenes["cornell"]
    cam = VC.camera("inside", sc)
    ok = VC.make_view(abi, cam, 5, 3, abi.VIEW_PINHOLE)
    buf = buffers(device, ok, 4, fill_nan=False)
    prm = abi.RadianceParams.make(0, 4, VC.DEPTH)

    def refused(word, view=ok, params=prm, accum=None, scratch=None, linear=None, packed=None):
        with pytest.raises(device.RenderError) as e:
            ctx.render_view(view, params, buf.accum.ptr if accum is None else accum, buf.scratch.ptr if scratch is None else scratch, linear, packed)
        assert e.value.rc == abi.ERR_INVALID and word in str(e.value), (word, str(e.value))

    bad = VC.make_view(abi, cam, 5, 3, abi.VIEW_PINHOLE); bad.model = 2
    refused("view.model", view=bad)
    refused("view.lens_radius", view=VC.make_view(abi, cam, 5, 3, abi.VIEW_PINHOLE, lens=(0.5, 0.0)))
    refused("view.focus_distance", view=VC.make_view(abi, cam, 5, 3, abi.VIEW_THIN_LENS, lens=(0.5, 0.0)))
    bad = VC.make_view(abi, cam, 5, 3, abi.VIEW_PINHOLE); bad.camera.forward[1] = float("nan")
    refused("view.camera", view=bad)
    bad = VC.make_view(abi, cam, 5, 3, abi.VIEW_PINHOLE); bad.reserved[3] = 1
    refused("view.reserved", view=bad)
    refused("view.width", view=VC.make_view(abi, cam, 0, 3, abi.VIEW_PINHOLE))
    refused("split the call", view=VC.make_view(abi, cam, 65536, 65536, abi.VIEW_PINHOLE))
    refused("params.sample_begin", params=abi.RadianceParams.make(4, 4, VC.DEPTH))
    refused("d_accum must be 16-byte aligned", accum=buf.accum.ptr + 4)
    refused("d_scratch must be 16-byte aligned", scratch=buf.scratch.ptr + 8)
    refused("d_out_linear must be 4-byte aligned", linear=buf.linear.ptr + 2)
    refused("d_out_packed must be 4-byte aligned", packed=buf.packed.ptr + 1)
    with pytest.raises(device.RenderError) as e:
        ctx.view_rays(ok, 0, buf.rays.ptr + 8)
    assert "d_rays must be 16-byte aligned" in str(e.value)
    with pytest.raises(device.RenderError) as e:
        ctx.render_view(None, prm, buf.accum.ptr, buf.scratch.ptr)
    assert "view is null" in str(e.value)
    torch.cuda.synchronize()
    ctx.check()
    assert all(t.untouched() for t in (buf.accum, buf.linear, buf.packed, buf.scratch, buf.rays))      # nothing was enqueued
    # one pixel, one sample: the oracle's 1 x 1 image
    one = VC.make_view(abi, cam, 1, 1, abi.VIEW_PINHOLE)
    sums, means, packed = one_call(device, abi, ctx, one, 1, VC.DEPTH, 0)
    _, want, _ = oracle_mod.render(sc, cam, abi.Settings(1, 1, 1, VC.DEPTH), abi.Options.make(seed=0), threads=1)
    assert means.tobytes() == want.reshape(1, 3).tobytes() and sums[0, :3].tobytes() == means[0].tobytes() and sums[0, 3] == 0
    assert packed[0] == packed_of(means)[0]
    sums2, _, _ = one_call(device, abi, ctx, one, 1, VC.DEPTH, 0)
    assert sums2.tobytes() == sums.tobytes()


# ---- 9: the command-line tool ------------------------------------------------------------------------------------------------------------------
def test_rt_render_through_a_view_of_the_scenes_own_pose_writes_the_plain_runs_png(native, tmp_path):
    """rt_render --view-position / --view-target / --view-fov with the pose the scene file states renders through mi355rt_context_render_view what the
    plain run renders through mi355rt_context_render: the PNG is the same file, byte for byte."""
    import json
    cli = pkg("build").build_cli()
    scene = SCENES["cornell"]
    cam = json.load(open(scene))["camera"]
    tr = cam["transform"]
    pos, at, fov = tr["position"], tr["look_at"], cam["fov"]
    common = [cli, scene, "--width", "48", "--height", "36", "--spp", "8", "--max-depth", "6"]
    plain, through = tmp_path / "plain.png", tmp_path / "view.png"
    subprocess.run(common + ["-o", str(plain)], check=True, capture_output=True, timeout=120)
    view = ["--view-position", ",".join(repr(float(v)) for v in pos), "--view-target", ",".join(repr(float(v)) for v in at), "--view-fov", repr(float(fov))]
    subprocess.run(common + ["-o", str(through)] + view, check=True, capture_output=True, timeout=120)
    assert plain.read_bytes() == through.read_bytes() and len(plain.read_bytes()) > 100
    # a moved pose and a lens each give another image of the same size
    for extra in (["--view-position", "0.5,1.2,3.0", "--view-target", "0,1,0"], view + ["--lens-radius", "0.05", "--focus-distance", "6.8"]):
        other = tmp_path / "other.png"
        subprocess.run(common + ["-o", str(other)] + extra, check=True, capture_output=True, timeout=120)
        assert other.read_bytes() != plain.read_bytes() and other.read_bytes()[:24] == plain.read_bytes()[:24]      # the same PNG header: 48 x 36
    bad = subprocess.run(common + ["-o", str(through), "--lens-radius", "0.05"], capture_output=True, timeout=120)
    assert bad.returncode != 0 and b"--view-position" in bad.stderr
