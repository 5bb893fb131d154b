"""The seven calls that take host buffers and give host buffers back (mi355rt_render, mi355rt_render_multi, mi355rt_render_progressive,
mi355rt_render_progressive_multi, mi355rt_trace_rays, mi355rt_occluded, mi355rt_denoise) are clients of the resident API: a context of their
own, an upload, the resident call, a copy back.  So each must give, bit for bit, what its resident twin gives; a failure of set_scene must come
back with set_scene's code and text after the call has torn its context down, and must leave the next call of the same kind working; an early
stop must leave the image and the stats of the samples done; a selection of no rows must touch nothing.  Every expected value is another
call's answer or a count that follows from the shapes (rows * width * samples) -- nothing here is specific to how the calls are built.

cornell at 16 x 12, 4 spp, depth 4; batches of 65 rays and segments (one more than a wave); device lists are [0, 0], so one GPU is enough."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import SCENES

pytestmark = pytest.mark.gpu

W, H, SPP, DEPTH, CHUNK = 16, 12, 4, 4, 3                 # chunks of 3 samples: 3 + 1, a short last chunk
SENT_PACKED, SENT_LINEAR, SENT_BYTE = 0xDEADBEEF, -7.0, 0xAB
RENDERS = ("render", "multi", "progressive", "progressive_multi")
STATS_INTS = ("samples", "rays", "rows_rendered", "bands", "grid_blocks", "block_threads", "kernel_vgprs", "kernel_sgprs")

_cache = {}


def _scene(host):
    if "scene" not in _cache:
        _cache["scene"] = host.LoadedScene(SCENES["cornell"], W, H, SPP, DEPTH)
    return _cache["scene"]


def _settings(abi, spp=SPP):
    return abi.Settings(W, H, spp, DEPTH)


def _resident(device, abi, sc, spp=SPP, opt=None):
    """Context.render of `spp` samples into device buffers: (packed [rows, W], linear [rows, W, 3], stats), computed once per (spp, options)."""
    key = ("resident", spp, None if opt is None else bytes(opt))
    if key not in _cache:
        rows = len(abi.rows_selected(H, opt))
        ctx = device.Context(0)
        try:
            ctx.set_scene(sc, sc.camera, _settings(abi, spp))
            packed = torch.zeros(rows * W, dtype=torch.int32, device="cuda")
            linear = torch.zeros(rows * W * 3, dtype=torch.float32, device="cuda")
            st = ctx.render(packed.data_ptr(), linear.data_ptr(), opt, want_stats=True)
            p, l = packed.cpu().numpy().view(np.uint32).reshape(rows, W), linear.cpu().numpy().reshape(rows, W, 3)
        finally:
            ctx.close()
        p.setflags(write=False); l.setflags(write=False)
        _cache[key] = (p, l, st)
    return _cache[key]


def _sentinel_stats(abi):
    st = abi.Stats()
    C.memset(C.addressof(st), SENT_BYTE, C.sizeof(st))
    return st


def _call(device, abi, kind, sc, st, opt=None, want_linear=True, stats=None, on_chunk=None):
    """One host-buffer render call into buffers of the whole image filled with sentinels: (rc, message, packed [H, W], linear [H, W, 3]).
    The selected rows come first; whatever follows them must still hold the sentinel."""
    L = device.lib()
    packed = np.full((H, W), SENT_PACKED, np.uint32)
    linear = np.full((H, W, 3), SENT_LINEAR, np.float32)
    head = (C.byref(sc.c), C.byref(sc.camera), C.byref(st), C.byref(opt) if opt is not None else None)
    out = (C.c_void_p(packed.ctypes.data), C.c_void_p(linear.ctypes.data) if want_linear else None, C.byref(stats) if stats is not None else None)
    devs = (C.c_int * 2)(0, 0)
    fn = None
    if on_chunk is not None:
        fn = abi.ProgressFn(lambda user, done, total, ptr: int(on_chunk(int(done), int(total), packed)))
    if kind == "render":
        rc = L.mi355rt_render(*head, *out)
    elif kind == "multi":
        rc = L.mi355rt_render_multi(*head, devs, 2, *out)
    elif kind == "progressive":
        rc = L.mi355rt_render_progressive(*head, C.c_uint32(CHUNK), fn, None, *out)
    else:
        rc = L.mi355rt_render_progressive_multi(*head, devs, 2, CHUNK, fn if fn is not None else abi.ProgressFn(), None, *out)
    return rc, L.mi355rt_last_error().decode(), packed, linear


def _assert_image(packed, linear, want_p, want_l, want_linear, what):
    rows = want_p.shape[0]
    assert np.array_equal(packed[:rows], want_p), f"{what}: packed"
    assert (packed[rows:] == SENT_PACKED).all(), f"{what}: packed written past the selected rows"
    if want_linear:
        assert np.array_equal(linear[:rows].view(np.uint32), want_l.view(np.uint32)), f"{what}: linear"
        assert (linear[rows:] == SENT_LINEAR).all(), f"{what}: linear written past the selected rows"
    else:
        assert (linear == SENT_LINEAR).all(), f"{what}: linear written though not asked for"


# ---- 1: each call equals its resident twin ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("want_linear,window,want_stats", [(True, False, True), (False, False, False), (True, True, False), (False, True, True)])
def test_render_equals_context_render(want_linear, window, want_stats, native, abi):
    host, device = native
    sc = _scene(host)
    opt = abi.Options.make(row_begin=2, row_end=11) if window else None
    want_p, want_l, want_st = _resident(device, abi, sc, SPP, opt)
    stats = _sentinel_stats(abi) if want_stats else None
    rc, msg, packed, linear = _call(device, abi, "render", sc, _settings(abi), opt, want_linear, stats)
    assert rc == 0, msg
    _assert_image(packed, linear, want_p, want_l, want_linear, "mi355rt_render")
    if want_stats:
        assert stats.samples == want_p.shape[0] * W * SPP and stats.rows_rendered == want_p.shape[0]
        assert [getattr(stats, f) for f in STATS_INTS] == [getattr(want_st, f) for f in STATS_INTS]


@pytest.mark.parametrize("window", [False, True])
def test_render_multi_equals_render(window, native, abi):
    host, device = native
    sc = _scene(host)
    opt = abi.Options.make(row_begin=2, row_end=11, strip_rows=0) if window else None        # strip_rows 0 -> strips of 4 rows
    one = abi.Options.make(row_begin=2, row_end=11) if window else None
    rows = len(abi.rows_selected(H, one))
    one_stats = abi.Stats()
    rc, msg, want_p, want_l = _call(device, abi, "render", sc, _settings(abi), one, True, one_stats)
    assert rc == 0, msg
    stats = _sentinel_stats(abi)
    rc, msg, packed, linear = _call(device, abi, "multi", sc, _settings(abi), opt, True, stats)
    assert rc == 0, msg
    _assert_image(packed, linear, want_p[:rows], want_l[:rows], True, "mi355rt_render_multi")
    assert (stats.samples, stats.rays, stats.rows_rendered) == (one_stats.samples, one_stats.rays, rows)     # counts are summed over the devices
    assert stats.block_threads == one_stats.block_threads and stats.kernel_vgprs == one_stats.kernel_vgprs


@pytest.mark.parametrize("kind", ["progressive", "progressive_multi"])
def test_progressive_calls_equal_the_render(kind, native, abi):
    host, device = native
    sc = _scene(host)
    p3, l3, _ = _resident(device, abi, sc, CHUNK)
    p4, l4, st4 = _resident(device, abi, sc, SPP)
    seen = []
    stats = _sentinel_stats(abi)
    rc, msg, packed, linear = _call(device, abi, kind, sc, _settings(abi), None, True, stats,
                                    on_chunk=lambda done, total, img: seen.append((done, total, img.copy())) or 0)
    assert rc == 0, msg
    assert [(d, t) for d, t, _ in seen] == [(CHUNK, SPP), (SPP, SPP)]                        # 3 + 1
    assert np.array_equal(seen[0][2], p3) and np.array_equal(seen[1][2], p4), "the image a callback saw"
    _assert_image(packed, linear, p4, l4, True, kind)
    assert (stats.samples, stats.rays, stats.rows_rendered) == (H * W * SPP, st4.rays, H)
    if kind == "progressive":                                                                # the launch figures are the last chunk's
        assert (stats.block_threads, stats.kernel_vgprs, stats.kernel_sgprs) == (st4.block_threads, st4.kernel_vgprs, st4.kernel_sgprs)
        assert stats.grid_blocks > 0
    else:                                                                                    # the multi context reports none
        assert (stats.grid_blocks, stats.block_threads, stats.kernel_vgprs, stats.kernel_sgprs) == (0, 0, 0, 0)
    # no callback, packed only, no stats: the one copy back is the last chunk's
    rc, msg, packed, linear = _call(device, abi, kind, sc, _settings(abi), None, False, None)
    assert rc == 0, msg
    _assert_image(packed, linear, p4, l4, False, kind + ", packed only")


def _camera_rays(sc, n, seed):
    """n rays from the camera into the box, un-normalised: float32 [n, 8] (origin, pad, direction, pad)."""
    rng = np.random.default_rng(seed)
    cam = sc.camera
    pos, fwd, right, up = (np.array(list(a), np.float32) for a in (cam.position, cam.forward, cam.right, cam.true_up))
    r = np.zeros((n, 8), np.float32)
    r[:, 0:3] = pos
    r[:, 4:7] = fwd + rng.uniform(-1, 1, (n, 1)).astype(np.float32) * cam.half_width * right + rng.uniform(-1, 1, (n, 1)).astype(np.float32) * cam.half_height * up
    r[:, 4:7] *= rng.uniform(0.5, 3.0, (n, 1)).astype(np.float32)
    return r


def _resident_queries(device, abi, sc):
    """Context.trace_rays and Context.occluded on 65 rays / segments: (rays, hits, segments, words), computed once."""
    if "queries" not in _cache:
        n = 65
        rays = _camera_rays(sc, n, 11)
        seg = rays.copy()
        seg[:, 7] = np.random.default_rng(12).uniform(0.5, 12.0, n).astype(np.float32)       # t_max: some in front of the first hit, some behind
        ctx = device.Context(0)
        try:
            ctx.set_scene(sc, sc.camera, _settings(abi))
            d_rays, d_seg = torch.from_numpy(rays).cuda(), torch.from_numpy(seg).cuda()
            d_hits = torch.zeros(n * 48, dtype=torch.uint8, device="cuda")
            d_words = torch.zeros(n, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            ctx.trace_rays(d_rays.data_ptr(), n, d_hits.data_ptr())
            ctx.occluded(d_seg.data_ptr(), n, d_words.data_ptr())
            torch.cuda.synchronize()
            hits = d_hits.cpu().numpy().view(abi.HIT_DTYPE).copy()
            words = d_words.cpu().numpy().view(np.uint32).copy()
        finally:
            ctx.close()
        assert (hits["primitive"] != abi.NO_HIT).any() and 0 < words.sum() < n, "the batch does not tell a query from a constant"
        _cache["queries"] = (rays, hits, seg, words)
    return _cache["queries"]


def test_query_one_shots_equal_the_context_queries(native, abi):
    """(also pinned, on larger batches of other scenes: test_gpu_ray_queries.py::test_one_shot_repeats_and_a_query_beside_a_render and
    test_gpu_occlusion.py::test_repeats_a_call_beside_a_render_and_the_refusals)"""
    host, device = native
    sc = _scene(host)
    rays, hits, seg, words = _resident_queries(device, abi, sc)
    assert device.trace_rays(sc, rays).tobytes() == hits.tobytes()
    assert device.occluded(sc, seg).tobytes() == words.tobytes()


def test_denoise_equals_context_denoise(native, abi):
    """(also pinned on a 48 x 36 render: test_gpu_denoise.py::test_aliasing_single_outputs_repeats_and_the_one_shot)"""
    host, device = native
    sc = _scene(host)
    _, lin, _ = _resident(device, abi, sc)
    n = H * W
    ctx = device.Context(0)
    try:
        ctx.set_scene(sc, sc.camera, _settings(abi))
        d_hits = torch.zeros(n * 48, dtype=torch.uint8, device="cuda")
        d_in = torch.from_numpy(lin.copy()).cuda()
        d_scratch = torch.zeros(device.denoise_scratch_bytes(W, H), dtype=torch.uint8, device="cuda")
        d_lin = torch.zeros(n * 3, dtype=torch.float32, device="cuda")
        d_packed = torch.zeros(n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.first_hits(d_hits.data_ptr())
        ctx.denoise(W, H, d_in.data_ptr(), d_hits.data_ptr(), d_scratch.data_ptr(), d_lin.data_ptr(), d_packed.data_ptr())
        torch.cuda.synchronize()
        hits = d_hits.cpu().numpy().view(abi.HIT_DTYPE).copy()
        want_lin, want_packed = d_lin.cpu().numpy().reshape(H, W, 3), d_packed.cpu().numpy().view(np.uint32).reshape(H, W)
    finally:
        ctx.close()
    for want_linear, want_packed_too in ((True, True), (True, False), (False, True)):
        got_lin, got_packed = device.denoise(lin, hits, want_linear=want_linear, want_packed=want_packed_too)
        assert (got_lin is None) == (not want_linear) and (got_packed is None) == (not want_packed_too)
        if want_linear:
            assert got_lin.tobytes() == want_lin.tobytes()
        if want_packed_too:
            assert got_packed.tobytes() == want_packed.tobytes()


# ---- 2: an early stop ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["progressive", "progressive_multi"])
def test_an_early_stop_leaves_the_image_and_the_stats_of_the_first_chunk(kind, native, abi):
    host, device = native
    sc = _scene(host)
    p3, l3, st3 = _resident(device, abi, sc, CHUNK)
    stops = []
    stats = _sentinel_stats(abi)
    rc, msg, packed, linear = _call(device, abi, kind, sc, _settings(abi), None, True, stats, on_chunk=lambda done, total, img: stops.append(done) or 1)
    assert rc == 0, msg
    assert stops == [CHUNK]
    _assert_image(packed, linear, p3, l3, True, kind + ", stopped after the first chunk")
    assert (stats.samples, stats.rays, stats.rows_rendered) == (H * W * CHUNK, st3.rays, H)


# ---- 3: a scene that set_scene refuses ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", RENDERS + ("trace_rays", "occluded"))
def test_a_refused_scene_is_reported_and_the_next_call_works(kind, native, abi):
    host, device = native
    sc = _scene(host)
    want_p, want_l, _ = _resident(device, abi, sc)
    rays, hits, seg, words = _resident_queries(device, abi, sc)
    L = device.lib()

    def call():
        if kind == "trace_rays":
            out = np.zeros(len(rays), abi.HIT_DTYPE)
            return L.mi355rt_trace_rays(C.byref(sc.c), C.c_void_p(rays.ctypes.data), len(rays), C.c_void_p(out.ctypes.data)), out
        if kind == "occluded":
            out = np.zeros(len(seg), np.uint32)
            return L.mi355rt_occluded(C.byref(sc.c), C.c_void_p(seg.ctypes.data), len(seg), C.c_void_p(out.ctypes.data)), out
        rc, _, packed, linear = _call(device, abi, kind, sc, _settings(abi))
        return rc, (packed, linear)

    p0 = sc.c.primitives[0]
    old = p0.material
    p0.material = 999                                                                        # out of range: set_scene refuses the scene
    try:
        rc, _ = call()
        msg = L.mi355rt_last_error().decode()
    finally:
        p0.material = old
    assert rc == abi.ERR_INVALID and "primitive material index" in msg, (rc, msg)             # set_scene's code and text, after the clean-up
    if kind == "multi":
        assert msg.startswith("device 0: ")
    if kind == "progressive_multi":
        assert msg.startswith("device 0 (part 0): ")
    rc, out = call()                                                                         # the very next call of the same kind
    assert rc == 0, L.mi355rt_last_error().decode()
    if kind == "trace_rays":
        assert out.tobytes() == hits.tobytes()
    elif kind == "occluded":
        assert out.tobytes() == words.tobytes()
    else:
        _assert_image(out[0], out[1], want_p, want_l, True, kind + " after a refused scene")


# ---- 4: a selection of no rows -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", RENDERS)
def test_an_empty_row_selection_touches_nothing(kind, native, abi):
    """row_begin == height with row_end 0 (= height) is accepted and selects no rows.  mi355rt_render then leaves *stats as it found it; the other
    three write their totals, which are all zero."""
    host, device = native
    sc = _scene(host)
    opt = abi.Options.make(row_begin=H)
    assert abi.rows_selected(H, opt) == []
    stats = _sentinel_stats(abi)
    rc, msg, packed, linear = _call(device, abi, kind, sc, _settings(abi), opt, True, stats)
    assert rc == 0, msg
    assert (packed == SENT_PACKED).all() and (linear == SENT_LINEAR).all()
    raw = bytes(stats)
    assert raw == (bytes([SENT_BYTE]) if kind == "render" else b"\0") * C.sizeof(stats), raw
