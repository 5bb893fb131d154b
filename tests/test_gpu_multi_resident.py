"""mi355rt_multi_context_*: the resident multi-device form (contexts, streams, staging and the row table kept across calls; the strips come
back by peer copies and one k_gather_strips launch on the caller's stream).  On a one-GPU box every part is device 0, listed several
times: every part still has its own context, stream and staging, and the exchange runs the same copy path.  Every image must equal the
one-device image of the same window, packed and linear bit for bit."""
import os

import numpy as np
import pytest
import torch

from conftest import SCENES

pytestmark = pytest.mark.gpu


def _scene(host, name, W, H, spp=5, depth=8):
    return host.LoadedScene(SCENES[name], W, H, spp, depth, skip_unknown_primitives=(name == "teapot"))


def _one_device(device, abi, sc, opt_kw):
    """The same window on ONE device through the one-shot call (strips of one row, one part)."""
    kw = {k: v for k, v in opt_kw.items() if k in ("row_begin", "row_end", "rng_mode", "seed")}
    return device.render(sc, sc.camera, sc.settings, abi.Options.make(**kw))


def _outputs(m, opt, offset=0):
    """Output tensors on cuda:0 filled with a pattern no render produces (unwritten rows show); `offset` elements in front of each."""
    rows, W = m.rows_selected(opt), m.settings.width
    packed = torch.full((offset + rows * W,), -1, dtype=torch.int32, device="cuda:0")[offset:]
    linear = torch.full((offset + rows * W * 3,), float("nan"), dtype=torch.float32, device="cuda:0")[offset:]
    return packed, linear


def _host(packed, linear, rows, W):
    return packed.cpu().numpy().view(np.uint32).reshape(rows, W), linear.cpu().numpy().reshape(rows, W, 3)


def _assert_same(mp, ml, gp, gl):
    assert mp.shape == gp.shape
    assert np.array_equal(mp, gp)
    assert np.array_equal(ml.view(np.uint32), gl.view(np.uint32))


def _render_and_compare(m, device, abi, sc, opt_kw, offset=0):
    opt = abi.Options.make(**opt_kw)
    packed, linear = _outputs(m, opt, offset)
    st = m.render(packed, linear, opt, want_stats=True)
    torch.cuda.synchronize()
    gp, gl, gst = _one_device(device, abi, sc, opt_kw)
    mp, ml = _host(packed, linear, gp.shape[0], sc.settings.width)
    _assert_same(mp, ml, gp, gl)
    assert (st.samples, st.rays, st.rows_rendered) == (gst.samples, gst.rays, gst.rows_rendered)
    return st


@pytest.mark.parametrize("name,W,H,devices,opt_kw", [
    ("cornell", 64, 48, [0, 0], {"strip_rows": 4}),
    ("cornell", 50, 50, [0, 0, 0], {"strip_rows": 0}),                   # 0 -> strips of 4; neither 50 rows nor 50 columns divide evenly
    ("teapot", 37, 37, [0] * 8, {"strip_rows": 1}),                      # 8 parts like a full node; rows of 37 words (dword path)
    ("cornell", 64, 48, [0, 0], {"strip_rows": 5, "row_begin": 7, "row_end": 41}),
    ("cornell", 64, 3, [0, 0, 0, 0], {"strip_rows": 1}),                 # 3 rows on 4 parts: one part is empty
    ("cornell", 64, 48, [0, 0], {"strip_rows": 4, "rng_mode": 1}),       # MI355RT_RNG_REF: the reference's per-row stream
])
def test_resident_multi_equals_one_device(name, W, H, devices, opt_kw, native, abi):
    host, device = native
    sc = _scene(host, name, W, H)
    m = device.MultiContext(devices)
    try:
        m.set_scene(sc, sc.camera, sc.settings)
        st = _render_and_compare(m, device, abi, sc, opt_kw)
        assert st.bands >= 1 and st.total_ms > 0
        if opt_kw.get("rng_mode", 0) == abi.RNG_CTR:
            assert st.render_kernel_ms > 0
        m.check()
    finally:
        m.close()


def test_unaligned_outputs_take_the_dword_path(native, abi):
    """Output pointers 4 bytes past a 16-byte boundary: rows of 64 words no longer start aligned on the destination side."""
    host, device = native
    sc = _scene(host, "cornell", 64, 48)
    m = device.MultiContext([0, 0])
    try:
        m.set_scene(sc, sc.camera, sc.settings)
        _render_and_compare(m, device, abi, sc, {"strip_rows": 4}, offset=1)
    finally:
        m.close()


def test_residency_across_options_and_scenes(native, abi):
    """One multi context, no set_scene in between: options A, then B (another window and strip size), then A again; then another scene
    at another resolution."""
    host, device = native
    sc = _scene(host, "cornell", 64, 48)
    a = {"strip_rows": 4}
    b = {"strip_rows": 3, "row_begin": 5, "row_end": 30, "seed": 11}
    m = device.MultiContext([0, 0, 0])
    try:
        m.set_scene(sc, sc.camera, sc.settings)
        for kw in (a, b, a):
            _render_and_compare(m, device, abi, sc, kw)
        sc2 = _scene(host, "teapot", 40, 24, spp=3, depth=6)
        m.set_scene(sc2, sc2.camera, sc2.settings)
        _render_and_compare(m, device, abi, sc2, {"strip_rows": 2})
        m.check()
    finally:
        m.close()


def test_asynchronous_renders_on_two_streams(native, abi):
    """Two enqueue-only renders (no stats) on two torch streams of device 0, the same row selection (nothing is re-allocated, so nothing
    waits on the host) but different seeds: the second must wait for the first's staging and workspaces.  Then synchronize and check()."""
    host, device = native
    sc = _scene(host, "cornell", 128, 96, spp=16, depth=8)
    kw1, kw2 = {"strip_rows": 4}, {"strip_rows": 4, "seed": 7}
    m = device.MultiContext([0, 0])
    try:
        m.set_scene(sc, sc.camera, sc.settings)
        o1, o2 = abi.Options.make(**kw1), abi.Options.make(**kw2)
        p1, l1 = _outputs(m, o1)
        p2, l2 = _outputs(m, o2)
        s1, s2 = torch.cuda.Stream(device=0), torch.cuda.Stream(device=0)
        torch.cuda.synchronize()
        assert m.render(p1, l1, o1, stream=s1) is None
        assert m.render(p2, l2, o2, stream=s2) is None
        torch.cuda.synchronize()
        m.check()
        for (p, l), kw in (((p1, l1), kw1), ((p2, l2), kw2)):
            gp, gl, _ = _one_device(device, abi, sc, kw)
            _assert_same(*_host(p, l, 96, 128), gp, gl)
        assert not np.array_equal(_host(p1, l1, 96, 128)[0], _host(p2, l2, 96, 128)[0])      # (the seeds do change the image)
    finally:
        m.close()


def test_multi_context_argument_checks(native, abi):
    host, device = native
    with pytest.raises(device.RenderError, match="empty"):
        device.MultiContext([])
    with pytest.raises(device.RenderError, match="out of range"):
        device.MultiContext([0, 99])
    sc = _scene(host, "cornell", 16, 8, spp=2, depth=3)
    m = device.MultiContext([0, 0])
    try:
        packed = torch.zeros(16 * 8, dtype=torch.int32, device="cuda:0")
        with pytest.raises(device.RenderError, match="no scene"):
            m.render(packed)
        m.set_scene(sc, sc.camera, sc.settings)
        with pytest.raises(device.RenderError, match="deals the strips itself"):
            m.render(packed, options=abi.Options.make(n_parts=2, part=1))
        L = device.lib()
        assert L.mi355rt_multi_context_render(m._h, None, None, None, None, None) == abi.ERR_INVALID
        assert b"d_out_packed is null" in L.mi355rt_last_error()
        m.render(packed, want_stats=True)                                 # the context is still usable
        m.check()
    finally:
        m.close()


def test_eight_parts_at_the_headline_frame(native, abi):
    """The frame the bench times (cornell 800x600x256 d30) on 8 parts with the default strips: rows of 800 packed and 2400 linear words
    take k_gather_strips' dwordx4 path from 8 staging areas, and the image must be the one-device image bit for bit, with its rays."""
    host, device = native
    sc = _scene(host, "cornell", 800, 600, spp=256, depth=30)
    m = device.MultiContext([0] * 8)
    try:
        m.set_scene(sc, sc.camera, sc.settings)
        st = _render_and_compare(m, device, abi, sc, {"strip_rows": 0})             # 0: the default strips of 4 rows
        assert st.samples == 800 * 600 * 256 and st.rows_rendered == 600
        m.check()
    finally:
        m.close()
