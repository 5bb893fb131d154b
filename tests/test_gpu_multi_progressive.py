"""Progressive rendering on the resident multi-device context (mi355rt_multi_context_render_progressive) and its one-shot form
(mi355rt_render_progressive_multi).  Every part keeps its running sums on its own device; after every chunk the images must be bit-identical,
packed and linear, to one mi355rt_context fed the same chunks, and the gathered sums to that context's d_accum.  On a one-GPU box every part
is device 0, listed several times: each part still has its own context, stream and sums, and the exchange runs the same peer-copy path."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import SCENES
from parity import assert_parity

pytestmark = pytest.mark.gpu


def _scene(host, name, W, H, spp, depth=8):
    return host.LoadedScene(SCENES[name], W, H, spp, depth, skip_unknown_primitives=(name == "teapot"))


def _window(abi, kw):
    """The options of the one-device comparison: the same window, one part."""
    return abi.Options.make(**{k: v for k, v in kw.items() if k in ("row_begin", "row_end", "seed", "flags")})


def _buffers(rows, W):
    """packed, linear and accum on cuda:0, filled with a pattern no render produces (unwritten pixels show)."""
    packed = torch.full((rows * W,), -1, dtype=torch.int32, device="cuda:0")
    linear = torch.full((rows * W * 3,), float("nan"), dtype=torch.float32, device="cuda:0")
    accum = torch.full((rows * W * 4,), float("nan"), dtype=torch.float32, device="cuda:0")
    return packed, linear, accum


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def _assert_bits(a, b, what):
    assert np.array_equal(_bits(a), _bits(b)), what


class _OneDevice:
    """One mi355rt_context with the same scene, fed the same chunks (Context.render_progressive)."""

    def __init__(self, device, sc, opt, rows):
        self.ctx = device.Context(0)
        self.ctx.set_scene(sc, sc.camera, sc.settings)
        self.opt, self.W = opt, sc.settings.width
        self.packed, self.linear, self.accum = _buffers(rows, self.W)

    def chunk(self, s0, s1):
        return self.ctx.render_progressive(s0, s1, self.accum.data_ptr(), self.packed.data_ptr(), self.linear.data_ptr(), self.opt, want_stats=True)

    def close(self):
        self.ctx.close()


@pytest.mark.parametrize("name,devices,chunks,opt_kw", [
    ("cornell", [0, 0], (1, 3, 4), {"strip_rows": 4}),                                 # lockstep kernel
    ("teapot", [0, 0, 0], (4, 2, 6), {"strip_rows": 2}),                               # wavefront kernel
    ("cornell", [0, 0, 0], (2, 5, 1), {"strip_rows": 3, "row_begin": 7, "row_end": 41}),   # a row window, strips of 3 over 3 parts
])
def test_chunked_sequence_equals_one_device(name, devices, chunks, opt_kw, native, oracle_mod, abi):
    host, device = native
    W, H, spp = 64, 48, sum(chunks)
    sc = _scene(host, name, W, H, spp)
    mopt, sopt = abi.Options.make(**opt_kw), _window(abi, opt_kw)
    rows = len(abi.rows_selected(H, sopt))
    one = _OneDevice(device, sc, sopt, rows)
    m = device.MultiContext(devices)
    try:
        m.set_scene(sc, sc.camera, sc.settings)
        assert m.rows_selected(mopt) == rows
        packed, linear, accum = _buffers(rows, W)
        s, rays = 0, 0
        for c in chunks:
            st = m.render_progressive(s, s + c, packed, linear, accum, mopt, want_stats=True)
            gst = one.chunk(s, s + c)
            s += c
            assert st.samples == rows * W * c and st.rows_rendered == rows
            assert st.rays == gst.rays
            rays += st.rays
            _assert_bits(packed, one.packed, f"packed image after {s} samples")
            _assert_bits(linear, one.linear, f"linear image after {s} samples")
            _assert_bits(accum, one.accum, f"gathered sums after {s} samples")
        m.check()
        # the whole frame at the summed spp, on one device, and the oracle in counter mode
        fp, fl, _ = _buffers(rows, W)
        fst = one.ctx.render(fp.data_ptr(), fl.data_ptr(), sopt, want_stats=True)
        _assert_bits(packed, fp, "final packed image against mi355rt_context_render")
        _assert_bits(linear, fl, "final linear image against mi355rt_context_render")
        assert rays == fst.rays
        op, ol, cnt = oracle_mod.render(sc, sc.camera, sc.settings, sopt)
        assert_parity(_bits(packed).reshape(rows, W), linear.cpu().numpy().reshape(rows, W, 3), op, ol, exact=True,
                      rows=abi.rows_selected(H, sopt), gpu_rays=rays, oracle_rays=cnt.rays)
    finally:
        m.close()
        one.close()


def test_sequence_rules(native, abi):
    host, device = native
    W, H = 32, 16
    sc = _scene(host, "cornell", W, H, 6, depth=5)
    kw = {"strip_rows": 2}
    mopt, sopt = abi.Options.make(**kw), _window(abi, kw)
    m = device.MultiContext([0, 0])
    try:
        m.set_scene(sc, sc.camera, sc.settings)
        packed, linear, accum = _buffers(H, W)
        one = _OneDevice(device, sc, sopt, H)
        m.render_progressive(0, 2, packed, linear, accum, mopt)
        one.chunk(0, 2)
        with pytest.raises(device.RenderError, match="last chunk ended at sample 2") as e:
            m.render_progressive(3, 5, packed, linear, accum, mopt)
        assert e.value.rc == abi.ERR_INVALID
        with pytest.raises(device.RenderError, match="rng_mode, seed or flags"):
            m.render_progressive(2, 4, packed, linear, accum, abi.Options.make(seed=9, **kw))
        with pytest.raises(device.RenderError, match="row selection"):
            m.render_progressive(2, 4, packed, linear, accum, abi.Options.make(strip_rows=1))
        with pytest.raises(device.RenderError, match="row selection"):
            m.render_progressive(2, 4, packed, linear, accum, abi.Options.make(row_begin=1, **kw))
        # a plain render of another window between two chunks leaves the sequence (and its sums) alone
        wopt = abi.Options.make(strip_rows=3, row_begin=3, row_end=11, seed=4)
        rp, rl, _ = _buffers(8, W)
        m.render(rp, rl, wopt, want_stats=True)
        gp, gl, _ = device.render(sc, sc.camera, sc.settings, _window(abi, {"row_begin": 3, "row_end": 11, "seed": 4}))
        assert np.array_equal(_bits(rp).reshape(8, W), gp) and np.array_equal(_bits(rl), gl.reshape(-1).view(np.uint32))
        m.render_progressive(2, 4, packed, linear, accum, mopt)       # the refused calls changed nothing either
        one.chunk(2, 4)
        for a, b, what in ((packed, one.packed, "packed"), (linear, one.linear, "linear"), (accum, one.accum, "sums")):
            _assert_bits(a, b, what + " after a plain render between chunks")
        # changed options need a restart at 0, which then gives the new image
        sopt2 = abi.Options.make(seed=3)
        m.render_progressive(0, 3, packed, linear, accum, abi.Options.make(seed=3, **kw))
        one2 = _OneDevice(device, sc, sopt2, H)
        one2.chunk(0, 3)
        _assert_bits(packed, one2.packed, "packed after a restart with other options")
        _assert_bits(accum, one2.accum, "sums after a restart with other options")
        one2.close()
        # set_scene ends the sequence; a restart gives the right image
        m.set_scene(sc, sc.camera, sc.settings)
        with pytest.raises(device.RenderError, match="none is open"):
            m.render_progressive(3, 6, packed, linear, accum, abi.Options.make(seed=3, **kw))
        m.render_progressive(0, 6, packed, linear, accum, mopt)
        one.chunk(4, 6)
        _assert_bits(packed, one.packed, "packed after set_scene and a restart")
        _assert_bits(linear, one.linear, "linear after set_scene and a restart")
        _assert_bits(accum, one.accum, "sums after set_scene and a restart")
        # refused outright
        with pytest.raises(device.RenderError, match="MI355RT_RNG_CTR") as e:
            m.render_progressive(0, 2, packed, linear, accum, abi.Options.make(rng_mode=abi.RNG_REF, **kw))
        assert e.value.rc == abi.ERR_INVALID
        with pytest.raises(device.RenderError, match="deals the strips itself"):
            m.render_progressive(0, 2, packed, options=abi.Options.make(n_parts=2, part=1))
        with pytest.raises(device.RenderError, match="sample_end"):
            m.render_progressive(2, 2, packed)
        m.render_progressive(6, 7, packed, linear, options=mopt)        # (still open after refusals; no sums asked for)
        one.chunk(6, 7)
        _assert_bits(packed, one.packed, "packed of a chunk without d_accum")
        m.check()
        one.close()
    finally:
        m.close()


def test_asynchronous_chunks_on_a_side_stream(native, abi):
    host, device = native
    W, H = 64, 48
    sc = _scene(host, "cornell", W, H, 8)
    kw = {"strip_rows": 4}
    mopt, sopt = abi.Options.make(**kw), _window(abi, kw)
    one = _OneDevice(device, sc, sopt, H)
    m = device.MultiContext([0, 0])
    try:
        m.set_scene(sc, sc.camera, sc.settings)
        packed, linear, accum = _buffers(H, W)
        side = torch.cuda.Stream(device=0)
        torch.cuda.synchronize()
        assert m.render_progressive(0, 3, packed, linear, accum, mopt, stream=side) is None
        assert m.render_progressive(3, 7, packed, linear, accum, mopt, stream=side) is None
        torch.cuda.synchronize()
        m.check()
        one.chunk(0, 3)
        one.chunk(3, 7)
        for a, b, what in ((packed, one.packed, "packed"), (linear, one.linear, "linear"), (accum, one.accum, "sums")):
            _assert_bits(a, b, what + " of enqueue-only chunks")
        st = m.render_progressive(7, 8, packed, linear, accum, mopt, want_stats=True)
        assert st.samples == H * W * (8 - 7) and st.rows_rendered == H and st.total_ms > 0
        one.chunk(7, 8)
        _assert_bits(accum, one.accum, "sums after the chunk with stats")
    finally:
        m.close()
        one.close()


def _single_device_callback_images(device, abi, sc, chunk):
    """mi355rt_render_progressive (one device, host buffers): the image every callback saw, and the final outputs."""
    W, H = sc.settings.width, sc.settings.height
    packed = np.zeros((H, W), np.uint32)
    linear = np.zeros((H, W, 3), np.float32)
    seen = []

    def cb(user, done, total, ptr):
        seen.append((done, total, np.ctypeslib.as_array(ptr, shape=(H * W,)).reshape(H, W).copy()))
        return 0

    fn = abi.ProgressFn(cb)
    rc = device.lib().mi355rt_render_progressive(C.byref(sc.c), C.byref(sc.camera), C.byref(sc.settings), None, C.c_uint32(chunk), fn, None,
                                                 C.c_void_p(packed.ctypes.data), C.c_void_p(linear.ctypes.data), None)
    assert rc == 0, device.lib().mi355rt_last_error()
    return seen, packed, linear


def test_one_shot_progressive_multi(native, abi):
    host, device = native
    W, H, spp, chunk = 64, 48, 10, 4
    sc = _scene(host, "cornell", W, H, spp)
    seen = []
    packed, linear, st = device.render_progressive_multi(sc, sc.camera, sc.settings, [0, 0, 0], chunk,
                                                         on_chunk=lambda done, total, img: seen.append((done, total, img.copy())) and False,
                                                         options=abi.Options.make(strip_rows=3))
    assert [(d, t) for d, t, _ in seen] == [(4, spp), (8, spp), (10, spp)]           # a short last chunk
    ref_seen, ref_packed, ref_linear = _single_device_callback_images(device, abi, sc, chunk)
    assert [(d, t) for d, t, _ in ref_seen] == [(d, t) for d, t, _ in seen]
    for (d, _, img), (_, _, ref) in zip(seen, ref_seen):
        assert np.array_equal(img, ref), f"callback image after {d} samples"
    gp, gl, gst = device.render(sc, sc.camera, sc.settings)                           # mi355rt_render
    assert np.array_equal(packed, gp) and np.array_equal(linear.view(np.uint32), gl.view(np.uint32))
    assert np.array_equal(ref_packed, gp) and np.array_equal(ref_linear.view(np.uint32), gl.view(np.uint32))
    assert st.samples == gst.samples and st.rays == gst.rays and st.rows_rendered == H
    # an early stop leaves the image of the samples done
    stops = []
    p4, l4, _ = device.render_progressive_multi(sc, sc.camera, sc.settings, [0, 0], chunk, on_chunk=lambda d, t, img: stops.append(d) or True)
    assert stops == [4]
    gp4, gl4, _ = device.render(sc, sc.camera, abi.Settings(W, H, 4, sc.settings.max_depth))
    assert np.array_equal(p4, gp4) and np.array_equal(l4.view(np.uint32), gl4.view(np.uint32))
    # no callback, packed only
    p, l, _ = device.render_progressive_multi(sc, sc.camera, sc.settings, [0, 0], 3, want_linear=False)
    assert l is None and np.array_equal(p, gp)


def test_headline_frame_in_chunks_of_64(native, abi):
    """cornell 800x600x256 d30 in four chunks of 64 on two parts ends bit-identical to the one-device frame."""
    host, device = native
    sc = _scene(host, "cornell", 800, 600, 256, depth=30)
    m = device.MultiContext([0, 0])
    try:
        m.set_scene(sc, sc.camera, sc.settings)
        opt = abi.Options.make(strip_rows=4)
        packed, linear, _ = _buffers(600, 800)
        samples = 0
        for s in range(0, 256, 64):
            samples += m.render_progressive(s, s + 64, packed, linear, options=opt, want_stats=True).samples
        m.check()
        assert samples == 800 * 600 * 256
    finally:
        m.close()
    gp, gl, _ = device.render(sc, sc.camera, sc.settings, abi.Options.make())
    assert np.array_equal(_bits(packed).reshape(600, 800), gp)
    assert np.array_equal(_bits(linear), gl.reshape(-1).view(np.uint32))
