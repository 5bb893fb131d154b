"""mi355rt_context_denoise / mi355rt_denoise on the GPU against tests/denoise_ref.py, the numpy restatement of the header's definition: the
linear result bit for bit (NaNs folded), the packed words against the oracle's color_to_u32 of the reference's linear result.  Real inputs
(a render and the first hits of the same context), synthetic inputs with the values a filter gets wrong at the sizes where the tiling can go
wrong, the plumbing (aliasing, one output only, guard words, repeats, a second stream, the one-shot) and the refusals on a live context."""
import types

import numpy as np
import pytest

import denoise_cases as cases
import denoise_ref as ref
import fuzz_scenes
from device_buffers import Guarded
from parity import assert_same_bits_nan_folded

pytestmark = pytest.mark.gpu

F = np.float32
GUARD = 256                                                              # bytes behind every output and behind the scratch


def pack(oracle_mod, lin):
    f = oracle_mod.lib().oracle_color_to_u32
    flat = lin.reshape(-1, 3)
    return np.array([f(float(r), float(g), float(b)) for r, g, b in flat], np.uint32).reshape(lin.shape[:2])


def buffers(device, lin, hits):
    """Device buffers of one call: input, hits, scratch, both outputs, each with GUARD bytes of the pattern behind it."""
    R, W = lin.shape[:2]
    n = R * W
    mk = lambda size, data=None: Guarded(size, data, GUARD)
    return types.SimpleNamespace(R=R, W=W, n=n, lin=mk(n * 12, np.array(lin, F, order="C")), hits=mk(n * 48, hits), scratch=mk(device.denoise_scratch_bytes(W, R)),
                                 out=mk(n * 12), packed=mk(n * 4))


def linear_of(b):
    return b.out.read(F, "denoise: the linear output").reshape(b.R, b.W, 3)


def packed_words(b):
    return b.packed.read(np.uint32, "denoise: the packed output").reshape(b.R, b.W)


def run(device, ctx, lin, hits, params=None, want_linear=True, want_packed=True, stream=None):
    import torch
    b = buffers(device, lin, hits)
    ctx.denoise(b.W, b.R, b.lin.ptr, b.hits.ptr, b.scratch.ptr, b.out.ptr if want_linear else None, b.packed.ptr if want_packed else None, params, stream)
    torch.cuda.synchronize()
    b.scratch.read(np.uint8, "denoise: the scratch")
    return b


def check(oracle_mod, device, abi, ctx, lin, hits, what, **kw):
    """One call with both outputs against the reference."""
    want = ref.denoise(lin, hits, **{**ref.DEFAULTS, **kw}) if kw else ref.denoise(lin, hits, **ref.DEFAULTS)
    b = run(device, ctx, lin, hits, abi.DenoiseParams.make(**kw) if kw else None)
    got = linear_of(b)
    assert_same_bits_nan_folded(got, want, what)
    got_packed, want_packed = packed_words(b), pack(oracle_mod, want)
    bad = np.argwhere(got_packed != want_packed)
    assert not len(bad), f"{what}: packed differs at {bad[:6].tolist()}: got {got_packed[tuple(bad[0])]:#x} want {want_packed[tuple(bad[0])]:#x} ({len(bad)} px)"
    return got, want


@pytest.fixture(scope="module")
def ctx(native):
    _, device = native
    c = device.Context(0)
    yield c
    c.close()


def render_and_first_hits(device, abi, sc, W, H, spp, depth):
    """(linear f32 [H, W, 3], hits HIT_DTYPE [H * W]) of one context: Context.render and Context.first_hits."""
    import torch
    c = device.Context(0)
    try:
        c.set_scene(sc, sc.camera, abi.Settings(W, H, spp, depth))
        packed = torch.zeros((H, W), dtype=torch.int32, device="cuda")
        linear = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
        hits = torch.zeros((W * H * 48,), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        c.render(packed.data_ptr(), linear.data_ptr(), abi.Options.make(rng_mode=abi.RNG_CTR))
        c.first_hits(hits.data_ptr())
        torch.cuda.synchronize()
        c.check()
        return linear.cpu().numpy(), hits.cpu().numpy().view(abi.HIT_DTYPE).copy()
    finally:
        c.close()


# ---- 1: real inputs ---------------------------------------------------------------------------------------------------------------------
def test_a_render_of_every_primitive_kind_with_its_first_hits(native, oracle_mod, abi, ctx):
    host, device = native
    sc = fuzz_scenes.random_scene(abi, host, 3, True, coincident=True)
    lin, hits = render_and_first_hits(device, abi, sc, 67, 45, 4, 4)
    miss = hits["primitive"] == abi.NO_HIT
    print("misses", int(miss.sum()), "of", len(hits), "distinct first primitives", len(set(hits["primitive"][~miss].tolist())))
    kinds = set(sc.c.primitives[int(p)].kind for p in hits["primitive"][~miss])
    print("kinds seen first", sorted(kinds))
    assert len(set(hits["primitive"][~miss].tolist())) >= 4 and len(kinds) >= 3          # several surfaces and kinds of guide in one frame
    got, _ = check(oracle_mod, device, abi, ctx, lin, hits, "fuzz scene 67x45x4", levels=5)
    assert (got != lin).any()


def test_cornell_box_with_the_defaults_and_the_quality_gate_on_the_device(native, oracle_mod, abi, ctx):
    host, device = native
    sc = cases.gate_scene(host)
    W, H = cases.GATE_W, cases.GATE_H
    noisy, hits = render_and_first_hits(device, abi, sc, W, H, cases.GATE_SPP, cases.GATE_DEPTH)
    got, _ = check(oracle_mod, device, abi, ctx, noisy, hits, "cornell 96x72x4 d8, defaults")
    clean, _ = render_and_first_hits(device, abi, sc, W, H, cases.GATE_REF_SPP, cases.GATE_DEPTH)      # the existing render call, 1024 spp
    e_noisy, e_out = ref.rmse(noisy, clean), ref.rmse(got, clean)
    print(f"RMSE noisy {e_noisy:.4f} denoised {e_out:.4f} ratio {e_out / e_noisy:.4f}")
    assert e_out / e_noisy <= cases.GATE_LIMIT, (e_out, e_noisy)


# ---- 2: synthetic inputs ----------------------------------------------------------------------------------------------------------------
# (W, H): one pixel; one column and one row (narrower than a tap's reach); smaller than a tile; two tiles by eight, every tile full; five tiles
# by nine with partial tiles on both edges.  At levels 8 the step reaches 128: most taps of every size are outside.
SIZES = [(1, 1), (1, 37), (37, 1), (5, 3), (64, 64), (131, 70)]
SIGMAS = [(2.0, 0.05), (0.4, 0.6)]
SYNTHETIC = [(W, H, lv, ns, sg) for (W, H) in SIZES for (lv, ns, sg) in ((5, 5, 0), (8, 0, 1))] + \
            [(131, 70, 0, 5, 0), (131, 70, 1, 8, 1), (131, 70, 3, 0, 0), (131, 70, 3, 8, 1), (64, 64, 1, 0, 0), (64, 64, 3, 8, 0), (5, 3, 1, 8, 1), (37, 1, 0, 0, 1)]


@pytest.mark.parametrize("W,H,levels,squarings,sg", SYNTHETIC)
def test_synthetic_images_and_guides(W, H, levels, squarings, sg, native, oracle_mod, abi, ctx):
    _, device = native
    lin, hits = cases.synthetic(abi, W, H, 1000 + W * 7 + H)
    if W * H >= 1000:                                                    # what the fixture must hold, asserted on the inputs
        assert np.isnan(lin).any() and np.isposinf(lin).any() and np.isneginf(lin).any() and (lin < 0).any()
        assert ((lin != 0) & (np.abs(lin) < np.finfo(F).tiny)).any()
        miss = hits["primitive"] == abi.NO_HIT
        assert miss.any() and np.isnan(hits["normal"]).any() and (hits["t"][~miss] == 0).any() and np.isnan(hits["t"]).any() and np.isposinf(hits["t"][~miss]).any()
    sc, sp = SIGMAS[sg]
    got, want = check(oracle_mod, device, abi, ctx, lin, hits, f"{W}x{H} levels {levels} squarings {squarings} sigma {sc}/{sp}",
                      levels=levels, normal_squarings=squarings, sigma_color=sc, sigma_plane=sp)
    if levels == 0:
        assert got.view(np.uint32).tobytes() == lin.view(np.uint32).tobytes()
    elif W * H >= 1000:
        assert (want != lin).any()


def test_the_gathering_form_of_the_first_two_levels_gives_the_same_bytes(native, oracle_mod, abi):
    """The diagnostic knob "denoise_staged" = 0 (the A/B of DESIGN.md 4.7): the levels with step 1 and 2 gather from global memory like the later
    ones instead of reading their tile and its halo from LDS.  Same definition, same bytes -- at every size where a tile is partial, alone in
    its row or column, or the halo leaves the window."""
    _, device = native
    c = device.Context(0)
    try:
        c.set_knob("denoise_staged", 0)
        for (W, H), levels in (((131, 70), 1), ((131, 70), 2), ((131, 70), 5), ((64, 64), 2), ((5, 3), 2), ((1, 37), 3), ((37, 1), 1), ((1, 1), 2)):
            lin, hits = cases.synthetic(abi, W, H, 1000 + W * 7 + H)
            check(oracle_mod, device, abi, c, lin, hits, f"gathers {W}x{H} levels {levels}", levels=levels)
    finally:
        c.close()


# ---- 3: plumbing ------------------------------------------------------------------------------------------------------------------------
def test_aliasing_single_outputs_repeats_and_the_one_shot(native, oracle_mod, abi, ctx):
    import torch
    _, device = native
    W, H = 131, 70
    lin, hits = cases.synthetic(abi, W, H, 1000 + W * 7 + H)
    both = run(device, ctx, lin, hits)
    want_lin, want_packed = linear_of(both), packed_words(both)
    assert_same_bits_nan_folded(want_lin, ref.denoise(lin, hits, **ref.DEFAULTS), "defaults")
    # twice: identical bytes
    again = run(device, ctx, lin, hits)
    assert linear_of(again).tobytes() == want_lin.tobytes() and packed_words(again).tobytes() == want_packed.tobytes()
    # one output only: the other buffer is not touched
    only_lin = run(device, ctx, lin, hits, want_packed=False)
    assert linear_of(only_lin).tobytes() == want_lin.tobytes() and only_lin.packed.untouched()
    only_packed = run(device, ctx, lin, hits, want_linear=False)
    assert packed_words(only_packed).tobytes() == want_packed.tobytes() and only_packed.out.untouched()
    # out == in
    for levels in (0, 1, 5):
        p = abi.DenoiseParams.make(levels=levels)
        sep = run(device, ctx, lin, hits, p)
        b = buffers(device, lin, hits)
        b.out.upload(np.array(lin, F, order="C"))
        torch.cuda.synchronize()
        ctx.denoise(W, H, b.out.ptr, b.hits.ptr, b.scratch.ptr, b.out.ptr, b.packed.ptr, p)
        torch.cuda.synchronize()
        assert linear_of(b).tobytes() == linear_of(sep).tobytes() and packed_words(b).tobytes() == packed_words(sep).tobytes(), levels
        b.scratch.read(np.uint8, "denoise: the scratch")
    # the one-shot: host buffers, a context of its own
    one_lin, one_packed = device.denoise(lin, hits)
    assert one_lin.tobytes() == want_lin.tobytes() and one_packed.tobytes() == want_packed.tobytes()
    one_lin, one_packed = device.denoise(lin, hits, abi.DenoiseParams.make(levels=2, normal_squarings=1, sigma_color=0.7, sigma_plane=0.2), want_packed=False)
    assert one_packed is None
    assert_same_bits_nan_folded(one_lin, ref.denoise(lin, hits, levels=2, normal_squarings=1, sigma_color=0.7, sigma_plane=0.2), "one-shot")
    assert device.denoise(lin, hits, want_linear=False)[1].tobytes() == want_packed.tobytes()


def test_a_call_on_a_second_stream_beside_a_render_of_the_same_context(native, oracle_mod, abi):
    import torch
    host, device = native
    sc = cases.gate_scene(host)
    W, H = cases.GATE_W, cases.GATE_H
    c = device.Context(0)
    try:
        c.set_scene(sc, sc.camera, abi.Settings(W, H, 64, cases.GATE_DEPTH))
        want_packed = torch.zeros((H, W), dtype=torch.int32, device="cuda")
        packed = torch.zeros((H, W), dtype=torch.int32, device="cuda")
        c.render(want_packed.data_ptr())
        lin, hits = cases.synthetic(abi, W, H, 77)
        alone = run(device, c, lin, hits)
        b = buffers(device, lin, hits)
        s_render, s_filter = torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()
        c.render(packed.data_ptr(), None, None, s_render.cuda_stream)
        c.denoise(W, H, b.lin.ptr, b.hits.ptr, b.scratch.ptr, b.out.ptr, b.packed.ptr, None, s_filter.cuda_stream)
        c.render(packed.data_ptr(), None, None, s_render.cuda_stream)
        torch.cuda.synchronize()
        c.check()
        assert linear_of(b).tobytes() == linear_of(alone).tobytes() and packed_words(b).tobytes() == packed_words(alone).tobytes()
        assert torch.equal(packed, want_packed)
    finally:
        c.close()


# ---- 4: refusals on a live context --------------------------------------------------------------------------------------------------------
def test_refusals_on_a_live_context_leave_the_outputs_untouched(native, abi, ctx):
    import torch
    _, device = native
    W, H = 5, 3
    lin, hits = cases.synthetic(abi, W, H, 9)
    b = buffers(device, lin, hits)
    i, h, s, o, p = b.lin.ptr, b.hits.ptr, b.scratch.ptr, b.out.ptr, b.packed.ptr
    P = abi.DenoiseParams.make
    calls = [lambda: ctx.denoise(W, H, 0, h, s, o, p), lambda: ctx.denoise(W, H, i, 0, s, o, p), lambda: ctx.denoise(W, H, i, h, 0, o, p),
             lambda: ctx.denoise(W, H, i, h, s, 0, 0), lambda: ctx.denoise(W, H, i, h + 8, s, o, p), lambda: ctx.denoise(W, H, i, h, s + 4, o, p),
             lambda: ctx.denoise(W, H, i + 2, h, s, o, p), lambda: ctx.denoise(W, H, i, h, s, o + 2, p), lambda: ctx.denoise(W, H, i, h, s, o, p + 1),
             lambda: ctx.denoise(0, H, i, h, s, o, p), lambda: ctx.denoise(W, 0, i, h, s, o, p), lambda: ctx.denoise(1 << 16, 1 << 15, i, h, s, o, p),
             lambda: ctx.denoise(W, H, i, h, s, o, p, P(levels=9)), lambda: ctx.denoise(W, H, i, h, s, o, p, P(normal_squarings=9)),
             lambda: ctx.denoise(W, H, i, h, s, o, p, P(sigma_color=0.0)), lambda: ctx.denoise(W, H, i, h, s, o, p, P(sigma_color=float("nan"))),
             lambda: ctx.denoise(W, H, i, h, s, o, p, P(sigma_plane=float("inf"))), lambda: ctx.denoise(W, H, i, h, s, o, p, P(sigma_plane=-1.0))]
    for k, call in enumerate(calls):
        with pytest.raises(device.RenderError) as e:
            call()
        assert e.value.rc == abi.ERR_INVALID, k
    torch.cuda.synchronize()
    assert b.out.untouched() and b.packed.untouched() and b.scratch.untouched()
    assert device.lib().mi355rt_context_check(ctx._h) == 0
    ctx.denoise(W, H, i, h, s, o, p)                                     # and the context still works
    torch.cuda.synchronize()
    assert_same_bits_nan_folded(linear_of(b), ref.denoise(lin, hits, **ref.DEFAULTS), "after the refusals")
