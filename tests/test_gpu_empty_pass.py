"""Pixels that see nothing cost nothing (rt_kernels.hip): where every camera-mask word of a refill pass of k_render_ctr_simple_qc is 0 the pass
builds no camera ray and walks nothing (FORM_EMPTY_PASS: every lane's "hit" stays false, so HitStock::append stores 1 * miss as it does for any
miss), and k_resolve reads no sample of a pixel whose word is 0 (ResolveParams.cam_mask: the row feeds 1 * miss to the same chain).  No bit may move.

Every case asserts first, through device.camera_masks, that its frame has the pixels the case is about, then renders on variant 14 and compares
packed pixels, linear f32, stats.samples and stats.rays bit for bit with
  * the same render with the knob cam_cull 0 (no table: neither side skips),
  * the library built with the kernel's steps at 0 (build.build_qc_form0: the camera pass without the shortcut),
  * the oracle.
The frames are the smallest with empty runs of every kind: cornell at 16 x 8 (columns 0, 1, 14 and 15 are empty: in processing order a run of four
that crosses the row's end) and the open box of test_gpu_nosky.py at 17 x 9 (an odd width; columns 0, 15 and 16) with a three-channel miss colour;
at 64 samples per pixel a pass is one pixel, at 67 and 100 it lies across two, at 256 most passes lie inside one."""
import importlib

import numpy as np
import pytest

import test_camera_masks as cmasks
import test_gpu_nosky as ns
import test_gpu_variant_matrix as vm
from conftest import load_for_both
from parity import assert_parity, assert_same_bits_nan_folded

pytestmark = pytest.mark.gpu

F = np.float32
PLAIN = ns.PLAIN


def _form0(device):
    return device.load(importlib.import_module("raytracer-rust_amd.build").build_qc_form0())


def render(device, abi, sc, cam, st, library=None, knobs=None, opt=None, share=None, chunks=None, want_linear=True, entry=PLAIN, variant=14):
    """(packed u32 [rows, W], linear f32 [rows, W, 3] or None, samples, rays, bands) of one fresh context.  chunks: progressive sample counts."""
    import torch
    ctx = device.Context(0, library=library)
    try:
        ctx.set_knob("kernel", variant)
        for name, value in (knobs or {}).items():
            ctx.set_knob(name, value)
        if share is not None:
            ctx.set_share(share)
        ctx.set_scene(sc, cam, st)
        assert ctx.kernel_variant() == variant and (entry is None or ctx.kernel_entry()[0] == entry)
        rows = ctx.rows_selected(opt)
        n = rows * st.width
        packed = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
        linear = torch.full((n * 3,), float("nan"), dtype=torch.float32, device="cuda:0") if want_linear else None
        lin_ptr = linear.data_ptr() if want_linear else None
        if chunks is None:
            stats = [ctx.render(packed.data_ptr(), lin_ptr, opt, want_stats=True)]
        else:
            accum = torch.full((n, 4), float("nan"), dtype=torch.float32, device="cuda:0")
            s, stats = 0, []
            for c in chunks:
                stats.append(ctx.render_progressive(s, s + c, accum.data_ptr(), packed.data_ptr(), lin_ptr, opt, want_stats=True))
                s += c
            assert s == st.samples_per_pixel
        ctx.check()
        render.last_row_tables = ctx.row_tables()
        return (packed.cpu().numpy().view(np.uint32).reshape(rows, st.width), linear.cpu().numpy().reshape(rows, st.width, 3) if want_linear else None,
                sum(x.samples for x in stats), sum(x.rays for x in stats), max(x.bands for x in stats))
    finally:
        ctx.close()


def same(a, b, what):
    assert np.array_equal(a[0], b[0]), f"{what}: {int((a[0] != b[0]).sum())} packed pixels differ"
    if a[1] is not None and b[1] is not None:
        assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), f"{what}: linear differs in {int((a[1].view(np.uint32) != b[1].view(np.uint32)).any(-1).sum())} px"
    assert (a[2], a[3]) == (b[2], b[3]), f"{what}: samples, rays {a[2:4]} vs {b[2:4]}"


def three_ways(device, abi, sc, cam, st, what, knobs=None, **kw):
    """The product's render, after checking it against cam_cull 0 and against the library with the kernel's steps at 0."""
    got = render(device, abi, sc, cam, st, knobs=knobs, **kw)
    same(got, render(device, abi, sc, cam, st, knobs=dict(knobs or {}, cam_cull=0), **kw), f"{what}: against cam_cull 0")
    same(got, render(device, abi, sc, cam, st, library=_form0(device), knobs=knobs, **kw), f"{what}: against the form-0 library")
    return got


def masks_of(device, sc, cam, st, opt=None):
    m = device.camera_masks(sc, cam, st, options=opt)
    assert m is not None
    return m


def has_both(m):
    return bool((m == 0).any() and (m != 0).any())


def runs(m):
    """Over the pixels in processing order (row-major): (an empty / non-empty neighbour pair exists, an empty pair exists, an empty pair across a row's end exists)."""
    e = (m == 0).reshape(-1)
    pair = e[:-1] & e[1:]
    last_of_row = (np.arange(e.size - 1) % m.shape[1]) == m.shape[1] - 1
    return bool((e[:-1] != e[1:]).any()), bool(pair.any()), bool((pair & last_of_row).any())


# ------------------------------------------------------------------------------------------------ the two frames
_scenes = {}


def frame(oracle_mod, host, name, spp, depth):
    """(scene, camera) of "cornell" (16 x 8) or "open" (the open box, 17 x 9, the three-channel miss colour)."""
    key = (name, spp, depth)
    if key not in _scenes:
        if name == "cornell":
            sc = load_for_both("cornell", oracle_mod, host, width=16, height=8, spp=spp, max_depth=depth)
        else:
            sc = ns._opening(oracle_mod, host, 17, 9, spp, depth)
        _scenes[key] = sc
    return _scenes[key], _scenes[key].camera


@pytest.mark.parametrize("depth", [1, 30])
@pytest.mark.parametrize("spp", [64, 67, 100, 256])
@pytest.mark.parametrize("name", ["cornell", "open"])
def test_frames_with_empty_pixels(name, spp, depth, native, oracle_mod, abi):
    host, device = native
    sc, cam = frame(oracle_mod, host, name, spp, depth)
    st = sc.settings
    m = masks_of(device, sc, cam, st)
    assert has_both(m)
    mixed, empty_pair, across_rows = runs(m)
    assert mixed and empty_pair and across_rows                      # a pass across two pixels finds: one empty and one not; both empty; both empty, one row apart
    opt = abi.Options.make(rng_mode=abi.RNG_CTR)
    got = three_ways(device, abi, sc, cam, st, f"{name} x {spp}, depth {depth}", opt=opt)
    op, ol, cnt = oracle_mod.render(sc, cam, st, opt)
    assert got[2] == cnt.samples == m.size * spp
    assert_parity(got[0], got[1], op, ol, exact=True, gpu_rays=got[3], oracle_rays=cnt.rays)
    if name == "open":                                                # the empty pixels hold the miss colour: the mean of spp equal samples
        assert (np.abs(got[1][m == 0] - ns.MISS) < 1e-6).all()


# ------------------------------------------------------------------------------------------------ further frames
def away_camera():
    from oracle import scene_loader
    return scene_loader.camera_new((0.0, 1.0, 3.0), (0.0, 1.0, 9.0), (0.0, 1.0, 0.0), F(45.0), F(2.0))


@pytest.mark.parametrize("spp", [64, 67])
def test_a_camera_that_sees_nothing(spp, native, oracle_mod, abi):
    """Every pass is empty: no ring entry is ever made, and the waves must still end."""
    host, device = native
    sc, _ = frame(oracle_mod, host, "open", spp, 30)
    cam, st = away_camera(), sc.settings
    assert (masks_of(device, sc, cam, st) == 0).all()
    opt = abi.Options.make(rng_mode=abi.RNG_CTR)
    got = three_ways(device, abi, sc, cam, st, f"nothing in view x {spp}", opt=opt)
    op, ol, cnt = oracle_mod.render(sc, cam, st, opt)
    assert got[2] == got[3] == 17 * 9 * spp                           # one ray per path
    assert_parity(got[0], got[1], op, ol, exact=True, gpu_rays=got[3], oracle_rays=cnt.rays)


def test_a_single_pixel_that_is_not_empty(native, oracle_mod, abi):
    host, device = native
    sc = cmasks.hand_scene(abi, [cmasks.quad_prim(abi, (0.02, 1, 0.02), (90, 0, 0), (3.2, 2.4, 0))])
    cam, st = cmasks.hand_camera(), abi.Settings(cmasks.HAND_W, cmasks.HAND_H, 64, 3)
    m = masks_of(device, sc, cam, st)
    assert int((m != 0).sum()) == 1
    opt = abi.Options.make(rng_mode=abi.RNG_CTR)
    got = three_ways(device, abi, sc, cam, st, "one pixel", opt=opt)
    op, ol, cnt = oracle_mod.render(sc, cam, st, opt)
    assert_parity(got[0], got[1], op, ol, exact=True, gpu_rays=got[3], oracle_rays=cnt.rays)


def test_bands_windows_strips_order_share_and_planes(native, oracle_mod, abi):
    """Everything that changes which words the two kernels read for a pixel, each against the whole frame's render (checked against the oracle above)."""
    host, device = native
    sc, cam = frame(oracle_mod, host, "cornell", 67, 30)
    st = sc.settings
    m = masks_of(device, sc, cam, st)
    full = render(device, abi, sc, cam, st, opt=abi.Options.make(rng_mode=abi.RNG_CTR))
    # four bands of 32 pixels = two rows: every band boundary lies between column 15 of a row and column 0 of the next, inside an empty run
    assert (m[:, [0, 1, 14, 15]] == 0).all()
    band = abi.Options.make(rng_mode=abi.RNG_CTR, workspace_bytes=67 * 12 * (16 * 8 // 4))
    got = three_ways(device, abi, sc, cam, st, "four bands", opt=band)
    assert got[4] == 4
    same(got, full, "four bands against one")
    for what, kw, rows in (("a row window", dict(row_begin=2, row_end=7), slice(2, 7)),
                           ("strips", dict(strip_rows=2, n_parts=2, part=1), [2, 3, 6, 7])):
        opt = abi.Options.make(rng_mode=abi.RNG_CTR, **kw)
        assert has_both(masks_of(device, sc, cam, st, opt))
        got = three_ways(device, abi, sc, cam, st, what, opt=opt)
        assert np.array_equal(got[0], full[0][rows]) and np.array_equal(got[1].view(np.uint32), full[1][rows].view(np.uint32)), what
    same(three_ways(device, abi, sc, cam, st, "row_order 1", opt=abi.Options.make(rng_mode=abi.RNG_CTR), knobs={"row_order": 1}), full, "row_order 1")
    natural, processing, _, _ = render.last_row_tables
    assert not np.array_equal(natural, processing)                    # (the knob does reorder this view: the resolve finds a pixel's word by its processing row)
    same(three_ways(device, abi, sc, cam, st, "set_share(4)", opt=abi.Options.make(rng_mode=abi.RNG_CTR), share=4), full, "set_share(4)")
    no_linear = three_ways(device, abi, sc, cam, st, "no linear plane", opt=abi.Options.make(rng_mode=abi.RNG_CTR), want_linear=False)
    same(no_linear, full, "without the linear plane")
    same(render(device, abi, sc, cam, st, knobs={"resolve_skip": 0}), full, "resolve_skip 0")


@pytest.mark.parametrize("chunks", [(3, 64), (64, 64)])
def test_progressive_chunks(chunks, native, oracle_mod, abi):
    """Running sums in d_accum: the second chunk's resolve loads them, for empty pixels too (sample0 != 0 in the second render launch)."""
    host, device = native
    sc, cam = frame(oracle_mod, host, "open", sum(chunks), 30)
    st = sc.settings
    assert has_both(masks_of(device, sc, cam, st))
    opt = abi.Options.make(rng_mode=abi.RNG_CTR)
    got = three_ways(device, abi, sc, cam, st, f"chunks {chunks}", opt=opt, chunks=chunks)
    same(got, render(device, abi, sc, cam, st, opt=opt), f"chunks {chunks} against one call")    # (sums of one pixel in sample order either way)
    op, ol, cnt = oracle_mod.render(sc, cam, st, opt)
    assert_parity(got[0], got[1], op, ol, exact=True, gpu_rays=got[3], oracle_rays=cnt.rays)


def test_a_miss_colour_that_is_not_finite(native, oracle_mod, abi):
    """-0.0, +inf and NaN: the constant goes through the same additions, 1 / spp, square root and pack as the stored samples."""
    host, device = native
    sc = ns._opening(oracle_mod, host, 17, 9, 67, 30)
    sc.c.miss_color[:] = [-0.0, float("inf"), float("nan")]
    cam, st = sc.camera, sc.settings
    assert has_both(masks_of(device, sc, cam, st))
    opt = abi.Options.make(rng_mode=abi.RNG_CTR)
    got = three_ways(device, abi, sc, cam, st, "miss (-0, inf, NaN)", opt=opt)
    op, ol, cnt = oracle_mod.render(sc, cam, st, opt)
    assert_same_bits_nan_folded(got[1], ol, "miss (-0, inf, NaN): linear against the oracle")
    assert np.array_equal(got[0], op) and got[3] == cnt.rays


def test_below_64_samples_per_pixel(native, oracle_mod, abi):
    """A pass spans more than two pixels: the camera pass is as it was; the resolve still skips (a pixel's word does not depend on the sample count)."""
    host, device = native
    sc, cam = frame(oracle_mod, host, "open", 7, 30)
    st = sc.settings
    assert has_both(masks_of(device, sc, cam, st))
    opt = abi.Options.make(rng_mode=abi.RNG_CTR)
    got = three_ways(device, abi, sc, cam, st, "7 spp", opt=opt)
    op, ol, cnt = oracle_mod.render(sc, cam, st, opt)
    assert_parity(got[0], got[1], op, ol, exact=True, gpu_rays=got[3], oracle_rays=cnt.rays)


def test_a_sky_texture_keeps_every_read(native, abi):
    """The twin stores a texel per miss, not a constant: its resolve gets no table, although the frame has empty pixels.  Equal to variant 3."""
    host, device = native
    fam, seed = "lambert_qc", vm.SEEDS[0]
    sc = vm._scene(abi, host, fam, seed)
    assert sc.c.sky_width != 0
    st, opt = abi.Settings(vm.WIDTH, vm.HEIGHT, 64, vm.DEPTH), vm._options(abi, fam)
    assert has_both(masks_of(device, sc, sc.camera, st))
    got = render(device, abi, sc, sc.camera, st, opt=opt, entry=ns.TWIN)
    same(got, render(device, abi, sc, sc.camera, st, opt=opt, variant=3, entry=None), "the twin against variant 3")
    same(got, render(device, abi, sc, sc.camera, st, opt=opt, entry=ns.TWIN, knobs={"cam_cull": 0}), "the twin against cam_cull 0")


def test_a_list_of_33_primitives_has_no_table(native, oracle_mod, abi):
    host, device = native
    prims = [cmasks.quad_prim(abi, (0.2, 1, 0.2), (90, 0, 0), (0.1 * k - 1.6, 0, 0)) for k in range(33)]
    sc = cmasks.hand_scene(abi, prims)
    cam, st = cmasks.hand_camera(), abi.Settings(cmasks.HAND_W, cmasks.HAND_H, 64, 3)
    assert device.camera_masks(sc, cam, st) is None
    opt = abi.Options.make(rng_mode=abi.RNG_CTR)
    got = three_ways(device, abi, sc, cam, st, "33 primitives", opt=opt)
    op, ol, cnt = oracle_mod.render(sc, cam, st, opt)
    assert_parity(got[0], got[1], op, ol, exact=True, gpu_rays=got[3], oracle_rays=cnt.rays)


# ------------------------------------------------------------------------------------------------ the resolve on its own
MISS_PROBE = F([0.25, -0.0, 3.5])


@pytest.mark.parametrize("with_accum", [False, True])
@pytest.mark.parametrize("spp", [1, 15, 16, 17, 256])
def test_resolve_with_mask_words(spp, with_accum, native):
    """mi355rt_debug_resolve_masked on 23 pixels (five full waves and a wave of three rows): pixels whose word is 0 hold garbage in the workspace
    and must come out as the plain path makes them from a workspace filled with 1 * miss; pixels with another word, and every pixel when the
    table is absent, come out as the plain path makes them from the workspace as it is."""
    import torch
    _, device = native
    P = 23
    rng = np.random.default_rng([spp, int(with_accum)])
    words = np.where(np.arange(P) % 3 == 1, 0, rng.integers(1, 1 << 32, P)).astype(np.uint32)       # 0 at pixels 1, 4, 7, ...: rows of one wave differ
    words[8:12] = 0                                                                                  # ... and one wave whose four rows are all empty
    real = rng.uniform(0.0, 2.0, (P, spp, 3)).astype(F)
    filled, garbage = real.copy(), real.copy()
    filled[words == 0] = F(1.0) * MISS_PROBE
    garbage[words == 0] = F("nan")
    start = rng.uniform(0.0, 9.0, (P, 4)).astype(F)
    inv = F(1.0) / F(spp + (5 if with_accum else 0))

    def run(rad, mask, masked_hook):
        d_rad = torch.from_numpy(rad.reshape(-1).copy()).cuda()
        packed = torch.full((P,), -1, dtype=torch.int32, device="cuda:0")
        linear = torch.full((P * 3,), float("nan"), dtype=torch.float32, device="cuda:0")
        accum = torch.from_numpy(start.copy()).cuda() if with_accum else None
        kw = dict(out_linear=linear.data_ptr(), accum=accum.data_ptr() if with_accum else 0, accum_load=with_accum)
        d_mask = torch.from_numpy(mask.view(np.int32).copy()).cuda() if mask is not None else None
        if masked_hook:
            device.debug_resolve_masked(d_rad.data_ptr(), packed.data_ptr(), spp, inv, P, d_mask.data_ptr() if mask is not None else 0, MISS_PROBE, **kw)
        else:
            device.debug_resolve(d_rad.data_ptr(), packed.data_ptr(), spp, inv, P, **kw)
        torch.cuda.synchronize()
        return (packed.cpu().numpy().view(np.uint32), linear.cpu().numpy().view(np.uint32),
                accum.cpu().numpy().view(np.uint32) if with_accum else np.zeros(0, np.uint32))

    want = run(filled, None, False)
    for what, got in (("mask words, garbage under the empty pixels", run(garbage, words, True)),
                      ("mask words over the filled workspace", run(filled, words, True)),
                      ("no table", run(filled, None, True)),
                      ("words that are all non-zero", run(filled, np.full(P, 7, np.uint32), True))):
        for a, b, plane in zip(got, want, ("packed", "linear", "accum")):
            assert np.array_equal(a, b), f"spp {spp}: {what}: {plane}"
    assert not np.array_equal(run(garbage, None, True)[1], want[1])   # (the garbage does show when it is read)
