"""The camera masks in k_render_ctr_simple_qc's camera pass: skipping a primitive that no camera ray of the pass's pixels can hit
leaves the candidate untouched, so with the diagnostic knob cam_cull 1 (the default) against 0 (no table: every primitive is tested) the packed
pixels, the linear f32 image and the ray count are the same BITS -- at every samples-per-pixel class of the pass (more than two pixels per pass,
exactly two, one), with an odd width, row windows and strips, a processing order that is not the output order, progressive chunks, and bands that
do not start at pixel 0.  One render is also checked whole against the CPU oracle."""
import numpy as np
import pytest
import torch

from conftest import SCENES
from fuzz_scenes import random_scene
from parity import assert_parity

pytestmark = pytest.mark.gpu

QC = 14                                                           # KERNEL_LOCKSTEP_SIMPLE_QC (rt_device.h)


def _render(device, sc, camera, st, cull, opt=None, knobs=(), chunks=None):
    """(packed u32, linear u32 bits, rays, bands) of one context with cam_cull = cull; chunks: progressive, (s0, s1) pairs."""
    ctx = device.Context(0)
    try:
        ctx.set_knob("cam_cull", cull)
        for k, v in knobs:
            ctx.set_knob(k, v)
        ctx.set_scene(sc, camera, st)
        assert ctx.kernel_variant() == QC
        n = ctx.rows_selected(opt) * st.width
        packed = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
        linear = torch.full((n * 3,), float("nan"), dtype=torch.float32, device="cuda:0")
        rays, bands = 0, 0
        if chunks is None:
            s = ctx.render(packed.data_ptr(), linear.data_ptr(), opt, want_stats=True)
            assert s.samples == n * st.samples_per_pixel
            rays, bands = s.rays, s.bands
        else:
            accum = torch.full((n * 4,), float("nan"), dtype=torch.float32, device="cuda:0")
            for s0, s1 in chunks:
                s = ctx.render_progressive(s0, s1, accum.data_ptr(), packed.data_ptr(), linear.data_ptr(), opt, want_stats=True)
                assert s.samples == n * (s1 - s0)
                rays += s.rays; bands = max(bands, s.bands)
        ctx.check()
        return packed.cpu().numpy().view(np.uint32), linear.cpu().numpy().view(np.uint32), rays, bands
    finally:
        ctx.close()


def _same(device, sc, camera, st, **kw):
    on, off = _render(device, sc, camera, st, 1, **kw), _render(device, sc, camera, st, 0, **kw)
    assert on[2] == off[2], ("rays", on[2], off[2])
    assert np.array_equal(on[0], off[0]), "packed pixels"
    assert np.array_equal(on[1], off[1]), "linear f32"
    return on


def _cornell(host, W, H, spp, depth=8):
    return host.LoadedScene(SCENES["cornell"], W, H, spp, depth)


@pytest.mark.parametrize("spp", [1, 7, 48, 64, 100, 256])
def test_every_class_of_pass(native, abi, spp):
    """A pass walks up to 64 consecutive samples: at 1 / 7 / 48 spp they span more than two pixels (no mask), at 64 and 100 one or two, at 256 one or
    two with most passes inside one pixel."""
    host, device = native
    sc = _cornell(host, 96, 72, spp)
    _same(device, sc, sc.camera, sc.settings)


def test_odd_width(native, abi):
    host, device = native
    sc = _cornell(host, 97, 72, 64)
    _same(device, sc, sc.camera, sc.settings)


@pytest.mark.parametrize("opt_kw", [{"row_begin": 13, "row_end": 40}, {"strip_rows": 4, "n_parts": 3, "part": 1},
                                    {"row_begin": 5, "row_end": 66, "strip_rows": 2, "n_parts": 3, "part": 2}])
def test_row_windows_and_strips(native, abi, opt_kw):
    host, device = native
    sc = _cornell(host, 96, 72, 64)
    _same(device, sc, sc.camera, sc.settings, opt=abi.Options.make(**opt_kw))


def test_processing_order_other_than_output_order(native, abi):
    host, device = native
    sc = _cornell(host, 96, 72, 64)
    ctx = device.Context(0)
    try:
        ctx.set_knob("row_order", 1)
        ctx.set_scene(sc, sc.camera, sc.settings)
        out = torch.zeros(96 * 72, dtype=torch.int32, device="cuda:0")
        ctx.render(out.data_ptr(), None, None, want_stats=True)
        natural, processing, _, cost = ctx.row_tables()
        assert len(cost) == 72 and not np.array_equal(natural, processing)              # the knob does reorder this view
    finally:
        ctx.close()
    ordered = _same(device, sc, sc.camera, sc.settings, knobs=(("row_order", 1),))
    plain = _render(device, sc, sc.camera, sc.settings, 1)
    assert np.array_equal(ordered[0], plain[0]) and np.array_equal(ordered[1], plain[1]) and ordered[2] == plain[2]


def test_progressive_chunks(native, abi):
    host, device = native
    sc = _cornell(host, 96, 72, 64)
    chunks = [(0, 16), (16, 32), (32, 48), (48, 64)]
    got = _same(device, sc, sc.camera, sc.settings, chunks=chunks)
    whole = _render(device, sc, sc.camera, sc.settings, 1)
    assert got[2] == whole[2]                                                             # the same paths (the sums are added in another order: no image comparison)
    sc = _cornell(host, 96, 72, 128)                                                      # ... and chunks of 64: masked passes with sample0 != 0
    _same(device, sc, sc.camera, sc.settings, chunks=[(0, 64), (64, 128)])


def test_three_or_more_bands(native, abi):
    host, device = native
    sc = _cornell(host, 96, 72, 64)
    opt = abi.Options.make(workspace_bytes=96 * 72 * 64 * 12 // 3 - 12 * 64 * 5)         # a little under a third of the frame: four bands, none a whole number of rows
    got = _same(device, sc, sc.camera, sc.settings, opt=opt)
    assert got[3] >= 3
    whole = _render(device, sc, sc.camera, sc.settings, 1)
    assert got[2] == whole[2] and np.array_equal(got[0], whole[0]) and np.array_equal(got[1], whole[1])


@pytest.mark.parametrize("seed", [101, 106])
def test_fuzz_quad_cube_scenes(native, abi, seed):
    host, device = native
    sc = random_scene(abi, host, seed, exact_only=True, n_prims=8, only_kinds=[abi.PRIM_QUAD, abi.PRIM_CUBE], lambert_only=True)
    st = abi.Settings(64, 48, 32, 6)
    _same(device, sc, sc.camera, st)
    st = abi.Settings(64, 48, 64, 6)                                                       # (at 32 spp no pass is masked; at 64 every one is)
    _same(device, sc, sc.camera, st)


def test_whole_image_against_the_oracle(native, oracle_mod, abi):
    host, device = native
    sc = _cornell(host, 96, 72, 32, depth=6)
    opt = abi.Options.make()
    gp, gl, rays, _ = _same(device, sc, sc.camera, sc.settings, opt=opt)
    op, ol, cnt = oracle_mod.render(sc, sc.camera, sc.settings, opt)
    assert_parity(gp.reshape(72, 96), gl.view(np.float32).reshape(72, 96, 3), op, ol, exact=True, gpu_rays=rays, oracle_rays=cnt.rays)
    sc = _cornell(host, 96, 72, 64, depth=6)                                               # ... and at 64 spp, where every pass is masked
    gp, gl, rays, _ = _render(device, sc, sc.camera, sc.settings, 1, opt=opt)
    op, ol, cnt = oracle_mod.render(sc, sc.camera, sc.settings, opt)
    assert_parity(gp.reshape(72, 96), gl.view(np.float32).reshape(72, 96, 3), op, ol, exact=True, gpu_rays=rays, oracle_rays=cnt.rays)
