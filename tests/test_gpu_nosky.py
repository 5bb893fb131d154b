"""Variant 14's two entry points.  k_render_ctr_simple_qc is compiled WITHOUT the HDR sky lookup (a miss returns the flat miss colour from scalar
registers), parks the paths' rays inside the empty ring of first hits during a refill pass, and is launched on scenes without a sky texture;
k_render_sky_simple_qc, the body with the lookup, takes the scenes that carry one.  The variant number is 14 for both.

What must hold: every image is the oracle's, bit for bit with equal ray counts (HDR-sky scenes: within the tolerance test_gpu_variant_matrix.py uses
for them, and bit for bit like variant 3, which runs the same device libm); misses in the refill pass and in bounces return the flat colour; the
rays a refill pass parks come back intact (a refill while lanes hold live paths: max_bounces 30 at fewer than 64 samples per pixel); bands, a share
of the device, progressive chunks, a row window and the camera masks change nothing; and the launch follows the scene that is resident NOW."""
import numpy as np
import pytest

import nonfinite_cases as nc
import test_gpu_variant_matrix as vm
from conftest import load_for_both
from parity import assert_parity
from test_gpu_nonfinite_radiance import like_oracle

pytestmark = pytest.mark.gpu

PLAIN, TWIN = "k_render_ctr_simple_qc", "k_render_sky_simple_qc"
WORKGROUPS_PER_CU = {PLAIN: 8, TWIN: 7}                               # 8 waves per SIMD without the lookup (64 VGPRs, 16 KB of LDS), 7 with it
MISS = np.float32([0.25, 0.5, 0.75])                                  # three distinct channels


def render14(device, abi, sc, st, opt=None, progressive=None, knobs=None, share=None, entry=PLAIN):
    """One render on a fresh context with variant 14 forced: (packed [rows, W], linear f32 [rows, W, 3], rays).  Asserts the variant and the entry point."""
    import torch
    opt = opt if opt is not None else abi.Options.make(rng_mode=abi.RNG_CTR)
    ctx = device.Context(0)
    try:
        ctx.set_knob("kernel", 14)
        for name, value in (knobs or {}).items():
            ctx.set_knob(name, value)
        if share is not None:
            ctx.set_share(share)
        ctx.set_scene(sc, sc.camera, st)
        assert ctx.kernel_variant() == 14
        assert ctx.kernel_entry()[0] == entry
        return _render_on(ctx, abi, st, opt, progressive)
    finally:
        ctx.close()


def _render_on(ctx, abi, st, opt, progressive=None):
    import torch
    rows = ctx.rows_selected(opt)
    n = rows * st.width
    packed = torch.zeros(n, dtype=torch.int32, device="cuda")
    linear = torch.zeros(n * 3, dtype=torch.float32, device="cuda")
    if progressive is None:
        stats = [ctx.render(packed.data_ptr(), linear.data_ptr(), opt, want_stats=True)]
    else:
        accum = torch.full((n, 4), float("nan"), dtype=torch.float32, device="cuda")
        s, stats = 0, []
        for c in progressive:
            stats.append(ctx.render_progressive(s, s + c, accum.data_ptr(), packed.data_ptr(), linear.data_ptr(), opt, want_stats=True))
            s += c
        assert s == st.samples_per_pixel
    torch.cuda.synchronize()
    return packed.cpu().numpy().view(np.uint32).reshape(rows, st.width), linear.cpu().numpy().reshape(rows, st.width, 3), sum(x.rays for x in stats)


# ------------------------------------------------------------------------------------------------ the scene of test_gpu_prehit.py
def _opening(oracle_mod, host, W, H, spp, depth):
    from oracle import scene_loader
    sc = load_for_both("cornell", oracle_mod, host, width=W, height=H, spp=spp, max_depth=depth)
    sc.c.miss_color[:] = [float(v) for v in MISS]
    sc.camera = scene_loader.camera_new((0.2, 1.0, 3.0), (0.0, 1.0, 0.0), (0.0, 1.0, 0.0), np.float32(45.0), np.float32(W / H))
    return sc


@pytest.mark.parametrize("W,H,spp", [(37, 29, 7), (53, 41, 3)])
@pytest.mark.parametrize("depth", [1, 30])
def test_misses_in_the_refill_pass_and_in_bounces(W, H, spp, depth, native, oracle_mod, abi):
    host, device = native
    sc = _opening(oracle_mod, host, W, H, spp, depth)
    opt = abi.Options.make(rng_mode=abi.RNG_CTR)
    gp, gl, rays = render14(device, abi, sc, sc.settings, opt)
    op, ol, cnt = oracle_mod.render(sc, sc.camera, sc.settings, opt)
    if depth == 1:                                                     # every path ends at its camera ray: the border is the flat miss colour, the light is in view
        flat = np.abs(ol - MISS).max(axis=-1) < 1e-6                   # (the mean of spp equal samples: the colour up to the rounding of 1 / spp)
        assert flat[:, 0].any() and flat[:, -1].any() and flat.mean() < 0.2
        assert (ol.max(axis=-1) > 1.0).any()
    else:                                                              # bounces leave through the opening: pixels lit by the miss colour beside the light's
        assert cnt.rays > 2 * W * H * spp
    assert cnt.samples == W * H * spp and (W * H * spp) % 64 != 0      # the last run ends on fewer than 64 samples
    assert_parity(gp, gl, op, ol, exact=True, gpu_rays=rays, oracle_rays=cnt.rays)


# ------------------------------------------------------------------------------------------------ cornell at 16 x 8
CW, CH = 16, 8
_cornell = {}


def _cornell_case(native, oracle_mod, abi, spp):
    """(scene, the oracle's frame, the one-shot frame of variant 14) at 16 x 8 x spp, computed once."""
    if spp not in _cornell:
        host, device = native
        sc = load_for_both("cornell", oracle_mod, host, width=CW, height=CH, spp=spp)
        opt = abi.Options.make(rng_mode=abi.RNG_CTR)
        op, ol, cnt = oracle_mod.render(sc, sc.camera, sc.settings, opt)
        _cornell[spp] = (sc, (op, ol, cnt.rays), render14(device, abi, sc, sc.settings, opt))
    return _cornell[spp]


@pytest.mark.parametrize("spp", [4, 64, 67, 256])
def test_cornell_sample_counts(spp, native, oracle_mod, abi):
    sc, (op, ol, orays), (gp, gl, rays) = _cornell_case(native, oracle_mod, abi, spp)
    assert_parity(gp, gl, op, ol, exact=True, gpu_rays=rays, oracle_rays=orays)


def test_cornell_bands_share_chunks_window_and_masks(native, oracle_mod, abi):
    host, device = native
    sc, _, full = _cornell_case(native, oracle_mod, abi, 67)
    st = sc.settings
    band = abi.Options.make(rng_mode=abi.RNG_CTR, workspace_bytes=67 * 12 * (CW * CH // 4))
    vm._same(render14(device, abi, sc, st, band), full, "four bands")
    vm._same(render14(device, abi, sc, st, share=2), full, "set_share(2)")
    vm._same(render14(device, abi, sc, st, progressive=(3, 64)), full, "progressive chunks 3 + 64")
    vm._same(render14(device, abi, sc, st, knobs={"cam_cull": 0}), render14(device, abi, sc, st, knobs={"cam_cull": 1}), "cam_cull 0 against 1")
    vm._same(render14(device, abi, sc, st, knobs={"cam_cull": 0}), full, "cam_cull 0")
    window = abi.Options.make(rng_mode=abi.RNG_CTR, row_begin=2, row_end=7)
    wp, wl, _ = render14(device, abi, sc, st, window)
    assert wp.shape[0] == 5
    assert np.array_equal(wl.view(np.uint32), full[1][2:7].view(np.uint32)) and np.array_equal(wp, full[0][2:7]), "rows 2..7"


# ------------------------------------------------------------------------------------------------ scenes with the 8 x 16 HDR map: the twin
@pytest.mark.parametrize("seed", vm.SEEDS[:2])
def test_sky_scenes_run_the_twin(seed, native, oracle_mod, abi):
    host, device = native
    fam = "lambert_qc"
    sc = vm._scene(abi, host, fam, seed)
    assert sc.c.sky_width == 16 and sc.c.sky_height == 8
    st, opt = abi.Settings(vm.WIDTH, vm.HEIGHT, vm.SPP, vm.DEPTH), vm._options(abi, fam)
    got = render14(device, abi, sc, st, opt, entry=TWIN)
    vm._same(got, vm.render_ctx(device, abi, sc, 3, st, opt), f"{fam} seed {seed}: variant 14 against variant 3")
    assert not vm.exact(fam, seed)
    vm._check_oracle(fam, seed, got, vm._oracle_of(oracle_mod, abi, fam, seed, sc, st, opt, (fam, seed, "frame")))


def test_poisoned_sky_on_the_twin(native, oracle_mod, abi):
    """inf, NaN and denormal texels (fuzz_scenes' `sky` poison on lambert_qc with the map, seed 0).  Held to the bound of test_gpu_nonfinite_radiance.py,
    which is tighter than the HDR-sky tolerance (that one counts every NaN pixel as an outlier): the oracle's words, every NaN one value."""
    host, device = native
    sc, st, opt = nc.scene(abi, host, "qc_sky", "sky"), nc.settings(abi), nc.options(abi, "qc_sky")
    got = render14(device, abi, sc, st, opt, entry=TWIN)
    shares = nc.class_shares(got[1])
    assert all(shares[c] >= 0.02 for c in (nc.NAN, nc.PINF, nc.DEN)), shares
    vm._same(got, vm.render_ctx(device, abi, sc, 3, st, opt), "poisoned sky: variant 14 against variant 3")
    op, ol, cnt = oracle_mod.render(sc, sc.camera, st, opt)
    like_oracle(got, (op, ol, cnt.rays), "poisoned sky, variant 14")


# ------------------------------------------------------------------------------------------------ the launch follows the resident scene
def test_one_context_three_scenes(native, abi):
    host, device = native
    fam = "lambert_qc"
    flat, sky = vm._scene(abi, host, fam, vm.SEEDS[2]), vm._scene(abi, host, fam, vm.SEEDS[0])
    assert flat.c.sky_width == 0 and sky.c.sky_width != 0
    st, opt = abi.Settings(vm.WIDTH, vm.HEIGHT, vm.SPP, vm.DEPTH), vm._options(abi, fam)
    fresh = {id(flat): render14(device, abi, flat, st, opt, entry=PLAIN), id(sky): render14(device, abi, sky, st, opt, entry=TWIN)}
    ctx = device.Context(0)
    try:
        ctx.set_knob("kernel", 14)
        for i, (sc, entry) in enumerate(((flat, PLAIN), (sky, TWIN), (flat, PLAIN))):
            ctx.set_scene(sc, sc.camera, st)
            assert ctx.kernel_variant() == 14
            name, workgroups, vgprs = ctx.kernel_entry()
            assert name == entry and workgroups == WORKGROUPS_PER_CU[entry], (i, name, workgroups, vgprs)
            vm._same(_render_on(ctx, abi, st, opt), fresh[id(sc)], f"set_scene number {i + 1} ({entry}) against a fresh context")
    finally:
        ctx.close()


def test_occupancy_of_the_two_entries(native, oracle_mod, abi):
    """The device holds 8 workgroups of the kernel without the lookup per CU (8 waves per SIMD), 7 of the twin, and the grid follows."""
    host, device = native
    sc = load_for_both("cornell", oracle_mod, host, width=64, height=64, spp=256)
    ctx = device.Context(0)
    try:
        ctx.set_scene(sc, sc.camera, sc.settings)
        assert ctx.kernel_variant() == 14                              # the automatic choice for cornell
        name, workgroups, vgprs = ctx.kernel_entry()
        assert (name, workgroups) == (PLAIN, WORKGROUPS_PER_CU[PLAIN]) and vgprs <= 64, (name, workgroups, vgprs)
    finally:
        ctx.close()
