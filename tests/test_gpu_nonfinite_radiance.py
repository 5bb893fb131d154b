"""Non-finite and out-of-range colours from the path end to the packed pixel, on every kernel variant.

The path ends multiply the throughput by a colour (thr * emitted, thr * miss colour, thr * black where a path runs out of depth); the
reference's arithmetic makes inf * 0 a NaN there, not black, and a negative or overflowing sum what it is.  The poisoned scenes of
tests/nonfinite_cases.py (conditions: test_nonfinite_radiance_cpu.py) are rendered by every variant that accepts them -- the acceptance
table and the knob forcing are test_gpu_variant_matrix.py's -- and must equal the oracle: linear f32 bit for bit with every NaN as one value
(x86 and gfx950 differ in the sign of a default NaN), packed equal, rays equal; the variants among themselves bit for bit, NaNs included.
"""
import numpy as np
import pytest

import nonfinite_cases as nc
import test_gpu_variant_matrix as vm
from parity import assert_same_bits_nan_folded

_oracle = {}


def oracle_of(oracle_mod, abi, host, poison, base, spp=nc.SPP, **opt_kw):
    key = (poison, base, spp, tuple(sorted(opt_kw.items())))
    if key not in _oracle:
        sc = nc.scene(abi, host, base, poison)
        opt = abi.Options.make(**opt_kw) if "rng_mode" in opt_kw else nc.options(abi, base, **opt_kw)     # reference-stream mode takes no flag
        op, ol, cnt = oracle_mod.render(sc, sc.camera, nc.settings(abi, spp), opt)
        _oracle[key] = (op, ol, cnt.rays)
    return _oracle[key]


def like_oracle(got, ora, what, rows=None):
    gp, gl, rays = got
    op, ol, orays = ora
    if rows is not None:
        op, ol = op[rows], ol[rows]
    assert_same_bits_nan_folded(gl, ol, f"{what}: linear against the oracle")
    assert np.array_equal(gp, op), f"{what}: {int((gp != op).sum())} packed pixels differ from the oracle's"
    if rows is None:
        assert rays == orays, f"{what}: rays {rays}, oracle {orays}"


@pytest.mark.gpu
@pytest.mark.parametrize("poison,base,classes", nc.CASES, ids=[f"{p}-{b}" for p, b, _ in nc.CASES])
def test_poisoned_scene_on_every_variant(poison, base, classes, native, oracle_mod, abi):
    host, device = native
    _, _, flagged, exact = nc.BASES[base]
    variants = nc.variants_of(abi, host, base)
    sc, st, opt = nc.scene(abi, host, base, poison), nc.settings(abi), nc.options(abi, base)
    first = None
    for v in variants:
        got = vm.render_ctx(device, abi, sc, v, st, opt)
        if exact:
            like_oracle(got, oracle_of(oracle_mod, abi, host, poison, base), f"{poison} on {base}, variant {v}")
        if first is None:
            first = (v, got)
            shares = nc.class_shares(got[1])
            assert all(shares[c] >= 0.02 for c in classes), (poison, base, shares)           # the device's image shows the classes too
        else:
            vm._same(got, first[1], f"{poison} on {base}: variant {v} against variant {first[0]}")
    if flagged and 8 in variants:                                       # the flag form of every product variant the scene accepts, forced
        f = nc.features_of(abi, sc)
        for forced in (1, 7, 10, 12, 13):
            if vm.accepts(forced, f):
                vm._same(vm.render_ctx(device, abi, sc, 8, st, opt, forced=forced), first[1], f"{poison} on {base}: flag form of {forced}")


@pytest.mark.gpu
@pytest.mark.parametrize("poison,base", nc.REF_CASES, ids=[f"{p}-{b}" for p, b in nc.REF_CASES])
def test_reference_stream_mode_on_poisoned_scenes(poison, base, native, oracle_mod, abi):
    host, device = native
    sc, st = nc.scene(abi, host, base, poison), nc.settings(abi)
    opt = abi.Options.make(rng_mode=abi.RNG_REF)                     # (the flag of the fixed-AABB bases needs counter mode)
    gp, gl, stats = device.render(sc, sc.camera, st, opt)
    like_oracle((gp, gl, stats.rays), oracle_of(oracle_mod, abi, host, poison, base, rng_mode=abi.RNG_REF), f"{poison} on {base}, reference stream")


@pytest.mark.gpu
@pytest.mark.parametrize("poison,base", nc.PATH_CASES, ids=[f"{p}-{b}" for p, b in nc.PATH_CASES])
def test_poisoned_scene_through_bands_rows_chunks_and_devices(poison, base, native, oracle_mod, abi):
    """At 7 spp: bands of 1 and 7 pixels, a row window and strip subsets, progressive chunks 1, 5, rest (image and sums against the one
    shot and the sample-order reference), and the resident multi-device context on devices (0, 0), one shot and progressive."""
    import torch
    host, device = native
    sc, st = nc.scene(abi, host, base, poison), nc.settings(abi, nc.SPP_PATHS)
    ora = oracle_of(oracle_mod, abi, host, poison, base, spp=nc.SPP_PATHS)
    W, spp = st.width, st.samples_per_pixel
    chunks = (1, 5, spp - 6)
    for v in nc.variants_of(abi, host, base):
        what = f"{poison} on {base}, variant {v}"
        full = vm.render_ctx(device, abi, sc, v, st, nc.options(abi, base))
        like_oracle(full, ora, what)
        for label, kw in (("bands of 1 pixel", dict(workspace_bytes=spp * 12 * 1)), ("bands of 7 pixels", dict(workspace_bytes=spp * 12 * 7))):
            vm._same(vm.render_ctx(device, abi, sc, v, st, nc.options(abi, base, **kw)), full, f"{what}, {label}")
        for label, kw in (("rows 5..13", dict(row_begin=5, row_end=13)), ("strips of 2, part 1 of 3", dict(strip_rows=2, n_parts=3, part=1)),
                          ("rows 3..17, strips of 1, part 0 of 4", dict(row_begin=3, row_end=17, n_parts=4, part=0))):
            opt = nc.options(abi, base, **kw)
            rows = abi.rows_selected(st.height, opt)
            gp, gl, _ = vm.render_ctx(device, abi, sc, v, st, opt)
            assert len(rows) > 0
            like_oracle((gp, gl, None), ora, f"{what}, {label}", rows=rows)
            assert np.array_equal(gl.view(np.uint32), full[1][rows].view(np.uint32)) and np.array_equal(gp, full[0][rows]), f"{what}, {label}"
        vm._same(vm.render_ctx(device, abi, sc, v, st, nc.options(abi, base), progressive=chunks), full, f"{what}, progressive chunks")
    # the sums of a progressive sequence on one context: equal to the one shot's image through the sample-order reference
    auto = device.render(sc, sc.camera, st, nc.options(abi, base))
    like_oracle((auto[0], auto[1], auto[2].rays), ora, f"{poison} on {base}, automatic variant")
    n = st.height * W

    def sequence(render):                                            # chunks 1, 5, rest through render(s0, s1, packed, linear, accum)
        packed = torch.zeros(n, dtype=torch.int32, device="cuda")
        linear = torch.zeros(n * 3, dtype=torch.float32, device="cuda")
        accum = torch.full((n * 4,), float("nan"), dtype=torch.float32, device="cuda")
        s = 0
        for c in chunks:
            render(s, s + c, packed, linear, accum)
            s += c
        torch.cuda.synchronize()
        return (packed.cpu().numpy().view(np.uint32).reshape(st.height, W), linear.cpu().numpy().reshape(st.height, W, 3),
                accum.cpu().numpy().reshape(st.height, W, 4))

    def check_sequence(got, what):
        gp, gl, acc = got
        assert np.array_equal(gl.view(np.uint32), auto[1].view(np.uint32)) and np.array_equal(gp, auto[0]), f"{what}: not the one-shot image"
        assert (acc[..., 3].view(np.uint32) == 0).all(), f"{what}: .w of the sums"
        with np.errstate(all="ignore"):
            want = (acc[..., :3] * (np.float32(1.0) / np.float32(spp))).astype(np.float32)      # renderer.rs:103 on the returned sums
        assert_same_bits_nan_folded(want, ora[1], f"{what}: the sums, scaled, against the oracle")

    ctx = device.Context(0)
    try:
        ctx.set_scene(sc, sc.camera, st)
        opt = nc.options(abi, base)
        one = sequence(lambda s0, s1, p, l, a: ctx.render_progressive(s0, s1, a.data_ptr(), p.data_ptr(), l.data_ptr(), opt, want_stats=True))
    finally:
        ctx.close()
    check_sequence(one, f"{poison} on {base}, one context, chunks")
    mc = device.MultiContext([0, 0])
    try:
        mc.set_scene(sc, sc.camera, st)
        opt = nc.options(abi, base)
        packed = torch.zeros(n, dtype=torch.int32, device="cuda")
        linear = torch.zeros(n * 3, dtype=torch.float32, device="cuda")
        stats = mc.render(packed, linear, opt, want_stats=True)
        torch.cuda.synchronize()
        mp, ml = packed.cpu().numpy().view(np.uint32).reshape(st.height, W), linear.cpu().numpy().reshape(st.height, W, 3)
        assert np.array_equal(ml.view(np.uint32), auto[1].view(np.uint32)) and np.array_equal(mp, auto[0]) and stats.rays == auto[2].rays, \
            f"{poison} on {base}: two parts, one shot, against one device"
        multi = sequence(lambda s0, s1, p, l, a: mc.render_progressive(s0, s1, p, l, a, opt, want_stats=True))
        mc.check()
    finally:
        mc.close()
    check_sequence(multi, f"{poison} on {base}, two parts, chunks")
    assert np.array_equal(multi[2].view(np.uint32), one[2].view(np.uint32)), f"{poison} on {base}: the gathered sums against one device's"
