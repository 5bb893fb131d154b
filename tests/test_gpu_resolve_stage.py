"""k_resolve, color_to_u32, k_gather_strips and k_gather_accum on their own, over non-finite and out-of-range radiance.

The renders feed these kernels finite radiance of a few units and a handful of spp values.  Here the reference build's probe
(csrc/refs/rt_resolve_probe.hip: the shipped launchers on the test's own buffers) runs them on every tail length, on band sizes around the
4-pixel wave and the 16-pixel workgroup, through row tables, with and without running sums, and on values a finite image cannot tell apart:
denormals, signed zeros, infinities, NaNs, sums that overflow midway.

The reference of the sum is numpy float32 over the pixels, acc = f32(acc + x[:, s]) in sample order from +0 (or the loaded sum), then
acc * f32(1 / f32(samples so far)) -- renderer.rs:100-103.  It is compared bit for bit with every NaN as one value
(parity.assert_same_bits_nan_folded).  The reference of the pack is the step function of the bit pattern whose 255 thresholds a bisection
with numpy float32 finds on the CPU (sqrt, clip, * 255, truncate -- color.rs:87-93); the device compares all 2^32 red patterns with it by
integer operations, and only the mismatch count and the first mismatching pattern come back.
"""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from parity import assert_same_bits_nan_folded, nan_folded_bits

F = np.float32
SPPS = list(range(1, 34)) + [47, 48, 49, 63, 64, 65, 255, 256, 257, 1000]
BAND_PIXELS = [1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 4099]
ROW_WIDTHS = [None, 1, 3, 64, 257]                      # None: no row table
PACKED_SENTINEL = 0xDEADBEEF
LINEAR_SENTINEL = 0x7FC12345                            # a NaN with a payload no arithmetic here makes
ACCUM_PREFILL = 0x7FFFDEAD                              # likewise
FLT_MAX = np.finfo(F).max
CLASSES = ("wide", "denormal", "one_nan", "one_pinf", "one_ninf", "both_inf", "overflow", "neg_zero", "negative", "benign")
BENIGN = CLASSES.index("benign")


# ------------------------------------------------------------------------------------------------------------------ inputs and references
def class_of(n_pixels, shift):
    """Pixel p is of class (p + shift) % 10; the position of its special sample is ((p + shift) // 10) % spp."""
    j = np.arange(n_pixels) + shift
    return j % len(CLASSES), j // len(CLASSES)


def make_radiance(n_pixels, spp, seed, shift=0):
    """float32 [n_pixels, spp, 3] of the value classes, dealt over the pixels in turn."""
    rng = np.random.default_rng([seed, n_pixels, spp])
    cls, pos = class_of(n_pixels, shift)
    pos = pos % spp
    x = np.zeros((n_pixels, spp, 3), F)
    for p in range(n_pixels):
        c = CLASSES[cls[p]]
        if c in ("wide", "one_nan", "one_pinf", "one_ninf", "both_inf"):
            # terms of one magnitude per channel (a window of 8 binades somewhere in 2^-140 ... 2^120), mixed signs: every partial sum rounds,
            # so the order of the additions shows in the last bits
            e = rng.integers(-140, 113, 3)
            m = rng.uniform(1.0, 2.0, (spp, 3)) * rng.choice([-1.0, 1.0], (spp, 3))
            x[p] = np.ldexp(m, (e[None, :] + rng.integers(0, 8, (spp, 3)))).astype(F)
            if c == "one_nan":
                x[p, pos[p], :] = np.nan
            elif c == "one_pinf":
                x[p, pos[p], :] = np.inf
            elif c == "one_ninf":
                x[p, pos[p], :] = -np.inf
            elif c == "both_inf":                                        # +inf and -inf at two positions (one sample: a single NaN)
                q = (pos[p] + 1 + int(rng.integers(0, max(spp - 1, 1)))) % spp
                x[p, pos[p], :] = np.inf
                x[p, q, :] = -np.inf if q != pos[p] else np.nan
        elif c == "denormal":
            x[p] = (rng.integers(-(1 << 10), 1 << 16, (spp, 3)).astype(np.float64) * 2.0 ** -149).astype(F)
        elif c == "overflow":                                            # FLT_MAX terms overflow at a position, then -FLT_MAX: stays +inf
            x[p] = rng.uniform(0.0, 1e30, (spp, 3)).astype(F)
            at = pos[p] % max(spp - 1, 1)                                # two FLT_MAX terms in a row (one sample: FLT_MAX alone, finite)
            x[p, at:at + 2, :] = FLT_MAX
            x[p, at + 2:at + 4, :] = -FLT_MAX
        elif c == "neg_zero":
            x[p] = F(-0.0)
        elif c == "negative":
            x[p] = -rng.uniform(0.0, 3.0, (spp, 3)).astype(F)
            x[p, pos[p], 1] = F(0.25)                                    # not every term negative: the total is
            x[p, 0, 0] -= F(1.0)
        else:                                                            # benign: finite radiance of a few units, what the renders produce
            x[p] = rng.uniform(0.0, 1.2 / spp, (spp, 3)).astype(F)
    return x


def sequential_sum(x, start=None):
    """acc = f32(acc + x[:, s]) for s in sample order, from +0 or `start` [P, 3]."""
    acc = np.zeros((x.shape[0], 3), F) if start is None else np.array(start, F)
    with np.errstate(all="ignore"):
        for s in range(x.shape[1]):
            acc = (acc + x[:, s, :]).astype(F)
    return acc


def pairwise_sum(x):
    with np.errstate(all="ignore"):
        while x.shape[1] > 1:
            if x.shape[1] & 1:
                x = np.concatenate([x, np.zeros_like(x[:, :1])], axis=1)
            x = (x[:, 0::2] + x[:, 1::2]).astype(F)
    return x[:, 0]


def scaled(acc, samples):
    with np.errstate(all="ignore"):
        return (acc * (F(1.0) / F(samples))).astype(F)


def pack_byte(bits):
    """The reference's byte of the f32 with these bits: sqrt, clamp(0, 1) where NaN stays, * 255, `as u32` (NaN -> 0), in numpy float32."""
    v = np.asarray(bits, np.uint32).view(F)
    with np.errstate(all="ignore"):
        r = np.sqrt(v)
        r = np.where(r < 0, F(0), np.where(r > 1, F(1), r)).astype(F)        # f32::clamp: NaN stays
        r = (r * F(255.0)).astype(F)
    return np.where(np.isnan(r), 0, np.clip(np.nan_to_num(r, nan=0.0), 0, 4294967295.0)).astype(np.uint32)


def pack_thresholds():
    """t[b - 1] = the smallest bit pattern in [+0, +inf] whose byte is >= b, for b = 1 ... 255 (the byte is monotone there)."""
    out = []
    for b in range(1, 256):
        lo, hi = 0, 0x7F800000                                             # byte(lo) < b <= byte(hi)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if int(pack_byte(np.array([mid], np.uint32))[0]) >= b:
                hi = mid
            else:
                lo = mid
        out.append(hi)
    return np.array(out, np.int64)


def expected_packed(x_pixel):
    """0x00RRGGBB of linear pixels [P, 3] through pack_byte."""
    b = pack_byte(np.ascontiguousarray(x_pixel, F).view(np.uint32))
    return (b[:, 0] << 16) | (b[:, 1] << 8) | b[:, 2]


def row_table(n_rows, seed):
    return np.random.default_rng([seed, n_rows]).permutation(n_rows).astype(np.uint32)


def destinations(band_pixel0, band_pixels, width, out_row):
    g = band_pixel0 + np.arange(band_pixels)
    if out_row is None:
        return g
    jp = g // width
    return out_row[jp].astype(np.int64) * width + (g - jp * width)


# ------------------------------------------------------------------------------------------------------------------ CPU: the references themselves
def test_reference_sum_is_order_sensitive_and_within_the_float64_bound():
    """The wide class must tell a reordered sum from the sequential one: the sequential reference differs from a pairwise (tree) sum in at
    least half of its pixels.  On the benign class the reference lies within spp * 2^-24 * sum|x| of the float64 sum (each of the spp
    additions rounds a partial sum that is at most sum|x|)."""
    for spp in (16, 17, 33, 64, 257):
        n = 400 * len(CLASSES)
        x = make_radiance(n, spp, seed=5)
        cls, _ = class_of(n, 0)
        wide = x[cls == 0]
        seq, tree = sequential_sum(wide), pairwise_sum(wide)
        assert np.isfinite(seq).all()
        differ = (seq.view(np.uint32) != tree.view(np.uint32)).any(-1).mean()
        assert differ >= 0.5, (spp, differ)
        rev = sequential_sum(wide[:, ::-1])
        assert (seq.view(np.uint32) != rev.view(np.uint32)).any(-1).mean() >= 0.5, spp
        ben = x[cls == BENIGN]
        ref64 = ben.astype(np.float64).sum(1)
        bound = spp * 2.0 ** -24 * np.abs(ben.astype(np.float64)).sum(1)
        assert (np.abs(sequential_sum(ben).astype(np.float64) - ref64) <= bound).all(), spp


def test_value_classes_hold_what_they_name():
    spp = 24
    n = len(CLASSES) * spp
    x = make_radiance(n, spp, seed=7)
    cls, pos = class_of(n, 0)
    acc = sequential_sum(x)
    by = {c: acc[cls == i] for i, c in enumerate(CLASSES)}
    assert np.isnan(by["one_nan"]).all() and np.isnan(by["both_inf"]).all()
    assert (by["one_pinf"] == np.inf).all() and (by["one_ninf"] == -np.inf).all() and (by["overflow"] == np.inf).all()
    assert (by["neg_zero"].view(np.uint32) == 0).all()                                     # -0 + ... + -0 from +0 is +0
    assert (by["negative"][:, 0] < 0).all() and (expected_packed(scaled(by["negative"], spp)) >> 16 == 0).all()
    d = by["denormal"]
    assert (np.abs(d) < np.finfo(F).tiny).all() and (d != 0).all()
    assert sorted(set((pos[cls == 2] % spp).tolist())) == list(range(spp))                 # the NaN sits at every sample position once
    assert (expected_packed(scaled(by["benign"], spp)) != 0).all()


def test_pack_thresholds_agree_with_the_oracle(oracle_mod):
    """Each threshold and its predecessor through the oracle's sqrt and color_to_u32, in every channel; negative, NaN and infinite patterns."""
    L = oracle_mod.lib()
    t = pack_thresholds()
    assert len(t) == 255 and (np.diff(t) > 0).all() and t[-1] == 0x3F800000                # byte 255 from 1.0 on
    for b, bits in enumerate(t, start=1):
        for w, want in ((bits, b), (bits - 1, b - 1)):
            r = float(np.array([w], np.uint32).view(F)[0])
            assert L.oracle_color_to_u32(r, r, r) == want * 0x010101, (b, hex(int(w)))
            assert int(pack_byte(np.array([w], np.uint32))[0]) == want
    for w, want in ((0x7F800000, 255), (0x7F7FFFFF, 255), (0x7FC00000, 0), (0xFFC00000, 0), (0x7F800001, 0), (0xFF800000, 0), (0x80000000, 0),
                    (0xBF800000, 0), (0x80000001, 0), (0x00000001, 0)):
        assert int(pack_byte(np.array([w], np.uint32))[0]) == want, hex(w)
        r = float(np.array([w], np.uint32).view(F)[0])
        assert L.oracle_color_to_u32(r, r, r) == want * 0x010101, hex(w)


def test_the_probe_calls_the_librarys_magic_div():
    """The probe's magic pair of `width` is the library's: it defines no magic_div of its own and calls the one definition, rt_prepare.cpp's (declared in
    rt_prepare.h, which rt_host.h brings in), which the render, first_hits and ambient_occlusion call too.  test_row_tables_place_every_pixel checks
    what the pair computes on the device, tests/test_render_plan.py on the CPU."""
    read = lambda path: open(os.path.join(ROOT, "raytracer-rust_amd/csrc", path)).read()
    definition = r"\bmagic_div\(uint32_t d, uint32_t& mul, uint32_t& shift\) \{"
    probe, api, prep = read("refs/rt_resolve_probe.hip"), read("device/rt_api.cpp"), read("device/rt_prepare.cpp")
    assert not re.search(definition, probe) and not re.search(definition, api) and len(re.findall(definition, prep)) == 1
    assert "magic_div(a.width, r.width_mul, r.width_shift);" in probe and '#include "../device/rt_host.h"' in probe
    assert "void magic_div(uint32_t d, uint32_t& mul, uint32_t& shift);" in read("device/rt_prepare.h")
    for f in sorted(os.listdir(os.path.join(ROOT, "raytracer-rust_amd/csrc/device"))):
        assert len(re.findall(definition, read(os.path.join("device", f)))) == (1 if f == "rt_prepare.cpp" else 0), f


# ------------------------------------------------------------------------------------------------------------------ GPU: k_resolve
def run_resolve(device, x, *, band_pixel0=0, width=None, out_row=None, want_linear=True, accum_mode="none", chunks=None, pad=5):
    """One resolve of x [P, spp, 3] (or one per chunk of samples, with running sums) into sentinel-filled buffers.  Returns
    (packed u32 [N], linear words u32 [N, 3] or None, accum words u32 [N, 4] or None, destinations [P]); N = the image and `pad` pixels more."""
    import torch
    P, spp, _ = x.shape
    dest = destinations(band_pixel0, P, width, out_row)
    n_img = (int(out_row.size) * width) if out_row is not None else band_pixel0 + P
    assert dest.max() < n_img and len(set(dest.tolist())) == P
    N = n_img + pad                                                    # every output buffer: N pixels (the kernel may write pixels < n_img only)
    packed = torch.full((N,), PACKED_SENTINEL - (1 << 32), dtype=torch.int32, device="cuda")
    linear = torch.full((N, 3), LINEAR_SENTINEL, dtype=torch.int32, device="cuda") if want_linear else None
    accum = torch.full((N, 4), ACCUM_PREFILL, dtype=torch.int32, device="cuda") if accum_mode != "none" else None
    d_row = torch.from_numpy(out_row.astype(np.int64)).to(torch.int32).cuda() if out_row is not None else None
    chunks = chunks or [spp]
    assert sum(chunks) == spp and (len(chunks) == 1 or accum_mode == "load")
    s0 = 0
    for c in chunks:
        rad = torch.from_numpy(np.ascontiguousarray(x[:, s0:s0 + c, :])).cuda()       # 3 * c * P floats: exactly what the launch reads
        s0 += c
        device.debug_resolve(rad.data_ptr(), packed.data_ptr(), c, F(1.0) / F(s0), P, band_pixel0=band_pixel0,
                             out_linear=linear.data_ptr() if want_linear else 0, accum=accum.data_ptr() if accum is not None else 0,
                             accum_load=accum_mode == "load" and s0 > c, out_row=d_row.data_ptr() if d_row is not None else 0, width=width or 0)
    torch.cuda.synchronize()
    as_u32 = lambda t: None if t is None else t.cpu().numpy().view(np.uint32)
    return as_u32(packed), as_u32(linear), as_u32(accum), dest


def check_resolve(got, x, what, accum_mode="none"):
    packed, linear, accum, dest = got
    spp = x.shape[1]
    acc = sequential_sum(x)
    pixel = scaled(acc, spp)
    assert_same_bits_nan_folded(linear[dest].view(F), pixel, f"{what}: linear") if linear is not None else None
    want_packed = expected_packed(pixel)
    bad = np.nonzero(packed[dest] != want_packed)[0]
    assert bad.size == 0, f"{what}: packed differs at pixel {bad[:5]}: got {[hex(int(v)) for v in packed[dest][bad[:5]]]} want {[hex(int(v)) for v in want_packed[bad[:5]]]} of {pixel[bad[:5]]}"
    outside = np.ones(packed.size, bool)
    outside[dest] = False
    assert (packed[outside] == PACKED_SENTINEL).all(), f"{what}: packed written outside the band"
    if linear is not None:
        assert (linear[outside] == LINEAR_SENTINEL).all(), f"{what}: linear written outside the band"
    if accum is not None:
        assert (accum[outside] == ACCUM_PREFILL).all(), f"{what}: sums written outside the band"
        assert (accum[dest] != ACCUM_PREFILL).all(), f"{what}: a word of the sums kept its pre-fill"
        assert (accum[dest][:, 3] == 0).all(), f"{what}: .w of the sums is not +0"
        assert_same_bits_nan_folded(accum[dest][:, :3].view(F), acc, f"{what}: sums")


def chunked(spp):
    """1, 15, 16, 17, rest -- as far as spp goes."""
    out, left = [], spp
    for c in (1, 15, 16, 17):
        if left > c:
            out.append(c); left -= c
    return out + [left]


@pytest.mark.gpu
@pytest.mark.parametrize("spp", SPPS)
def test_resolve_every_tail_and_band(spp, native):
    """Every spp x band_pixels; band_pixel0, the row table's width, out_linear and the sums' mode take their values in turn, so that each
    meets every spp and every band size."""
    _, device = native
    for bi, P in enumerate(BAND_PIXELS):
        k = SPPS.index(spp) + bi
        width = ROW_WIDTHS[k % len(ROW_WIDTHS)]
        band_pixel0 = (0, 7, 64, 1001)[(k // len(ROW_WIDTHS)) % 4]
        accum_mode = ("none", "store", "load")[(k // 3) % 3] if spp > 1 else ("none", "store")[k % 2]
        want_linear = (k % 4) != 3
        out_row = None
        if width is not None:
            out_row = row_table(-(-(band_pixel0 + P) // width) + 2, seed=k)
        x = make_radiance(P, spp, seed=11, shift=k)
        what = f"spp {spp}, {P} px from {band_pixel0}, row width {width}, sums {accum_mode}, linear {want_linear}"
        got = run_resolve(device, x, band_pixel0=band_pixel0, width=width, out_row=out_row, want_linear=want_linear, accum_mode=accum_mode,
                          chunks=chunked(spp) if accum_mode == "load" else None)
        check_resolve(got, x, what, accum_mode)


@pytest.mark.gpu
@pytest.mark.parametrize("spp", SPPS)
def test_resolve_value_classes_at_every_sample_position(spp, native):
    """10 * spp pixels: every class with its special sample (the NaN, the infinity, the overflow) at every position s < spp; one shot without
    sums, one shot storing them, and in chunks reloading them -- the three must agree with the reference and so with each other."""
    _, device = native
    P = len(CLASSES) * spp
    x = make_radiance(P, spp, seed=13)
    for mode in ("none", "store") + (("load",) if spp > 1 else ()):
        got = run_resolve(device, x, accum_mode=mode, chunks=chunked(spp) if mode == "load" else None)
        check_resolve(got, x, f"spp {spp}, classes, sums {mode}", mode)
    if spp > 2:                                                          # other cuts: the first sample alone, the last alone, halves
        for chunks in ([1, spp - 1], [spp - 1, 1], [spp // 2, spp - spp // 2]):
            check_resolve(run_resolve(device, x, accum_mode="load", chunks=chunks), x, f"spp {spp}, classes, chunks {chunks}", "load")


@pytest.mark.gpu
@pytest.mark.parametrize("width", [1, 3, 64, 257])
def test_row_tables_place_every_pixel(width, native):
    """Under a permutation table every pixel of a band that starts and ends inside a row lands at out_row[g / width] * width + g % width --
    the magic pair of the width over every g the band holds -- and the rows the band does not touch keep the sentinel."""
    _, device = native
    for band_pixel0, P in ((0, 5 * width), (width // 2 + 1, 4 * width + 1), (3 * width - 1, 2), (1000 * width + 7, 3 * width)):
        n_rows = -(-(band_pixel0 + P) // width) + 3
        out_row = row_table(n_rows, seed=width)
        x = make_radiance(P, 3, seed=17, shift=BENIGN)
        for mode in ("none", "store"):
            check_resolve(run_resolve(device, x, band_pixel0=band_pixel0, width=width, out_row=out_row, accum_mode=mode), x,
                          f"row width {width}, {P} px from {band_pixel0}, sums {mode}", mode)


PACK_BAND = 1 << 24


@pytest.mark.gpu
def test_pack_every_bit_pattern(native):
    """spp 1, inv_spp 1: red runs over all 2^32 bit patterns in bands of 2^24 pixels, green and blue over every 257th pattern (offsets
    0x3F000000 and 0x7F000000: around 0.5, and the infinities and NaNs).  Expected: the step function of pack_thresholds() for +0 ... +inf, 0
    for negative and NaN patterns.  The linear plane must hold the input's bits (0 + x is x for everything but -0, which gives +0, and NaN):
    a flushed denormal shows there.  No stride: the sweep is complete."""
    import torch
    _, device = native
    thr = torch.from_numpy(pack_thresholds()).cuda()
    idx = torch.arange(PACK_BAND, dtype=torch.int64, device="cuda")
    packed = torch.empty(PACK_BAND, dtype=torch.int32, device="cuda")
    linear = torch.empty((PACK_BAND, 3), dtype=torch.int32, device="cuda")
    rad = torch.empty((PACK_BAND, 3), dtype=torch.int32, device="cuda")

    def byte_of(w):                                                   # w: int64 patterns in [0, 2^32)
        b = torch.bucketize(w.contiguous(), thr, right=True)
        return torch.where(w > 0x7F800000, torch.zeros_like(b), b)    # NaN patterns and everything with the sign bit

    total_bad = 0
    first = None
    for band in range((1 << 32) // PACK_BAND):
        i = idx + band * PACK_BAND
        w = torch.stack([i, (i * 257 + 0x3F000000) & 0xFFFFFFFF, (i * 257 + 0x7F000000) & 0xFFFFFFFF], dim=1)
        rad.copy_(torch.where(w >= (1 << 31), w - (1 << 32), w).to(torch.int32))
        packed.fill_(PACKED_SENTINEL - (1 << 32)); linear.fill_(LINEAR_SENTINEL)
        device.debug_resolve(rad.data_ptr(), packed.data_ptr(), 1, 1.0, PACK_BAND, out_linear=linear.data_ptr())
        want = (byte_of(w[:, 0]) << 16) | (byte_of(w[:, 1]) << 8) | byte_of(w[:, 2])
        bad = (packed.to(torch.int64) & 0xFFFFFFFF) != want
        lw = linear.to(torch.int64) & 0xFFFFFFFF
        is_nan = (w & 0x7FFFFFFF) > 0x7F800000
        lin_want = torch.where(w == 0x80000000, torch.zeros_like(w), w)
        lin_bad = torch.where(is_nan, (lw & 0x7FFFFFFF) <= 0x7F800000, lw != lin_want).any(dim=1)
        n_bad = int((bad | lin_bad).sum())
        if n_bad and first is None:
            j = int(torch.nonzero(bad | lin_bad)[0])
            first = (band, [hex(int(v)) for v in w[j]], hex(int(packed[j]) & 0xFFFFFFFF), hex(int(want[j])), [hex(int(v)) for v in lw[j]])
        total_bad += n_bad
    assert total_bad == 0, f"{total_bad} patterns pack or pass wrongly; first (band, input words, packed, expected, linear words): {first}"


# ------------------------------------------------------------------------------------------------------------------ GPU: the gathers
def tables(n_rows):
    ident = np.arange(n_rows, dtype=np.uint32)
    inter = np.concatenate([ident[0::2], ident[1::2]])                # staging holds the even rows, then the odd ones ... read back interleaved
    return {"identity": ident, "reversed": ident[::-1].copy(), "interleaved": np.argsort(inter, kind="stable").astype(np.uint32)}


@pytest.mark.gpu
@pytest.mark.parametrize("width", [1, 3, 4, 5, 64, 257])
def test_gathers_move_bits(width, native):
    """Random 32-bit words (NaN payloads, denormals, both zeros among them) through k_gather_strips and k_gather_accum: bit for bit, no NaN
    folding; identity, reversed and interleaved tables; 16-byte aligned and misaligned sources and destinations; with and without the
    linear plane; more rows than the grid has workgroups (2048); and the destination's words before and after the rows keep theirs."""
    import torch
    _, device = native
    rng = np.random.default_rng(width)
    for n_rows in (1, 7, 2100):
        for name, table in tables(n_rows).items():
            d_table = torch.from_numpy(table.astype(np.int64)).to(torch.int32).cuda()
            for src_off, dst_off in ((0, 0), (1, 0), (0, 3), (2, 2), (4, 4)):
                for with_linear in (False, True):
                    PAD = 8
                    words = {k: rng.integers(0, 1 << 32, n_rows * width * k + 2 * PAD, dtype=np.uint64).astype(np.uint32) for k in (1, 3)}
                    words[1][:6] = [0x7FC00001, 0xFFC12345, 0x7F800001, 0x00000001, 0x80000000, 0xFF800000]
                    src = {k: torch.from_numpy(v.view(np.int32)).cuda() for k, v in words.items()}
                    fill = {k: rng.integers(0, 1 << 32, n_rows * width * k + 2 * PAD, dtype=np.uint64).astype(np.uint32) for k in (1, 3)}
                    dst = {k: torch.from_numpy(v.view(np.int32)).cuda() for k, v in fill.items()}
                    sp, dp = src[1][src_off:], dst[1][dst_off:]                       # the planes start src_off / dst_off words into 16-byte aligned buffers
                    sl, dl = src[3][src_off:], dst[3][dst_off:]
                    assert src[1].data_ptr() % 16 == 0 and dst[1].data_ptr() % 16 == 0
                    # extents: each plane holds n_rows * width * k words from its start (PAD >= the largest offset remains behind it)
                    device.debug_gather(d_table.data_ptr(), n_rows, width, src_packed=sp.data_ptr(), dst_packed=dp.data_ptr(),
                                        src_linear=sl.data_ptr() if with_linear else 0, dst_linear=dl.data_ptr() if with_linear else 0)
                    for k, on in ((1, True), (3, with_linear)):
                        got = dst[k].cpu().numpy().view(np.uint32)
                        want = fill[k].copy()
                        if on:
                            rows = words[k][src_off:src_off + n_rows * width * k].reshape(n_rows, width * k)
                            want[dst_off:dst_off + n_rows * width * k] = rows[table].reshape(-1)
                        assert np.array_equal(got, want), (f"{name} table, {n_rows} rows of {width}, plane of {k} words, source +{src_off}, destination +{dst_off}: "
                                                           f"{int((got != want).sum())} words differ, first at {int(np.nonzero(got != want)[0][0])}")
            # the sums: float4 per pixel, both sides on 16 bytes (the contract of the progressive calls)
            a_words = rng.integers(0, 1 << 32, (n_rows + 2) * width * 4, dtype=np.uint64).astype(np.uint32)
            a_words[:4] = [0x7FC00001, 0xFFC12345, 0x00000001, 0x80000000]
            a_fill = rng.integers(0, 1 << 32, (n_rows + 2) * width * 4, dtype=np.uint64).astype(np.uint32)
            a_src, a_dst = torch.from_numpy(a_words.view(np.int32)).cuda(), torch.from_numpy(a_fill.view(np.int32)).cuda()
            one = width * 4                                                           # the destination's rows start one row in; a row before and one behind stay
            device.debug_gather(d_table.data_ptr(), n_rows, width, accum_src=a_src.data_ptr(), accum_dst=a_dst[one:].data_ptr())
            got = a_dst.cpu().numpy().view(np.uint32)
            want = a_fill.copy()
            want[one:one + n_rows * one] = a_words[:n_rows * one].reshape(n_rows, one)[table].reshape(-1)
            assert np.array_equal(got, want), f"sums, {name} table, {n_rows} rows of {width}: {int((got != want).sum())} words differ"
