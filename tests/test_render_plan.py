"""The plan of a render call without a GPU (csrc/device/rt_prepare.cpp plan_render, halve_bands, render_band, row_tables and magic_div through
mi355rt_debug_plan_render -- the functions mi355rt_context_render itself calls): the refusals and their precedence, the variant that is launched,
the bands and the geometry of each band's launch against the model of tests/test_gpu_fullsize.py, the halving of bands that do not fit, the
magic pairs and the row tables of the processing order.  The CPU twin of what test_gpu_parity / fullsize / row_order / robustness / share and the
variant matrix exercise end to end; tests/test_gpu_render_plan.py ties the hook to the call."""
import itertools

import numpy as np
import pytest

import test_gpu_variant_matrix as M
from test_gpu_fullsize import RUN_LIMIT, WORK_SHARDS, _band_model, _band_plan, _boundary_rows

LOCKSTEP_MESHFREE = (0, 3, 9, 14)                       # rt_device.h VARIANT_TABLE: FAMILY_LOCKSTEP and compiled without meshes
WAVEFRONT = (7, 8, 10, 11, 12, 13)
FLAGS_TEXT = "options.flags has unknown bits"
FIXED_TEXT = "MI355RT_FLAG_FIXED_AABB needs MI355RT_RNG_CTR (the replay mode reproduces the reference as it is)"
PROGRESSIVE_TEXT = "progressive rendering needs MI355RT_RNG_CTR (the reference stream of a row is sequential over its pixels)"
WORKSPACE_TEXT = "workspace_bytes too small for one pixel (needs spp * 12 bytes)"


def runs(v):
    """(shortest, longest) run of samples a wave of variant v claims (rt_device.h: RUN_WAVEFRONT fixed, BATCH_MIN .. BATCH_MAX guided)."""
    return (256, 256) if v in WAVEFRONT else (128, 256)


def refused(device, abi, settings, options=None, **kw):
    with pytest.raises(device.RenderError) as e:
        device.plan_render(settings, options, **kw)
    assert e.value.rc == abi.ERR_INVALID
    return str(e.value).split(": ", 1)[1]


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_their_texts_and_their_precedence(native, abi):
    _, device = native
    st = abi.Settings(33, 35, 3, 6)
    O = abi.Options.make
    # 1. what select_rows refuses
    assert refused(device, abi, st, O(row_begin=5, row_end=36)) == "row selection out of range"
    assert refused(device, abi, st, O(n_parts=2, part=2)) == "row selection out of range"
    assert refused(device, abi, st, O(rng_mode=7)) == "options.rng_mode"
    bad = O()
    bad.abi_version = 3
    assert refused(device, abi, st, bad) == "options.abi_version mismatch"
    assert refused(device, abi, st, O(row_begin=5, row_end=36, flags=2)) == "row selection out of range"               # ... before the flags
    # 2. unknown flag bits, 3. the flag in the replay mode
    assert refused(device, abi, st, O(flags=2)) == FLAGS_TEXT
    assert refused(device, abi, st, O(flags=2 | abi.FLAG_FIXED_AABB, rng_mode=abi.RNG_REF)) == FLAGS_TEXT               # 2 before 3
    assert refused(device, abi, st, O(flags=abi.FLAG_FIXED_AABB, rng_mode=abi.RNG_REF)) == FIXED_TEXT
    assert refused(device, abi, st, O(flags=abi.FLAG_FIXED_AABB, rng_mode=abi.RNG_REF, workspace_bytes=8), s0=1, s1=2) == FIXED_TEXT   # 3 before 5 and 6
    assert refused(device, abi, st, O(flags=abi.FLAG_FIXED_AABB, rng_mode=abi.RNG_REF, row_begin=4, row_end=4)) == FIXED_TEXT           # ... and before 4
    # 4. an empty selection is OK and wins over 5 and 6
    for opt in (O(row_begin=7, row_end=7, workspace_bytes=8), O(strip_rows=35, n_parts=2, part=1, workspace_bytes=8),
                O(row_begin=7, row_end=7, rng_mode=abi.RNG_REF)):
        for kw in ({}, dict(s0=1, s1=2, have_accum=True)):
            r = device.plan_render(st, opt, **kw)
            assert (r.plan.n_bands, r.plan.total_pixels, len(r.bands), len(r.natural)) == (0, 0, 0, 0)
    # 5. the replay mode renders whole sample ranges without sums
    ref = O(rng_mode=abi.RNG_REF)
    assert refused(device, abi, st, ref, have_accum=True) == PROGRESSIVE_TEXT
    assert refused(device, abi, st, ref, s0=1) == PROGRESSIVE_TEXT
    assert refused(device, abi, st, ref, s1=2) == PROGRESSIVE_TEXT
    assert refused(device, abi, st, O(rng_mode=abi.RNG_REF, workspace_bytes=8), s1=2) == PROGRESSIVE_TEXT              # (the workspace is not the replay mode's)
    r = device.plan_render(st, O(rng_mode=abi.RNG_REF, workspace_bytes=8, seed=(5 << 32) | 9))
    assert (r.plan.rng_mode, r.plan.n_bands, r.plan.block_threads, len(r.bands)) == (abi.RNG_REF, 1, 64, 0)
    assert (r.plan.seed, r.plan.seed_lo, r.plan.seed_hi) == ((5 << 32) | 9, 9, 5)
    # 6. a workspace below one pixel
    assert refused(device, abi, st, O(workspace_bytes=3 * 12 - 1)) == WORKSPACE_TEXT
    assert refused(device, abi, st, O(workspace_bytes=8)) == WORKSPACE_TEXT
    assert refused(device, abi, st, O(workspace_bytes=12), s0=2, s1=4, have_accum=True) == WORKSPACE_TEXT
    assert device.plan_render(st, O(workspace_bytes=12), s0=2, s1=3, have_accum=True).plan.band_pixels == 1
    assert device.plan_render(st, O(workspace_bytes=3 * 12)).plan.band_pixels == 1


# ---------------------------------------------------------------------------------------------------------------- the band plan
def check_invariants(r, v, slots, grid_div):
    p, b = r.plan, r.bands
    assert p.n_bands == len(b) and p.total_pixels == int(b["band_pixels"].astype(np.int64).sum())
    assert b["band_pixel0"].astype(np.int64).tolist() == [0] + np.cumsum(b["band_pixels"].astype(np.int64))[:-1].tolist()   # the bands tile [0, total) in order
    assert (b["band_pixels"][:-1] == p.band_pixels).all() and 1 <= b["band_pixels"][-1] <= p.band_pixels
    samples = b["band_samples"].astype(np.int64)
    assert (samples == b["band_pixels"].astype(np.int64) * p.spp).all() and (samples < 1 << 31).all()
    run_min, run_max = runs(v)
    shard = b["shard_samples"].astype(np.int64)
    assert (shard % run_max == 0).all() and (WORK_SHARDS * shard >= samples).all()
    waves = p.block_threads // 64
    assert p.block_threads == M.block_threads(v) and p.resident == max(1, slots // grid_div)
    assert (b["grid"] >= 1).all() and (b["grid"] <= max(1, slots // grid_div)).all()
    assert (b["grid"] <= np.maximum(1, -(-(-(-samples // run_min)) // waves))).all()
    assert (b["guided_div"] >= 1).all()


def test_bands_and_launches_follow_the_model(native, abi):
    """Small shapes over the workspace sizes at which the plan takes another path: the default (one band), exactly one pixel, 3 and 7 pixels, one
    sample short of two pixels; whole and partial sample ranges; a lockstep and a wavefront kernel, a device that holds few workgroups and one
    that holds many, a share of it."""
    _, device = native
    n = 0
    for width, rows, spp in itertools.product((1, 33, 64), (1, 7, 35), (1, 3, 256)):
        st = abi.Settings(width, 40, spp, 8)
        for (s0, s1), v_slots_div in itertools.product(((0, spp), (spp // 2, spp)) if spp > 1 else ((0, 1), (5, 6)),
                                                       ((14, 1024, 1), (10, 7, 1), (11, 512, 4))):
            v, slots, grid_div = v_slots_div
            launch = s1 - s0
            for ws in (0, launch * 12, 3 * launch * 12, 7 * launch * 12, 2 * launch * 12 - 12):
                r = device.plan_render(st, abi.Options.make(row_begin=2, row_end=2 + rows, workspace_bytes=ws), s0=s0, s1=s1, have_accum=s0 != 0,
                                       variant=v, has_mesh=v == 10, block_slots=slots, grid_div=grid_div, guided_mult=16)
                run_min, run_max = runs(v)
                band_pixels, bands = _band_model(width * rows, launch, ws, run_min, run_max, M.block_threads(v) // 64, max(1, slots // grid_div), 16)
                assert r.plan.band_pixels == band_pixels and r.bands.tolist() == bands, (width, rows, spp, s0, s1, v, ws)
                assert (r.plan.spp, r.plan.sample0, r.plan.accum_load, r.plan.variant, r.plan.order_groups) == (launch, s0, int(s0 != 0), v, 0)
                assert r.plan.inv_spp == np.float32(1.0) / np.float32(s1) and r.natural.tolist() == list(range(2, 2 + rows))
                check_invariants(r, v, slots, grid_div)
                n += 1
    assert n == 27 * 2 * 3 * 5


def test_settings_words_are_the_arithmetic_the_kernels_expect(native, abi):
    _, device = native
    for width, height in ((1, 1), (3, 7), (800, 600), (1920, 1080), (4097, 33), ((1 << 24) - 1, 3)):
        p = device.plan_render(abi.Settings(width, height, 2, 4), abi.Options.make(row_begin=0, row_end=1, seed=0xFFFFFFFF00000001)).plan
        assert (p.width, p.width_f, p.height_f) == (width, float(width), float(height))
        assert p.inv_width_rn == np.float32(1.0) / np.float32(width) and p.inv_height_rn == np.float32(1.0) / np.float32(height)   # RN(1 / x)
        assert (p.seed_lo, p.seed_hi, p.sample0, p.accum_load, p.rng_mode) == (1, 0xFFFFFFFF, 0, 0, abi.RNG_CTR)


def test_pinned_plans_the_gpu_tests_rely_on(native, abi):
    _, device = native
    r = device.plan_render(abi.Settings(64, 48, 4, 8), abi.Options.make(workspace_bytes=3 * 4 * 12), variant=14)     # tests/test_gpu_parity.py: a band of 3 pixels
    assert (r.plan.n_bands, r.plan.band_pixels) == (1024, 3) and (r.bands["band_pixels"] == 3).all()
    r = device.plan_render(abi.Settings(1920, 1080, 4096, 30), variant=13)                                           # BASELINE config 5
    assert (r.plan.n_bands, r.plan.band_pixels) == (4, 524280)
    assert _boundary_rows(1920, 4096, r.bands.tolist()) == (4, [273, 546, 819], [34, 68, 102, 136, 170, 204, 238]) == _band_plan(1920, 1080, 4096)
    assert (r.bands["band_samples"].astype(np.int64) < (1 << 31) - 16 * RUN_LIMIT + 1).all()
    r = device.plan_render(abi.Settings(800, 600, 256, 30), variant=13)
    assert r.plan.n_bands == 1 and _boundary_rows(800, 256, r.bands.tolist()) == _band_plan(800, 600, 256)
    r = device.plan_render(abi.Settings(1280, 720, 1024, 16), variant=11)                                            # veach-mis: one band of 943 718 400 samples
    assert r.plan.n_bands == 1 and r.bands["band_samples"][0] == 1280 * 720 * 1024


def test_halving_walks_down_to_one_pixel_and_the_row_probe_never_halves(native, abi):
    _, device = native
    st = abi.Settings(5, 3, 2, 4)
    cost = np.arange(3, dtype=np.float32)
    opt = abi.Options.make(workspace_bytes=5 * 2 * 12)                   # a band of 5 of the 15 pixels
    seen = []
    for h in range(6):
        r = device.plan_render(st, opt, row_cost=cost, halvings=h, variant=14)
        seen.append((r.halved, r.plan.band_pixels, r.plan.n_bands, r.plan.order_groups))
        assert len(r.bands) == r.plan.n_bands and int(r.bands["band_pixels"].sum()) == 15 and (r.bands["band_pixels"][:-1] == r.plan.band_pixels).all()
    assert seen == [(0, 5, 3, 24), (1, 3, 5, 24), (2, 2, 8, 24), (3, 1, 15, 24), (3, 1, 15, 24), (3, 1, 15, 24)]    # order_groups: the bands before any halving
    for h in (0, 1, 4):
        r = device.plan_render(st, opt, halvings=h, row_probe=True, variant=9)
        assert (r.halved, r.plan.band_pixels, r.plan.n_bands) == (0, 5, 3) and r.bands["band_pixel0"].tolist() == [0, 5, 10]   # a band = a row
    r = device.plan_render(abi.Settings(1920, 1080, 4096, 30), halvings=2, variant=13)                                # the OOM ladder of test_gpu_robustness
    assert (r.halved, r.plan.band_pixels, r.plan.n_bands) == (2, 131070, 16)


# ---------------------------------------------------------------------------------------------------------------- the variant
def test_flag_form_and_degenerate_renders_over_the_whole_table(native, abi):
    """MI355RT_FLAG_FIXED_AABB launches VARIANT_TABLE[v].fixed_aabb on a list with a mesh and v otherwise; an empty list and max_depth == 0 go
    to k_render_ctr_mesh exactly from the lockstep kernels compiled without meshes."""
    _, device = native
    form = {v: (v if M.CAPABILITY[v][4] == "free" else 4 if v == 2 else 8) for v in M.CAPABILITY}
    form.update({v: v for v in set(M.FLAG_FORMS) | M.RETIRED})
    assert sorted(form) == list(range(device.KERNEL_VARIANTS))

    def planned(v, flag, has_mesh, n_prims=3, depth=5):
        rows = dict(row_begin=1, row_end=1) if v in M.RETIRED else {}     # (a retired variant has no launch to plan: an empty selection)
        p = device.plan_render(abi.Settings(7, 5, 2, depth), abi.Options.make(flags=abi.FLAG_FIXED_AABB if flag else 0, **rows), variant=v,
                               has_mesh=has_mesh, n_prims=n_prims).plan
        assert p.fixed_aabb == int(flag)
        return p

    for v in range(device.KERNEL_VARIANTS):
        assert planned(v, True, True).variant == form[v], v
        assert planned(v, True, False).variant == planned(v, False, True).variant == planned(v, False, False).variant == v, v
        for n_prims, depth in ((0, 5), (3, 0), (0, 0)):
            for flag, mesh in itertools.product((False, True), repeat=2):
                launched = form[v] if flag and mesh else v
                want = 1 if launched in LOCKSTEP_MESHFREE else launched
                assert planned(v, flag, mesh, n_prims, depth).variant == want, (v, n_prims, depth, flag, mesh)
        if v not in M.RETIRED:
            p = planned(v, False, False)
            assert p.block_threads == M.block_threads(v)
            b = device.plan_render(abi.Settings(64, 64, 64, 5), variant=v).bands
            assert b["shard_samples"][0] == 64 * 64 * 64 // WORK_SHARDS and b["grid"][0] == min(512, -(-(64 * 64 * 64 // runs(v)[0]) // (p.block_threads // 64)))
    assert device.plan_render(abi.Settings(7, 5, 2, 0), variant=14).plan.block_threads == 256       # the plain loop's workgroup, not the QC kernel's
    with pytest.raises(device.RenderError):
        device.plan_render(abi.Settings(7, 5, 2, 5), variant=5)                                     # a band record of a retired variant
    with pytest.raises(device.RenderError):
        device.plan_render(abi.Settings(7, 5, 2, 5), variant=device.KERNEL_VARIANTS)


# ---------------------------------------------------------------------------------------------------------------- magic_div
def test_magic_pairs_divide_every_dividend_below_two_to_the_31(native, abi):
    _, device = native
    for d in (1, 2, 3, 7, 33, 64, 255, 256, 800, 1920, 4096, (1 << 24) - 1):
        p = device.plan_render(abi.Settings(d, 1, 1, 1)).plan                                       # the pair of the width ...
        q = device.plan_render(abi.Settings(1, 1, min(d, (1 << 30) - 1), 1)).plan                   # ... and of the samples per pixel: one function
        assert d >= 1 << 30 or (p.width_mul, p.width_shift) == (q.spp_mul, q.spp_shift)
        assert (p.spp_mul, p.spp_shift) == (0, 0) == (q.width_mul, q.width_shift)
        if d == 1:
            assert (p.width_mul, p.width_shift) == (0, 0)                  # the kernels read mul == 0 as "the quotient is n"
            continue
        top = ((1 << 31) - 1) // d
        ks = sorted({k for k in (1, 2, 3, 5, 1000, 65535, 65536, top // 3, top // 2, top - 1, top) if 1 <= k <= top})
        n = np.array([0, (1 << 31) - 1] + [k * d + e for k in ks for e in (-1, 0, 1) if k * d + e < 1 << 31], np.uint64)
        q = ((n * np.uint64(p.width_mul)) >> np.uint64(32)) >> np.uint64(p.width_shift)             # umulhi(n, mul) >> shift: n * mul < 2^63
        assert p.width_mul < 1 << 32 and (q == n // np.uint64(d)).all(), d


# ---------------------------------------------------------------------------------------------------------------- row tables
def test_row_tables_deal_dear_rows_first_and_cheap_rows_last(native, abi):
    """The CPU twin of test_gpu_row_order.py::test_dear_rows_first_sky_rows_last_in_every_group on a cost of the test's own: 64 rows, one band = 8
    groups, the top 16 rows cheap (sky)."""
    _, device = native
    st = abi.Settings(96, 64, 4, 12)
    rng = np.random.default_rng(3)
    cost = np.concatenate([np.ones(16), 1.5 + rng.random(48)]).astype(np.float32)
    r = device.plan_render(st, row_cost=cost, variant=13)
    natural, processing, out_row = r.natural, r.processing, r.out_row
    assert r.plan.order_groups == 8 and r.plan.n_bands == 1
    assert list(natural) == list(range(64)) and sorted(processing) == list(range(64)) and sorted(out_row) == list(range(64))
    assert all(natural[out_row[j]] == processing[j] for j in range(64))
    per = [processing[g * 8:(g + 1) * 8] for g in range(8)]
    for rows in per:
        c = cost[rows]
        assert all(c[i] >= c[i + 1] for i in range(len(c) - 1))                              # dearest first inside a group
    assert abs(sum(cost[per[0]]) - sum(cost[per[-1]])) <= cost.max()                         # and the groups cost about the same
    assert all(cost[rows[-1]] <= np.sort(cost)[8] for rows in per)                           # the last row of every group is among the cheapest
    assert [int(rows[-1]) for rows in per] == list(range(8, 16))                             # equal costs keep image order (stable sort)
    # more bands, more groups: 8 bands of 8 rows -> 64 groups, one row each = the rows by decreasing cost
    r = device.plan_render(st, abi.Options.make(workspace_bytes=96 * 8 * 4 * 12), row_cost=cost, variant=13)
    assert (r.plan.n_bands, r.plan.order_groups) == (8, 64)
    assert r.processing.tolist() == sorted(range(64), key=lambda y: -cost[y])
    # no cost, or the replay mode: image order
    for kw in (dict(), dict(options=abi.Options.make(rng_mode=abi.RNG_REF), row_cost=cost)):
        r = device.plan_render(st, **kw)
        assert r.plan.order_groups == 0 and r.natural.tolist() == r.processing.tolist() == r.out_row.tolist() == list(range(64))
    # more groups than rows: every row a group of its own
    opt = abi.Options.make(row_begin=20, row_end=23)
    r = device.plan_render(st, opt, row_cost=cost, variant=13)
    assert r.plan.order_groups == 8 and r.natural.tolist() == [20, 21, 22]
    assert r.processing.tolist() == sorted((20, 21, 22), key=lambda y: -cost[y]) and [r.natural[j] for j in r.out_row] == r.processing.tolist()
    # a strided selection (one of two parts, strips of 4 rows), and a cost shorter than the image: the rows behind it cost nothing
    opt = abi.Options.make(strip_rows=4, n_parts=2, part=1)
    for c in (cost, cost[:40]):
        r = device.plan_render(st, opt, row_cost=c, variant=13)
        sel = abi.rows_selected(64, opt)
        assert r.natural.tolist() == sel and sorted(r.processing.tolist()) == sel and sorted(r.out_row.tolist()) == list(range(32))
        assert [r.natural[j] for j in r.out_row] == r.processing.tolist()
        full = np.concatenate([c, np.zeros(64 - len(c), np.float32)])
        for g in range(8):
            cg = full[r.processing[g * 4:(g + 1) * 4]]
            assert all(cg[i] >= cg[i + 1] for i in range(3)), (len(c), g)
