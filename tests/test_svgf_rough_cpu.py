"""The rough inputs of tests/test_gpu_svgf_rough.py and the reference it compares with, without a GPU.

tests/svgf_cases.py's plane gives the geometry weight G(p, q) of include/mi355rt_svgf.h the values 0 and 1 only, so a kernel with one squaring too
few, a division by sigma_plane * t_q or no absolute value passes every case made from it.  Here, as CONDITIONS on the reference alone (measured with
svgf_cases.ROUGH_SEED = 11 and BUMPY_SEED = 5; the figures are in the tests' comments and printed again by every run):
  1. svgf_cases.rough and svgf_cases.bumpy are what they say, and are not vacuous: thousands of distinct G strictly inside (0, 1) in the filter and in
     the spatial estimate, all five ways out of accumulate, NaN and finite pixels in every filter output;
  2. each parameter is SENSITIVE: changing normal_squarings, sigma_plane, sigma_luminance or the variance image changes at least one pixel in ten;
  3. tests/svgf_ref.py's vectorised slicing is bit-identical to tests/svgf_scalar.py, a second restatement of the header one pixel and one tap at a time;
  4. the variant library's plan (build.SVGF_GRID3_DEFINES) gives the grids the GPU tests rely on: 3 workgroups for 9 and for 45 tiles."""
import os
import subprocess

import numpy as np
import pytest

import denoise_cases
import reproject_cases as RC
import svgf_cases as SC
import svgf_ref as SR
import svgf_scalar as SS
from conftest import ROOT, pkg
from parity import assert_same_bits_nan_folded, nan_folded_bits

F = np.float32
BIG = [s for s in SC.ROUGH_SIZES if s[0] * s[1] >= 33 * 9]                # the sizes of which > 1000 distinct G inside (0, 1) are asked
ONE_IN_TEN = 0.1
_ids = lambda s: f"{s[0]}x{s[1]}"


@pytest.fixture
def seen_G(monkeypatch):
    """Spies on svgf_ref.geometry_weight: returns a function giving the number of distinct values strictly inside (0, 1) since its last call."""
    seen, real = [], SR.geometry_weight

    def spy(*args):
        G = real(*args)
        seen.append(np.asarray(G).ravel())
        return G

    def inside():
        g = np.unique(np.concatenate(seen))
        seen.clear()
        return int(((g > 0) & (g < 1)).sum()), set(np.unique(g[(g <= 0) | (g >= 1) | np.isnan(g)]).tolist())
    monkeypatch.setattr(SR, "geometry_weight", spy)
    return inside


def share(a, b):
    """The share of pixels in which a and b differ in a bit (NaNs folded)."""
    n = a.shape[0] * (a.shape[1] if a.ndim == 3 else 1)
    a, b = a.reshape(n, -1), b.reshape(n, -1)
    same = (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
    return float((~same.all(axis=1)).mean())


def restart(abi, W, H, **params):
    """variance_out of svgf_ref.accumulate without a previous frame on rough's records: every pixel's spatial estimate."""
    _, _, hits, colour = SC.rough(abi, W, H)
    return SR.accumulate(RC.view(abi, RC.canonical(abi), W, H), None, hits, colour, params=abi.SvgfAccumulateParams.make(**params))[2]


# ---- 1: the inputs ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SC.ROUGH_SIZES + [(1, 1), (5, 3)], ids=_ids)
def test_rough_is_the_denoisers_synthetic_case_with_a_seeded_variance(size, abi):
    W, H = size
    n = W * H
    hist, var, hits, colour = SC.rough(abi, W, H)
    lin, want_hits = denoise_cases.synthetic(abi, W, H, SC.ROUGH_SEED)
    assert hits is want_hits and colour.tobytes() == lin.tobytes()                 # imported, not copied
    assert hist.shape == (n, 4) and hist[:, :3].tobytes() == colour.tobytes() and (hist[:, 3] == 1).all()
    assert var.shape == (n,) and var.dtype == F and not var.flags.writeable and not hist.flags.writeable
    assert SC.rough(abi, W, H)[1] is var                                          # computed once
    if n < 4:
        assert (var < 0).sum() == 1
        return
    tiny = np.isfinite(var) & (var > 0) & (var < np.finfo(F).tiny)
    for what, mask in (("1e30", var == F(1e30)), ("a denormal", tiny), ("negative", np.isfinite(var) & (var < 0)), ("NaN", np.isnan(var)), ("+inf", var == np.inf), ("-inf", var == -np.inf)):
        assert mask.any(), what
    odd = (var == F(1e30)) | tiny | ~np.isfinite(var) | (var < 0)
    plain = var[~odd]
    assert (plain >= 0).all() and (plain < F(0.05)).all()
    left = np.zeros((H, W), bool)
    left[:, : W // 4] = True
    assert (var[left.reshape(-1) & ~odd] == 0).all() and (W < 4 or (var[left.reshape(-1)] == 0).any())
    assert len(np.unique(var[~left.reshape(-1) & ~odd])) > (n - left.sum()) // 2          # uniform elsewhere, not a constant


@pytest.mark.parametrize("size", BIG, ids=_ids)
def test_rough_gives_the_geometry_weight_thousands_of_values_inside_0_1(size, abi, seen_G):
    """Measured (distinct G in (0, 1): filter at 5 levels / spatial estimate): 33 x 9: 5277 / 5545; 70 x 17: 14195 / 15149; 131 x 70: 36481 / 25939.
    The plane's cases give none."""
    W, H = size
    hist, var, hits, _ = SC.rough(abi, W, H)
    out = SR.filter(hist, var, hits, W, H)
    in_filter, edges = seen_G()
    restart(abi, W, H)
    in_spatial, edges_s = seen_G()
    print(f"{W} x {H}: distinct G in (0, 1): filter {in_filter}, spatial estimate {in_spatial}; NaN pixels {int(np.isnan(out).any(-1).sum())}, finite {int(np.isfinite(out).all(-1).sum())}")
    assert in_filter > 1000 and in_spatial > 1000
    assert {0.0, 1.0} <= edges and {0.0, 1.0} <= edges_s                           # the misses' and the cut-off taps' values are still there


@pytest.mark.parametrize("cur_size,prev_size", SC.BUMPY_SIZES, ids=_ids)
def test_bumpy_keeps_all_five_ways_out_and_gives_g_values_inside_0_1(cur_size, prev_size, abi, seen_G):
    """Measured (temporal, short history, moment restart, no history, miss; distinct G in (0, 1)): 33 x 9 from 33 x 9: [219 38 10 27 3], 6496;
    70 x 17 from 70 x 17: [849 143 111 84 3], 43202; 33 x 9 from 20 x 7: [201 16 12 65 3], 6496."""
    case = SC.bumpy(abi, cur_size, prev_size)
    way = SC.reference(case)[3]
    inside, _ = seen_G()
    counts = np.bincount(way, minlength=5)
    print(cur_size, "from", prev_size, "ways out:", counts, "distinct G in (0, 1):", inside)
    assert (counts >= 1).all() and inside > 1000
    if cur_size[0] * cur_size[1] > 33 * 9:
        return                                                                     # (the record-by-record comparison with the plane's case: on the two small pairs)
    flat = SC.build(abi, cur_size, prev_size)
    SC.reference(flat)
    assert seen_G() == (0, {0.0, 1.0})                                             # the plane gives G the values 0 and 1 and no other
    assert [(a, b) for a, b, *_ in case["placed"]] == [(a, b) for a, b, *_ in flat["placed"]] and case["added"] == flat["added"]
    for name, kept in (("hits_cur", [j for _, j, *_ in case["placed"]] + [j for _, j, _ in case["added"]] + [len(way) - 2, len(way) - 1]),
                       ("hits_prev", [q for _, _, q, _ in case["placed"] if q is not None] + [q for _, _, qs in case["added"] for q in qs])):
        a, b = case[name], flat[name]
        assert a[kept].tobytes() == b[kept].tobytes(), name                        # the crafted records are untouched
        moved = np.ones(len(a), bool)
        moved[kept] = False
        moved &= b["primitive"] != RC.NO_HIT
        assert (a["normal"][moved] != b["normal"][moved]).any(axis=1).all() and (a["position"][moved, 2] != b["position"][moved, 2]).all(), name
        assert a[~moved].tobytes() == b[~moved].tobytes() and (a["position"][:, :2] == b["position"][:, :2]).all() and (a["t"][moved] == b["t"][moved]).all(), name
        assert np.allclose(np.linalg.norm(a["normal"][moved].astype(np.float64), axis=1), 1.0, atol=1e-6)


# ---- 2: each parameter is sensitive ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SC.ROUGH_SIZES, ids=_ids)
def test_every_filter_parameter_changes_a_pixel_in_ten(size, abi):
    """Measured shares of differing pixels, 5 levels (squarings 5 vs 4, sigma_plane 0.05 vs 0.06, sigma_luminance 1 vs 1.1, the variance image vs a
    constant 0.02): 1 x 37: 0.43 0.70 0.57 0.73; 37 x 1: 0.27 0.22 0.70 0.89; 33 x 9: 0.83 0.80 0.86 0.91; 70 x 17: 0.53 0.47 0.78 0.92;
    131 x 70: 0.37 0.26 0.85 0.94."""
    W, H = size
    hist, var, hits, _ = SC.rough(abi, W, H)
    base = SR.filter(hist, var, hits, W, H)
    assert np.isnan(base).any(-1).any() and np.isfinite(base).all(-1).any()        # the folded comparison is exercised both ways
    pairs = {"normal_squarings 5 vs 4": SR.filter(hist, var, hits, W, H, normal_squarings=4), "sigma_plane 0.05 vs 0.06": SR.filter(hist, var, hits, W, H, sigma_plane=0.06),
             "sigma_luminance 1 vs 1.1": SR.filter(hist, var, hits, W, H, sigma_luminance=1.1), "the variance vs a constant 0.02": SR.filter(hist, np.full(W * H, 0.02, F), hits, W, H)}
    shares = {k: share(base, v) for k, v in pairs.items()}
    print(f"{W} x {H}:", {k: round(v, 3) for k, v in shares.items()})
    assert min(shares.values()) >= ONE_IN_TEN, shares


@pytest.mark.parametrize("size", SC.ROUGH_SIZES, ids=_ids)
def test_every_parameter_of_the_spatial_estimate_changes_a_pixel_in_ten(size, abi):
    """Measured (squarings 5 vs 4, 5 vs 0, sigma_plane 0.05 vs 0.06): 1 x 37: 0.51 0.51 0.86; 37 x 1: 0.30 0.30 0.32; 33 x 9: 0.76 0.77 0.75;
    70 x 17: 0.45 0.45 0.45; 131 x 70: 0.19 0.19 0.19 (the lowest: the denoiser's runs of misses cover most of that frame)."""
    W, H = size
    base = restart(abi, W, H)
    assert not np.isnan(base).any() and (base >= 0).all()
    shares = {"normal_squarings 5 vs 4": share(base, restart(abi, W, H, normal_squarings=4)), "normal_squarings 5 vs 0": share(base, restart(abi, W, H, normal_squarings=0)),
              "sigma_plane 0.05 vs 0.06": share(base, restart(abi, W, H, sigma_plane=0.06)), "min_temporal 4 vs 1": share(base, restart(abi, W, H, min_temporal=1))}
    print(f"{W} x {H}:", {k: round(v, 3) for k, v in shares.items()})
    assert min(shares.values()) >= ONE_IN_TEN, shares


# ---- 3: the scalar anchor --------------------------------------------------------------------------------------------------------------------
ANCHOR_PARAMS = dict(normal_squarings=3, sigma_luminance=0.7, sigma_plane=0.3)     # no default among them


@pytest.mark.parametrize("size", [(5, 3), (33, 9)], ids=_ids)
def test_the_reference_is_the_scalar_restatement_bit_for_bit(size, abi):
    W, H = size
    hist, var, hits, colour = SC.rough(abi, W, H)
    levels = SS.filter_levels(hist, var, hits, W, H, 5, **ANCHOR_PARAMS)
    for k in (1, 2, 5):
        assert_same_bits_nan_folded(SR.filter_levels(hist, var, hits, W, H, k, **ANCHOR_PARAMS), levels[k].reshape(H, W, 4), f"{W} x {H}: filter_levels at {k} levels")
    assert np.isnan(levels[5]).any() and np.isfinite(levels[5]).all(axis=1).any()
    for params in (dict(), dict(min_temporal=1, normal_squarings=3, sigma_plane=0.3), dict(min_temporal=2, normal_squarings=0, sigma_plane=0.6)):
        want = SS.spatial_variance(hits, colour, W, H, **params)
        assert_same_bits_nan_folded(restart(abi, W, H, **params), want, f"{W} x {H}: the spatial estimate with {params}")
        assert (want > 0).any() and (W * H < 64 or (want == 0).any())


def test_the_scalar_restatement_tells_a_subtly_wrong_geometry_weight(abi, monkeypatch):
    """What the plane cannot see: svgf_ref with one squaring fewer, or with the tap's t in the place of the centre's, differs from the anchor on rough in more
    than a pixel in ten.  The plane's case of the same size gives the first the very same bytes, and sees the second in 2 words of 2079 (the crafted record
    whose t is NaN, and one neighbour)."""
    W, H = 33, 9
    hist, var, hits, _ = SC.rough(abi, W, H)
    want = SS.filter_levels(hist, var, hits, W, H, 2)[2].reshape(H, W, 4)
    flat = SC.build(abi, (W, H), (W, H))
    flat_want = SC.reference(flat)
    real = SR.geometry_weight

    def one_squaring_fewer(n, P, t, miss, p, q, normal_squarings, sigma_plane):
        return real(n, P, t, miss, p, q, normal_squarings - 1, sigma_plane)

    def t_of_the_tap(n, P, t, miss, p, q, normal_squarings, sigma_plane):
        t_q = t.copy()
        t_q[p] = t[q]                                                              # (geometry_weight reads t at p only)
        return real(n, P, t_q, miss, p, q, normal_squarings, sigma_plane)

    seen_by_the_plane = {"one_squaring_fewer": 0, "t_of_the_tap": 2}
    for wrong in (one_squaring_fewer, t_of_the_tap):
        monkeypatch.setattr(SR, "geometry_weight", wrong)
        differing = share(SR.filter_levels(hist, var, hits, W, H, 2), want)
        print(wrong.__name__, "differs from the anchor in", round(differing, 3), "of the pixels")
        assert differing >= ONE_IN_TEN, wrong.__name__
        words = sum(int((nan_folded_bits(g) != nan_folded_bits(w)).sum()) for g, w in zip(SC.reference(flat)[:3], flat_want[:3]))
        print(wrong.__name__, "changes", words, "words of the plane's accumulate")
        assert words <= seen_by_the_plane[wrong.__name__]
    monkeypatch.setattr(SR, "geometry_weight", real)
    assert_same_bits_nan_folded(SR.filter_levels(hist, var, hits, W, H, 2), want, "unbroken")


# ---- 4: the variant library's plan -----------------------------------------------------------------------------------------------------------
GRID_MAIN = """#include <stdio.h>
#include "svgf_plan.h"
using namespace mi355rt_svgf;
int main() {
    static char buf[4096] __attribute__((aligned(64)));
    const unsigned sizes[3][2] = {{33, 9}, {70, 17}, {131, 70}};
    for (auto& s : sizes) {
        FilterPlan fp{}; AccumulatePlan ap{}; std::string why;
        mi355rt_view v{}; v.width = s[0]; v.height = s[1]; v.camera.forward[2] = v.camera.right[0] = v.camera.true_up[1] = 1.0f; v.camera.half_width = v.camera.half_height = 1.0f; v.flags = 1u;
        if (plan_filter(0, s[0], s[1], nullptr, buf, buf + 64, buf + 128, buf + 192, buf + 256, nullptr, fp, why)) { printf("%s\\n", why.c_str()); return 1; }
        if (plan_accumulate(0, &v, nullptr, nullptr, buf, buf + 64, nullptr, nullptr, nullptr, buf + 128, buf + 192, buf + 256, ap, why)) { printf("%s\\n", why.c_str()); return 1; }
        printf("%u %u %u %u %u\\n", MAX_BLOCKS, fp.n_tiles, fp.grid, ap.k.n_tiles, ap.grid);
    }
    return 0;
}
"""


def test_the_variant_librarys_plan_walks_every_tile_loop_more_than_once(tmp_path):
    """svgf_plan.cpp compiled with build.SVGF_GRID3_DEFINES, as build_svgf_grid3 compiles it: 3 workgroups for 9 tiles (3 trips each) and for 45 (15 each);
    without the define, the product's cap and a workgroup per tile."""
    build = pkg("build")
    svgf_dir = os.path.join(ROOT, "raytracer-rust_amd", "csrc", "svgf")
    src = tmp_path / "grid_main.cpp"
    src.write_text(GRID_MAIN)
    rows = {}
    for name, defines in (("product", []), ("grid3", build.SVGF_GRID3_DEFINES)):
        exe = str(tmp_path / name)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", svgf_dir, *[f"-D{d}" for d in defines], "-o", exe, str(src), os.path.join(svgf_dir, "svgf_plan.cpp")])
        rows[name] = [tuple(int(v) for v in line.split()) for line in subprocess.check_output([exe], text=True).splitlines()]
    assert rows["product"] == [(1 << 20, 4, 4, 4, 4), (1 << 20, 9, 9, 9, 9), (1 << 20, 45, 45, 45, 45)]
    assert rows["grid3"] == [(3, 4, 3, 4, 3), (3, 9, 3, 9, 3), (3, 45, 3, 45, 3)]
    assert build.build_svgf_grid3.__name__ not in open(os.path.join(ROOT, "__graft_entry__.py")).read()      # the product path never builds or loads it
    assert "grid3" not in open(os.path.join(ROOT, "raytracer-rust_amd", "svgf.py")).read()
