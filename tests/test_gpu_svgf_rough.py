"""mi355rt_svgf_accumulate and mi355rt_svgf_filter on the GPU where tests/test_gpu_svgf.py's plane cannot see them: on guides that give the geometry
weight G(p, q) thousands of values strictly inside (0, 1), with every weight parameter away from its default, on a variance image accumulate never
writes (negative, denormal, 1e30, NaN, +-inf), and through the second and later trips of every kernel's tile loop.  Every output bit for bit (NaNs
folded) against tests/svgf_ref.py, which tests/test_svgf_rough_cpu.py holds against a scalar restatement on these very inputs and whose sensitivity
to each parameter it measures; the buffers, their guards and the input-unchanged checks are test_gpu_svgf's.

  1. the filter on svgf_cases.rough: a column, a row and three tiled sizes, three parameter sets, both level forms, each staged kernel as the last level;
  2. the spatial estimate on rough's records: accumulate without a previous frame, normal_squarings x sigma_plane x min_temporal;
  3. accumulate on svgf_cases.bumpy: the reprojection's taps and the spatial estimate on perturbed normals and depths, two parameter sets;
  4. the tile loops' later trips: libmi355rt_svgf_grid3.so (build.build_svgf_grid3: grids of at most 3 workgroups, so a workgroup walks 3 tiles of
     70 x 17 and 15 of 131 x 70; the staged kernels restage LDS that holds the previous tile) against the same references."""
import numpy as np
import pytest

import reproject_cases as RC
import svgf_cases as SC
import svgf_ref as SR
import test_gpu_svgf as T                              # Guarded buffers, run_filter, AccumulateBuffers, the guard and input-unchanged checks, the two comparisons
from conftest import pkg
from device_buffers import Guarded

pytestmark = pytest.mark.gpu

F = np.float32
FILTER_SETS = [(5, 5, 1.0, 0.05), (8, 0, 0.4, 0.6), (3, 8, 4.0, 0.01)]     # (levels, normal_squarings, sigma_luminance, sigma_plane)
FILTER_CASES = [(size, s) for size in SC.ROUGH_SIZES for s in FILTER_SETS] + [((70, 17), (1, 0, 0.4, 0.6)), ((70, 17), (2, 0, 0.4, 0.6))]     # ... and k_svgf_last_staged1 / 2
SPATIAL_SIZES = [(33, 9), (70, 17), (131, 70)]
SPATIAL_SETS = [(sq, sp, mt) for sq in (0, 5, 8) for sp in (0.05, 0.6) for mt in (1, 4)]     # (normal_squarings, sigma_plane, min_temporal)
BUMPY_SETS = [(5, 0.05), (0, 0.6)]                                          # (normal_squarings, sigma_plane): the defaults, and far from them
LOOP_SIZES = [(70, 17), (131, 70)]                                          # 9 and 45 tiles: 3 and 15 trips of a workgroup of the variant library
LOOP_LEVELS = [1, 2, 3, 5]
_size = lambda s: f"{s[0]}x{s[1]}"
_set = lambda s: "-".join(f"{v:g}" for v in s)


@pytest.fixture(scope="module")
def svgf():
    pkg("build").build_svgf()
    return pkg("svgf")


@pytest.fixture(scope="module")
def post():
    pkg("build").build_post()
    return pkg("post")


@pytest.fixture(scope="module")
def grid3(svgf):
    """The variant library, bound to the same call wrappers; the product path never loads it."""
    lib = svgf.open_library(pkg("build").build_svgf_grid3())
    assert lib.lib() is not svgf.lib() and lib.path != pkg("build").SVGF_SO
    return lib


# ---- references: computed once, shared, read-only ---------------------------------------------------------------------------------------------
_refs = {}


def _once(key, make):
    if key not in _refs:
        v = make()
        for a in (v if isinstance(v, tuple) else (v,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _refs[key] = v
    return _refs[key]


def filter_reference(abi, size, levels, squarings, sigma_luminance, sigma_plane):
    W, H = size
    hist, var, hits, _ = SC.rough(abi, W, H)
    return _once(("filter", size, levels, squarings, sigma_luminance, sigma_plane),
                 lambda: SR.filter(hist, var, hits, W, H, levels=levels, normal_squarings=squarings, sigma_luminance=sigma_luminance, sigma_plane=sigma_plane))


def restart_case(abi, size, squarings, sigma_plane, min_temporal):
    """rough's records and colour as an accumulate WITHOUT a previous frame (the previous buffers are one unused pixel), and its reference."""
    W, H = size
    _, _, hits, colour = SC.rough(abi, W, H)
    cam = RC.canonical(abi)
    params = abi.SvgfAccumulateParams.make(min_temporal=min_temporal, normal_squarings=squarings, sigma_plane=sigma_plane)
    case = dict(cur=RC.view(abi, cam, W, H), prev=RC.view(abi, cam, 1, 1), hits_cur=hits, color_cur=colour, hits_prev=np.zeros(1, abi.HIT_DTYPE),
                hist_prev=np.zeros((1, 4), F), moments_prev=np.zeros((1, 2), F), params=params)
    return case, _once(("restart", size, squarings, sigma_plane, min_temporal), lambda: SR.accumulate(case["cur"], None, hits, colour, params=params))


def bumpy_case(abi, cur_size, prev_size, squarings, sigma_plane):
    base = _once(("bumpy", cur_size, prev_size), lambda: SC.bumpy(abi, cur_size, prev_size, flat=T.synthetic(abi, cur_size, prev_size)[0]))     # (the plane's case is test_gpu_svgf's, built once for both files)
    p = base["params"]
    case = dict(base, params=abi.SvgfAccumulateParams.make(p.max_history, p.normal_min, p.plane_tolerance, p.min_temporal, squarings, sigma_plane))
    return case, _once(("bumpy", cur_size, prev_size, squarings, sigma_plane), lambda: SC.reference(case))


def filter_in_both_forms(lib, abi, size, params, what):
    levels, squarings, sigma_luminance, sigma_plane = params
    W, H = size
    hist, var, hits, _ = SC.rough(abi, W, H)
    want = filter_reference(abi, size, *params)
    assert np.isnan(want).any(-1).any() and np.isfinite(want).all(-1).any()        # the folded comparison is exercised both ways
    kw = dict(levels=levels, normal_squarings=squarings, sigma_luminance=sigma_luminance, sigma_plane=sigma_plane)
    T.assert_is_filter(T.run_filter(lib, abi, W, H, hist, var, hits, **kw), want, f"{what} {size} {params}")
    T.assert_is_filter(T.run_filter(lib, abi, W, H, hist, var, hits, flags=abi.SVGF_GATHERS_ONLY, **kw), want, f"{what} {size} {params}, gathers only")


# ---- 1: the filter on rough guides and a variance accumulate never writes ---------------------------------------------------------------------------
@pytest.mark.parametrize("size,params", FILTER_CASES, ids=[f"{_size(s)}-{_set(p)}" for s, p in FILTER_CASES])
def test_filter_on_rough_guides_is_the_reference_bit_for_bit_in_both_forms(size, params, native, svgf, abi):
    filter_in_both_forms(svgf, abi, size, params, "filter")


# ---- 2: the spatial estimate on rough guides --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("squarings,sigma_plane,min_temporal", SPATIAL_SETS, ids=[_set(s) for s in SPATIAL_SETS])
@pytest.mark.parametrize("size", SPATIAL_SIZES, ids=_size)
def test_the_spatial_estimate_on_rough_guides_is_the_reference_bit_for_bit(size, squarings, sigma_plane, min_temporal, native, svgf, abi):
    case, want = restart_case(abi, size, squarings, sigma_plane, min_temporal)
    assert set(np.unique(want[3])) == {SR.NO_HISTORY, SR.MISS} and (want[2] > 0).any()       # every hit goes through k_svgf_spatial
    T.assert_is_accumulate(T.run_accumulate(svgf, case, prev=False), want, f"{size} squarings {squarings} sigma_plane {sigma_plane} min_temporal {min_temporal}")


# ---- 3: accumulate on bumpy guides ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("squarings,sigma_plane", BUMPY_SETS, ids=[_set(s) for s in BUMPY_SETS])
@pytest.mark.parametrize("cur_size,prev_size", SC.BUMPY_SIZES, ids=_size)
def test_accumulate_on_bumpy_guides_is_the_reference_bit_for_bit(cur_size, prev_size, squarings, sigma_plane, native, svgf, abi):
    case, want = bumpy_case(abi, cur_size, prev_size, squarings, sigma_plane)
    assert len(np.unique(want[3])) == 5                                           # every way out is taken
    T.assert_is_accumulate(T.run_accumulate(svgf, case), want, f"{cur_size} from {prev_size}, squarings {squarings} sigma_plane {sigma_plane}")


def test_hist_out_on_bumpy_guides_is_what_the_reprojection_writes_on_the_same_buffers(native, svgf, post, abi):
    import torch
    case, _ = bumpy_case(abi, (70, 17), (70, 17), *BUMPY_SETS[0])
    b = T.AccumulateBuffers(case)
    b.call(svgf)
    hc, cc, hp, mp, _ = (buf.ptr for _, buf in b.inputs)
    rep = Guarded(b.n * 16)
    post.reproject(case["cur"], case["prev"], hc, cc, hp, mp, rep.ptr, None, None, case["reproject_params"])
    torch.cuda.synchronize()
    assert b.read()[0].tobytes() == rep.read(F, "reproject's hist_out").reshape(-1, 4).tobytes()


# ---- 4: the tile loops' later trips -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", LOOP_LEVELS)
@pytest.mark.parametrize("size", LOOP_SIZES, ids=_size)
def test_filter_through_the_later_trips_of_the_tile_loops(size, levels, native, grid3, abi):
    filter_in_both_forms(grid3, abi, size, (levels,) + FILTER_SETS[0][1:], "grid3 filter")


@pytest.mark.parametrize("size", LOOP_SIZES, ids=_size)
def test_the_spatial_estimate_through_the_later_trips_of_the_tile_loops(size, native, grid3, abi):
    case, want = restart_case(abi, size, 5, 0.05, 4)
    T.assert_is_accumulate(T.run_accumulate(grid3, case, prev=False), want, f"grid3 {size} without prev")


def test_accumulate_through_the_later_trips_of_the_tile_loops(native, grid3, abi):
    case, want = bumpy_case(abi, (70, 17), (70, 17), *BUMPY_SETS[0])
    T.assert_is_accumulate(T.run_accumulate(grid3, case), want, "grid3 (70, 17) from (70, 17)")
