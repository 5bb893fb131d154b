"""tests/parity.py on host arrays (no GPU): the oracle's own image against perturbed copies of itself.  The contract must reject one
flipped mantissa bit in exact mode, allow exactly its counted outliers in tolerant mode, and name the pixels it rejects."""
import math
import os
import re

import numpy as np
import pytest

from conftest import load_for_both
from parity import allowed, assert_parity, oracle_threads

W, H = 160, 90                      # N = 14 400: 2 L2 outliers and 15 8-bit differences allowed


@pytest.fixture(scope="module")
def image(native, oracle_mod, abi):
    host, _ = native
    sc = load_for_both("cornell", oracle_mod, host, width=W, height=H, spp=2, max_depth=4)
    op, ol, cnt = oracle_mod.render(sc, sc.camera, sc.settings, abi.Options.make(), threads=oracle_threads())
    assert ol.mean() > 0.05
    return op, ol, int(cnt.rays)


def _pixels(k, seed=0):
    """k distinct pixels (row, x), in row-major order."""
    flat = np.random.default_rng(seed).choice(np.arange(W * H), size=k, replace=False)
    return [(int(i) // W, int(i) % W) for i in sorted(flat)]


def _reported(msg):
    return [(int(a), int(b)) for a, b in re.findall(r"\((\d+), (\d+)\)", msg.split("first (row, x):")[1].split(";")[0])]


def test_allowed_counts():
    assert allowed(W * H) == (2, 15)
    assert allowed(96 * 54) == (1, 6)                     # a small image may still carry one outlier
    assert allowed(1280 * 720) == (93, 922)


def test_identical_images_pass_both_modes(image):
    op, ol, rays = image
    assert_parity(op.copy(), ol.copy(), op, ol, exact=True, gpu_rays=rays, oracle_rays=rays)
    assert_parity(op.copy(), ol.copy(), op, ol, exact=False, gpu_rays=rays, oracle_rays=rays)


def test_one_flipped_mantissa_bit_fails_exact_mode(image):
    op, ol, rays = image
    gl = ol.copy()
    y, x = _pixels(1, seed=1)[0]
    gl.view(np.uint32)[y, x, 1] ^= 1                       # the last bit of one channel of one pixel
    with pytest.raises(AssertionError, match="not bit-identical") as e:
        assert_parity(op, gl, op, ol, exact=True)
    assert _reported(str(e.value)) == [(y, x)]
    assert_parity(op, gl, op, ol, exact=False)             # far inside the tolerant contract
    with pytest.raises(AssertionError, match="ray counts differ"):
        assert_parity(op, ol, op, ol, exact=True, gpu_rays=rays + 1, oracle_rays=rays)
    gp = op.copy(); gp[y, x] ^= 1
    with pytest.raises(AssertionError, match="not bit-identical"):
        assert_parity(gp, ol, op, ol, exact=True)


def test_l2_outliers_are_counted(image):
    op, ol, _ = image
    k = allowed(W * H)[0]
    px = _pixels(k + 1, seed=2)
    gl = ol.copy()
    for y, x in px[:k]:
        gl[y, x, 0] += 2e-3
    assert_parity(op, gl, op, ol, exact=False)
    y, x = px[k]
    gl[y, x, 2] -= 2e-3
    with pytest.raises(AssertionError, match=rf"{k + 1} of {W * H} px beyond L2") as e:
        assert_parity(op, gl, op, ol, exact=False)
    assert _reported(str(e.value).split("L2 outliers:")[1]) == px


def test_a_non_finite_pixel_is_an_outlier(image):
    op, ol, _ = image
    gl = ol.copy()
    (y0, x0), (y1, x1), (y2, x2) = _pixels(3, seed=3)
    gl[y0, x0, 0] = np.nan; gl[y1, x1, 1] = np.inf; gl[y2, x2, 2] += 1.0
    with pytest.raises(AssertionError, match=r"^3 of"):
        assert_parity(op, gl, op, ol, exact=False)


def test_8bit_differences_are_counted(image):
    op, ol, _ = image
    k = allowed(W * H)[1]
    px = _pixels(k + 1, seed=4)
    gp = op.copy()
    for y, x in px[:k]:
        gp[y, x] ^= 0x010000
    assert_parity(gp, ol, op, ol, exact=False)
    y, x = px[k]
    gp[y, x] ^= 0x000001
    with pytest.raises(AssertionError, match=rf"{k + 1} 8-bit px differ") as e:
        assert_parity(gp, ol, op, ol, exact=False)
    assert _reported(str(e.value).split("8-bit differences:")[1]) == px[:10]


def test_ray_count_bound(image):
    op, ol, rays = image
    rel = 1e-3
    slack = math.floor(rel * rays)
    assert slack >= 1
    assert_parity(op, ol, op, ol, exact=False, gpu_rays=rays + slack, oracle_rays=rays, ray_rel=rel)
    assert_parity(op, ol, op, ol, exact=False, gpu_rays=rays - slack, oracle_rays=rays, ray_rel=rel)
    with pytest.raises(AssertionError, match="ray counts differ"):
        assert_parity(op, ol, op, ol, exact=False, gpu_rays=rays + slack + 1, oracle_rays=rays, ray_rel=rel)
    with pytest.raises(AssertionError, match="ray counts differ"):
        assert_parity(op, ol, op, ol, exact=False, gpu_rays=rays + 1, oracle_rays=rays)      # ray_rel defaults to 0


def test_rows_map_to_absolute_rows_and_name_the_worst(image):
    """A row subset reports image rows; a whole bad row (a band or shard boundary, say) leads the list of worst rows."""
    op, ol, _ = image
    rows = [0, 7, 44, 45, 89]
    sub_p, sub_l = op[rows], ol[rows]
    gl = sub_l.copy()
    gl[3, :, 0] += 0.5                                     # all of image row 45
    gl[1, 5, 1] += 0.5                                     # one pixel of image row 7
    with pytest.raises(AssertionError) as e:
        assert_parity(sub_p, gl, sub_p, sub_l, exact=False, rows=rows)
    msg = str(e.value).split("L2 outliers:")[1]
    assert _reported(msg)[:2] == [(7, 5), (45, 0)]
    assert f"rows with most (row (count)): 45 ({W}), 7 (1)" in msg
    with pytest.raises(AssertionError):
        assert_parity(sub_p, sub_l, sub_p, sub_l, exact=True, rows=rows[:-1])      # the map must cover the rows compared


def test_oracle_threads(monkeypatch):
    monkeypatch.delenv("OMP_NUM_THREADS", raising=False)
    n = oracle_threads()
    assert 1 <= n <= 16 and n <= len(os.sched_getaffinity(0))
    monkeypatch.setenv("OMP_NUM_THREADS", "3")
    assert oracle_threads() == min(3, n)
    monkeypatch.setenv("OMP_NUM_THREADS", "64")
    assert oracle_threads() == n


def test_nan_folded_comparison_takes_any_nan_for_a_nan_and_nothing_else():
    """assert_same_bits_nan_folded: NaNs of any sign and payload are one value; a NaN paired with a number, a zero of the other sign, an
    infinity of the other sign and a denormal paired with zero are differences."""
    from parity import assert_same_bits_nan_folded, nan_folded_bits
    words = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF, 0x7F800000, 0xFF800000, 0x00000000, 0x80000000, 0x00000001, 0x3F800000], np.uint32)
    a = words.view(np.float32)
    b = a.copy().view(np.uint32)
    b[:4] = [0xFFC00000, 0x7FC12345, 0x7FC00000, 0x7FA00000]              # other NaNs in the NaN places
    assert_same_bits_nan_folded(a, b.view(np.float32), "NaNs of any payload")
    assert (nan_folded_bits(a)[:4] == 0x7FC00000).all() and (nan_folded_bits(a)[4:] == words[4:]).all()
    for i, other in ((0, 1.0), (0, np.inf), (0, 0.0), (9, np.nan), (4, np.nan), (5, np.nan), (6, np.nan),      # a NaN paired with a number, both ways
                     (4, -np.inf), (6, -0.0), (7, 0.0), (8, 0.0), (9, np.float32(1.0000001))):
        c = a.copy()
        c[i] = other
        with pytest.raises(AssertionError, match="1 of 10 words differ"):
            assert_same_bits_nan_folded(c, a, "one word")
    with pytest.raises(AssertionError, match=r"1 pair a NaN with a number"):
        c = a.copy(); c[0] = 2.0
        assert_same_bits_nan_folded(c, a, "NaN against 2")
    with pytest.raises(AssertionError, match="shapes"):
        assert_same_bits_nan_folded(a[:3], a[:4], "shapes")
