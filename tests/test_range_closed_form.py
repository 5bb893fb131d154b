"""The closed form behind ray_direction's second normalisation (rt_math.h: renorm_t, renorm_in_range, renorm_scale), restated in numpy and compared
with what it replaces -- float32(1) / sqrt_f32(x), numpy's correctly rounded f32 square root and division, which the device's short forms are proven
equal to (tools/verify/short_arithmetic.hip) -- for EVERY float x with |x - 1| <= 2^-13: 2048 below 1, 1 itself, 1024 above.  No GPU.

  t = fma(x, 2^22, -2^22)        exact in f32: (x - 1) * 2^22 has at most 24 significant bits for these x; computed here in f64, where it is exact too
  guard: |t| <= 512
  r = fma(-2^-23, floor(t), 1)   exact: an integer of magnitude at most 512 times 2^-23, subtracted from 1

The GPU program tools/verify/range_arithmetic.hip repeats the comparison on the shipped functions over all 2^32 x (tests/test_gpu_range_arithmetic.py)."""
import numpy as np

F = np.float32


def _closed(x):
    t = np.float64(x) * 2.0 ** 22 - 2.0 ** 22                       # the fma's exact value ...
    assert np.array_equal(t, np.float64(F(t)))                      # ... is a float: the fma's rounding does nothing
    ok = np.abs(t) <= 512.0
    r = 1.0 - 2.0 ** -23 * np.floor(t)
    assert np.array_equal(r[ok], np.float64(F(r[ok])))              # and so is the result
    return ok, F(r)


def _range():
    lo, hi = F(1) - F(2.0 ** -13), F(1) + F(2.0 ** -13)
    bits = np.arange(lo.view(np.uint32), hi.view(np.uint32) + 1, dtype=np.uint32)   # positive floats are ordered like their bits
    return bits.view(F)


def test_closed_form_equals_one_over_sqrt_on_every_float_of_the_range():
    x = _range()
    assert len(x) == 3073 and x[0] == F(1) - F(2.0 ** -13) and x[-1] == F(1) + F(2.0 ** -13) and x[2048] == F(1)
    ok, r = _closed(x)
    assert ok.all()                                                 # the guard passes the whole range
    want = F(1) / np.sqrt(x, dtype=F)
    assert want.dtype == F and np.array_equal(r.view(np.uint32), want.view(np.uint32))
    assert len(np.unique(r)) > 1000                                 # a step function with many steps, not a constant


def test_the_floats_just_outside_fail_the_guard():
    x = _range()
    below, above = np.nextafter(x[0], F(0)), np.nextafter(x[-1], F(2))
    outside = np.array([below, above, F(0), F(1e-8), F(0.5), F(2), F(np.inf), F(np.nan)], F)
    t = np.float64(outside) * 2.0 ** 22 - 2.0 ** 22
    with np.errstate(invalid="ignore"):
        assert not (np.abs(t) <= 512.0).any()                       # NaN compares false: the device's `!(|t| <= 512)` sends it away
    assert np.float64(below) * 2.0 ** 22 - 2.0 ** 22 == -512.25 and np.float64(above) * 2.0 ** 22 - 2.0 ** 22 == 512.5


def test_a_once_normalised_vector_lands_in_the_range():
    """What the guard is for: len2 of a vector that normalized() scaled is within a few ulps of 1, far inside 2^-13."""
    rng = np.random.default_rng(7)
    v = rng.standard_normal((200000, 3)).astype(F)
    l2 = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
    u = v * (F(1) / np.sqrt(l2, dtype=F))[:, None]
    x = (u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2]
    assert x.dtype == F and np.abs(np.float64(x) - 1.0).max() <= 8 * 2.0 ** -24
    ok, r = _closed(x)
    assert ok.all() and np.array_equal(r.view(np.uint32), (F(1) / np.sqrt(x, dtype=F)).view(np.uint32))
