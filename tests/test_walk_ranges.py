"""Which lists may run on k_render_ctr_simple_qc (variant 14), decided without a GPU (csrc/device/rt_prepare.cpp: PreparedScene::walk_bounded, choose_variant;
through mi355rt_debug_prepare_scene).  The kernel's list walk tests the range of the quads' short division once per walk, from the rays' origins, and
looks only for denormals in front of the cubes' short reciprocals (rt_intersect.h, BOUNDED); both lean on bounded records: |D| <= 2^99 in every quad,
every entry of the 3 x 3 part of world_to_object and of zd at most 2^100 in every cube where the entry is finite, and no plane constant NaN or infinite.  A list outside the bounds goes to
k_render_ctr_simple (variant 3), whose tests are per primitive.  The last test repeats the kernel's f32 arithmetic at the bounds."""
import itertools

import numpy as np
import pytest

from conftest import load_for_both
from test_camera_masks import cube_prim, hand_scene, quad_prim

F = np.float32
QC, SIMPLE = 14, 3                       # KERNEL_LOCKSTEP_SIMPLE_QC, KERNEL_LOCKSTEP_SIMPLE (rt_device.h)
INF, NAN = float("inf"), float("nan")


def _quad(abi, D):
    q = quad_prim(abi, (2, 1, 2), (0, 0, 0), (0, -1, 0))
    q.data[12] = D
    return q


def _cube(abi, k, v):
    """An ordinary cube with word k of its world_to_object (column-major, 16 words) set to v."""
    c = cube_prim(abi, (1, 1.5, 0.7), (10, 20, 30), (0.5, 0.2, 0))
    c.data[16 + k] = v
    return c


def _variant(device, abi, prims, forced=-1):
    return device.prepare_scene(hand_scene(abi, [quad_prim(abi, (3, 1, 3), (0, 0, 0), (0, -1, 0))] + prims), forced).variant


def test_cornell_still_selects_the_kernel(native, oracle_mod, abi):
    host, device = native
    sc = load_for_both("cornell", oracle_mod, host, width=16, height=12, spp=1, max_depth=3)
    assert device.prepare_scene(sc).variant == QC


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_the_quad_bound_is_two_to_the_99(native, abi, sign):
    host, device = native
    edge = float(F(2.0 ** 99))
    assert _variant(device, abi, [_quad(abi, sign * edge)]) == QC
    assert _variant(device, abi, [_quad(abi, sign * float(np.nextafter(F(edge), F(INF))))]) == SIMPLE
    assert _variant(device, abi, [_quad(abi, sign * 2.0 ** 105)]) == SIMPLE


@pytest.mark.parametrize("k", [0, 1, 2, 4, 5, 6, 8, 9, 10])       # the 3 x 3 part of world_to_object (column-major: w2o[4 * column + row])
def test_the_cube_bound_is_two_to_the_100(native, abi, k):
    host, device = native
    edge = float(F(2.0 ** 100))
    for sign in (1.0, -1.0):
        assert _variant(device, abi, [_cube(abi, k, sign * edge)]) == QC
        assert _variant(device, abi, [_cube(abi, k, sign * float(np.nextafter(F(edge), F(INF))))]) == SIMPLE


def test_records_that_are_not_finite(native, abi):
    """A plane constant that is NaN or infinite does not qualify.  A cube entry that is NaN or infinite does: it can only make the object-space direction
    NaN or infinite, never a finite magnitude of 2^126 or more, and the short reciprocal is exact on both (rt_math.h recip_normal_range) -- such records
    (a cube of zero scale on one axis, tests/test_camera_masks.py) ran on this kernel before and keep their camera masks."""
    host, device = native
    for v in (INF, -INF, NAN):
        assert _variant(device, abi, [_quad(abi, v)]) == SIMPLE, v
        for k in (0, 5, 10, 12, 13, 14):                            # (12 .. 14: zd = translation * 0 is NaN for a translation that is not finite)
            assert _variant(device, abi, [_cube(abi, k, v)]) == QC, (k, v)
    for k in (12, 13, 14):
        assert _variant(device, abi, [_cube(abi, k, 2.0 ** 120)]) == QC                      # zd is 0 for a finite translation, whatever its size
    assert _variant(device, abi, [_quad(abi, 1.0), _cube(abi, 0, 1.0)]) == QC


def test_a_forced_kernel_is_not_kept_on_a_list_out_of_bounds(native, abi):
    host, device = native
    for prims in ([_quad(abi, 2.0 ** 105)], [_cube(abi, 5, 2.0 ** 101)], [_quad(abi, NAN)]):
        auto = _variant(device, abi, prims)
        assert auto == SIMPLE and _variant(device, abi, prims, forced=QC) == auto
    assert _variant(device, abi, [_quad(abi, 2.0 ** 99)], forced=QC) == QC
    assert _variant(device, abi, [_quad(abi, 2.0 ** 99)], forced=SIMPLE) == SIMPLE           # the general kernel takes either list


def test_the_numerator_stays_inside_the_proven_range_at_the_bounds():
    """hit_quad: num = D - ((n.x * o.x + n.y * o.y) + n.z * o.z) in f32, in that order.  With every |o| component below 2^60 (the walk's test), every
    normal component at most 2^25 (the host refuses more than 2^20) and |D| <= 2^99, |num| < 2^100: div_bounded's proven range."""
    top = np.nextafter(F(2.0 ** 60), F(0.0))
    n_max, d_max = F(2.0 ** 25), F(2.0 ** 99)
    signs = list(itertools.product((F(1.0), F(-1.0)), repeat=3))
    worst = F(0.0)
    for so in signs:
        for sn in signs:
            for sd in (F(1.0), F(-1.0)):
                o = [s * top for s in so]
                n = [s * n_max for s in sn]
                dot = F(F(F(n[0] * o[0]) + F(n[1] * o[1])) + F(n[2] * o[2]))
                num = F(sd * d_max - dot)
                assert np.isfinite(num) and abs(num) < F(2.0 ** 100), (so, sn, sd, num)
                worst = max(worst, abs(num))
    assert worst > d_max                                              # (the cases do push beyond |D|: the bound is used)
    # ... and the origin test itself: the first value that counts as wide is 2^60; NaN and infinities count as wide (`!(m < 2^60)`)
    assert top < F(2.0 ** 60) and not (F(2.0 ** 60) < F(2.0 ** 60)) and not (F(NAN) < F(2.0 ** 60)) and not (F(INF) < F(2.0 ** 60))
    # the cube: three products of a matrix entry of at most 2^100 with a direction component of at most 1 + 2^-21, summed, stay far below 2^126
    m, dmax = F(2.0 ** 100), F(1.0) + F(2.0 ** -21)
    assert F(F(F(m * dmax) + F(m * dmax)) + F(m * dmax)) < F(2.0 ** 102)
