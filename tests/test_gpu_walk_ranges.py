"""k_render_ctr_simple_qc (variant 14) decides the argument ranges of its short division and short reciprocals once per walk (rt_intersect.h, BOUNDED):
one wave-uniform bit from the rays' origins for every quad of the list, one denormal test per cube, and a host-side bound on the records that lets a list
use the kernel at all (rt_prepare.cpp, walk_bounded).  These scenes reach each of the three on purpose, next to ordinary geometry, bit for bit against
the oracle (plain IEEE arithmetic on the CPU): packed pixels, linear f32 words and the ray count, with and without the camera masks.

About the first scene.  A quad is a candidate only where |n . d| >= 1e-4, so a ray from an ordinary origin meets a plane through the origin within
|n . o| / 1e-4 -- no first hit of this camera can lie beyond 2^60 on a quad with D = 0, whatever its extent.  What puts origins beyond 2^60 is a wall
far away: `far_wall` stands 2^61 behind the scene, every camera ray that leaves the ordinary geometry lands on it, and the bounce from there starts
beyond 2^60 (a wide wave) and comes down on the 2^64 quad far out, while the paths that stay among the floor, the cube and the light keep their waves
narrow.  The scene builder is the one of tests/test_gpu_extreme_scales.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

QC = 14                                                           # KERNEL_LOCKSTEP_SIMPLE_QC (rt_device.h)
F = np.float32


def _scene(abi, host, wide_quad=False, far_wall=False, huge_cube=False, huge_quad=False, flat_cube=False):
    from oracle import scene_loader as L
    mats = []

    def mat(kind, albedo=(0, 0, 0), p0=0.0):
        m = abi.Material(); m.kind = kind; m.albedo[:] = [float(F(v)) for v in albedo]; m.p0 = float(F(p0)); mats.append(m); return len(mats) - 1

    grey, red, light = mat(abi.MAT_LAMBERT_SOLID, (0.7, 0.7, 0.7)), mat(abi.MAT_LAMBERT_SOLID, (0.8, 0.2, 0.1)), mat(abi.MAT_EMISSIVE, (4, 4, 4))
    prims = []

    def quad(scale, translate, material, euler=(0.0, 0.0, 0.0), grow=1.0):
        m = L.mat4_from_scale_rotation_translation([F(v) for v in scale], L.quat_from_euler_yxz_deg(*[F(v) for v in euler]), [F(v) for v in translate])
        d = np.array(L.quad_from_matrix(m), F)
        if grow != 1.0:                                                   # base and edges times a power of two (the constructor's own cross product would overflow):
            d[0:9] *= F(grow)                                             # the unit normal stays, D = n . base and 1 / |e|^2 are the constructor's for the grown quad
            with np.errstate(all="ignore"):                               # (1 / |e|^2 is 0 once |e|^2 overflows)
                d[12] = F(F(d[9] * d[0] + d[10] * d[1]) + d[11] * d[2])
                for k, e in ((13, d[3:6]), (14, d[6:9])):
                    e2 = F(F(e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
                    d[k] = F(1.0) / e2
        p = abi.Primitive(); p.kind = abi.PRIM_QUAD; p.material = material; p.data[0:15] = [float(v) for v in d]; prims.append(p)

    def cube(scale, translate, material, euler=(20.0, 30.0, 10.0)):
        m = L.mat4_from_scale_rotation_translation([F(v) for v in scale], L.quat_from_euler_yxz_deg(*[F(v) for v in euler]), [F(v) for v in translate])
        p = abi.Primitive(); p.kind = abi.PRIM_CUBE; p.material = material
        p.data[0:16] = [float(v) for v in m]; p.data[16:32] = [float(v) for v in L.mat4_inverse(m)]; prims.append(p)

    quad((8, 1, 8), (0, -1, 0), grey)                                   # an ordinary floor ...
    cube((1.5, 1.5, 1.5), (0.5, 0.0, -1.0), red)                        # ... an ordinary cube ...
    quad((3, 1, 3), (0, 4, 0), light, euler=(0.0, 180.0, 0.0))          # ... and a light above them
    if wide_quad:
        quad((1, 1, 1), (0, 0, 0), grey, grow=2.0 ** 64)                 # edges of 2^64 through the origin: D = 0, a unit normal
    if far_wall:
        quad((4, 1, 4), (0, 0, -1), grey, euler=(90.0, 0.0, 0.0), grow=2.0 ** 61)   # edges of 2^63, facing the camera from 2^61 away (|D| = 2^61, inside the bound)
    if huge_quad:
        quad((1, 1, 1), (0, -1, 0), grey, grow=2.0 ** 105)               # a floor 2^105 below: |D| = 2^105 with a unit normal, outside the bound of 2^99.  (The older
                                                                        # file's quad((2^40, 1, 2^40), (0, -2^105, 0)) stores a ZERO normal and D = 0 -- the constructor's
                                                                        # |e0 x e1|^2 overflows -- so its record is inside the bound.)
    if flat_cube:
        with np.errstate(all="ignore"):
            cube((1.0, 0.0, 1.0), (-1.5, 0.5, 0.5), grey)               # zero scale on one axis: its world_to_object is infinities and NaN
    if huge_cube:
        cube((2.0 ** 115, 40.0, 40.0), (0, 0, 0), grey, euler=(0.0, 0.0, 0.0))   # w2o = diag(2^-115, 1/40, 1/40), inside the bound: the object-space direction's x
                                                                        # is a denormal for every ray with |d.x| < 2^-11
    sc = L.LoadedScene(); sc.materials, sc.primitives, sc.meshes, sc.triangles = mats, prims, [], np.zeros((0, 12), F)
    sc.finalize(); sc.c.miss_color[:] = [0.5, 0.6, 0.7]
    sc._keep = host.attach_bvh(sc)
    sc.camera = L.camera_new((0.0, 1.0, 6.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), F(55.0), F(4.0 / 3.0))
    return sc


W, H, SPP, DEPTH = 96, 72, 8, 6
SEEDS = (11, 12345)
_oracle = {}


def _expected(oracle_mod, abi, name, sc, seed):
    """The oracle's render of a scene, computed once and shared by the cam_cull cases."""
    if (name, seed) not in _oracle:
        _oracle[(name, seed)] = oracle_mod.render(sc, sc.camera, abi.Settings(W, H, SPP, DEPTH), abi.Options.make(rng_mode=abi.RNG_CTR, seed=seed))
    return _oracle[(name, seed)]


def _check(device, oracle_mod, abi, name, sc, cull, want_qc):
    import torch
    st = abi.Settings(W, H, SPP, DEPTH)
    for seed in SEEDS:
        opt = abi.Options.make(rng_mode=abi.RNG_CTR, seed=seed)
        ctx = device.Context(0)
        try:
            ctx.set_knob("cam_cull", cull)
            ctx.set_scene(sc, sc.camera, st)
            assert (ctx.kernel_variant() == QC) == want_qc, ctx.kernel_variant()
            packed = torch.full((W * H,), -1, dtype=torch.int32, device="cuda:0")
            linear = torch.full((W * H * 3,), float("nan"), dtype=torch.float32, device="cuda:0")
            s = ctx.render(packed.data_ptr(), linear.data_ptr(), opt, want_stats=True)
            ctx.check()
            gp, gl = packed.cpu().numpy().view(np.uint32), linear.cpu().numpy().view(np.uint32)
        finally:
            ctx.close()
        op, ol, cnt = _expected(oracle_mod, abi, name, sc, seed)
        assert s.rays == cnt.rays, (seed, s.rays, cnt.rays)
        assert np.array_equal(gl, np.asarray(ol).view(np.uint32).reshape(-1)), (seed, "linear f32")
        assert np.array_equal(gp, np.asarray(op).view(np.uint32).reshape(-1)), (seed, "packed pixels")


def _plane_hit_distance(sc, abi, i, d):
    """t of the camera ray with direction `d` on the plane of quad i (f32, the quad test's order)."""
    q = [F(v) for v in sc.c.primitives[i].data[0:15]]
    n, D = q[9:12], q[12]
    o = [F(v) for v in sc.camera.position]
    with np.errstate(all="ignore"):
        den = F(F(n[0] * d[0] + n[1] * d[1]) + n[2] * d[2])
        num = D - F(F(n[0] * o[0] + n[1] * o[1]) + n[2] * o[2])
        return float(num / den), float(den)


@pytest.mark.parametrize("cull", [0, 1])
def test_wide_for_some_waves_narrow_for_others(native, oracle_mod, abi, cull):
    host, device = native
    sc = _scene(abi, host, wide_quad=True, far_wall=True)
    assert device.prepare_scene(sc).variant == QC
    wide_q = [F(v) for v in sc.c.primitives[3].data[0:15]]
    assert max(abs(v) for v in wide_q[3:9]) == 2.0 ** 64 and wide_q[12] == 0.0 and sorted(abs(v) for v in wide_q[9:12]) == [0.0, 0.0, 1.0]
    t_far, den = _plane_hit_distance(sc, abi, 4, [F(v) for v in sc.camera.forward])                # the view axis ends on the far wall, beyond 2^60 ...
    assert abs(den) > 0.5 and 2.0 ** 60 < t_far < 2.0 ** 62
    down = np.array([0.0, -1.0, -1.0], F) / F(np.sqrt(2.0))
    t_near, _ = _plane_hit_distance(sc, abi, 3, [F(v) for v in down])                               # ... and a ray towards the ground meets the 2^64 quad within a few units
    assert 0.0 < t_near < 10.0
    _check(device, oracle_mod, abi, "wide", sc, cull, True)


@pytest.mark.parametrize("cull", [0, 1])
def test_denormal_object_space_direction(native, oracle_mod, abi, cull):
    host, device = native
    sc = _scene(abi, host, huge_cube=True)
    got = device.prepare_scene(sc)
    assert got.variant == QC
    assert float(np.abs(got.prims["d"][3][0:9]).max()) < 0.03 and float(got.prims["d"][3][0]) == 2.0 ** -115
    _check(device, oracle_mod, abi, "denormal", sc, cull, True)


@pytest.mark.parametrize("cull", [0, 1])
def test_records_out_of_bounds_leave_the_kernel(native, oracle_mod, abi, cull):
    host, device = native
    sc = _scene(abi, host, huge_quad=True)
    got = device.prepare_scene(sc)
    auto = got.variant
    assert abs(float(got.prims["d"][3][3])) == 2.0 ** 105 and sorted(abs(float(v)) for v in got.prims["d"][3][0:3]) == [0.0, 0.0, 1.0]
    assert auto != QC and device.prepare_scene(sc, QC).variant == auto
    _check(device, oracle_mod, abi, "out_of_bounds", sc, cull, False)


@pytest.mark.parametrize("cull", [0, 1])
def test_a_cube_record_that_is_not_finite_stays_on_the_kernel(native, oracle_mod, abi, cull):
    host, device = native
    sc = _scene(abi, host, flat_cube=True)
    got = device.prepare_scene(sc)
    assert got.variant == QC and not np.isfinite(got.prims["d"][3][0:9]).all()
    _check(device, oracle_mod, abi, "flat", sc, cull, True)
