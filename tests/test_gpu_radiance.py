"""Radiance queries on the resident scene (mi355rt_context_trace_radiance, mi355rt_trace_radiance): whole paths along caller-supplied rays.

The reference is oracle.render itself, because any ray can be a camera ray (tests/radiance_cases.py): the test makes a camera's rays on the host,
sample by sample, calls the query once per sample with [s, s + 1) carrying d_accum, and compares the means after the last call with the oracle's
linear image -- bit for bit where the path is only + - * / sqrt, within the parity contract (tests/parity.py) where libm is on it.  The chunking
and refill tests compare runs of the kernels with each other, anchored by the former."""
import numpy as np
import pytest

import fuzz_scenes
import radiance_cases as RC
import scene_shapes as SS
from conftest import load_for_both
from device_buffers import PATTERN, RadianceBuffers, packed_of
from parity import assert_parity, assert_same_bits_nan_folded

pytestmark = pytest.mark.gpu

F = np.float32


# ---- device plumbing ------------------------------------------------------------------------------------------------------------------
def buffers(device, n, samples, fill_nan=True):
    """The buffers of one query of n rays and up to `samples` samples per call."""
    return RadianceBuffers("trace_radiance", n, device.radiance_scratch_bytes(n, samples), fill_nan=fill_nan)


def query(ctx, abi, buf, begin, end, depth, seed=0, stream=None, want_linear=True):
    prm = abi.RadianceParams.make(begin, end, depth, seed)
    ctx.trace_radiance(prm, buf.rays.ptr, buf.n, buf.accum.ptr, buf.scratch.ptr, buf.linear.ptr if want_linear else None, stream)


def context_for(device, abi, sc):
    ctx = device.Context(0)
    ctx.set_scene(sc, abi.Camera(), abi.Settings(1, 1, 1, 1))             # a view the queries never look at
    return ctx


def render_by_query(device, abi, oracle_mod, sc, cam, W, H, S, depth, seed=0):
    """The image of `cam` through the query: one call per sample with that sample's camera rays, the sums carried.  float32 [H, W, 3]."""
    ctx = context_for(device, abi, sc)
    try:
        sums, means = buffers(device, W * H, 1).by_query(ctx, abi, S, lambda s: RC.camera_rays(oracle_mod, abi, cam, W, H, s, seed), depth, seed)
        assert (sums[:, 3].view(np.uint32) == 0).all()                      # the fourth word of a sum is written +0
        return means.reshape(H, W, 3)
    finally:
        ctx.close()


def oracle_linear(oracle_mod, abi, sc, cam, W, H, S, depth, seed=0):
    _, linear, _ = oracle_mod.render(sc, cam, abi.Settings(W, H, S, depth), abi.Options.make(seed=seed), threads=4)
    return linear


# ---- 1: exact against oracle.render ------------------------------------------------------------------------------------------------------
def quad_centres(sc):
    out = []
    for i in range(sc.c.n_primitives):
        p = sc.c.primitives[i]
        if p.kind == SS.QUAD:
            d = np.array(list(p.data[0:9]), np.float64)
            out.append(d[0:3] + 0.5 * d[3:6] + 0.5 * d[6:9])
    return np.array(out)


def _wall_camera(sc):
    """ON a wall of the cornell box: the camera sits at the centre of the list's first quad, in its plane, and looks across the box."""
    from oracle import scene_loader as L
    c = quad_centres(sc)
    middle = c.mean(axis=0)
    at = middle + np.array([0.3, -0.2, 0.1]) * np.linalg.norm(c[0] - middle)
    return L.camera_new(tuple(float(F(v)) for v in c[0]), tuple(float(F(v)) for v in at), (0.0, 1.0, 0.0), F(70.0), F(4.0 / 3.0))


def _away_camera(sc):
    """Outside the box, looking away from it: every ray misses."""
    from oracle import scene_loader as L
    m = quad_centres(sc).mean(axis=0)
    return L.camera_new((float(m[0]), float(m[1]), float(m[2]) + 30.0), (float(m[0]), float(m[1]), float(m[2]) + 60.0), (0.0, 1.0, 0.0), F(40.0), F(4.0 / 3.0))


_scenes = {}


def materials_scene(abi, host):
    """Spheres, planes, quads and cubes under every exact material kind: dielectric, metal (mirror and fuzzed), checker, plastic."""
    if "materials" not in _scenes:
        _scenes["materials"] = fuzz_scenes.random_scene(abi, host, 12, True, only_kinds=[abi.PRIM_SPHERE, abi.PRIM_PLANE, abi.PRIM_QUAD, abi.PRIM_CUBE],
                                                        every_material=True)
    return _scenes["materials"]


def exact_case(name, abi, host, oracle_mod):
    """name -> (scene, camera, W, H, S, depth, seed)."""
    cornell = lambda W=16, H=12: load_for_both("cornell", oracle_mod, host, width=W, height=H, spp=1, max_depth=8)
    if name == "cornell":
        sc = cornell(); return sc, sc.camera, 16, 12, 8, 8, 0
    if name == "cornell_seed_high_word":
        sc = cornell(); return sc, sc.camera, 16, 12, 8, 8, 0xFFFFFFFF
    if name == "cornell_13x7":
        sc = cornell(13, 7); return sc, sc.camera, 13, 7, 8, 8, 0
    if name == "cornell_depth1":
        sc = cornell(); return sc, sc.camera, 16, 12, 8, 1, 0
    if name == "cornell_depth0":
        sc = cornell(); return sc, sc.camera, 16, 12, 8, 0, 0
    if name == "cornell_on_a_wall":
        sc = cornell(); return sc, _wall_camera(sc), 16, 12, 4, 8, 0
    if name == "cornell_looking_away":
        sc = cornell(); return sc, _away_camera(sc), 16, 12, 4, 8, 0
    if name.startswith("shapes_"):                                       # the off-view cameras of tests/scene_shapes.py on its mesh-free camera scene
        sc = SS.camera_scene(abi, host, "meshfree")
        return sc, SS.camera(name[len("shapes_"):], abi, sc), 16, 12, 4, SS.DEPTH, 0
    if name == "mesh":                                                   # a list with meshes, no sky, no rough conductor: k_radiance_paths_mesh
        sc = SS.camera_scene(abi, host, "mesh"); return sc, sc.camera, 12, 9, 4, SS.DEPTH, 0
    if name == "materials":
        sc = materials_scene(abi, host); return sc, sc.camera, 16, 12, 6, 8, 0
    raise KeyError(name)


EXACT = ["cornell", "cornell_seed_high_word", "cornell_13x7", "cornell_depth1", "cornell_depth0", "cornell_on_a_wall", "cornell_looking_away",
         "shapes_inside", "shapes_sheared", "shapes_wide", "shapes_looking_down", "mesh", "materials"]


@pytest.mark.parametrize("name", EXACT)
def test_camera_rays_give_the_oracles_image_bit_for_bit(name, native, oracle_mod, abi):
    host, device = native
    sc, cam, W, H, S, depth, seed = exact_case(name, abi, host, oracle_mod)
    want = oracle_linear(oracle_mod, abi, sc, cam, W, H, S, depth, seed)
    got = render_by_query(device, abi, oracle_mod, sc, cam, W, H, S, depth, seed)
    assert_same_bits_nan_folded(got, want, name)
    if name == "cornell_depth0":
        assert (got.view(np.uint32) == 0).all()                             # every word +0
    elif name == "cornell_looking_away":
        miss = np.array(list(sc.c.miss_color), F)
        assert (got == miss[None, None, :]).all()                           # all misses
    else:
        assert len(np.unique(got.reshape(-1, 3), axis=0)) > 1              # an image, not a constant


def test_the_mesh_case_runs_the_mesh_kernel_and_the_materials_case_holds_them(native, abi):
    host, _ = native
    sc = SS.camera_scene(abi, host, "mesh")
    assert abi.PRIM_MESH in {sc.c.primitives[i].kind for i in range(sc.c.n_primitives)} and not sc.c.sky_rgb
    sc = materials_scene(abi, host)
    used = {sc.c.materials[sc.c.primitives[i].material].kind for i in range(sc.c.n_primitives)}
    assert {abi.MAT_DIELECTRIC, abi.MAT_METAL, abi.MAT_LAMBERT_CHECKER} <= used
    assert abi.PRIM_MESH not in {sc.c.primitives[i].kind for i in range(sc.c.n_primitives)}


# ---- 2: the scenes with libm on the path ----------------------------------------------------------------------------------------------
# name, W, H, spp, depth: the smallest image tests/test_gpu_parity.py renders of each
TOLERANT = [("veach", 64, 36, 8, 16), ("teapot", 64, 48, 4, 16), ("semesterbild", 64, 48, 8, 30)]


@pytest.mark.parametrize("name,W,H,S,depth", TOLERANT)
def test_tolerant_scenes_meet_the_parity_contract(name, W, H, S, depth, native, oracle_mod, abi):
    """Veach (rough conductors), teapot (the sky lookup behind miss_colour), semesterbild (a mesh and rough conductors).  Both packed images are
    made from the linear ones by the same numpy sqrt, clamp and truncate."""
    host, device = native
    sc = load_for_both(name, oracle_mod, host, width=W, height=H, spp=S, max_depth=depth)
    want = oracle_linear(oracle_mod, abi, sc, sc.camera, W, H, S, depth)
    got = render_by_query(device, abi, oracle_mod, sc, sc.camera, W, H, S, depth)
    assert_parity(packed_of(got), got, packed_of(want), want, exact=False)


# ---- 3: chunking and refill: runs of the kernels against each other -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def cornell_ctx(native, oracle_mod, abi):
    host, device = native
    sc = load_for_both("cornell", oracle_mod, host, width=8, height=8, spp=1, max_depth=8)
    ctx = context_for(device, abi, sc)
    yield ctx, sc
    ctx.close()


DEPTH = 12


def one_call(device, abi, ctx, rays, S, depth=DEPTH, seed=5):
    import torch
    buf = buffers(device, len(rays), S)
    buf.rays.upload(rays)
    query(ctx, abi, buf, 0, S, depth, seed)
    torch.cuda.synchronize()
    return buf.read()


_whole = {}


def whole(device, abi, ctx, S):
    """[0, S) of the fixed rays in one call with the default K: computed once, shared, read-only."""
    if S not in _whole:
        sums, means = one_call(device, abi, ctx, RC.fixed_rays(abi), S)
        sums.setflags(write=False); means.setflags(write=False)
        _whole[S] = (sums, means)
    return _whole[S]


@pytest.mark.parametrize("S", [1, 15, 16, 17, 40])
def test_any_chunking_gives_the_words_of_one_call(S, native, abi, cornell_ctx):
    import torch
    _, device = native
    ctx, _ = cornell_ctx
    rays = RC.fixed_rays(abi)
    sums, means = whole(device, abi, ctx, S)
    assert np.isfinite(sums).all() and (sums[:, :3] > 0).any()             # the NaN the sums were pre-filled with was not read
    # S calls of one sample
    buf = buffers(device, len(rays), 1)
    buf.rays.upload(rays)
    for s in range(S):
        query(ctx, abi, buf, s, s + 1, DEPTH, 5)
    torch.cuda.synchronize()
    got_sums, got_means = buf.read()
    assert got_sums.tobytes() == sums.tobytes() and got_means.tobytes() == means.tobytes(), "S calls of one sample"
    # [0, a), [a, S) for an uneven a; the scratch is sized for the larger chunk
    if S > 1:
        a = {15: 4, 16: 5, 17: 16, 40: 17}[S]
        buf = buffers(device, len(rays), max(a, S - a))
        buf.rays.upload(rays)
        query(ctx, abi, buf, 0, a, DEPTH, 5)
        query(ctx, abi, buf, a, S, DEPTH, 5)
        torch.cuda.synchronize()
        got_sums, got_means = buf.read()
        assert got_sums.tobytes() == sums.tobytes() and got_means.tobytes() == means.tobytes(), f"[0, {a}), [{a}, {S})"
    ctx.check()


@pytest.mark.parametrize("K", [1, 2, 64])
def test_items_per_lane_does_not_change_a_word(K, native, abi, cornell_ctx):
    _, device = native
    ctx, _ = cornell_ctx
    S = 17                                                                  # 300 * 17 = 5100 items: 80 waves at K = 1, 2 at K = 64 (the second one 1004 items long)
    sums, means = whole(device, abi, ctx, S)
    try:
        ctx.set_knob("radiance_items", K)
        got_sums, got_means = one_call(device, abi, ctx, RC.fixed_rays(abi), S)
    finally:
        ctx.set_knob("radiance_items", 0)
    assert got_sums.tobytes() == sums.tobytes() and got_means.tobytes() == means.tobytes()


def test_one_ray_and_no_ray(native, abi, cornell_ctx):
    import torch
    _, device = native
    ctx, _ = cornell_ctx
    rays = RC.fixed_rays(abi)
    sums, means = whole(device, abi, ctx, 17)
    got_sums, got_means = one_call(device, abi, ctx, rays[5:6], 17)
    assert got_sums.tobytes() == sums[5:6].tobytes() and got_means.tobytes() == means[5:6].tobytes()
    buf = buffers(device, 1, 17)
    buf.rays.upload(rays[5:6])
    query(ctx, abi, buf, 0, 17, DEPTH, 5, want_linear=False)                # without the optional means
    torch.cuda.synchronize()
    s1, l1 = buf.read()
    assert s1.tobytes() == sums[5:6].tobytes() and (l1.view(np.uint8) == PATTERN).all()
    buf = buffers(device, 0, 1)                                             # n_rays == 0: MI355RT_OK, nothing written
    ctx.trace_radiance(abi.RadianceParams.make(0, 1, 4), None, 0, None, None, None, None)
    torch.cuda.synchronize()
    buf.read()


def test_the_one_shot_equals_the_context_call(native, abi, cornell_ctx):
    _, device = native
    ctx, sc = cornell_ctx
    rays = RC.fixed_rays(abi)
    sums, means = whole(device, abi, ctx, 17)
    a, l = device.trace_radiance(sc, rays, abi.RadianceParams.make(0, 5, DEPTH, 5))
    a2, l2 = device.trace_radiance(sc, rays, abi.RadianceParams.make(5, 17, DEPTH, 5), accum=a)
    assert a2.tobytes() == sums.tobytes() and l2.tobytes() == means.tobytes()
    assert not np.array_equal(a, a2)                                        # (the first call's sums were not changed in place)
    a3, l3 = device.trace_radiance(sc, rays, abi.RadianceParams.make(0, 17, DEPTH, 5), want_linear=False)
    assert a3.tobytes() == sums.tobytes() and l3 is None


def test_beside_a_render_of_the_same_context(native, oracle_mod, abi):
    """A query enqueued on a second stream while a render of the same context is in flight: both results are those of their solo runs."""
    import torch
    host, device = native
    W, H = 64, 48
    sc = load_for_both("cornell", oracle_mod, host, width=W, height=H, spp=16, max_depth=8)
    ctx = device.Context(0)
    try:
        ctx.set_scene(sc, sc.camera, sc.settings)
        rays = RC.fixed_rays(abi)
        want_sums, want_means = one_call(device, abi, ctx, rays, 17)
        want_packed = torch.zeros((H, W), dtype=torch.int32, device="cuda")
        ctx.render(want_packed.data_ptr())
        torch.cuda.synchronize()
        s_render, s_query = torch.cuda.Stream(), torch.cuda.Stream()
        packed = torch.zeros((H, W), dtype=torch.int32, device="cuda")
        buf = buffers(device, len(rays), 17)
        buf.rays.upload(rays)
        torch.cuda.synchronize()
        ctx.render(packed.data_ptr(), None, None, s_render.cuda_stream)
        query(ctx, abi, buf, 0, 17, DEPTH, 5, stream=s_query.cuda_stream)
        ctx.render(packed.data_ptr(), None, None, s_render.cuda_stream)
        torch.cuda.synchronize()
        ctx.check()
        got_sums, got_means = buf.read()
        assert got_sums.tobytes() == want_sums.tobytes() and got_means.tobytes() == want_means.tobytes()
        assert torch.equal(packed, want_packed)
    finally:
        ctx.close()
