"""Closest-hit ray queries on the resident scene (mi355rt_context_trace_rays, mi355rt_context_first_hits, mi355rt_trace_rays) against the
oracle's per-ray hook, oracle.scene_hit: position, normal, t, front_face bit for bit (NaNs folded), WHICH primitive won, and the whole record
for misses.

The oracle reports the winner's material, not its list index.  So every scene here first gives each primitive a material record of its own
(a copy of the one it had; primitive.material = its list index): the oracle's material then IS the winning primitive, and with the coincident
primitives of the fuzz scenes the tie-break order of hittable.rs:45-58 is checked (the first wins for sphere, plane and quad, the last for
cube and mesh)."""
import ctypes as C
import functools

import numpy as np
import pytest

import fuzz_scenes
import kat_f32 as K
from device_buffers import Guarded
from parity import assert_same_bits_nan_folded

pytestmark = pytest.mark.gpu

F = np.float32


# ---- scenes, built once -------------------------------------------------------------------------------------------------------------
def own_materials(abi, sc):
    n = sc.c.n_primitives
    mats = (abi.Material * n)()
    for i in range(n):
        mats[i] = sc.c.materials[sc.c.primitives[i].material]
        sc.c.primitives[i].material = i
    sc._own_mats = mats
    sc.c.materials, sc.c.n_materials = mats, n
    return sc


_scenes = {}


def scene(name, abi, host):
    if name not in _scenes:
        make = {"kinds": lambda: fuzz_scenes.random_scene(abi, host, 3, True, coincident=True),
                "fourkinds": lambda: fuzz_scenes.random_scene(abi, host, 3, True, only_kinds=[abi.PRIM_SPHERE, abi.PRIM_PLANE, abi.PRIM_QUAD, abi.PRIM_CUBE],
                                                              coincident=True),
                "deep": lambda: fuzz_scenes.random_scene(abi, host, 5, True, big_mesh_tris=3000),
                "meshfree": lambda: fuzz_scenes.random_scene(abi, host, 7, True, only_kinds=[abi.PRIM_QUAD, abi.PRIM_CUBE], lambert_only=True)}[name]
        _scenes[name] = own_materials(abi, make())
    return _scenes[name]


def kinds_rays():
    rng = np.random.default_rng(3)
    n = 2048 + 37
    o = np.zeros((n, 3), F); d = np.zeros((n, 3), F)
    for i in range(n):
        o[i] = rng.uniform(-4, 4, 3)
        d[i] = rng.normal(size=3) * rng.uniform(0.5, 3)                  # un-normalised on purpose
    return o, d


def deep_rays(sc):
    rng = np.random.default_rng(55)
    centre = np.array(sc.c.primitives[sc.c.n_primitives - 1].data[12:15], np.float64)
    p = rng.normal(size=(512, 3)); p = p / np.linalg.norm(p, axis=1, keepdims=True) * 4.0 + centre
    target = centre + rng.uniform(-1.2, 1.2, (512, 3))
    return p.astype(F), (target - p).astype(F)


def camera_dirs(cam, W, H):
    """Camera::get_ray's direction (camera.rs:34-41) for the centre of every pixel, numpy float32 in the reference's operation order; normalised
    once here (get_ray), the second time by Ray::new -- in the oracle's hook."""
    x, y = np.arange(W, dtype=F), np.arange(H, dtype=F)
    u, v = (x + F(0.5)) / F(W), (y + F(0.5)) / F(H)
    ax = (F(2.0) * u - F(1.0)) * F(cam.half_width)
    ay = (F(1.0) - F(2.0) * v) * F(cam.half_height)
    right, up, fwd = (np.array(list(a), F) for a in (cam.right, cam.true_up, cam.forward))
    raw = fwd[None, None, :] + (right[None, None, :] * ax[None, :, None] + up[None, None, :] * ay[:, None, None])
    assert raw.dtype == F
    out = np.zeros((H, W, 3), F)
    for j in range(H):
        for i in range(W):
            out[j, i] = K.normalized(raw[j, i])
    return out


# ---- the oracle's answers, computed once per (scene, rays) ----------------------------------------------------------------------------
_oracle = {}


def oracle_hits(key, oracle_mod, abi, sc, origins, dirs):
    if key not in _oracle:
        out = np.zeros(len(origins), abi.HIT_DTYPE)
        for i, (o, d) in enumerate(zip(origins, dirs)):
            hit, r = oracle_mod.scene_hit(sc, o, d)
            if hit:
                out[i]["position"], out[i]["normal"], out[i]["t"] = r[0:3], r[3:6], r[6]
                out[i]["material"] = out[i]["primitive"] = int(r[7])     # own_materials(): the material index is the list index
                out[i]["front_face"] = int(r[8])
            else:
                out[i]["t"], out[i]["primitive"], out[i]["material"] = F(np.inf), abi.NO_HIT, abi.NO_HIT
        out.setflags(write=False)
        _oracle[key] = out
    return _oracle[key]


def assert_records(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    for f in ("primitive", "material", "front_face", "_pad"):
        bad = np.argwhere(got[f] != want[f])
        assert not len(bad), f"{what}: {f} differs at {bad[:6].tolist()}: got {got[f][tuple(bad[0])]} want {want[f][tuple(bad[0])]} ({len(bad)} records)"
    for f in ("position", "t", "normal"):
        assert_same_bits_nan_folded(got[f], want[f], f"{what}: {f}")
    miss = want["primitive"] == 0xFFFFFFFF
    assert got[miss].tobytes() == want[miss].tobytes(), f"{what}: a miss record is not (0, 0, 0, +inf, 0, 0, 0, 0, NO_HIT, NO_HIT, 0, 0)"


# ---- device plumbing ------------------------------------------------------------------------------------------------------------------
def to_device_rays(abi, origins, dirs):
    import torch
    r = np.zeros((len(origins), 8), F)
    r[:, 0:3], r[:, 4:7] = origins, dirs
    r[:, 3], r[:, 7] = F(np.nan), F(-1e30)                              # the pads are ignored
    return torch.from_numpy(r).cuda()


def hit_buffer(n):
    """n hit records with eight records of guard bytes behind them."""
    return Guarded(n * 48, guard=8 * 48)


def read_hits(abi, buf):
    return buf.read(abi.HIT_DTYPE, "the query's hit records")


def context_for(device, abi, sc, W=64, H=48, spp=1, depth=1):
    ctx = device.Context(0)
    ctx.set_scene(sc, sc.camera, abi.Settings(W, H, spp, depth))
    return ctx


def trace(device, abi, ctx, origins, dirs, stream=None):
    import torch
    n = len(origins)
    rays, hits = to_device_rays(abi, origins, dirs), hit_buffer(n)
    torch.cuda.synchronize()
    ctx.trace_rays(rays.data_ptr(), n, hits.ptr, stream)
    torch.cuda.synchronize()
    return read_hits(abi, hits)


def first_hits(device, abi, ctx, n, options=None):
    import torch
    hits = hit_buffer(n)
    torch.cuda.synchronize()
    ctx.first_hits(hits.ptr, options)
    torch.cuda.synchronize()
    return read_hits(abi, hits)


# ---- 1: every kind, arbitrary rays ------------------------------------------------------------------------------------------------------
def test_every_primitive_kind_with_arbitrary_rays(native, oracle_mod, abi):
    host, device = native
    sc = scene("kinds", abi, host)
    o, d = kinds_rays()
    want = oracle_hits("kinds", oracle_mod, abi, sc, o, d)
    # what the fixture must exercise, asserted on the ORACLE's answers
    assert sc.c.n_primitives == 30
    hit = want["primitive"] != abi.NO_HIT
    kinds = np.array([sc.c.primitives[int(p)].kind for p in want["primitive"][hit]])
    wins = np.bincount(kinds, minlength=5)
    print("misses", int((~hit).sum()), "wins per kind", wins.tolist(), "front", int(want["front_face"][hit].sum()), "back", int((want["front_face"][hit] == 0).sum()),
          "distinct winners", len(set(want["primitive"][hit].tolist())))
    assert (wins >= 20).all() and (~hit).sum() >= 200, (wins, (~hit).sum())
    assert (want["front_face"][hit] == 1).any() and (want["front_face"][hit] == 0).any()
    ctx = context_for(device, abi, sc)
    try:
        got = trace(device, abi, ctx, o, d)                              # 2048 + 37: the last wave and the last workgroup are partial
        assert_records(got, want, "2085 rays")
        for n in (1, 63, 64, 65):
            part = trace(device, abi, ctx, o[:n], d[:n])
            assert part.tobytes() == got[:n].tobytes(), n
    finally:
        ctx.close()


# ---- 2: a deep tree ---------------------------------------------------------------------------------------------------------------------
def test_a_deep_tree(native, oracle_mod, abi):
    host, device = native
    sc = scene("deep", abi, host)
    o, d = deep_rays(sc)
    want = oracle_hits("deep", oracle_mod, abi, sc, o, d)
    big = sc.c.n_primitives - 1
    assert sc.c.primitives[big].kind == abi.PRIM_MESH and sc.c.meshes[sc.c.primitives[big].mesh].node_count > 2000
    n_big, n_miss = int((want["primitive"] == big).sum()), int((want["primitive"] == abi.NO_HIT).sum())
    print("big-mesh wins", n_big, "misses", n_miss, "others", len(want) - n_big - n_miss)
    assert n_big >= 100 and n_miss >= 50, (n_big, n_miss)
    ctx = context_for(device, abi, sc, 32, 24)
    try:
        assert_records(trace(device, abi, ctx, o, d), want, "512 rays at the big mesh")
    finally:
        ctx.close()


# ---- 3: per-pixel first hits ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,W,H", [("kinds", 64, 48), ("deep", 32, 24), ("meshfree", 32, 24)])
def test_first_hits_of_every_pixel(name, W, H, native, oracle_mod, abi):
    host, device = native
    sc = scene(name, abi, host)
    dirs = camera_dirs(sc.camera, W, H).reshape(-1, 3)
    origins = np.tile(np.array(list(sc.camera.position), F), (W * H, 1))
    want = oracle_hits((name, "camera", W, H), oracle_mod, abi, sc, origins, dirs)
    n_miss = int((want["primitive"] == abi.NO_HIT).sum())
    print(name, "misses", n_miss, "of", W * H)
    if name == "meshfree":
        assert n_miss > (W * H) // 2 and n_miss < W * H                  # a mostly-missing view
    ctx = context_for(device, abi, sc, W, H)
    try:
        assert ctx.kernel_variant() in ((3, 14) if name == "meshfree" else (7, 10, 12, 13))      # the mesh-free form / the form with the BVH walk
        whole = first_hits(device, abi, ctx, W * H)
        assert_records(whole, want, f"{name} {W}x{H}")
        opt = abi.Options.make(row_begin=3, row_end=H - 2, strip_rows=2, n_parts=3, part=1, rng_mode=7, seed=99, workspace_bytes=1)   # (rng_mode, seed, workspace: ignored)
        rows = abi.rows_selected(H, opt)
        assert 0 < len(rows) < H and ctx.rows_selected(abi.Options.make(row_begin=3, row_end=H - 2, strip_rows=2, n_parts=3, part=1)) == len(rows)
        some = first_hits(device, abi, ctx, len(rows) * W, opt)
        assert some.tobytes() == whole.reshape(H, W)[rows].tobytes()
        assert first_hits(device, abi, ctx, W * H).tobytes() == whole.tobytes()       # back to the whole image: the first table again
    finally:
        ctx.close()


# ---- 4: degenerate rays -----------------------------------------------------------------------------------------------------------------
def test_degenerate_rays(native, oracle_mod, abi):
    host, device = native
    sc = scene("kinds", abi, host)
    o, d = degenerate_rays()
    want = oracle_hits("degenerate", oracle_mod, abi, sc, o, d)
    ctx = context_for(device, abi, sc)
    try:
        got = trace(device, abi, ctx, o, d)
    finally:
        ctx.close()
    for i in range(len(o)):
        print(i, o[i].tolist(), d[i].tolist(), "oracle", want[i], "device", got[i])
    assert_records(got, want, "24 degenerate rays")


def degenerate_rays():
    nan, inf = float("nan"), float("inf")
    dirs = [(0, 0, 0), (1e-5, 0, 0), (0, -1e-30, 0), (0, -1e30, 0), (0, -1, 0), (nan, 1, 0), (inf, 0, 0), (1, 0, 0)]
    origins = [(0, 1, 9), (0, 0, 0), (nan, 0, 0)]
    return np.array([oo for oo in origins for _ in dirs], F), np.array([dd for _ in origins for dd in dirs], F)


# ---- 4b: the mesh-free ray-buffer form (k_query_rays) -------------------------------------------------------------------------------------
def test_arbitrary_and_degenerate_rays_on_a_mesh_free_list(native, oracle_mod, abi):
    """A list without a mesh is walked by the mesh-free instantiation: the quad's short division behind its ballot, the cube's short reciprocals,
    the carried object-space point, the shared finish_hit tail -- shortcuts whose range arguments (rt_intersect.h) were written for the render
    kernels' own rays.  Here the caller's rays go through them: un-normalised, huge, tiny, NaN and infinite, on sphere, plane, quad and cube
    with coincident copies of each."""
    host, device = native
    sc = scene("fourkinds", abi, host)
    assert sc.c.n_meshes == 0 and {sc.c.primitives[i].kind for i in range(sc.c.n_primitives)} == {abi.PRIM_SPHERE, abi.PRIM_PLANE, abi.PRIM_QUAD, abi.PRIM_CUBE}
    o, d = kinds_rays()
    want = oracle_hits("fourkinds", oracle_mod, abi, sc, o, d)
    hit = want["primitive"] != abi.NO_HIT
    wins = np.bincount(np.array([sc.c.primitives[int(p)].kind for p in want["primitive"][hit]]), minlength=5)
    print("misses", int((~hit).sum()), "wins per kind", wins.tolist(), "front", int(want["front_face"][hit].sum()), "back", int((want["front_face"][hit] == 0).sum()))
    assert (wins[:4] >= 20).all() and wins[4] == 0 and (~hit).sum() >= 200, (wins, (~hit).sum())
    assert (want["front_face"][hit] == 1).any() and (want["front_face"][hit] == 0).any()
    od, dd = degenerate_rays()
    want_d = oracle_hits("fourkinds degenerate", oracle_mod, abi, sc, od, dd)
    ctx = context_for(device, abi, sc)
    try:
        assert ctx.kernel_variant() in (0, 3, 9, 11, 14)                  # a mesh-free render variant: set_scene saw no mesh, the queries take the mesh-free form
        got = trace(device, abi, ctx, o, d)
        got_d = trace(device, abi, ctx, od, dd)
        for n in (1, 63, 64, 65):
            assert trace(device, abi, ctx, o[:n], d[:n]).tobytes() == got[:n].tobytes(), n
    finally:
        ctx.close()
    for i in range(len(od)):
        print(i, od[i].tolist(), dd[i].tolist(), "oracle", want_d[i], "device", got_d[i])
    assert_records(got, want, "2085 rays, mesh-free list")
    assert_records(got_d, want_d, "24 degenerate rays, mesh-free list")
    rays = np.zeros(len(o), abi.RAY_DTYPE)
    rays["origin"], rays["direction"] = o, d
    assert device.trace_rays(sc, rays).tobytes() == got.tobytes()         # the one-shot on the same list


# ---- 5: plumbing ------------------------------------------------------------------------------------------------------------------------
def test_one_shot_repeats_and_a_query_beside_a_render(native, oracle_mod, abi):
    import torch
    host, device = native
    sc = scene("kinds", abi, host)
    o, d = kinds_rays()
    W, H = 96, 64
    ctx = context_for(device, abi, sc, W, H, spp=32, depth=8)
    try:
        alone = trace(device, abi, ctx, o, d)
        assert trace(device, abi, ctx, o, d).tobytes() == alone.tobytes()             # twice on one context, nothing uploaded in between
        rays = np.zeros(len(o), abi.RAY_DTYPE)
        rays["origin"], rays["direction"] = o, d
        assert device.trace_rays(sc, rays).tobytes() == alone.tobytes()               # the one-shot: host buffers, a context of its own
        r8 = np.zeros((len(o), 8), F); r8[:, 0:3], r8[:, 4:7] = o, d
        assert device.trace_rays(sc, r8[:100]).tobytes() == alone[:100].tobytes()
        assert len(device.trace_rays(sc, rays[:0])) == 0
        # a query on its own stream while a render of the same context runs on another
        s_render, s_query = torch.cuda.Stream(), torch.cuda.Stream()
        packed = torch.zeros((H, W), dtype=torch.int32, device="cuda")
        want_packed = torch.zeros((H, W), dtype=torch.int32, device="cuda")
        ctx.render(want_packed.data_ptr())
        d_rays, d_hits, d_px = to_device_rays(abi, o, d), hit_buffer(len(o)), hit_buffer(W * H)
        torch.cuda.synchronize()
        ctx.render(packed.data_ptr(), None, None, s_render.cuda_stream)
        ctx.trace_rays(d_rays.data_ptr(), len(o), d_hits.ptr, s_query.cuda_stream)
        ctx.first_hits(d_px.ptr, None, s_query.cuda_stream)
        ctx.render(packed.data_ptr(), None, None, s_render.cuda_stream)
        torch.cuda.synchronize()
        ctx.check()
        assert read_hits(abi, d_hits).tobytes() == alone.tobytes()
        assert read_hits(abi, d_px).tobytes() == first_hits(device, abi, ctx, W * H).tobytes()
        assert torch.equal(packed, want_packed)
        # refusals: nothing is launched, nothing is written
        L = device.lib()
        fresh = hit_buffer(4)
        torch.cuda.synchronize()
        with pytest.raises(device.RenderError) as e:
            ctx.first_hits(fresh.ptr, abi.Options.make(flags=abi.FLAG_FIXED_AABB))
        assert e.value.rc == abi.ERR_UNSUPPORTED
        for call in (lambda: ctx.first_hits(fresh.ptr + 4), lambda: ctx.first_hits(0), lambda: ctx.first_hits(fresh.ptr, abi.Options.make(flags=2)),
                     lambda: ctx.first_hits(fresh.ptr, abi.Options.make(n_parts=2, part=2)),
                     lambda: ctx.first_hits(fresh.ptr, abi.Options(3, 0, 0, 0, 0, 1, 1, 0, 0, 0)),
                     lambda: ctx.trace_rays(d_rays.data_ptr() + 8, 2, fresh.ptr), lambda: ctx.trace_rays(d_rays.data_ptr(), 2, fresh.ptr + 4),
                     lambda: ctx.trace_rays(0, 2, fresh.ptr), lambda: ctx.trace_rays(d_rays.data_ptr(), 2, 0)):
            with pytest.raises(device.RenderError) as e:
                call()
            assert e.value.rc == abi.ERR_INVALID
        ctx.trace_rays(0, 0, 0)                                                        # n_rays == 0: a no-op
        torch.cuda.synchronize()
        assert fresh.untouched()
        assert L.mi355rt_context_check(ctx._h) == 0
        empty = device.Context(0)                                                      # a context without a scene
        try:
            with pytest.raises(device.RenderError) as e:
                empty.trace_rays(d_rays.data_ptr(), 2, fresh.ptr)
            assert e.value.rc == abi.ERR_INVALID
        finally:
            empty.close()
    finally:
        ctx.close()
