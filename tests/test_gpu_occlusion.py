"""The occlusion queries on the GPU (mi355rt_context_occluded, mi355rt_occluded, mi355rt_context_ambient_occlusion) against tests/occlusion_ref.py:
every word and every float bit for bit.

Segments: the rule out = (hit && t < t_max) on the oracle's closest hit, with t_max placed AT the oracle's t, one step above it, at half and
twice of it, at +inf, NaN, 0, -1 and EPSILON -- on the five-kind fuzz scene with coincident copies, on the mesh-free list, on degenerate rays
and in a deep tree.  The trap scene separates an exact early exit from one that stops inside a mesh's tree.  Ambient occlusion: the kernel's
rays are restated in numpy float32 (pcg4d in uint32) and answered by the oracle, one call per (pixel, sample) shared by the cases."""
import numpy as np
import pytest

import occlusion_ref as R
import test_gpu_ray_queries as Q
from conftest import load_for_both
from device_buffers import Guarded

pytestmark = pytest.mark.gpu

F = np.float32
U = np.uint32
EPS = F(1e-4)


# ---- device plumbing ------------------------------------------------------------------------------------------------------------------
def segments_of(abi, origins, dirs, t_max):
    s = np.zeros(len(origins), abi.SEGMENT_DTYPE)
    s["origin"], s["direction"], s["t_max"] = origins, dirs, t_max
    s["_pad0"] = F(np.nan)                                              # ignored
    return s


def run_occluded(ctx, seg, n=None, stream=None):
    import torch
    n = len(seg) if n is None else n
    d_seg = torch.from_numpy(np.ascontiguousarray(seg).view(F).reshape(-1, 8).copy()).cuda()
    d_out = Guarded(n * 4, guard=8 * 4)
    torch.cuda.synchronize()
    ctx.occluded(d_seg.data_ptr(), n, d_out.ptr, stream)
    torch.cuda.synchronize()
    out = d_out.read(U, "occluded: the words")
    assert np.isin(out, (0, 1)).all(), "a word was not written (or is neither 0 nor 1)"
    return out


def variants(want):
    """(ray index, t_max) pairs: hits get {t, nextafter(t), t / 2, 2 t, +inf, NaN, 0, -1, EPSILON}, misses {1, +inf, NaN}; and the rule's answers."""
    idx, tm = [], []
    for i, h in enumerate(want):
        if h["primitive"] != R.NO_HIT:
            t = F(h["t"])
            with np.errstate(over="ignore", invalid="ignore"):
                vs = [t, np.nextafter(t, F(np.inf)), F(0.5) * t, F(2.0) * t, F(np.inf), F(np.nan), F(0.0), F(-1.0), EPS]
        else:
            vs = [F(1.0), F(np.inf), F(np.nan)]
        idx += [i] * len(vs); tm += vs
    idx, tm = np.array(idx), np.array(tm, F)
    expect = R.occluded_from_t(want["primitive"][idx] != R.NO_HIT, want["t"][idx], tm)
    return idx, tm, expect


def check_segments(abi, ctx, want, o, d, what, sizes=()):
    idx, tm, expect = variants(want)
    seg = segments_of(abi, o[idx], d[idx], tm)
    got = run_occluded(ctx, seg)
    bad = np.flatnonzero(got != expect)
    assert not len(bad), f"{what}: {len(bad)} of {len(got)} words differ, first ray {idx[bad[0]]} t_max {tm[bad[0]]!r} oracle {want[idx[bad[0]]]} got {got[bad[0]]}"
    hit = want["primitive"] != abi.NO_HIT
    ordered = hit & ~np.isnan(want["t"])
    first = np.flatnonzero(np.r_[True, idx[1:] != idx[:-1]])            # the first variant of every ray
    at_t, above_t = got[first[ordered]], got[first[ordered] + 1]
    assert (at_t == 0).all() and (above_t == 1).all(), f"{what}: t_max = t must give 0 and nextafter(t) 1"
    print(what, "segments", len(seg), "ones", int(got.sum()), "rays", len(want), "hits", int(hit.sum()), "NaN t", int((hit & ~ordered).sum()))
    for n in sizes:
        assert run_occluded(ctx, seg[:n]).tobytes() == got[:n].tobytes(), (what, n)
    return seg, got


# ---- 1: segments on every kind, the mesh-free list, degenerate rays, a deep tree ----------------------------------------------------------
def test_segments_on_every_primitive_kind(native, oracle_mod, abi):
    host, device = native
    sc = Q.scene("kinds", abi, host)
    o, d = Q.kinds_rays()
    want = Q.oracle_hits("kinds", oracle_mod, abi, sc, o, d)
    od, dd = Q.degenerate_rays()
    want_d = Q.oracle_hits("degenerate", oracle_mod, abi, sc, od, dd)
    ctx = Q.context_for(device, abi, sc)
    try:
        check_segments(abi, ctx, want, o, d, "2085 rays, five kinds", sizes=(1, 63, 64, 65))
        check_segments(abi, ctx, want_d, od, dd, "24 degenerate rays, five kinds")
    finally:
        ctx.close()


def test_segments_on_a_mesh_free_list(native, oracle_mod, abi):
    host, device = native
    sc = Q.scene("fourkinds", abi, host)
    assert sc.c.n_meshes == 0
    o, d = Q.kinds_rays()
    want = Q.oracle_hits("fourkinds", oracle_mod, abi, sc, o, d)
    od, dd = Q.degenerate_rays()
    want_d = Q.oracle_hits("fourkinds degenerate", oracle_mod, abi, sc, od, dd)
    ctx = Q.context_for(device, abi, sc)
    try:
        seg, got = check_segments(abi, ctx, want, o, d, "2085 rays, mesh-free list", sizes=(1, 63, 64, 65))
        check_segments(abi, ctx, want_d, od, dd, "24 degenerate rays, mesh-free list")
        assert device.occluded(sc, seg).tobytes() == got.tobytes()                            # the one-shot on the same list
    finally:
        ctx.close()


def test_segments_in_a_deep_tree(native, oracle_mod, abi):
    host, device = native
    sc = Q.scene("deep", abi, host)
    o, d = Q.deep_rays(sc)
    want = Q.oracle_hits("deep", oracle_mod, abi, sc, o, d)
    big = sc.c.n_primitives - 1
    assert sc.c.meshes[sc.c.primitives[big].mesh].node_count > 2000 and int((want["primitive"] == big).sum()) >= 100
    ctx = Q.context_for(device, abi, sc, 32, 24)
    try:
        check_segments(abi, ctx, want, o, d, "512 rays at the big mesh")
    finally:
        ctx.close()


def test_an_unordered_candidate_late_in_the_list_keeps_the_rule(native, oracle_mod, abi):
    """A plane in front, then a sphere whose discriminant overflows to inf - inf for a ray from far away: the reference accepts that NaN candidate
    (sphere.rs's negated comparisons), the closest t ends as NaN and the answer is 0 -- although the plane had left a candidate below t_max.
    Such rays lie outside the bound inside which the kernel leaves the list early (mi355rt.h), so they walk it to its end."""
    host, device = native
    from oracle import scene_loader as L
    sc = L.LoadedScene()
    m = abi.Material(); m.kind = abi.MAT_LAMBERT_SOLID; m.albedo[:] = [0.5, 0.5, 0.5]
    plane = abi.Primitive(); plane.kind = abi.PRIM_PLANE; plane.data[0:6] = [0.0, 0.0, 0.0, 0.0, 0.0, 1.0]
    sphere = abi.Primitive(); sphere.kind = abi.PRIM_SPHERE; sphere.data[0:4] = [0.0, 0.0, -5.0, 1.0]
    sc.materials, sc.primitives = [m], [plane, sphere]
    sc.finalize()
    sc._keep = host.attach_bvh(sc)
    sc.camera = L.camera_new((0.0, 1.0, 9.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), F(50.0), F(4.0 / 3.0))
    Q.own_materials(abi, sc)
    o = np.array([[0.0, 0.0, 1e20], [0.0, 0.0, 10.0], [0.3, 0.2, 1e20], [0.0, 0.0, 3e4]], F)
    d = np.array([[0.0, 0.0, -1.0]] * 4, F)
    want = Q.oracle_hits("nan tail", oracle_mod, abi, sc, o, d)
    print(want)
    assert np.isnan(want["t"][0]) and want["primitive"][0] == 1 and want["t"][1] == 10.0 and want["primitive"][1] == 0
    ctx = Q.context_for(device, abi, sc, 8, 8)
    try:
        check_segments(abi, ctx, want, o, d, "a NaN candidate behind an ordered one")
        # whole waves of the first ray with t_max = +inf: every lane holds the plane's candidate below t_max after the first primitive
        n = 130
        got = run_occluded(ctx, segments_of(abi, np.tile(o[0], (n, 1)), np.tile(d[0], (n, 1)), F(np.inf)))
        assert not got.any(), "the closest t is NaN: not below +inf"
        got = run_occluded(ctx, segments_of(abi, np.tile(o[3], (n, 1)), np.tile(d[3], (n, 1)), F(np.inf)))
        assert got.all()                                                                       # inside the bound: the wave may leave after the plane
    finally:
        ctx.close()


# ---- 2: the trap scene --------------------------------------------------------------------------------------------------------------------
TRAP_X, TRAP_Y = (-0.2137, -0.0291, 0.0173, 0.2219, 0.4561), (-0.1234, 0.0312, 0.1456)     # sheet A only, both, both, sheet B only, neither


def trap_scene(abi, host, scale, b_first):
    """A mesh of two tilted sheets of six triangles each -- A around z = 0 over x in [-0.3, 0.1], B around z = 0.2 over x in [-0.1, 0.3] -- under an
    object_to_world that scales by `scale`, then a plane far behind it on either side."""
    from oracle import scene_loader as L
    tilt = lambda x, z0: z0 + 0.02 * x

    def sheet(x0, z0):
        v = []
        for k in range(3):
            xa, xb = x0 + 0.4 * k / 3, x0 + 0.4 * (k + 1) / 3
            p = [(xa, -0.2, tilt(xa, z0)), (xb, -0.2, tilt(xb, z0)), (xb, 0.2, tilt(xb, z0)), (xa, 0.2, tilt(xa, z0))]
            v += [p[0], p[1], p[2], p[0], p[2], p[3]]
        return v
    a, b = sheet(-0.3, 0.0), sheet(-0.1, 0.2)
    verts = np.array((b + a) if b_first else (a + b), F)
    tris = L._triangles_from_indexed(verts, np.arange(len(verts)).reshape(-1, 3))
    sc = L.LoadedScene()
    m = abi.Material(); m.kind = abi.MAT_LAMBERT_SOLID; m.albedo[:] = [0.5, 0.5, 0.5]
    mat = L.mat4_from_scale_rotation_translation([F(scale)] * 3, L.quat_from_euler_yxz_deg(F(0), F(0), F(0)), [F(0)] * 3)
    mp = abi.Primitive(); mp.kind = abi.PRIM_MESH; mp.mesh = 0
    mp.data[0:16] = [float(v) for v in mat]; mp.data[16:32] = [float(v) for v in L.mat4_inverse(mat)]
    mesh = abi.Mesh(); mesh.first_triangle, mesh.triangle_count = 0, len(tris)
    planes = []
    for z in (5000.0, -5000.0):
        p = abi.Primitive(); p.kind = abi.PRIM_PLANE; p.data[0:6] = [0.0, 0.0, z, 0.0, 0.0, 1.0]
        planes.append(p)
    sc.materials, sc.primitives, sc.meshes, sc.triangles = [m], [mp] + planes, [mesh], tris
    sc.finalize()
    sc._keep = host.attach_bvh(sc)
    sc.camera = L.camera_new((0.0, 1.0, 9.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), F(50.0), F(4.0 / 3.0))
    return Q.own_materials(abi, sc)


def trap_rays(scale):
    o, d = [], []
    for side, z0, dz in (("below", -0.05, 1.0), ("above", 0.25, -1.0)):
        for x in TRAP_X:
            for y in TRAP_Y:
                o.append((x * scale, y * scale, z0 * scale)); d.append((0.0, 0.0, dz))
    return np.array(o, F), np.array(d, F)


@pytest.mark.parametrize("b_first", [False, True])
def test_the_trap_scene(b_first, native, oracle_mod, abi):
    host, device = native
    for scale, t_max in ((1000.0, 1.0), (1e-3, 1000.0)):
        sc = trap_scene(abi, host, scale, b_first)
        o, d = trap_rays(scale)
        want = Q.oracle_hits(("trap", scale, b_first), oracle_mod, abi, sc, o, d)
        expect = R.occluded_from_t(want["primitive"] != abi.NO_HIT, want["t"], F(t_max)).reshape(2, len(TRAP_X), len(TRAP_Y))
        prim = want["primitive"].reshape(2, len(TRAP_X), len(TRAP_Y))
        t = want["t"].reshape(2, len(TRAP_X), len(TRAP_Y))
        print("scale", scale, "B first", b_first, "\nprimitive", prim.tolist(), "\nt", t.tolist())
        # on the CPU first: the oracle's answers are what the scene was built for (column: A only, both, both, B only, neither)
        if scale == 1000.0:
            # t_world = t_obj / 1000: the nearer sheet lies below EPSILON and, being the final best, rejects the whole mesh
            assert expect[0].tolist() == [[0] * 3, [0] * 3, [0] * 3, [1] * 3, [0] * 3]         # from below A is the nearer sheet: only "B only" is a mesh hit
            assert expect[1].tolist() == [[1] * 3, [0] * 3, [0] * 3, [0] * 3, [0] * 3]         # from above B is
            mesh_hit = prim == 0
            assert (mesh_hit == (expect == 1)).all() and (t[mesh_hit] > 2e-4).all() and (t[mesh_hit] < 3e-4).all()
            assert (t[~mesh_hit] > 4000).all() and ((prim[~mesh_hit] == 1) | (prim[~mesh_hit] == 2)).all()      # the plane behind, far above t_max
        else:
            # the counter-case, t_world = t_obj * 1000: both sheets lie above EPSILON and every ray through a sheet is occluded
            assert expect[0].tolist() == expect[1].tolist() == [[1] * 3] * 4 + [[0] * 3]
            assert (prim[:, :4] == 0).all() and (t[:, :4] > 40).all() and (t[:, :4] < 260).all()
        ctx = Q.context_for(device, abi, sc, 8, 8)
        try:
            got = run_occluded(ctx, segments_of(abi, o, d, F(t_max)))
            assert got.tolist() == expect.reshape(-1).tolist(), (scale, b_first)
            check_segments(abi, ctx, want, o, d, f"trap scene x{scale}")
        finally:
            ctx.close()


# ---- 3: ambient occlusion -------------------------------------------------------------------------------------------------------------------
def run_ao(device, abi, ctx, W, H, params, options=None, stream=None):
    """first_hits and ambient_occlusion for the same options -> (hit records, float32 [rows * W]); guard floats behind the output stay untouched."""
    import torch
    rows = abi.rows_selected(H, options)
    n = len(rows) * W
    d_hits, d_out = Q.hit_buffer(n), Guarded(n * 4, guard=8 * 4)
    torch.cuda.synchronize()
    ctx.first_hits(d_hits.ptr, options, stream)
    ctx.ambient_occlusion(d_hits.ptr, d_out.ptr, params, options, stream)
    torch.cuda.synchronize()
    return Q.read_hits(abi, d_hits), d_out.read(F, "ambient_occlusion: the floats"), rows


def assert_ao(got, want, what):
    bad = np.flatnonzero(got.view(U) != want.view(U))
    assert not len(bad), f"{what}: {len(bad)} of {len(got)} floats differ, first at {bad[0]}: got {got[bad[0]]!r} want {want[bad[0]]!r}"


_refs = {}
_calls = {"total": 0}


def reference(oracle_mod, name, sc):
    if name not in _refs:
        _refs[name] = R.AoReference(oracle_mod, sc)
    return _refs[name]


def check_ao(device, abi, ref, ctx, W, H, cases, options=None, what=""):
    hits = None
    for samples, seed, radius in cases:
        before = ref.calls
        h, got, rows = run_ao(device, abi, ctx, W, H, abi.AoParams.make(samples, seed, radius), options)
        if hits is not None:
            assert h.tobytes() == hits.tobytes()
        hits = h
        want = ref.ao(h, W, rows, samples, seed, radius)
        _calls["total"] += ref.calls - before
        n_hit = int((h["primitive"] != abi.NO_HIT).sum())
        print(what, "samples", samples, "seed", seed, "radius", radius, "pixels", len(h), "hits", n_hit, "mean", float(got.mean()), "distinct", len(np.unique(got)),
              "oracle calls so far", _calls["total"])
        assert_ao(got, want, f"{what} samples {samples} seed {seed} radius {radius}")
        assert (got[h["primitive"] == abi.NO_HIT].view(U) == F(1.0).view(U)).all()
    return hits


def test_ambient_occlusion_on_every_primitive_kind(native, oracle_mod, abi):
    host, device = native
    sc = Q.scene("kinds", abi, host)
    W, H = 16, 12
    ref = reference(oracle_mod, "kinds", sc)
    ctx = Q.context_for(device, abi, sc, W, H)
    other = device.Context(0)
    try:
        hits = check_ao(device, abi, ref, ctx, W, H, [(64, 1, np.inf), (64, 1, 0.25), (1, 1, np.inf), (4, 1, 0.25), (4, 2, np.inf)], what="five kinds 16x12")
        assert (hits["primitive"] != abi.NO_HIT).sum() >= 64
        # the other way of dealing (pixel, sample) pairs to lanes gives the same bits (diagnostic knob; the product ships one form)
        other.set_knob("ao_form", 1)
        other.set_scene(sc, sc.camera, abi.Settings(W, H, 1, 1))
        check_ao(device, abi, ref, other, W, H, [(64, 1, 0.25), (4, 2, np.inf)], what="five kinds 16x12, a pixel per lane")
    finally:
        ctx.close(); other.close()


def test_ambient_occlusion_with_a_row_selection(native, oracle_mod, abi):
    host, device = native
    W, H = 33, 9
    sc = load_for_both("cornell", oracle_mod, host, width=W, height=H, spp=1, max_depth=1)
    ref = reference(oracle_mod, "cornell 33x9", sc)
    opt = abi.Options.make(row_begin=2, row_end=8)
    assert abi.rows_selected(H, opt) == [2, 3, 4, 5, 6, 7]
    ctx = Q.context_for(device, abi, sc, W, H)
    try:
        hits = check_ao(device, abi, ref, ctx, W, H, [(4, 5, np.inf), (4, 5, 0.25), (1, 6, np.inf), (4, 6, 0.25)], opt, what="cornell 33x9 rows 2..8")
        assert len(hits) == 6 * W
        # the rows' ABSOLUTE y addresses the draws: the whole image's rows 2 .. 7 are the selection's
        whole_hits, whole, _ = run_ao(device, abi, ctx, W, H, abi.AoParams.make(4, 5, 0.25))
        _, some, _ = run_ao(device, abi, ctx, W, H, abi.AoParams.make(4, 5, 0.25), opt)
        assert whole.reshape(H, W)[2:8].tobytes() == some.tobytes()
    finally:
        ctx.close()


def test_ambient_occlusion_of_a_mostly_missing_view(native, oracle_mod, abi):
    host, device = native
    sc = Q.scene("meshfree", abi, host)
    W, H = 12, 8
    ref = reference(oracle_mod, "meshfree", sc)
    ctx = Q.context_for(device, abi, sc, W, H)
    try:
        hits = check_ao(device, abi, ref, ctx, W, H, [(256, 3, np.inf), (256, 3, 0.25), (64, 3, 0.25)], what="mesh-free 12x8")
        n_miss = int((hits["primitive"] == abi.NO_HIT).sum())
        assert W * H // 2 < n_miss < W * H - 4, n_miss
    finally:
        ctx.close()
    print("oracle calls of the ambient-occlusion tests so far", _calls["total"])
    assert _calls["total"] < 40000


# ---- 4: protocol ----------------------------------------------------------------------------------------------------------------------------
def test_repeats_a_call_beside_a_render_and_the_refusals(native, oracle_mod, abi):
    import torch
    host, device = native
    sc = Q.scene("kinds", abi, host)
    o, d = Q.kinds_rays()
    want = Q.oracle_hits("kinds", oracle_mod, abi, sc, o, d)
    idx, tm, expect = variants(want[:400])
    seg = segments_of(abi, o[idx], d[idx], tm)
    W, H = 96, 64
    ctx = Q.context_for(device, abi, sc, W, H, spp=32, depth=8)
    try:
        alone = run_occluded(ctx, seg)
        assert alone.tolist() == expect.tolist()
        assert run_occluded(ctx, seg).tobytes() == alone.tobytes()                            # twice on one context
        assert device.occluded(sc, seg).tobytes() == alone.tobytes()                          # the one-shot: host buffers, a context of its own
        assert device.occluded(sc, seg.view(F).reshape(-1, 8)[:100]).tobytes() == alone[:100].tobytes()
        assert len(device.occluded(sc, seg[:0])) == 0
        prm = abi.AoParams.make(4, 9, np.inf)
        opt = abi.Options.make(row_begin=8, row_end=24)
        _, ao_alone, rows = run_ao(device, abi, ctx, W, H, prm, opt)
        _, ao_again, _ = run_ao(device, abi, ctx, W, H, prm, opt)
        assert ao_again.tobytes() == ao_alone.tobytes() and 0.0 < ao_alone.mean() < 1.0
        # both calls on their own stream while a render of the same context runs on another
        s_render, s_query = torch.cuda.Stream(), torch.cuda.Stream()
        packed = torch.zeros((H, W), dtype=torch.int32, device="cuda")
        want_packed = torch.zeros((H, W), dtype=torch.int32, device="cuda")
        ctx.render(want_packed.data_ptr())
        d_seg = torch.from_numpy(seg.view(F).reshape(-1, 8).copy()).cuda()
        d_words = torch.full((len(seg) + 8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        d_hits = Q.hit_buffer(len(rows) * W)
        d_ao = torch.full((len(rows) * W + 8,), -7.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ctx.render(packed.data_ptr(), None, None, s_render.cuda_stream)
        ctx.occluded(d_seg.data_ptr(), len(seg), d_words.data_ptr(), s_query.cuda_stream)
        ctx.first_hits(d_hits.ptr, opt, s_query.cuda_stream)
        ctx.ambient_occlusion(d_hits.ptr, d_ao.data_ptr(), prm, opt, s_query.cuda_stream)
        ctx.render(packed.data_ptr(), None, None, s_render.cuda_stream)
        torch.cuda.synchronize()
        ctx.check()
        words, ao = d_words.cpu().numpy(), d_ao.cpu().numpy()
        assert words[:len(seg)].astype(U).tobytes() == alone.tobytes() and (words[len(seg):] == 0x5A5A5A5A).all()
        assert ao[:len(rows) * W].tobytes() == ao_alone.tobytes() and (ao[len(rows) * W:] == -7.0).all()
        assert torch.equal(packed, want_packed)
        # refusals on a live context: nothing is launched, nothing is written
        fresh = torch.full((64,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        p, hp = fresh.data_ptr(), d_hits.ptr
        with pytest.raises(device.RenderError) as e:
            ctx.ambient_occlusion(hp, p, prm, abi.Options.make(flags=abi.FLAG_FIXED_AABB))
        assert e.value.rc == abi.ERR_UNSUPPORTED
        refused = [lambda: ctx.occluded(d_seg.data_ptr() + 8, 2, p), lambda: ctx.occluded(d_seg.data_ptr(), 2, p + 2), lambda: ctx.occluded(0, 2, p),
                   lambda: ctx.occluded(d_seg.data_ptr(), 2, 0),
                   lambda: ctx.ambient_occlusion(hp + 4, p, prm, opt), lambda: ctx.ambient_occlusion(hp, p + 1, prm, opt), lambda: ctx.ambient_occlusion(0, p, prm, opt),
                   lambda: ctx.ambient_occlusion(hp, 0, prm, opt), lambda: ctx.ambient_occlusion(hp, p, prm, abi.Options.make(flags=2)),
                   lambda: ctx.ambient_occlusion(hp, p, prm, abi.Options.make(n_parts=2, part=2)), lambda: ctx.ambient_occlusion(hp, p, prm, abi.Options.make(row_begin=9, row_end=3)),
                   lambda: ctx.ambient_occlusion(hp, p, prm, abi.Options.make(row_end=H + 1)), lambda: ctx.ambient_occlusion(hp, p, prm, abi.Options(3, 0, 0, 0, 0, 1, 1, 0, 0, 0)),
                   lambda: ctx.ambient_occlusion(hp, p, abi.AoParams(3, 0, 1.0, 0), opt), lambda: ctx.ambient_occlusion(hp, p, abi.AoParams(512, 0, 1.0, 0), opt),
                   lambda: ctx.ambient_occlusion(hp, p, abi.AoParams(16, 0, float("nan"), 0), opt), lambda: ctx.ambient_occlusion(hp, p, abi.AoParams(16, 0, 0.0, 0), opt),
                   lambda: ctx.ambient_occlusion(hp, p, abi.AoParams(16, 0, 1.0, 5), opt)]
        for k, call in enumerate(refused):
            with pytest.raises(device.RenderError) as e:
                call()
            assert e.value.rc == abi.ERR_INVALID, k
        ctx.occluded(0, 0, 0)                                                                  # n == 0: a no-op
        ctx.ambient_occlusion(0, 0, prm, abi.Options.make(row_begin=5, row_end=5))             # an empty selection: a no-op
        torch.cuda.synchronize()
        assert (fresh.cpu().numpy() == 0x5A5A5A5A).all()
        assert device.lib().mi355rt_context_check(ctx._h) == 0
        empty = device.Context(0)                                                              # a context without a scene
        try:
            for call in (lambda: empty.occluded(d_seg.data_ptr(), 2, p), lambda: empty.ambient_occlusion(hp, p, prm)):
                with pytest.raises(device.RenderError) as e:
                    call()
                assert e.value.rc == abi.ERR_INVALID
        finally:
            empty.close()
    finally:
        ctx.close()
