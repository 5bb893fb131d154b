"""Known-answer tests for the BSDFs and primitives the reference-held golden image does not exercise:
Plastic, checker, Metal (fuzz 0 and > 0), Dielectric (both faces, TIR), Beckmann / GGX, sphere (outside / inside /
tangent), quad (edges, back face, parallel ray), plane (both faces, |denom| at EPS), cube (zero direction components, an origin
on a slab plane, the 1e-4 face band at edges and corners, a thin cube), triangles in meshes (u = 0, v = 0, u + v = 1, |a| at EPS,
duplicates, a scaled and rotated mesh) and coincident primitives of every kind, whose list order picks the material.  The expected
values come from tests/kat_f32.py -- numpy float32 written from the Rust formulas -- and must equal the oracle's per-function hooks
bit for bit (transcendental BSDFs: a few ulps).  The gpu twin runs the same cases through the device code (k_debug_scatter / k_debug_hit behind the C ABI
library's diagnostic hooks).
"""
import ctypes as C

import numpy as np
import pytest

import kat_f32 as K
from conftest import pkg

f32 = np.float32


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def material(abi, kind, albedo=(0, 0, 0), aux=(0, 0, 0), p0=0.0, eta=(0, 0, 0), k=(0, 0, 0)):
    m = abi.Material()
    m.kind = kind
    m.albedo[:] = albedo; m.aux[:] = aux; m.p0 = p0; m.eta[:] = eta; m.k[:] = k
    return m


def unit(v):
    return K.normalized(K.V(*v))


def scatter_cases(abi):
    """(name, abi.Material, expected-fn(rd, p, n, front, draws), transcendental?)"""
    cu_eta, cu_k = (0.200, 1.090, 1.420), (3.910, 2.570, 2.300)          # MetalType::Cu, tungsten/materials.rs:118-121
    al = lambda c: K.V(*c)
    return [
        ("lambert", material(abi, abi.MAT_LAMBERT_SOLID, (0.7, 0.6, 0.5)),
         lambda rd, p, n, ff, d: K.scatter_lambert(al((0.7, 0.6, 0.5)), rd, p, n, d), False),
        ("checker", material(abi, abi.MAT_LAMBERT_CHECKER, (0.9, 0.8, 0.1), (0.1, 0.2, 0.3), 1.0 / 0.37),
         lambda rd, p, n, ff, d: K.scatter_lambert(K.checker_value(al((0.9, 0.8, 0.1)), al((0.1, 0.2, 0.3)), f32(1.0 / 0.37), p), rd, p, n, d), False),
        ("metal_mirror", material(abi, abi.MAT_METAL, (0.8, 0.8, 0.9), p0=0.0),
         lambda rd, p, n, ff, d: K.scatter_metal(al((0.8, 0.8, 0.9)), f32(0.0), rd, p, n, d), False),
        ("metal_fuzz", material(abi, abi.MAT_METAL, (0.8, 0.6, 0.2), p0=0.35),
         lambda rd, p, n, ff, d: K.scatter_metal(al((0.8, 0.6, 0.2)), f32(0.35), rd, p, n, d), False),
        ("glass", material(abi, abi.MAT_DIELECTRIC, p0=1.5),
         lambda rd, p, n, ff, d: K.scatter_dielectric(f32(1.5), ff, rd, p, n, d), False),
        ("plastic", material(abi, abi.MAT_PLASTIC, (0.2, 0.5, 0.9), p0=1.9),
         lambda rd, p, n, ff, d: K.scatter_plastic(al((0.2, 0.5, 0.9)), f32(1.9), rd, p, n, d), False),
        ("beckmann_cu", material(abi, abi.MAT_ROUGH_BECKMANN, (1, 1, 1), p0=0.1, eta=cu_eta, k=cu_k),
         lambda rd, p, n, ff, d: K.scatter_rough(al((1, 1, 1)), f32(0.1), al(cu_eta), al(cu_k), False, rd, p, n, d), True),
        ("ggx_cu", material(abi, abi.MAT_ROUGH_GGX, (0.9, 0.95, 1.0), p0=0.3, eta=cu_eta, k=cu_k),
         lambda rd, p, n, ff, d: K.scatter_rough(al((0.9, 0.95, 1.0)), f32(0.3), al(cu_eta), al(cu_k), True, rd, p, n, d), True),
    ]


def scatter_inputs():
    """(rd, p, n, front_face, counters): incidence from normal to grazing, both faces, negative checker cells, axis-aligned and
    oblique normals (to_world's two `up` choices)."""
    rng = np.random.default_rng(7)
    out = []
    normals = [unit((0, 1, 0)), unit((0, 0, 1)), unit((0.3, -0.8, 0.52)), unit((-1, 0.02, 0.01))]
    for i in range(40):
        n = normals[i % len(normals)]
        # a direction against the normal (the hit record's normal always faces the ray), from steep to grazing
        t = K.normalized(K.cross(n, K.V(0.37, 0.61, -0.7)))
        graze = f32([0.02, 0.3, 0.7, 0.95, 0.999][i % 5])
        rd = K.normalized(t * graze - n * f32(np.sqrt(max(0.0, 1.0 - float(graze) ** 2))))
        p = K.V(*(rng.uniform(-3, 3, 3)))
        ctr = tuple(int(v) for v in rng.integers(0, 2 ** 32, 2)) + (int(rng.integers(0, 800)), int(rng.integers(0, 256)), int(rng.integers(1, 30)))
        out.append((rd, p, n, (i % 3) != 0, ctr))
    return out


def hit_scene_for(abi, prims):
    sc = abi.Scene()
    arr = (abi.Primitive * len(prims))(*prims)
    mats = (abi.Material * 1)(material(abi, abi.MAT_LAMBERT_SOLID, (0.5, 0.5, 0.5)))
    sc.primitives, sc.n_primitives, sc.materials, sc.n_materials = arr, len(prims), mats, 1
    sc.miss_color[:] = (0.5, 0.5, 0.5)
    sc._keep = (arr, mats)
    return sc


def sphere_prim(abi, c, r):
    p = abi.Primitive(); p.kind = abi.PRIM_SPHERE; p.material = 0
    p.data[0:4] = [c[0], c[1], c[2], r]
    return p


def quad_prim(abi, q):
    p = abi.Primitive(); p.kind = abi.PRIM_QUAD; p.material = 0
    p.data[0:15] = [*q["base"], *q["e0"], *q["e1"], *q["n"], q["d"], q["inv0"], q["inv1"]]
    return p


def list_scene_for(abi, prims, n_mats, meshes=()):
    """A scene of `prims` (list order) over n_mats Lambert materials (material i is index i: the winner is visible) and `meshes`:
    [(triangles [k, 12] f32)], each with ONE leaf over all its triangles in index order -- what bvh.rs:24-33 builds for k <= 4."""
    sc = abi.Scene()
    arr = (abi.Primitive * len(prims))(*prims)
    mats = (abi.Material * n_mats)(*[material(abi, abi.MAT_LAMBERT_SOLID, (0.5, 0.5, 0.5)) for _ in range(n_mats)])
    sc.primitives, sc.n_primitives, sc.materials, sc.n_materials = arr, len(prims), mats, n_mats
    sc.miss_color[:] = (0.5, 0.5, 0.5)
    keep = [arr, mats]
    if meshes:
        tri_rows = np.concatenate(meshes, axis=0).astype(np.float32)
        tris = (abi.Triangle * len(tri_rows))()
        C.memmove(tris, tri_rows.ctypes.data, tri_rows.nbytes)
        ms, nodes, idx, t0 = (abi.Mesh * len(meshes))(), (abi.BvhNode * len(meshes))(), [], 0
        for m, t in enumerate(meshes):
            assert len(t) <= 4
            v = t[:, 0:9].reshape(-1, 3)
            nodes[m].bmin[:] = [float(x) for x in v.min(0)]; nodes[m].bmax[:] = [float(x) for x in v.max(0)]
            nodes[m].first_index, nodes[m].index_count = 0, len(t)
            ms[m].first_triangle, ms[m].triangle_count, ms[m].first_node, ms[m].node_count = t0, len(t), m, 1
            ms[m].first_index, ms[m].index_count, ms[m].max_depth = len(idx), len(t), 0
            idx += list(range(len(t))); t0 += len(t)
        ic = (C.c_uint32 * len(idx))(*idx)
        sc.meshes, sc.n_meshes, sc.triangles, sc.n_triangles = ms, len(meshes), tris, len(tri_rows)
        sc.nodes, sc.n_nodes, sc.tri_indices, sc.n_tri_indices = nodes, len(meshes), ic, len(idx)
        keep += [tris, ms, nodes, ic]
    sc._keep = keep
    return sc


def plane_prim(abi, p1, n, mat=0):
    p = abi.Primitive(); p.kind = abi.PRIM_PLANE; p.material = mat
    p.data[0:6] = [*p1, *n]
    return p


def xform_prim(abi, kind, o2w, w2o, mat=0, mesh=0):
    p = abi.Primitive(); p.kind = kind; p.material = mat; p.mesh = mesh
    p.data[0:16] = [float(v) for v in o2w]; p.data[16:32] = [float(v) for v in w2o]
    return p


def trs(scale, euler_deg, trans):
    """(object_to_world, world_to_object) as the loader makes them (glam from_scale_rotation_translation, Mat4::inverse)."""
    from oracle import scene_loader as L
    o2w = L.mat4_from_scale_rotation_translation([f32(v) for v in scale], L.quat_from_euler_yxz_deg(*[f32(v) for v in euler_deg]), [f32(v) for v in trans])
    return np.asarray(o2w, np.float32), np.asarray(L.mat4_inverse(np.asarray(o2w, np.float32)), np.float32)


def triangles(*tris):
    """[(v0, v1, v2)] -> [k, 12] f32 rows with Triangle::new's normal (triangle.rs:14-18)."""
    out = []
    for v0, v1, v2 in tris:
        v0, v1, v2 = K.V(*v0), K.V(*v1), K.V(*v2)
        out.append(np.concatenate([v0, v1, v2, K.normalized(K.cross(v1 - v0, v2 - v0))]))
    return np.array(out, np.float32)


def around_eps(make_dir, dot_of):
    """Two directions make_dir(c): the last whose |dot_of(d)| lies below EPS and the first at or above it (bisection over c)."""
    lo, hi = 0.0, 1e-2
    assert abs(dot_of(make_dir(lo))) < K.EPS <= abs(dot_of(make_dir(hi)))
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        if abs(dot_of(make_dir(mid))) < K.EPS:
            lo = mid
        else:
            hi = mid
    return [make_dir(lo), make_dir(hi)]


def list_hit_cases(abi):
    """Plane, cube, triangle / mesh and coincident-primitive cases (ISSUE: known answers for plane, cube and mesh hits): each expected value
    is hit_list over the restated primitive tests of tests/kat_f32.py, the winner's material included."""
    inf = f32(np.inf)
    cases = []
    # ---- plane (plane.rs): both faces, |denom| just below / at EPS, the origin on the plane
    p1, pn = K.V(0.0, -1.0, 0.0), unit((0.2, 1.0, 0.1))
    tang = K.normalized(K.cross(pn, K.V(0.31, -0.52, 0.8)))
    rays_p = [(K.V(0.3, 2.0, 0.5), (0.1, -1.0, 0.2)), (K.V(0.3, -4.0, 0.5), (0.1, 1.0, -0.2)),          # front, back face
              (p1.copy(), (0.1, -1.0, 0.2)), (p1 + tang * f32(2.0), (0.3, 1.0, 0.0)), (K.V(0.0, 1.0, 0.0), (0.0, 1.0, 0.0))]   # origin on the plane, moving away
    for d in around_eps(lambda c: K.normalized(tang - pn * f32(c)), lambda d: K.dot(pn, K.normalized(d))):
        rays_p.append((K.V(0.2, 0.5, -0.3), tuple(float(v) for v in d)))
    cases.append(("plane", list_scene_for(abi, [plane_prim(abi, p1, pn)], 1), rays_p,
                  lambda o, d: K.hit_list([(0, lambda ro, rd, a, b: K.hit_plane(p1, pn, ro, rd, a, b))], o, d)))
    # ---- cube (cube.rs): axis-aligned and rotated, zero direction components, an origin on a slab plane, the 1e-4 band at edges / corners,
    # inside, just missing, a thin cube
    cubes = [("cube_axis_aligned", trs((2.0, 1.0, 1.5), (0, 0, 0), (0.0, 0.0, 3.0))), ("cube_unit", trs((1, 1, 1), (0, 0, 0), (0, 0, 0))),
             ("cube_rotated", trs((1.3, 0.7, 2.1), (23.0, -41.0, 67.0), (0.4, -0.3, 2.5))), ("cube_thin", trs((1.0, 1e-3, 1.0), (10.0, 0.0, -5.0), (0.0, 0.5, 2.0)))]
    for name, (o2w, w2o) in cubes:
        rays = [(K.V(0.1, 0.2, -5.0), (0.0, 0.0, 1.0)), (K.V(-6.0, 0.1, 3.1), (1.0, 0.0, 0.0)), (K.V(0.05, 7.0, 2.9), (0.0, -1.0, 0.0)),   # along the axes
                (K.V(0.2, 0.3, -4.0), (-0.04, 0.01, 1.0)), (K.V(0.0, 0.0, 2.0), (0.3, -0.2, 0.9)), (K.V(0.0, 0.45, 2.0), (0.0, 1.0, 0.0)),  # oblique, from inside
                (K.V(-3.0, -2.0, -1.0), (0.5, 0.35, 0.6)), (K.V(1.01, 0.0, -4.0), (0.0, 0.0, 1.0)), (K.V(0.0, 0.5001, -4.0), (0.0, 0.0, 1.0))]  # corner-ish, just missing
        cw = lambda x, y, z: K.mat4_vec4(o2w, x, y, z, 1.0)        # world point of an object-space point
        for po, dobj in [((-0.5, 0.1, 0.2), (0.0, 0.0, 1.0)), ((0.5, -0.5, 0.1), (0.0, 0.0, -1.0)),        # origin ON a slab plane with a zero component (0 * inf)
                         ((0.1, 3.0, 0.49995), (0.0, -1.0, 0.0)), ((0.49997, 3.0, 0.49996), (0.0, -1.0, 0.0)),  # y face inside the band of the z (and x) edge
                         ((3.0, 0.49993, -0.49998), (-1.0, 0.0, 0.0)), ((0.49996, 0.49996, -3.0), (0.0, 0.0, 1.0)),  # x face at the y-z band / a corner ray
                         ((0.3, -3.0, 0.49990), (0.0, 1.0, 0.0)), ((-3.0, 0.2, 0.5), (1.0, 0.0, 0.0))]:            # the band's far end, grazing the z = 0.5 face
            dw = K.mat4_vec4(o2w, dobj[0], dobj[1], dobj[2], 0.0)
            rays.append((cw(*po), tuple(float(v) for v in dw)))
        cases.append((name, list_scene_for(abi, [xform_prim(abi, abi.PRIM_CUBE, o2w, w2o)], 1), rays,
                      lambda o, d, o2w=o2w, w2o=w2o: K.hit_list([(0, lambda ro, rd, a, b: K.hit_cube(o2w, w2o, ro, rd, a, b))], o, d)))
    # ---- triangles (bvh.rs:99-116) through a mesh (mesh_object.rs:263-329): u = 0, v = 0, u + v = 1 exactly (the untransformed mesh
    # below has u = x and v = y for rays along +z), just outside, |a| around EPS, duplicates in one leaf (the first in leaf order wins)
    ident = np.eye(4, dtype=np.float32).reshape(16)
    tri = triangles(((0, 0, 2), (1, 0, 2), (0, 1, 2.5)))
    rays_t = [(K.V(x, y, -3.0), (0.0, 0.0, 1.0)) for x, y in ((0.0, 0.3), (0.4, 0.0), (0.25, 0.75), (0.5, 0.5), (0.0, 0.0), (1.0, 0.0), (0.0, 1.0),
                                                              (-1e-7, 0.3), (0.4, -1e-7), (0.25, 0.7500001), (0.3, 0.3))]
    e1, e2 = tri[0, 3:6] - tri[0, 0:3], tri[0, 6:9] - tri[0, 0:3]
    centroid = (tri[0, 0:3] + tri[0, 3:6] + tri[0, 6:9]) / f32(3)
    for d in around_eps(lambda c: K.normalized(K.normalized(e1 + e2) + tri[0, 9:12] * f32(c)), lambda d: K.dot(e1, K.cross(K.normalized(d), e2))):
        rays_t.append((centroid - d * f32(3.0), tuple(float(v) for v in d)))
    def mesh_hit(o2w, w2o, t):
        v = t[:, 0:9].reshape(-1, 3)
        node = [(v.min(0), v.max(0), 0, 0, 0, len(t))]
        return lambda ro, rd, a, b: K.hit_mesh(o2w, w2o, node, list(range(len(t))), t, ro, rd, a, b)
    cases.append(("triangle_edges", list_scene_for(abi, [xform_prim(abi, abi.PRIM_MESH, ident, ident)], 1, [tri]), rays_t,
                  lambda o, d: K.hit_list([(0, mesh_hit(ident, ident, tri))], o, d)))
    # a scaled, rotated mesh of three triangles; rays at their centroids, edges and vertices in world space
    o2w, w2o = trs((1.7, 0.6, 1.1), (35.0, 110.0, -20.0), (0.5, -0.2, 3.0))
    tm = triangles(((-0.8, -0.5, 0.1), (0.7, -0.4, -0.2), (0.0, 0.8, 0.3)), ((0.2, 0.1, -0.6), (0.9, 0.9, 0.4), (-0.3, 0.6, 0.7)),
                   ((-0.9, 0.7, -0.5), (-0.2, -0.9, 0.6), (0.5, 0.2, -0.9)))
    eye = K.V(0.3, 0.8, -4.0)
    rays_m = []
    for t in tm:
        v0, v1, v2 = t[0:3], t[3:6], t[6:9]
        for bary in ((1 / 3, 1 / 3), (0.0, 0.5), (0.5, 0.0), (0.5, 0.5), (0.0, 0.0), (0.2, 0.79)):
            pobj = v0 + (v1 - v0) * f32(bary[0]) + (v2 - v0) * f32(bary[1])
            rays_m.append((eye, tuple(float(x) for x in K.mat4_vec4(o2w, *pobj, 1.0) - eye)))
    cases.append(("mesh_rotated", list_scene_for(abi, [xform_prim(abi, abi.PRIM_MESH, o2w, w2o)], 1, [tm]), rays_m,
                  lambda o, d: K.hit_list([(0, mesh_hit(o2w, w2o, tm))], o, d)))
    # duplicate triangles in one leaf: the same triangle, its cyclic rotation and its reversed winding (front_face tells them apart)
    base = ((-0.6, -0.4, 0.2), (0.8, -0.3, -0.1), (0.1, 0.9, 0.4))
    td = triangles(base, base, (base[1], base[2], base[0]), (base[0], base[2], base[1]))
    tdr = triangles((base[0], base[2], base[1]), base, (base[1], base[2], base[0]))
    rays_d = [(eye, tuple(float(x) for x in K.mat4_vec4(o2w, *p, 1.0) - eye)) for p in ((0.1, 0.05, 0.15), (-0.3, -0.2, 0.15), (0.4, 0.1, 0.0), (0.05, 0.6, 0.3))]
    rays_d += [(K.V(0.1, 0.05, -3.0), (0.0, 0.0, 1.0)), (K.V(0.1, 0.05, 3.0), (0.0, 0.0, -1.0))]
    for name, t in (("mesh_duplicate_triangles", td), ("mesh_duplicate_triangles_reversed_first", tdr)):
        for m2w, w2m in ((ident, ident), (o2w, w2o)):
            cases.append((name, list_scene_for(abi, [xform_prim(abi, abi.PRIM_MESH, m2w, w2m)], 1, [t]), rays_d,
                          lambda o, d, m2w=m2w, w2m=w2m, t=t: K.hit_list([(0, mesh_hit(m2w, w2m, t))], o, d)))
    # ---- coincident primitives of every kind with different materials: repeated next to itself and again after another primitive;
    # the list walk keeps the FIRST of equal t (hittable.rs:45-58, t < t_max strict in sphere / plane / quad / triangle; cube and mesh
    # compare their world t non-strictly, so there the LATER copy wins -- whatever hit_list says is the answer)
    c0, r0 = K.V(0.2, -0.1, 1.5), f32(0.9)
    q = K.quad_from_corners(K.V(-1.0, -0.8, 1.0), K.V(2.0, 0.1, 0.3), K.V(-0.2, 1.5, 0.4))
    oc, wc = trs((1.2, 0.9, 1.4), (15.0, 30.0, 5.0), (0.1, 0.0, 2.0))
    pp1, ppn = K.V(0.0, 0.0, 2.5), unit((0.1, 0.2, -1.0))
    other = sphere_prim(abi, K.V(3.0, 3.0, 9.0), f32(0.5)); other.material = 3
    kinds = [("sphere", lambda m: _with_mat(sphere_prim(abi, c0, r0), m), lambda ro, rd, a, b: K.hit_sphere(c0, r0, ro, rd, a, b)),
             ("plane", lambda m: plane_prim(abi, pp1, ppn, m), lambda ro, rd, a, b: K.hit_plane(pp1, ppn, ro, rd, a, b)),
             ("quad", lambda m: _with_mat(quad_prim(abi, q), m), lambda ro, rd, a, b: K.hit_quad(q, ro, rd, a, b)),
             ("cube", lambda m: xform_prim(abi, abi.PRIM_CUBE, oc, wc, m), lambda ro, rd, a, b: K.hit_cube(oc, wc, ro, rd, a, b)),
             ("mesh", lambda m: xform_prim(abi, abi.PRIM_MESH, o2w, w2o, m), mesh_hit(o2w, w2o, tm))]
    rng = np.random.default_rng(5)
    rays_c = [(K.V(*rng.uniform(-0.4, 0.4, 3)) + K.V(0.0, 0.3, -5.0), tuple(float(v) for v in K.V(*rng.uniform(-0.12, 0.12, 3)) + K.V(0.0, 0.0, 1.0))) for _ in range(10)]
    rays_c += [(eye, tuple(float(x) for x in K.mat4_vec4(o2w, *(tm[0, 0:3] + tm[0, 3:6] + tm[0, 6:9]) / f32(3), 1.0) - eye))]
    for kname, make, fn in kinds:
        prims = [make(1), make(2), other, make(4)]
        meshes = [tm] if kname == "mesh" else []
        cases.append((f"coincident_{kname}", list_scene_for(abi, prims, 5, meshes), rays_c,
                      lambda o, d, fn=fn: K.hit_list([(1, fn), (2, fn), (3, lambda ro, rd, a, b: K.hit_sphere(K.V(3.0, 3.0, 9.0), f32(0.5), ro, rd, a, b)), (4, fn)], o, d)))
    return cases


def _with_mat(p, m):
    p.material = m
    return p


def hit_cases(abi):
    """(name, abi.Scene, rays[(o, d)], expected-fn(o, d_normalised)); the plane, cube, mesh and coincident-primitive cases follow
    (list_hit_cases), whose expected function also names the winning material."""
    c, r = K.V(0.25, -0.5, 2.0), f32(1.3)
    q = K.quad_from_corners(K.V(-1.0, 0.2, 3.0), K.V(2.0, 0.1, 0.3), K.V(-0.2, 1.5, 0.4))
    rays_s = [(K.V(0, 0, -5), (0.05, -0.1, 1)), (K.V(0, 0, -5), (0.25, -0.5, 7.0)), (K.V(0.25, -0.5, 2.0), (0.3, 0.2, -1)),      # outside, centre, from inside
              (K.V(0.3, -0.4, 2.2), (-1, 0.5, 0.2)), (K.V(1.55, -0.5, -4), (0, 0, 1)), (K.V(1.5501, -0.5, -4), (0, 0, 1)),           # inside, tangent, just missing
              (K.V(0, 0, 5), (0, 0, 1)), (K.V(5, 5, 5), (-1, -1.1, -0.6))]                                                           # behind, oblique
    rays_q = [(K.V(0, 1, -2), (0, 0, 1)), (K.V(0, 1, 8), (0, 0, -1)),                                  # front and back face
              (K.V(-1.0, 0.2, -2), (0, 0, 1)), (K.V(-1.00005, 0.2, -2), (0, 0, 1)), (K.V(-1.001, 0.2, -2), (0, 0, 1)),   # on the corner, inside the EPS rim, outside it
              (K.V(0, 1, -2), (2.0, 0.1, 0.3)), (K.V(0.9, 1.7, -2), (0.01, -0.02, 1)), (K.V(0, 1, 3.5), (0, 0, 1))]       # parallel to the plane, near the far edge, behind
    return [
        ("sphere", hit_scene_for(abi, [sphere_prim(abi, c, r)]), rays_s, lambda o, d: K.hit_sphere(c, r, o, d, K.EPS, f32(np.inf))),
        ("quad", hit_scene_for(abi, [quad_prim(abi, q)]), rays_q, lambda o, d: K.hit_quad(q, o, d, K.EPS, f32(np.inf))),
    ] + list_hit_cases(abi)


def texture_fixture(abi):
    """An 8 x 4 RGBA8 image with a distinct colour per texel + the material that samples it (h_offset 0.3)."""
    rgba = np.zeros((4, 8, 4), np.uint8)
    for y in range(4):
        for x in range(8):
            rgba[y, x] = (10 + 30 * x, 20 + 50 * y, 255 - 25 * x - 7 * y, 255)
    tex = abi.Texture(rgba.ctypes.data_as(C.POINTER(C.c_uint8)), 8, 4)
    textures = (abi.Texture * 1)(tex)
    mat = material(abi, abi.MAT_TEXTURE, (0.9, 0.8, 0.7), p0=0.3)
    mat.texture = 0
    return rgba, textures, mat


def texture_normals():
    """Unit normals whose equirect coordinates stay at least 2 % of a texel away from every texel border (acos / atan2 ulps
    cannot change the texel), over all octants and both poles."""
    rgba = np.zeros((4, 8, 4), np.uint8)
    rng = np.random.default_rng(11)
    out = []
    while len(out) < 48:
        n = K.normalized(K.V(*rng.normal(size=3)))
        _, (fx, fy) = K.texture_value(rgba, f32(0.3), n)
        if min(fx % 1, 1 - fx % 1, fy % 1, 1 - fy % 1) > 0.02:
            out.append(n)
    return out + [K.V(0, 1, 0), K.V(0, -1, 0)]


def check_scatter(name, want, got, transcendental):
    ok, o, d, a = want
    assert bool(got[0]) == ok, name
    if not ok:
        return
    if transcendental:                       # ln / atan / sin / cos differ by ulps between libms
        assert np.allclose(got[1:4], o, rtol=2e-6, atol=1e-6) and np.allclose(got[4:7], d, rtol=1e-5, atol=2e-6) and np.allclose(got[7:10], a, rtol=2e-4, atol=1e-6), name
    else:
        assert np.array_equal(_bits(got[1:4]), _bits(o)) and np.array_equal(_bits(got[4:7]), _bits(d)) and np.array_equal(_bits(got[7:10]), _bits(a)), \
            (name, got[1:10], o, d, a)


def check_hit(name, want, hit, out9):
    assert hit == (want is not None), (name, out9)
    if want is None:
        return
    if len(want) == 5:                                       # a list case: the material of the winner too
        assert int(out9[7]) == want[4], (name, "material", out9, want)
        want = want[:4]
    t, p, n, front = want
    assert np.array_equal(_bits(out9[0:3]), _bits(p)) and np.array_equal(_bits(out9[3:6]), _bits(n)) and _bits([out9[6]])[0] == _bits([t])[0], (name, out9, want)
    assert bool(out9[8]) == bool(front), name


def test_philox_and_float_conversions_of_the_independent_restatement(oracle_mod):
    for args in [(0, 0, 0, 0, 0, 0), (0xa4093822, 0x299f31d0, 0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (1, 2, 3, 4, 5, 6)]:
        assert K.philox(*args) == [int(v) for v in oracle_mod.philox(*args)]
        assert K.pcg4d(*args[:4]) == [int(v) for v in oracle_mod.pcg4d(*args[:4])]
        assert K.ctr_block(*args) == [int(v) for v in oracle_mod.ctr_block(*args, gen=2)] == [int(v) for v in oracle_mod.ctr_block(*args)]   # (2 = the generator in force)
    for w in [0, 1, 0xFF, 0x100, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 0x12345678]:
        assert _bits([K.u01(w)])[0] == _bits([oracle_mod.lib().oracle_u32_to_f01(w)])[0]
        assert _bits([K.range11(w)])[0] == _bits([oracle_mod.lib().oracle_u32_to_range11(w)])[0]


def test_oracle_scatter_equals_the_numpy_known_answers(oracle_mod, abi):
    L = oracle_mod.lib()
    n_checked = 0
    for name, mat, expect, transcendental in scatter_cases(abi):
        for rd, p, n, ff, ctr in scatter_inputs():
            want = expect(rd, p, n, ff, K.CtrDraws(*ctr))
            out = np.zeros(10, np.float32)
            o = np.zeros(3, np.float32)
            rc = L.oracle_scatter_ctr(C.byref(mat), o.ctypes.data, rd.ctypes.data, p.ctypes.data, n.ctypes.data, int(ff), *ctr, out.ctypes.data)
            assert rc == 0
            check_scatter(name, want, out, transcendental)
            n_checked += 1
    assert n_checked == 8 * 40


def test_oracle_texture_material_equals_the_numpy_known_answers(oracle_mod, abi):
    """TextureMaterial (parser.rs:199-243): Lambert bounce, attenuation = albedo * the texel the hit NORMAL selects."""
    rgba, textures, mat = texture_fixture(abi)
    L = oracle_mod.lib()
    L.oracle_set_textures.argtypes = [C.POINTER(abi.Texture), C.c_uint32]
    L.oracle_set_textures(textures, 1)
    try:
        seen = set()
        for i, n in enumerate(texture_normals()):
            rd, p, ctr = K.normalized(-n + K.V(0.1, 0.05, -0.02)), K.V(0.5, -1.0, 2.0), (7, 9, i, 3, 2)
            want = K.scatter_texture(K.V(0.9, 0.8, 0.7), rgba, f32(0.3), rd, p, n, K.CtrDraws(*ctr))
            out = np.zeros(10, np.float32)
            assert L.oracle_scatter_ctr(C.byref(mat), np.zeros(3, np.float32).ctypes.data, rd.ctypes.data, p.ctypes.data, n.ctypes.data, 1, *ctr, out.ctypes.data) == 0
            check_scatter("texture", want, out, False)
            seen.add(tuple(out[7:10]))
        assert len(seen) >= 20                                  # many different texels were reached
    finally:
        L.oracle_set_textures(None, 0)


def test_dielectric_total_internal_reflection_takes_no_draw(oracle_mod, abi):
    """Inside glass at a grazing angle: cannot_refract short-circuits the random draw (material.rs:145) and the ray reflects."""
    n = unit((0, 1, 0))
    rd = K.normalized(K.V(0.9, -0.2, 0.1))
    p = K.V(0.1, 0.2, 0.3)
    want = K.scatter_dielectric(f32(1.5), False, rd, p, n, K.CtrDraws(1, 2, 3, 4, 5))
    assert np.array_equal(_bits(want[2]), _bits(K.normalized(K.normalized(K.reflect(K.normalized(rd), n)))))
    out = np.zeros(10, np.float32)
    mat = material(abi, abi.MAT_DIELECTRIC, p0=1.5)
    oracle_mod.lib().oracle_scatter_ctr(C.byref(mat), np.zeros(3, np.float32).ctypes.data, rd.ctypes.data, p.ctypes.data, n.ctypes.data, 0, 1, 2, 3, 4, 5, out.ctypes.data)
    check_scatter("tir", want, out, False)


def test_oracle_primitive_hits_equal_the_numpy_known_answers(oracle_mod, abi):
    for name, sc, rays, expect in hit_cases(abi):
        for o, d in rays:
            dn = K.normalized(K.V(*d))                           # Ray::new
            hit, out9 = oracle_mod.scene_hit(sc, o, np.asarray(d, np.float32))
            check_hit(name, expect(o, dn), hit, out9)


@pytest.mark.gpu
def test_gpu_scatter_and_hits_equal_the_numpy_known_answers(native, abi):
    """The same known answers through the DEVICE code: scatter_pre / diffuse_finish / hit_scene as the render kernels call them."""
    host, device = native
    cases = scatter_cases(abi)
    mats = (abi.Material * len(cases))(*[c[1] for c in cases])
    inputs = scatter_inputs()
    recs, wants = [], []
    for mi, (name, _, expect, transcendental) in enumerate(cases):
        for rd, p, n, ff, ctr in inputs:
            recs.append((mi, ff, rd, p, n, ctr))
            wants.append((name, expect(rd, p, n, ff, K.CtrDraws(*ctr)), transcendental))
    got = device.debug_scatter(mats, recs)
    for (name, want, transcendental), g in zip(wants, got):
        check_scatter(name, want, g, transcendental)
    rgba, textures, tmat = texture_fixture(abi)
    trecs, twants = [], []
    for i, n in enumerate(texture_normals()):
        rd, p, ctr = K.normalized(-n + K.V(0.1, 0.05, -0.02)), K.V(0.5, -1.0, 2.0), (7, 9, i, 3, 2)
        trecs.append((0, True, rd, p, n, ctr))
        twants.append(K.scatter_texture(K.V(0.9, 0.8, 0.7), rgba, f32(0.3), rd, p, n, K.CtrDraws(*ctr)))
    for want, g in zip(twants, device.debug_scatter((abi.Material * 1)(tmat), trecs, textures=textures)):
        check_scatter("texture", want, g, False)
    for name, sc, rays, expect in hit_cases(abi):
        out = device.debug_hit(sc, [(o, K.V(*d)) for o, d in rays])
        for (o, d), g in zip(rays, out):
            check_hit(name, expect(o, K.normalized(K.V(*d))), bool(g[9]), g[:9])
