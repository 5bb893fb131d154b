"""Seeded random scenes that exercise EVERY primitive kind (sphere, plane, quad, cube, mesh) and EVERY material kind,
built directly as ABI arrays (through the oracle-side f32 helpers for matrices / quads)."""
import ctypes as C

import numpy as np


def random_scene(abi, host, seed, exact_only, n_prims=14, mesh_tris=60, only_kinds=None, lambert_only=False, identity_meshes=False, no_metal=False,
                 no_specular=False, textures=False, sky=False, coincident=False, big_mesh_tris=0, every_material=False, poison=None):
    """The options after no_metal are off by default, and then the scene of a seed is the one earlier versions made:
      no_specular    no metal and no dielectric (what the no-specular lockstep / mesh-free wavefront kernels accept);
      textures       two small RGBA8 textures whose neighbouring texels differ, and texture materials (h_offset != 0) over them;
      sky            an HDR sky map (float32 [8, 16, 3]) instead of the flat miss colour;
      coincident     every third primitive and the first of each kind repeated with another material right behind itself, and once more at
                     the end of the list
                     (equal t: the list order decides); meshes also repeat some of their triangles with the opposite winding;
      big_mesh_tris  > 0: one more mesh of that many small triangles (its tree passes LDS_NODE_CAP and WF_SHALLOW_NODES);
      every_material the first primitives take the material kinds in turn, so that every material of the list is hit-able;
      poison         a name of POISONS: non-finite or out-of-range values written into COLOURS of the finished scene (emitters, the miss
                     colour, sky texels, albedos) -- never into geometry, roughness, IOR or the camera, and no draw is made for it.
    They draw from a generator of their own, so the draws of the options before them stay what they were."""
    from oracle import scene_loader as L
    rng = np.random.default_rng(seed)
    F = np.float32
    mats = []

    def mat(kind, albedo=(0, 0, 0), aux=(0, 0, 0), p0=0.0, eta=(0, 0, 0), k=(0, 0, 0)):
        m = abi.Material(); m.kind = kind
        m.albedo[:] = [float(F(v)) for v in albedo]; m.aux[:] = [float(F(v)) for v in aux]; m.p0 = float(F(p0))
        m.eta[:] = [float(F(v)) for v in eta]; m.k[:] = [float(F(v)) for v in k]
        mats.append(m); return len(mats) - 1

    col = lambda lo=0.1, hi=0.95: tuple(rng.uniform(lo, hi, 3))
    kinds = [mat(abi.MAT_LAMBERT_SOLID, col()), mat(abi.MAT_LAMBERT_CHECKER, col(), col(), p0=1.0 / rng.uniform(0.2, 1.5)),
             mat(abi.MAT_METAL, col(), p0=0.0), mat(abi.MAT_METAL, col(), p0=rng.uniform(0.05, 0.6)),
             mat(abi.MAT_DIELECTRIC, p0=rng.uniform(1.2, 1.9)), mat(abi.MAT_EMISSIVE, tuple(rng.uniform(1, 6, 3))),
             mat(abi.MAT_PLASTIC, col(), p0=rng.uniform(1.2, 1.8)), mat(abi.MAT_NULL), mat(abi.MAT_LAMBERT_SOLID, col())]
    if lambert_only:                                                 # what the Lambert-only lockstep kernel (k_render_ctr_simple) is picked for:
        del mats[:]                                                  # the materials ARRAY holds nothing but Lambert (solid) / Emissive / Null
        kinds = [mat(abi.MAT_LAMBERT_SOLID, col()), mat(abi.MAT_EMISSIVE, tuple(rng.uniform(1, 6, 3))), mat(abi.MAT_NULL), mat(abi.MAT_LAMBERT_SOLID, col())]
    if no_metal:                                                     # the wavefront kernels' pruned instantiations: no MI355RT_MAT_METAL in the list
        kinds = [k for k in kinds if mats[k].kind != abi.MAT_METAL]
    if no_specular:
        kinds = [k for k in kinds if mats[k].kind not in (abi.MAT_METAL, abi.MAT_DIELECTRIC)]
    if not exact_only:
        cu = ((0.2, 1.09, 1.42), (3.91, 2.57, 2.30))
        kinds += [mat(abi.MAT_ROUGH_GGX, col(), p0=rng.uniform(0.02, 0.5), eta=cu[0], k=cu[1]),
                  mat(abi.MAT_ROUGH_BECKMANN, col(), p0=rng.uniform(0.02, 0.5), eta=cu[0], k=cu[1])]

    rng2 = np.random.default_rng([seed, 0x5eed])
    tex_arrays = []
    if textures:
        for h, w in ((4, 8), (6, 5)):
            img = rng2.integers(0, 256, (h, w, 4), dtype=np.uint8)
            img[..., 0] = (np.arange(w)[None, :] * 37 + np.arange(h)[:, None] * 91) % 256           # neighbouring texels always differ
            tex_arrays.append(np.ascontiguousarray(img))
        for t in range(len(tex_arrays)):
            k = mat(abi.MAT_TEXTURE, tuple(rng2.uniform(0.1, 0.95, 3)), p0=float(rng2.uniform(0.1, 0.9)))
            mats[k].texture = t
            kinds.append(k)

    def matrix():
        q = L.quat_from_euler_yxz_deg(F(rng.uniform(-180, 180)), F(rng.uniform(-180, 180)), F(rng.uniform(-180, 180)))
        return L.mat4_from_scale_rotation_translation([F(v) for v in rng.uniform(0.4, 2.0, 3)], q, [F(v) for v in rng.uniform(-3, 3, 3)])

    prims, tri_chunks, meshes = [], [], []
    if only_kinds is not None:
        order = [only_kinds[i % len(only_kinds)] for i in range(n_prims)]
    else:
        order = [abi.PRIM_SPHERE, abi.PRIM_PLANE, abi.PRIM_QUAD, abi.PRIM_CUBE, abi.PRIM_MESH] + list(rng.integers(0, 5, n_prims - 5))
    if big_mesh_tris > 0:
        order = list(order) + [abi.PRIM_MESH]
    n_tri = 0
    for pi, kind in enumerate(order):
        big = big_mesh_tris > 0 and pi == len(order) - 1
        p = abi.Primitive(); p.kind = int(kind); p.material = int(kinds[rng.integers(0, len(kinds))])
        if every_material and pi < len(kinds):
            p.material = int(kinds[pi])
        if kind == abi.PRIM_SPHERE:
            p.data[0:4] = [float(F(v)) for v in rng.uniform(-3, 3, 3)] + [float(F(rng.uniform(0.3, 1.2)))]
        elif kind == abi.PRIM_PLANE:
            n = L.normalized(L.v3(*rng.normal(size=3)))
            p.data[0:6] = [0.0, float(F(-4.0 - rng.uniform(0, 1))), 0.0] + [float(v) for v in (L.v3(0, 1, 0) if rng.random() < 0.5 else n)]
        elif kind == abi.PRIM_QUAD:
            p.data[0:15] = [float(v) for v in L.quad_from_matrix(matrix())]
        elif kind == abi.PRIM_CUBE:
            m = matrix(); p.data[0:16] = [float(v) for v in m]; p.data[16:32] = [float(v) for v in L.mat4_inverse(m)]
        else:
            m = matrix(); p.data[0:16] = [float(v) for v in m]; p.data[16:32] = [float(v) for v in L.mat4_inverse(m)]
            if identity_meshes:                                        # untransformed meshes (OBJ data in world space): what k_render_ctr_wf_nometal_ident is picked for
                ident = [1.0 if (k % 5) == 0 else 0.0 for k in range(16)]
                p.data[0:16] = ident; p.data[16:32] = ident
            if big:                                                          # small triangles scattered through the unit box: a deep tree
                nt = big_mesh_tris
                v = (rng2.uniform(-1, 1, size=(nt, 1, 3)) + rng2.uniform(-0.06, 0.06, size=(nt, 3, 3))).astype(F)
            else:
                nt = mesh_tris if mesh_tris > 0 else int(rng.integers(1, 4))          # mesh_tris <= 0: tiny meshes of 1..3 triangles
                v = rng.uniform(-1, 1, size=(nt, 3, 3)).astype(F)
                v[: nt // 4, :, 2] = F(0.25)                                   # a coplanar patch: zero-thickness leaf boxes (App. B-1)
            if coincident:                                                   # repeated triangles: copies of the first fifth at the end of the mesh,
                v = np.concatenate([v, v[: max(1, nt // 5)][:, [0, 2, 1]]], axis=0)   # wound the other way (other t arithmetic: the winner shows)
                nt = len(v)
            idx = np.arange(nt * 3).reshape(nt, 3)
            tris = L._triangles_from_indexed(v.reshape(-1, 3), idx)
            mesh = abi.Mesh(); mesh.first_triangle, mesh.triangle_count = n_tri, len(tris)
            n_tri += len(tris); tri_chunks.append(tris); meshes.append(mesh); p.mesh = len(meshes) - 1
        prims.append(p)
    if coincident:                                                       # equal t, other material: next to itself and once more at the end
        reps = []
        firsts = {int(q.kind): i for i, q in reversed(list(enumerate(prims)))}     # ... and the first primitive of every kind
        for i in sorted(set(range(0, len(prims), 3)) | set(firsts.values())):
            q = abi.Primitive(); C.pointer(q)[0] = prims[i]
            q.material = int(kinds[(kinds.index(prims[i].material) + 1) % len(kinds)])
            reps.append((i, q))
        tail = []
        for i, q in reversed(reps):
            r = abi.Primitive(); C.pointer(r)[0] = q
            r.material = int(kinds[(kinds.index(q.material) + 1) % len(kinds)])
            prims.insert(i + 1, q)
            tail.append(r)
        prims.extend(tail)

    sc = L.LoadedScene()
    if sky:
        sc.sky = (rng2.uniform(0.05, 1.0, (8, 16, 3)) * rng2.choice([1.0, 4.0], (8, 16, 1))).astype(F)
    sc.materials, sc.primitives, sc.meshes = mats, prims, meshes
    sc.triangles = np.concatenate(tri_chunks, axis=0) if tri_chunks else np.zeros((0, 12), F)
    sc.finalize()
    sc.c.miss_color[:] = [float(F(v)) for v in rng.uniform(0.2, 0.8, 3)]
    if tex_arrays:
        sc._tex_arrays = tex_arrays
        sc._textures = (abi.Texture * len(tex_arrays))(*[abi.Texture(a.ctypes.data_as(C.POINTER(C.c_uint8)), a.shape[1], a.shape[0]) for a in tex_arrays])
        sc.c.textures, sc.c.n_textures = sc._textures, len(tex_arrays)
    if poison is not None:
        apply_poison(abi, sc, poison)
    sc._keep = host.attach_bvh(sc)
    sc.camera = L.camera_new((0.0, 1.0, 9.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), F(50.0), F(4.0 / 3.0))
    return sc


_INF, _NAN = float("inf"), float("nan")
_FOUR = {"inf": (_INF, _INF, _INF), "mixed": (_INF, -_INF, _NAN), "overflow": (3e38, 3e38, 1e-42), "signed": (-1.0, -0.0, 1e-40)}
# name -> (what is poisoned, the colour).  "lambert": the albedo of EVERY solid Lambert material (0 * inf at lights, inf * 0 where a path runs
# out of depth); "sky": texels of the HDR map (the scene must be made with sky=True).
POISONS = {**{f"emissive_{k}": ("emissive", v) for k, v in _FOUR.items()}, **{f"miss_{k}": ("miss", v) for k, v in _FOUR.items()},
           "sky": ("sky", None),
           "lambert_zero": ("lambert", (0.0, 0.0, 0.0)), "lambert_gt1": ("lambert", (1.5, 4.0, 1.0000001)), "lambert_inf": ("lambert", (_INF, _INF, _INF)),
           "lambert_negative": ("lambert", (-0.5, -2.0, -0.0)),
           "metal_inf": ("metal", (_INF, _INF, _INF)), "checker_nan": ("checker", (_NAN, _NAN, _NAN)), "rough_inf": ("rough", (_INF, _INF, _INF))}


def apply_poison(abi, sc, name):
    """Writes the poison `name` into the colours of the finalized scene `sc` (its ctypes arrays).  Raises if the scene holds nothing to poison."""
    what, colour = POISONS[name]
    F = np.float32
    if what == "miss":
        sc.c.miss_color[:] = [float(F(v)) for v in colour]
        return
    if what == "sky":
        sky = sc._sky_np                                               # [H, W, 3]: a pattern over the texels, every fourth stays as drawn
        h, w, _ = sky.shape
        k = (np.arange(h)[:, None] * 5 + np.arange(w)[None, :]) % 8
        sky[k == 1] = F(np.inf)
        sky[k == 3] = F(np.nan)
        sky[k == 5] = F(1e-41)                                         # denormal
        sky[k == 7] = (F(np.inf), F(1e-45), F(0.5))
        return
    kinds = {"emissive": (abi.MAT_EMISSIVE,), "lambert": (abi.MAT_LAMBERT_SOLID,), "metal": (abi.MAT_METAL,), "checker": (abi.MAT_LAMBERT_CHECKER,),
             "rough": (abi.MAT_ROUGH_GGX, abi.MAT_ROUGH_BECKMANN)}[what]
    hit = 0
    for i in range(sc.c.n_materials):
        m = sc.c.materials[i]
        if m.kind in kinds:
            if what == "checker":
                m.aux[:] = [float(F(v)) for v in colour]                 # the checker's second colour
            else:
                m.albedo[:] = [float(F(v)) for v in colour]
            hit += 1
    if not hit:
        raise ValueError(f"poison {name}: the scene holds no such material")
