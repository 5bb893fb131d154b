"""Scenes off the three constants of the other test scenes (not a test, not a conftest): cameras that are not "from +z towards the origin, up = y",
lists longer than 32 primitives, and mesh tables in which primitive k does not use mesh k.  tests/test_scene_shapes_cpu.py checks on the
oracle that every camera, list and table below is seen by the rays of the frames tests/test_gpu_scene_shapes.py renders; that module then
compares the kernels with the oracle on them, bit for bit.

Everything here is exact_only (no texture, no HDR sky, no rough conductor): only + - * / sqrt is on the path."""
import ctypes as C

import numpy as np

from fuzz_scenes import random_scene

F = np.float32
SPHERE, PLANE, QUAD, CUBE, MESH = range(5)
DEPTH = 6
IDENTITY = [1.0 if (k % 5) == 0 else 0.0 for k in range(16)]


# ---------------------------------------------------------------------------------------------------------------- cameras
def _new(position, look_at, up, fov, aspect=4.0 / 3.0):
    def make(abi, sc):
        from oracle import scene_loader as L
        return L.camera_new(position, look_at, up, F(fov), F(aspect))
    return make


def cubes_of(sc):
    return [i for i in range(sc.c.n_primitives) if sc.c.primitives[i].kind == CUBE]


def _inside(abi, sc):
    """From the centre of the scene's cube that holds the centres of most other primitives (the first such; in the camera scenes below that is
    room_cube()), towards the origin -- or, from a cube around the origin, towards the fuzz camera's position.  100 degrees wide: the more of the
    cube's inside is in view, the more of what stands in it."""
    from oracle import scene_loader as L
    c = sc.c
    centres = []
    for i in range(c.n_primitives):
        p = c.primitives[i]
        d = np.array(list(p.data), np.float64)
        if p.kind in (CUBE, MESH):
            centres.append(d[12:15])
        elif p.kind == QUAD:
            centres.append(d[0:3] + 0.5 * d[3:6] + 0.5 * d[6:9])
        elif p.kind == SPHERE:
            centres.append(d[0:3])
        else:
            centres.append(np.full(3, 1e9))
    best, most = None, -1
    for i in cubes_of(sc):
        w2o = np.array(list(c.primitives[i].data[16:32]), np.float64).reshape(4, 4).T      # (column-major in the record)
        held = 0
        for k, p in enumerate(centres):
            if k != i and abs(p[0]) < 1e8:
                q = w2o @ np.array([p[0], p[1], p[2], 1.0])
                held += bool(np.all(np.abs(q[:3]) < 0.75))
        if held > most:
            best, most = i, held
    pos = tuple(float(F(v)) for v in c.primitives[best].data[12:15])
    at = (0.0, 0.0, 0.0) if float(np.linalg.norm(pos)) > 0.5 else (0.0, 1.0, 9.0)
    return L.camera_new(pos, at, (0.0, 1.0, 0.0), F(100.0), F(4.0 / 3.0))


def _sheared(abi, sc):
    """Filled in by hand: forward is not unit, right and true_up are neither unit nor orthogonal to each other or to forward."""
    cam = abi.Camera()
    cam.position[:] = [2.0, 1.5, 8.0]
    cam.forward[:] = [-0.5, -0.3, -2.0]
    cam.right[:] = [1.5, 0.2, 0.3]
    cam.true_up[:] = [0.3, 0.8, 0.1]
    cam.half_width, cam.half_height = 0.7, 0.4
    return cam


# class -> (maker(abi, scene), (width, height) of the frame)
CAMERAS = {
    "baseline": (_new((0.0, 1.0, 9.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 50.0), (40, 30)),
    "rolled_oblique": (_new((4.0, 3.0, 5.5), (0.3, -0.2, 0.1), (0.3, 1.0, 0.2), 55.0), (40, 30)),
    "from_minus_z": (_new((-2.0, 1.5, -8.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 50.0), (40, 30)),
    "looking_down": (_new((0.3, 9.0, 0.2), (0.0, 0.0, 0.0), (0.0, 0.0, -1.0), 50.0), (40, 30)),
    "wide": (_new((0.5, 0.5, 3.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 150.0), (40, 30)),
    "narrow": (_new((20.0, 15.0, 65.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 3.0), (40, 30)),
    "anamorphic": (_new((-3.0, 2.0, 8.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 40.0, 3.0), (24, 40)),
    "inside": (_inside, (40, 30)),
    "far_tele": (_new((4.0e3, 3.0e3, 5.0e3), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 0.06), (40, 30)),
    "sheared": (_sheared, (40, 30)),
}


def camera(name, abi, sc):
    return CAMERAS[name][0](abi, sc)


def frame(name):
    return CAMERAS[name][1]


_records = {}


def camera_records(oracle_mod, abi, sc, cam, W, H, key):
    """The oracle's first-hit records (abi.HIT_DTYPE [H * W], read-only) of the pixel centres of `cam` on `sc`, once per key.  The scene gets a
    material record per primitive (test_gpu_ray_queries.own_materials: the image stays what it was), so that a record names the PRIMITIVE
    that won."""
    import test_gpu_ray_queries as Q
    if key not in _records:
        dirs = Q.camera_dirs(cam, W, H).reshape(-1, 3)
        origins = np.tile(np.array(list(cam.position), F), (W * H, 1))
        _records[key] = Q.oracle_hits(("scene_shapes",) + tuple(key), oracle_mod, abi, per_ray_scene(abi, sc), origins, dirs)
    return _records[key]


def per_ray_scene(abi, sc):
    """The scene to hand to the oracle's per-ray hook (oracle.scene_hit) for `sc`: itself, or its twin (table_scene: unused_big_first); both with
    a material record per primitive."""
    import test_gpu_ray_queries as Q
    Q.own_materials(abi, sc)
    twin = getattr(sc, "oracle_twin", None)
    return sc if twin is None else Q.own_materials(abi, twin)


def winners(abi, records):
    """(share of hits, sorted distinct winning primitives, wins per primitive index as a dict)."""
    hit = records["primitive"] != abi.NO_HIT
    idx, counts = np.unique(records["primitive"][hit], return_counts=True)
    return float(hit.mean()), [int(i) for i in idx], {int(i): int(n) for i, n in zip(idx, counts)}


def basis(cam):
    return np.array([list(cam.forward), list(cam.right), list(cam.true_up)], np.float64)


# ---------------------------------------------------------------------------------------------------------------- lists
LENGTHS = (1, 31, 32, 33, 64, 65, 257, 1000)
FAMILY_LENGTHS = {"qc": LENGTHS, "meshfree": LENGTHS, "mesh": tuple(n for n in LENGTHS if n <= 257)}
RUN_SHAPES = ("one_long_run", "runs_of_one")
RUN_LENGTH = 301


def _materials(abi, rng, lambert_only=False, no_metal=False, no_specular=False):
    """The exact material kinds, as fuzz_scenes.random_scene lists them."""
    mats = []

    def mat(kind, albedo=(0, 0, 0), aux=(0, 0, 0), p0=0.0):
        m = abi.Material(); m.kind = kind
        m.albedo[:] = [float(F(v)) for v in albedo]; m.aux[:] = [float(F(v)) for v in aux]; m.p0 = float(F(p0))
        mats.append(m)

    col = lambda lo=0.1, hi=0.95: tuple(rng.uniform(lo, hi, 3))
    mat(abi.MAT_LAMBERT_SOLID, col()); mat(abi.MAT_EMISSIVE, tuple(rng.uniform(1, 6, 3))); mat(abi.MAT_NULL); mat(abi.MAT_LAMBERT_SOLID, col())
    if not lambert_only:
        mat(abi.MAT_LAMBERT_CHECKER, col(), col(), p0=1.0 / rng.uniform(0.2, 1.5)); mat(abi.MAT_PLASTIC, col(), p0=rng.uniform(1.2, 1.8))
        if not no_specular:
            mat(abi.MAT_DIELECTRIC, p0=rng.uniform(1.2, 1.9))
            if not no_metal:
                mat(abi.MAT_METAL, col(), p0=0.0); mat(abi.MAT_METAL, col(), p0=rng.uniform(0.05, 0.6))
    return mats


def _finish(abi, host, mats, prims, meshes, tri_chunks, miss):
    from oracle import scene_loader as L
    sc = L.LoadedScene()
    sc.materials, sc.primitives, sc.meshes = mats, prims, meshes
    sc.triangles = np.concatenate(tri_chunks, axis=0) if len(tri_chunks) else np.zeros((0, 12), F)
    sc.finalize()
    sc.c.miss_color[:] = [float(F(v)) for v in miss]
    sc._keep = host.attach_bvh(sc)
    sc.camera = camera("baseline", abi, sc)
    return sc


def room_cube(abi, material):
    """A cube of edge 3 beside the origin, large enough to hold parts of its neighbours: where the camera class `inside` stands."""
    from oracle import scene_loader as L
    m = L.mat4_from_scale_rotation_translation([F(3.0), F(3.0), F(3.0)], L.quat_from_euler_yxz_deg(F(10.0), F(20.0), F(30.0)), [F(-2.2), F(0.3), F(-0.5)])
    p = abi.Primitive(); p.kind, p.material = CUBE, material
    p.data[0:16] = [float(v) for v in m]; p.data[16:32] = [float(v) for v in L.mat4_inverse(m)]
    return p


def _list(abi, host, family, n, seed, no_metal=False, no_specular=False, room=False):
    """meshfree: sphere / plane / quad / cube; mesh: every fifth primitive (the first among them) a mesh of about 8 triangles.  The primitives
    shrink as the list grows -- their summed area stays about that of the view, so that the first hits have many winners -- and a list holds at
    most two planes, both ABOVE every camera of the table (far_tele stands at y = 3000): a plane fills the half of all directions that face it, and every camera here
    looks downwards, so that some of its rays can leave the scene.  room: one more primitive, room_cube()."""
    from oracle import scene_loader as L
    rng = np.random.default_rng([seed, n, {"meshfree": 1, "mesh": 2}[family]])
    mats = _materials(abi, rng, no_metal=no_metal, no_specular=no_specular)
    size = float(min(1.0, (40.0 / n) ** 0.5))
    prims, meshes, chunks, n_tri, planes = [], [], [], 0, 0

    def matrix():
        q = L.quat_from_euler_yxz_deg(F(rng.uniform(-180, 180)), F(rng.uniform(-180, 180)), F(rng.uniform(-180, 180)))
        return L.mat4_from_scale_rotation_translation([F(v * size) for v in rng.uniform(0.6, 2.0, 3)], q, [F(v) for v in rng.uniform(-3, 3, 3)])

    for i in range(n):
        kind = int(rng.integers(0, 4))
        if family == "mesh" and i % 5 == 0:
            kind = MESH
        elif n == 1:
            kind = SPHERE                                                # (a quad or a cube alone would be a list of the qc family)
        if kind == PLANE:
            planes += 1
            if planes > 2:
                kind = QUAD
        p = abi.Primitive(); p.kind = kind
        p.material = i if i < len(mats) else int(rng.integers(0, len(mats)))
        if kind == SPHERE:
            p.data[0:4] = [float(F(v)) for v in rng.uniform(-3, 3, 3)] + [float(F(size * rng.uniform(0.3, 1.0)))]
        elif kind == PLANE:
            nrm = L.normalized(L.v3(*(0.25 * rng.normal(size=3) + np.array([0.0, 1.0, 0.0]))))          # the first level, the second tilted
            p.data[0:6] = [0.0, float(F(4000.0 + 500.0 * planes + rng.uniform(0, 1))), 0.0] + [float(v) for v in (L.v3(0, 1, 0) if planes == 1 else nrm)]
        elif kind == QUAD:
            p.data[0:15] = [float(v) for v in L.quad_from_matrix(matrix())]
        else:
            m = matrix(); p.data[0:16] = [float(v) for v in m]; p.data[16:32] = [float(v) for v in L.mat4_inverse(m)]
            if kind == MESH:
                v = rng.uniform(-1, 1, size=(8, 3, 3)).astype(F)
                v[:2, :, 2] = F(0.25)
                tris = L._triangles_from_indexed(v.reshape(-1, 3), np.arange(24).reshape(8, 3))
                mesh = abi.Mesh(); mesh.first_triangle, mesh.triangle_count = n_tri, len(tris)
                n_tri += len(tris); chunks.append(tris); meshes.append(mesh); p.mesh = len(meshes) - 1
        prims.append(p)
    if room:
        prims.append(room_cube(abi, 0))
    return _finish(abi, host, mats, prims, meshes, chunks, rng.uniform(0.2, 0.8, 3))


_lists = {}


def list_scene(abi, host, family, n):
    """The list of `family` with n primitives (built once)."""
    if (family, n) not in _lists:
        if family == "qc":
            sc = random_scene(abi, host, 500 + n, exact_only=True, n_prims=n, only_kinds=[QUAD, CUBE], lambert_only=True)
        else:
            sc = _list(abi, host, family, n, seed=11)
        _lists[(family, n)] = sc
    return _lists[(family, n)]


def run_scene(abi, host, shape):
    """301 quads and cubes: 300 quads then one cube (one long run_end run), or quad / cube alternating (runs of one)."""
    if shape not in _lists:
        kinds = [QUAD] * (RUN_LENGTH - 1) + [CUBE] if shape == "one_long_run" else [QUAD, CUBE]
        sc = random_scene(abi, host, 901, exact_only=True, n_prims=RUN_LENGTH, only_kinds=kinds, lambert_only=True)
        if shape == "one_long_run":                                      # the cube at the end of the run stands in front of the quads, so that it is seen
            from oracle import scene_loader as L
            mats, prims, meshes, _, miss = _parts(abi, sc)
            m = L.mat4_from_scale_rotation_translation([F(1.0), F(0.8), F(1.2)], L.quat_from_euler_yxz_deg(F(25.0), F(40.0), F(10.0)), [F(0.6), F(0.9), F(5.0)])
            prims[-1].data[0:16] = [float(v) for v in m]; prims[-1].data[16:32] = [float(v) for v in L.mat4_inverse(m)]
            sc = _finish(abi, host, mats, prims, meshes, [], miss)
        _lists[shape] = sc
    return _lists[shape]


# The scenes the cameras look at: a quad / cube list of 24 (k_render_ctr_simple_qc, with a mask table), a mesh-free list without metal and
# dielectric (the lockstep kernels 0 / 9 and the mesh-free wavefront kernel 11 take it), a list with meshes and without metal (1 / 7 / 10 / 13).
CAMERA_SCENES = ("qc", "meshfree", "mesh")


def camera_scene(abi, host, which):
    key = ("camera", which)
    if key not in _lists:
        if which in ("qc", "qc2"):
            base = random_scene(abi, host, QC_SEEDS[which], exact_only=True, n_prims={"qc": 23, "qc2": 31}[which], only_kinds=[QUAD, CUBE],
                                lambert_only=True)
            mats, prims, meshes, chunks, miss = _parts(abi, base)
            sc = _finish(abi, host, mats, prims + [room_cube(abi, 0)], meshes, [], miss)
        elif which == "meshfree":
            sc = _list(abi, host, "meshfree", 29, seed=21, no_specular=True, room=True)
        else:
            sc = _list(abi, host, "mesh", 29, seed=22, no_metal=True, room=True)
        _lists[key] = sc
    return _lists[key]


# ---------------------------------------------------------------------------------------------------------------- mesh tables
MESH_TABLES = ("reversed", "shared_mixed", "shared_identity", "unused_big_first", "meshes_without_mesh_primitives", "one_triangle_instanced")
TABLE_KINDS = [MESH, QUAD, MESH, SPHERE, MESH, CUBE, MESH]
BIG_TRIS = 9000
INSTANCE_SEED = 84
TABLE_SEEDS = {"reversed": 31, "shared_mixed": 32, "shared_identity": 32, "unused_big_first": 33, "meshes_without_mesh_primitives": 35}
QC_SEEDS = {"qc": 100, "qc2": 106}


def _copy(abi, p):
    q = abi.Primitive(); C.pointer(q)[0] = p
    return q


def _parts(abi, sc):
    """Copies of a finished scene's lists, to build another scene from."""
    c = sc.c
    mats = []
    for i in range(c.n_materials):
        m = abi.Material(); C.pointer(m)[0] = c.materials[i]; mats.append(m)
    prims = [_copy(abi, c.primitives[i]) for i in range(c.n_primitives)]
    meshes = []
    for i in range(c.n_meshes):
        m = abi.Mesh(); m.first_triangle, m.triangle_count = c.meshes[i].first_triangle, c.meshes[i].triangle_count; meshes.append(m)
    return mats, prims, meshes, [sc._tri_np.copy()], list(c.miss_color)


def mesh_prims(sc):
    return [i for i in range(sc.c.n_primitives) if sc.c.primitives[i].kind == MESH]


def _other_material(mats, prims, i):
    """A material index of another Lambert / plastic kind than primitive i's, so that the winner of two coincident users shows in the image."""
    return next(k for k in range(len(mats)) if k != prims[i].material and mats[k].kind in (0, 1, 5) and bytes(mats[k]) != bytes(mats[prims[i].material]))


def _table(abi, host, shape):
    from oracle import scene_loader as L
    if shape == "one_triangle_instanced":
        rng = np.random.default_rng(INSTANCE_SEED)
        mats = _materials(abi, rng, no_metal=True)
        v = np.array([[-0.6, -0.5, -0.2], [0.6, -0.5, 0.1], [0.0, 0.6, 0.3]], F)          # (not in a coordinate plane: a box of zero thickness is never hit)
        tris = L._triangles_from_indexed(v, np.arange(3).reshape(1, 3))
        mesh = abi.Mesh(); mesh.first_triangle, mesh.triangle_count = 0, 1
        prims = []
        for k in range(40):                                              # an 8 x 5 grid facing the fuzz camera, each under a transform of its own
            gx, gy = k % 8, k // 8
            q = L.quat_from_euler_yxz_deg(F(rng.uniform(-25, 25)), F(rng.uniform(-25, 25)), F(rng.uniform(-180, 180)))
            m = L.mat4_from_scale_rotation_translation([F(s) for s in rng.uniform(1.3, 1.8, 3)], q,
                                                       [F(-4.2 + 1.2 * gx), F(-1.6 + 1.3 * gy), F(rng.uniform(-1, 1))])
            p = abi.Primitive(); p.kind, p.mesh, p.material = MESH, 0, int(k % len(mats))
            p.data[0:16] = [float(x) for x in m]; p.data[16:32] = [float(x) for x in L.mat4_inverse(m)]
            prims.append(p)
        return _finish(abi, host, mats, prims, [mesh], [tris], (0.4, 0.5, 0.7))
    ident = shape == "shared_identity"
    big = shape == "unused_big_first"
    base = random_scene(abi, host, TABLE_SEEDS[shape], exact_only=True, n_prims=len(TABLE_KINDS), only_kinds=TABLE_KINDS,
                        mesh_tris=12, no_metal=True, identity_meshes=ident, big_mesh_tris=BIG_TRIS if big else 0)
    mats, prims, meshes, chunks, miss = _parts(abi, base)
    users = [i for i, p in enumerate(prims) if p.kind == MESH]
    if shape == "reversed":
        for k, i in enumerate(users):
            prims[i].mesh = len(meshes) - 1 - k
    elif shape == "shared_mixed":                                        # the first mesh once more, untransformed, behind the list
        q = _copy(abi, prims[users[0]])
        q.data[0:16] = IDENTITY; q.data[16:32] = IDENTITY
        q.material = _other_material(mats, prims, users[0])
        prims.append(q)
    elif shape == "shared_identity":                                     # coincident: the same mesh in the same place under another material
        q = _copy(abi, prims[users[0]])
        q.material = _other_material(mats, prims, users[0])
        prims.insert(users[1], q)
    elif shape == "unused_big_first":                                    # the big mesh moves to the front of the table and loses its primitive
        assert prims[-1].kind == MESH and prims[-1].mesh == len(meshes) - 1 and meshes[-1].triangle_count > BIG_TRIS * 0.9
        prims.pop()
        meshes = [meshes[-1]] + meshes[:-1]
        for p in prims:
            if p.kind == MESH:
                p.mesh += 1
    elif shape == "meshes_without_mesh_primitives":                      # a cube where each mesh stood; the table and its trees stay
        for i in users:
            prims[i].kind, prims[i].mesh = CUBE, 0
    sc = _finish(abi, host, mats, prims, meshes, chunks, miss)
    if shape == "unused_big_first":
        # The oracle's per-ray hook builds the whole scene, the unused tree included, for every ray it is asked about.  Its twin holds the first
        # triangle of the big mesh only: the same primitives and the same used meshes at the same indices, so the same answers (the CPU tests compare some).
        one = abi.Mesh(); one.first_triangle, one.triangle_count = meshes[0].first_triangle, 1
        sc.oracle_twin = _finish(abi, host, mats, prims, [one] + meshes[1:], chunks, miss)
    return sc


def table_scene(abi, host, shape):
    if ("table", shape) not in _lists:
        sc = _table(abi, host, shape)
        if shape == "shared_identity":                                   # untransformed meshes all lie in the unit box: a closer look
            from oracle import scene_loader as L
            sc.camera = L.camera_new((1.5, 1.0, 3.5), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), F(50.0), F(4.0 / 3.0))
        _lists[("table", shape)] = sc
    return _lists[("table", shape)]


# ---------------------------------------------------------------------------------------------------------------- what a scene holds
def features_of(abi, sc):
    """The scene's features in the form test_gpu_variant_matrix.accepts reads."""
    c = sc.c
    prims = frozenset(c.primitives[i].kind for i in range(c.n_primitives))
    forms = frozenset("identity" if list(c.primitives[i].data[16:32]) == IDENTITY else "transformed" for i in range(c.n_primitives) if c.primitives[i].kind == MESH)
    return dict(mats=frozenset(c.materials[c.primitives[i].material].kind for i in range(c.n_primitives)), prims=prims, mesh_forms=forms)


def accepted_variants(M, abi, sc):
    """The forceable variants (test_gpu_variant_matrix.CAPABILITY) that accept the scene, the reference build's included."""
    f = features_of(abi, sc)
    return sorted(v for v in M.CAPABILITY if M.accepts(v, f))
