"""tests/scene_shapes.py without a GPU: that its cameras, lists and mesh tables are what their names say; that the rays of the frames
tests/test_gpu_scene_shapes.py renders see them (conditions on the ORACLE's first hits, so that the GPU comparisons are not vacuous); the camera
masks of k_render_ctr_simple_qc under the new cameras (no clear bit is wrong); and the prepared records of the mesh tables (node_begin is the
root of mesh primitive.mesh, whichever primitive names it).

The conditions: every camera hits something in at least 10 % of its pixel centres, misses in at least 2 % (not `inside`: all its rays end on
its own cube's walls) and sees at least 3 distinct primitives; a list of 65 or more has at least 16 distinct winners with list index >= 32, the
list of 1000 at least 16 with index >= 256; every mesh primitive of a mesh table wins at least 5 pixel centres.  One exception follows from the
comparison rule itself: of two coincident users of one mesh (shared_identity) the first in the list wins every tie, so the second wins nothing;
that it wins nothing IS the check."""
import math

import numpy as np
import pytest

import scene_shapes as S
import test_camera_masks as CM
import test_gpu_variant_matrix as M
import test_scene_prepare as P

F = np.float32
LOCKSTEP = (0, 3, 9, 14)


def _say(capsys, line):
    with capsys.disabled():
        print("\n    " + line, end="")


# ---------------------------------------------------------------------------------------------------------------- the camera table
def test_camera_classes_are_what_their_names_say(native, abi):
    host, _ = native
    sc = S.camera_scene(abi, host, "qc")
    cams = {name: S.camera(name, abi, sc) for name in S.CAMERAS}
    b = {name: S.basis(cam) for name, cam in cams.items()}
    base = cams["baseline"]
    assert bytes(base) == bytes(sc.camera) and list(base.position) == [0.0, 1.0, 9.0] and list(base.right) == [1.0, 0.0, 0.0] and base.forward[0] == 0.0
    assert np.all(np.abs(b["rolled_oblique"]) > 0.05), "all nine components of the basis are far from zero"
    assert b["from_minus_z"][0][2] > 0.9
    assert math.degrees(math.acos(-b["looking_down"][0][1])) < 3.0 and abs(b["looking_down"][2][2] + 1.0) < 0.01
    assert abs(cams["wide"].half_height - math.tan(math.radians(75.0))) < 1e-5
    assert abs(cams["narrow"].half_height - math.tan(math.radians(1.5))) < 1e-7 and 65.0 < np.linalg.norm(list(cams["narrow"].position)) < 75.0
    W, H = S.frame("anamorphic")
    assert abs(cams["anamorphic"].half_width / cams["anamorphic"].half_height - 3.0) < 1e-6 and W / H < 1.0
    assert abs(cams["far_tele"].half_height - math.tan(math.radians(0.03))) < 1e-9 and np.linalg.norm(list(cams["far_tele"].position)) > 7000.0
    f, r, u = b["sheared"]
    assert abs(np.linalg.norm(f) - 1) > 0.5 and abs(np.linalg.norm(r) - 1) > 0.3 and abs(np.linalg.norm(u) - 1) > 0.1
    assert abs(f @ r) > 0.5 and abs(f @ u) > 0.3 and abs(r @ u) > 0.3
    for name in set(S.CAMERAS) - {"sheared"}:                            # camera_new's are orthonormal
        assert np.allclose(b[name] @ b[name].T, np.eye(3), atol=1e-5), name
    for which in S.CAMERA_SCENES + ("qc2",):                             # `inside` stands inside a cube of each scene it is used with
        s2 = S.camera_scene(abi, host, which)
        pos = np.array(list(S.camera("inside", abi, s2).position) + [1.0])
        inside = [i for i in S.cubes_of(s2) if np.all(np.abs((np.array(list(s2.c.primitives[i].data[16:32])).reshape(4, 4).T @ pos)[:3]) < 0.45)]
        assert inside, which


@pytest.mark.parametrize("which", S.CAMERA_SCENES + ("qc2",))
def test_every_camera_sees_its_scene(which, native, oracle_mod, abi, capsys):
    host, device = native
    sc = S.camera_scene(abi, host, which)
    got = device.prepare_scene(sc)
    assert sc.c.n_primitives <= 32
    assert (got.variant == 14) == which.startswith("qc") and (which != "mesh" or got.variant in (10, 13)) and (which != "meshfree" or got.variant == 9)
    for name in S.CAMERAS:
        W, H = S.frame(name)
        share, who, _ = S.winners(abi, S.camera_records(oracle_mod, abi, sc, S.camera(name, abi, sc), W, H, ("camera", which, name)))
        _say(capsys, f"{which:8s} {name:15s} {W}x{H}: hit {100 * share:5.1f} %  miss {100 - 100 * share:5.1f} %  distinct winners {len(who)}")
        assert share >= 0.10, (which, name)
        assert name == "inside" or 1.0 - share >= 0.02, (which, name)
        assert len(who) >= 3, (which, name)


# ---------------------------------------------------------------------------------------------------------------- the lists
@pytest.mark.parametrize("family", list(S.FAMILY_LENGTHS))
def test_long_lists_are_seen_behind_index_32_and_256(family, native, oracle_mod, abi, capsys):
    host, device = native
    for n in S.FAMILY_LENGTHS[family]:
        sc = S.list_scene(abi, host, family, n)
        c = sc.c
        assert c.n_primitives == n
        kinds = [c.primitives[i].kind for i in range(n)]
        got = device.prepare_scene(sc)
        masks = device.camera_masks(sc, sc.camera, abi.Settings(40, 30, 1, S.DEPTH))
        if family == "qc":
            assert got.variant == 14 and set(kinds) <= {S.QUAD, S.CUBE}
            assert (masks is not None) == (n <= 32), "a table up to 32 primitives, none above"
        else:
            assert masks is None and kinds.count(S.PLANE) <= 2
            assert got.variant in ((0, 3, 14) if family == "meshfree" else (7, 13))
            if n >= 31:
                assert {S.SPHERE, S.PLANE, S.QUAD, S.CUBE} <= set(kinds)
                mats = {c.materials[c.primitives[i].material].kind for i in range(n)}
                assert mats == {M.LAMBERT, M.CHECKER, M.METAL, M.DIELECTRIC, M.EMISSIVE, M.PLASTIC, M.NULL}, "every exact material"
            if family == "mesh":
                assert [i for i in range(n) if kinds[i] == S.MESH] == list(range(0, n, 5)) and all(c.meshes[m].triangle_count == 8 for m in range(c.n_meshes))
        share, who, _ = S.winners(abi, S.camera_records(oracle_mod, abi, sc, sc.camera, 40, 30, ("list", family, n)))
        far32, far256 = sum(i >= 32 for i in who), sum(i >= 256 for i in who)
        _say(capsys, f"{family:8s} N = {n:4d}: variant {got.variant:2d}  hit {100 * share:5.1f} %  distinct winners {len(who):3d}, with index >= 32: {far32:3d}, >= 256: {far256:3d}")
        if n >= 65:
            assert far32 >= 16, (family, n, far32)
        if n == 1000:
            assert far256 >= 16, (family, n, far256)


def test_run_shapes(native, oracle_mod, abi, capsys):
    host, device = native
    n = S.RUN_LENGTH
    for shape in S.RUN_SHAPES:
        sc = S.run_scene(abi, host, shape)
        got = device.prepare_scene(sc)
        assert got.variant == 14 and sc.c.n_primitives == n and device.camera_masks(sc, sc.camera, abi.Settings(40, 30, 1, S.DEPTH)) is None
        want = [n - 1] * (n - 1) + [n] if shape == "one_long_run" else list(range(1, n + 1))
        assert got.prims["run_end"].tolist() == want, shape
        share, who, _ = S.winners(abi, S.camera_records(oracle_mod, abi, sc, sc.camera, 40, 30, ("run", shape)))
        _say(capsys, f"{shape:12s} N = {n}: hit {100 * share:5.1f} %  distinct winners {len(who)}, with index >= 32: {sum(i >= 32 for i in who)}")
        assert sum(i >= 32 for i in who) >= 16
        if shape == "one_long_run":
            assert n - 1 in who, "the cube behind the run of 300 quads is seen"


# ---------------------------------------------------------------------------------------------------------------- the mesh tables
def _table_users(sc):
    return [(i, sc.c.primitives[i].mesh) for i in S.mesh_prims(sc)]


EXPECT = {   # shape -> (variant, inline_steps, the mesh of each mesh primitive in list order)
    "reversed": (13, 1, [3, 2, 1, 0]),
    "shared_mixed": (13, 1, [0, 1, 2, 3, 0]),
    "shared_identity": (12, 1, [0, 0, 1, 2, 3]),
    "unused_big_first": (13, 1, [1, 2, 3, 4]),
    "meshes_without_mesh_primitives": (0, 0, []),
    "one_triangle_instanced": (13, 1, [0] * 40),
}


@pytest.mark.parametrize("shape", S.MESH_TABLES)
def test_mesh_tables_prepare_by_mesh_index_and_every_user_is_seen(shape, native, oracle_mod, abi, capsys):
    host, device = native
    sc = S.table_scene(abi, host, shape)
    c = sc.c
    got = device.prepare_scene(sc)
    variant, inline_steps, table = EXPECT[shape]
    users = _table_users(sc)
    assert [m for _, m in users] == table and (got.variant, got.inline_steps) == (variant, inline_steps), (shape, users, got.variant, got.inline_steps)
    assert c.n_meshes > 0 and c.n_nodes > 0 and all(c.meshes[m].node_count > 0 for m in range(c.n_meshes))
    ident = [i for i, _ in users if list(c.primitives[i].data[16:32]) == S.IDENTITY]
    if shape == "shared_mixed":
        assert ident == [users[-1][0]] and users[0][1] == users[-1][1] == 0
    if shape == "shared_identity":
        a, b = users[0][0], users[1][0]
        assert len(ident) == len(users) and bytes(c.primitives[a].data) == bytes(c.primitives[b].data)
    if shape == "unused_big_first":
        assert c.meshes[0].node_count > M.LDS_NODE_CAP and all(c.meshes[m].node_count <= 64 for m in range(1, c.n_meshes)) and 0 not in table
        m0 = c.materials[c.primitives[users[0][0]].material]
        kind = m0.kind
        m0.kind = abi.MAT_METAL                                          # ... and with metal in the list the automatic choice is 7
        try:
            assert device.prepare_scene(sc).variant == 7
        finally:
            m0.kind = kind
        twin = sc.oracle_twin                                            # what the oracle's per-ray hook is asked instead: the same but for the unused tree
        assert twin.c.n_primitives == c.n_primitives and twin.c.n_meshes == c.n_meshes and twin.c.meshes[0].triangle_count == 1
        assert all(bytes(twin.c.primitives[i].data) == bytes(c.primitives[i].data) and twin.c.primitives[i].mesh == c.primitives[i].mesh
                   and twin.c.primitives[i].kind == c.primitives[i].kind for i in range(c.n_primitives))
        assert all((twin.c.meshes[m].first_triangle, twin.c.meshes[m].triangle_count) == (c.meshes[m].first_triangle, c.meshes[m].triangle_count) for m in range(1, c.n_meshes))
        assert twin._tri_np.tobytes() == sc._tri_np.tobytes()
    if shape == "meshes_without_mesh_primitives":
        assert got.variant in LOCKSTEP and not users and (got.prims["node_begin"] == 0).all()
    if shape == "one_triangle_instanced":
        assert c.n_meshes == 1 and c.meshes[0].triangle_count == 1 and c.meshes[0].node_count == 1 and c.nodes[c.meshes[0].first_node].index_count == 1
        assert len({bytes(c.primitives[i].data) for i, _ in users}) == 40
    # the records: node_begin is the root of mesh p.mesh, and the device walk from it visits that mesh's triangles in the reference's order
    nodes, idx, tris = P.inputs(sc)
    want_tri = np.concatenate([tris[:, 0:3], tris[:, 3:6] - tris[:, 0:3], tris[:, 6:9] - tris[:, 0:3], tris[:, 9:12]], axis=1)
    dev_tri = np.concatenate([got.tris[k] for k in ("v0", "e1", "e2", "n")], axis=1)
    roots = [bytes(c.nodes[c.meshes[m].first_node].bmin) + bytes(c.nodes[c.meshes[m].first_node].bmax) for m in range(c.n_meshes)]
    assert len(set(roots)) == c.n_meshes, "the meshes' root boxes tell them apart"
    rng = np.random.default_rng(5)
    choice = {}
    for node in nodes:
        choice.setdefault(node["bmin"].tobytes() + node["bmax"].tobytes(), bool(rng.random() < 0.7))
    begin = {}
    for i, m in users:
        root = int(got.prims["node_begin"][i])
        assert begin.setdefault(m, root) == root, "two users of one mesh share its root"
        assert root == m, "level 0 of every mesh comes first, in table order"
        at = got.nodes[root]
        assert at["bmin"].tobytes() + at["bmax"].tobytes() == roots[m], (shape, i, m)
        mesh = c.meshes[m]
        mn, mi = nodes[mesh.first_node:mesh.first_node + mesh.node_count], idx[mesh.first_index:mesh.first_index + mesh.index_count]
        for hit in (lambda box: True, choice.__getitem__):
            want = [mesh.first_triangle + t for t in P._reference_walk(mn, mi, hit)]
            have = P._device_walk(got.nodes, root, hit)
            assert len(have) == len(want) and np.array_equal(dev_tri[have].view(np.uint32), want_tri[want].view(np.uint32)), (shape, i, m)
        assert sorted(mesh.first_triangle + t for t in P._reference_walk(mn, mi, lambda box: True)) == list(range(mesh.first_triangle, mesh.first_triangle + mesh.triangle_count))
    assert len(set(begin.values())) == len(begin)
    # the oracle sees every user
    _, who, wins = S.winners(abi, S.camera_records(oracle_mod, abi, sc, sc.camera, 40, 30, ("table", shape)))
    _say(capsys, f"{shape:30s} variant {got.variant:2d}: pixel centres won by each mesh primitive (primitive: mesh: wins) "
         + " ".join(f"{i}:{m}:{wins.get(i, 0)}" for i, m in users))
    if shape == "unused_big_first":                                      # the twin answers as the scene itself does: every 37th pixel centre asked of both
        import test_gpu_ray_queries as Q
        rec = S.camera_records(oracle_mod, abi, sc, sc.camera, 40, 30, ("table", shape))
        dirs = Q.camera_dirs(sc.camera, 40, 30).reshape(-1, 3)[::37]
        origins = np.tile(np.array(list(sc.camera.position), F), (len(dirs), 1))
        own = Q.oracle_hits(("table", shape, "the scene itself"), oracle_mod, abi, Q.own_materials(abi, sc), origins, dirs)
        assert own.tobytes() == rec[::37].tobytes() and (own["primitive"] != abi.NO_HIT).sum() >= 3
    loser = users[1][0] if shape == "shared_identity" else None
    for i, m in users:
        if i == loser:
            assert wins.get(i, 0) == 0, "of two coincident users the earlier one in the list wins every tie"
        else:
            assert wins.get(i, 0) >= 5, (shape, i, m, wins.get(i, 0))
    if shape == "meshes_without_mesh_primitives":
        assert len(who) >= 3


# ---------------------------------------------------------------------------------------------------------------- camera masks
def _mask_scene(which, native, oracle_mod, abi, W, H):
    host, _ = native
    return CM.cornell(oracle_mod, host, W, H) if which == "cornell" else S.camera_scene(abi, host, which)


@pytest.mark.parametrize("which", ["qc", "qc2", "cornell"])
def test_masks_never_cull_a_hit_under_the_table_cameras(which, native, oracle_mod, abi, capsys):
    """Every table camera.  On the cornell geometry the vacuity conditions above are not asked (nothing stands inside its cubes, and its walls
    fill some views): only that no clear bit is wrong and that something is culled."""
    host, device = native
    for name in S.CAMERAS:
        W, H = S.frame(name)
        sc = _mask_scene(which, native, oracle_mod, abi, W, H)
        cam = S.camera(name, abi, sc)
        n = sc.c.n_primitives
        masks = device.camera_masks(sc, cam, abi.Settings(W, H, 1, 3))
        assert masks is not None and masks.shape == (H, W), (which, name)
        bad, asked = CM.culled_hits(abi, oracle_mod, sc, cam, W, H, masks)
        bits = sum(((masks >> np.uint32(i)) & 1).astype(np.int64) for i in range(n))
        _say(capsys, f"masks {which:8s} {name:15s}: {int((masks != 0).sum()):4d} of {W * H} pixels not empty, {float(bits.mean()):5.2f} of {n} bits per pixel, {asked} rays asked")
        assert not bad, (which, name, bad[:10])
        full = np.uint32((1 << n) - 1)
        assert int(masks.max()) <= int(full)
        assert (masks != 0).any()
        if name != "inside":
            assert (masks != full).any() and asked > 1000, "the masks cull"
        elif which != "cornell":
            room = n - 1
            assert (((masks >> np.uint32(room)) & 1) == 1).all(), "the cube the camera stands in is kept everywhere"


@pytest.mark.parametrize("which", ["qc", "qc2", "cornell"])
def test_sheared_and_nan_cameras_get_a_correct_table_or_keep_every_bit(which, native, oracle_mod, abi):
    host, device = native
    W, H = 40, 30
    sc = _mask_scene(which, native, oracle_mod, abi, W, H)
    full = np.uint32((1 << sc.c.n_primitives) - 1)
    nan_cams = []
    for field, k in (("right", 1), ("forward", 2), ("true_up", 0), ("position", 1)):
        cam = S.camera("rolled_oblique", abi, sc)
        getattr(cam, field)[k] = float("nan")
        nan_cams.append(cam)
    cam = S.camera("rolled_oblique", abi, sc); cam.half_height = float("nan"); nan_cams.append(cam)
    cam = S.camera("sheared", abi, sc); cam.right[2] = float("inf"); nan_cams.append(cam)
    for cam in [S.camera("sheared", abi, sc)] + nan_cams:
        masks = device.camera_masks(sc, cam, abi.Settings(W, H, 1, 3))
        assert masks is not None and masks.shape == (H, W)
        if not (masks == full).all():
            with np.errstate(all="ignore"):
                bad, _ = CM.culled_hits(abi, oracle_mod, sc, cam, W, H, masks)
            assert not bad, bad[:10]
