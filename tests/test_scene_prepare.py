"""Scene preparation without a GPU (csrc/device/rt_prepare.cpp through mi355rt_debug_prepare_scene): the refusals of malformed scenes, the walk the
two-link BVH encodes, its storage order, the primitive records and the choice of the kernel variant.  The CPU twin of tests/test_gpu_validation.py
and of test_gpu_variant_matrix.py::test_forced_variants_follow_the_capability_table: what those check behind a context is checked here on the
arrays set_scene would upload."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import test_gpu_variant_matrix as M
from conftest import ROOT, load_for_both
from fuzz_scenes import random_scene

f32 = np.float32
NODE_LINK_BITS, NODE_END, NODE_MAX_LEAF = 26, (1 << 26) - 1, 63           # rt_device.h
LDS_NODE_CAP = M.LDS_NODE_CAP
IN_NODE = np.dtype([("bmin", "<f4", 3), ("bmax", "<f4", 3), ("left", "<u4"), ("right", "<u4"), ("first_index", "<u4"), ("index_count", "<u4")])

_cache = {}


def shipped(name, oracle_mod, host):
    if name not in _cache:
        _cache[name] = load_for_both(name, oracle_mod, host, width=16, height=12, spp=1, max_depth=3)
    return _cache[name]


def fat_leaf_scene(abi, host):
    """The mesh scene of test_gpu_parity.py::test_caller_built_bvh_with_fat_leaves with its first mesh under ONE leaf that holds all its triangles."""
    if "fat" not in _cache:
        sc = random_scene(abi, host, 77, exact_only=True, n_prims=6, mesh_tris=150, only_kinds=[abi.PRIM_MESH, abi.PRIM_QUAD, abi.PRIM_SPHERE])
        c = sc.c
        mesh = c.meshes[0]
        n = mesh.triangle_count
        assert n > 2 * NODE_MAX_LEAF
        leaf = abi.BvhNode()
        leaf.bmin[:], leaf.bmax[:] = list(c.nodes[mesh.first_node].bmin), list(c.nodes[mesh.first_node].bmax)
        leaf.first_index, leaf.index_count = 0, n
        nodes = (abi.BvhNode * (c.n_nodes + 1))(*[c.nodes[i] for i in range(c.n_nodes)], leaf)
        idx = (C.c_uint32 * (c.n_tri_indices + n))(*[c.tri_indices[i] for i in range(c.n_tri_indices)], *range(n))
        mesh.first_node, mesh.node_count, mesh.first_index, mesh.index_count = c.n_nodes, 1, c.n_tri_indices, n
        c.nodes, c.n_nodes = C.cast(nodes, C.POINTER(abi.BvhNode)), len(nodes)
        c.tri_indices, c.n_tri_indices = C.cast(idx, C.POINTER(C.c_uint32)), len(idx)
        sc._fat = (nodes, idx)
        _cache["fat"] = sc
    return _cache["fat"]


def soup_scene(abi, host):
    """Two meshes of random triangles whose trees together pass LDS_NODE_CAP."""
    if "soup" not in _cache:
        sc = random_scene(abi, host, 5, exact_only=True, n_prims=2, mesh_tris=9000, only_kinds=[abi.PRIM_MESH])     # (trees deeper than the cap reaches: inner nodes lie behind it)
        assert sc.c.n_meshes == 2 and sc.c.n_nodes > LDS_NODE_CAP
        _cache["soup"] = sc
    return _cache["soup"]


def inputs(sc):
    """The scene's BVH arrays as numpy: nodes [IN_NODE], leaf indices, triangles float32 [n, 12] (v0, v1, v2, normal)."""
    c = sc.c
    nodes = np.frombuffer(C.string_at(c.nodes, c.n_nodes * IN_NODE.itemsize), IN_NODE) if c.n_nodes else np.zeros(0, IN_NODE)
    idx = np.frombuffer(C.string_at(c.tri_indices, c.n_tri_indices * 4), np.uint32) if c.n_tri_indices else np.zeros(0, np.uint32)
    tris = np.frombuffer(C.string_at(c.triangles, c.n_triangles * 48), np.float32).reshape(-1, 12) if c.n_triangles else np.zeros((0, 12), f32)
    return nodes, idx, tris


def refusal(device, sc):
    try:
        device.prepare_scene(sc)
    except device.RenderError as e:
        return e.rc, str(e)
    return 0, ""


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_malformed_scenes_are_refused(native, oracle_mod, abi):
    """Every mutation of test_gpu_validation.py's test_bad_indices_and_kinds_are_rejected, with its return code and message, and the malformed
    trees, radius, sky and texture index that only this file reaches; the scene prepares again, to the same bytes, after all of them."""
    host, device = native
    sc = load_for_both("semesterbild", oracle_mod, host, width=16, height=12, spp=1, max_depth=3)
    c = sc.c
    before = device.prepare_scene(sc)
    INVALID = abi.ERR_INVALID

    def mutated(obj, field, value, index=None):
        old = getattr(obj, field) if index is None else getattr(obj, field)[index]
        if index is None:
            setattr(obj, field, value)
        else:
            getattr(obj, field)[index] = value
        got = refusal(device, sc)
        if index is None:
            setattr(obj, field, old)
        else:
            getattr(obj, field)[index] = old
        return got

    p0, m0, mesh, root = c.primitives[0], c.materials[0], c.meshes[0], c.nodes[c.meshes[0].first_node]
    rc, msg = mutated(p0, "material", 999)
    assert rc == INVALID and "material" in msg
    rc, msg = mutated(p0, "kind", 17)
    assert rc == INVALID and "kind" in msg
    assert mutated(m0, "kind", 99)[0] == INVALID
    rc, msg = mutated(mesh, "node_count", c.n_nodes + 5)
    assert rc == INVALID and "node range" in msg
    rc, msg = mutated(root, "left", 0)                               # a cycle: the root's left child is the root
    assert rc == INVALID and ("cycle" in msg or "malformed" in msg)
    leaf_idx = next(i for i in range(c.n_nodes) if c.nodes[i].index_count > 0)
    k = c.nodes[leaf_idx].first_index
    old = c.tri_indices[k]; c.tri_indices[k] = 10 ** 6
    rc, msg = refusal(device, sc); c.tri_indices[k] = old
    assert rc == INVALID and "triangle id" in msg
    # ... and what only this file reaches
    rc, msg = mutated(root, "left", mesh.node_count + 7)
    assert rc == INVALID and "child index out of range" in msg
    rc, msg = mutated(root, "right", root.left)                      # a shared child: two parents
    assert rc == INVALID and "shared" in msg
    rc, msg = mutated(c.nodes[leaf_idx], "first_index", mesh.index_count)
    assert rc == INVALID and "leaf index range" in msg
    rc, msg = mutated(mesh, "node_count", 0)
    assert rc == INVALID and "node range" in msg
    sphere = next(c.primitives[i] for i in range(c.n_primitives) if c.primitives[i].kind == abi.PRIM_SPHERE)
    for r in (0.0, 9.9e-5, -9.9e-5):
        rc, msg = mutated(sphere, "data", r, index=3)
        assert rc == INVALID and "sphere radius" in msg, r
    assert not c.sky_rgb and c.sky_width == 0
    c.sky_width, c.sky_height = 4, 2                                  # dimensions without pixels
    rc, msg = refusal(device, sc); c.sky_width, c.sky_height = 0, 0
    assert rc == INVALID and "sky" in msg
    pixels = (C.c_float * 24)()
    c.sky_rgb = C.cast(pixels, C.POINTER(C.c_float)); c.sky_width = 4  # pixels and one dimension
    rc, msg = refusal(device, sc); c.sky_rgb = C.POINTER(C.c_float)(); c.sky_width = 0
    assert rc == INVALID and "sky" in msg
    assert c.n_textures == 0 and m0.texture == 0
    rc, msg = mutated(m0, "kind", abi.MAT_TEXTURE)                    # texture 0 of none
    assert rc == INVALID and "texture index" in msg
    after = device.prepare_scene(sc)
    assert after[:2] == before[:2] and all(a.tobytes() == b.tobytes() for a, b in zip(after[2:], before[2:]))


def test_a_scaled_quad_normal_is_refused(native, oracle_mod, abi):
    """test_gpu_validation.py's test of the same name, without the render."""
    host, device = native
    sc = load_for_both("cornell", oracle_mod, host, width=16, height=12, spp=1, max_depth=3)
    quad = next(sc.c.primitives[i] for i in range(sc.c.n_primitives) if sc.c.primitives[i].kind == abi.PRIM_QUAD)
    old = quad.data[10]
    for bad in (3.0e7, float("inf"), float("nan")):
        quad.data[10] = bad
        rc, msg = refusal(device, sc)
        assert rc == abi.ERR_INVALID and "quad normal" in msg, (bad, rc, msg)
    quad.data[10] = old
    assert refusal(device, sc)[0] == 0


# ---------------------------------------------------------------------------------------------------------------- the walk
def _mesh_prims(sc, prepared, abi):
    return [(i, sc.c.primitives[i].mesh, int(prepared.prims["node_begin"][i])) for i in range(sc.c.n_primitives) if sc.c.primitives[i].kind == abi.PRIM_MESH]


def _device_walk(dn, root, hit):
    """The kernels' walk over the two links: inner hit -> a; leaf hit -> its triangles, then the escape; miss -> the escape.  A node with
    infinite bounds (a chunk of a fat leaf) is hit by every ray.  Returns the device triangle indices in visit order."""
    out, i, steps = [], root, 0
    a, b, bmin, bmax = dn["a"], dn["b"], dn["bmin"], dn["bmax"]
    while i != NODE_END:
        assert i < len(dn) and steps <= len(dn), "the walk left the array or does not end"
        steps += 1
        count, escape = int(b[i]) >> NODE_LINK_BITS, int(b[i]) & NODE_END
        infinite = bool(np.all(np.isinf(bmin[i])) and np.all(np.isinf(bmax[i])))
        if not (infinite or hit(bmin[i].tobytes() + bmax[i].tobytes())):
            i = escape
        elif count == 0:
            i = int(a[i])
        else:
            out.extend(range(int(a[i]), int(a[i]) + count))
            i = escape
    return out


def _reference_walk(nodes, idx, hit):
    """Left-then-right recursion over the INPUT tree of one mesh (bvh.rs:142-156).  Returns the mesh's triangle ids in visit order."""
    out, stack = [], [0]
    while stack:
        n = nodes[stack.pop()]
        if not hit(n["bmin"].tobytes() + n["bmax"].tobytes()):
            continue
        if n["index_count"] > 0:
            out.extend(int(t) for t in idx[n["first_index"]:n["first_index"] + n["index_count"]])
        else:
            stack.append(int(n["right"])); stack.append(int(n["left"]))
    return out


@pytest.mark.parametrize("which", ["semesterbild", "teapot", "fat_leaf", "two_soups"])
def test_links_encode_the_left_then_right_walk(which, native, oracle_mod, abi):
    """Under one hit / miss choice per input node (keyed by the node's box, which both arrays carry bit for bit) the device walk and the
    recursion over the caller's tree visit the same triangles in the same order, every walk ends at NODE_END, and every DevTri is
    v0, v1 - v0, v2 - v0 and the normal of its triangle, in float32."""
    host, device = native
    sc = {"fat_leaf": lambda: fat_leaf_scene(abi, host), "two_soups": lambda: soup_scene(abi, host)}.get(which, lambda: shipped(which, oracle_mod, host))()
    got = device.prepare_scene(sc)
    nodes, idx, tris = inputs(sc)
    want_tri = np.concatenate([tris[:, 0:3], tris[:, 3:6] - tris[:, 0:3], tris[:, 6:9] - tris[:, 0:3], tris[:, 9:12]], axis=1)   # float32 throughout
    dev_tri = np.concatenate([got.tris[k] for k in ("v0", "e1", "e2", "n")], axis=1)
    assert dev_tri.dtype == want_tri.dtype == np.float32
    meshes = _mesh_prims(sc, got, abi)
    assert meshes
    if which == "fat_leaf":
        chunks = int(np.isinf(got.nodes["bmin"]).all(axis=1).sum())                               # the fat leaf became a chain of chunk leaves
        assert chunks == -(-sc.c.meshes[0].triangle_count // NODE_MAX_LEAF) >= 3
    if which == "two_soups":
        assert len(got.nodes) > LDS_NODE_CAP
    patterns = [("all hit", lambda box: True), ("all miss", lambda box: False)]
    for seed in (1, 2, 3):
        rng = np.random.default_rng(seed)
        choice = {}
        for n in nodes:
            choice.setdefault(n["bmin"].tobytes() + n["bmax"].tobytes(), bool(rng.random() < 0.7))
        patterns.append((f"random {seed}", choice.__getitem__))
    covered = np.zeros(len(dev_tri), bool)
    for name, hit in patterns:
        for _, m, root in meshes:
            mesh = sc.c.meshes[m]
            mn = nodes[mesh.first_node:mesh.first_node + mesh.node_count]
            mi = idx[mesh.first_index:mesh.first_index + mesh.index_count]
            want = [mesh.first_triangle + t for t in _reference_walk(mn, mi, hit)]
            have = _device_walk(got.nodes, root, hit)
            assert len(have) == len(want), (which, name, m, len(have), len(want))
            assert np.array_equal(dev_tri[have].view(np.uint32), want_tri[want].view(np.uint32)), (which, name, m)
            if name == "all hit":
                assert have == list(range(have[0], have[0] + len(have))), "triangles are stored in leaf-visit order"
                covered[have] = True
            if name == "all miss":
                assert not have
    assert covered.all(), "every device triangle is reached by the walk of some mesh primitive"


# ---------------------------------------------------------------------------------------------------------------- storage order
@pytest.mark.parametrize("which", ["semesterbild", "teapot", "two_soups"])
def test_nodes_are_stored_top_levels_first_then_subtrees_in_preorder(which, native, oracle_mod, abi):
    """The first LDS_NODE_CAP device nodes are the first nodes in (level, mesh, breadth-first) order; behind them every subtree lies in
    pre-order: an inner node's left child is the next index, its right child follows the whole left subtree."""
    host, device = native
    sc = soup_scene(abi, host) if which == "two_soups" else shipped(which, oracle_mod, host)
    got = device.prepare_scene(sc)
    nodes, _, _ = inputs(sc)
    dn = got.nodes
    c = sc.c
    roots = {m: root for _, m, root in _mesh_prims(sc, got, abi)}
    assert sorted(roots) == list(range(c.n_meshes)), "every mesh is used by a primitive in these scenes"
    total = sum(c.meshes[m].node_count for m in range(c.n_meshes))
    assert len(dn) == total, "no fat leaves here: one device node per input node"
    if which != "semesterbild":
        assert total > LDS_NODE_CAP
    dev_of, levels, size = {}, [], {}
    for m in range(c.n_meshes):
        mn = nodes[c.meshes[m].first_node:c.meshes[m].first_node + c.meshes[m].node_count]
        dev_of[(m, 0)] = roots[m]
        level, L = [0], 0
        while level:                                                  # breadth-first: the device index of a left child is its parent's `a`, a right
            if len(levels) <= L:                                      # child's its left sibling's escape
                levels.append([])
            levels[L] += [(m, n) for n in level]
            nxt = []
            for n in level:
                if mn[n]["index_count"] == 0:
                    left, right = int(mn[n]["left"]), int(mn[n]["right"])
                    dev_of[(m, left)] = int(dn["a"][dev_of[(m, n)]])
                    dev_of[(m, right)] = int(dn["b"][dev_of[(m, left)]]) & NODE_END
                    nxt += [left, right]
            level, L = nxt, L + 1
        for n in reversed([n for lv in levels for mm, n in lv if mm == m]):       # subtree sizes, children before parents
            size[(m, n)] = 1 if mn[n]["index_count"] > 0 else 1 + size[(m, int(mn[n]["left"]))] + size[(m, int(mn[n]["right"]))]
        for n in range(len(mn)):
            assert dn["bmin"][dev_of[(m, n)]].tobytes() == mn[n]["bmin"].tobytes() and dn["bmax"][dev_of[(m, n)]].tobytes() == mn[n]["bmax"].tobytes()
    assert sorted(dev_of.values()) == list(range(total))
    order = [key for lv in levels for key in lv]                       # level by level, mesh by mesh, breadth-first within
    head = min(total, LDS_NODE_CAP)
    assert [dev_of[key] for key in order[:head]] == list(range(head))
    checked = 0
    for (m, n), i in dev_of.items():
        mn = nodes[c.meshes[m].first_node:]
        if i >= LDS_NODE_CAP and mn[n]["index_count"] == 0:
            left, right = (m, int(mn[n]["left"])), (m, int(mn[n]["right"]))
            assert dev_of[left] == i + 1 and dev_of[right] == i + 1 + size[left], (m, n, i)
            checked += 1
    assert (checked > 0) == (total > LDS_NODE_CAP)


# ---------------------------------------------------------------------------------------------------------------- records
def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_primitive_records(native, oracle_mod, abi):
    host, device = native
    scenes = [shipped(n, oracle_mod, host) for n in ("cornell", "veach", "semesterbild", "teapot")] + [M._scene(abi, host, "mesh_transformed_nometal", 0)]
    kinds_seen = set()
    for sc in scenes:
        c = sc.c
        got = device.prepare_scene(sc)
        assert len(got.prims) == c.n_primitives
        kinds = [c.primitives[i].kind for i in range(c.n_primitives)]
        for i in range(c.n_primitives):
            p, d = c.primitives[i], got.prims[i]
            data = np.array(list(p.data), np.float32)
            kinds_seen.add(p.kind)
            assert (d["kind"], d["material"]) == (p.kind, p.material)
            assert d["mat0"].tobytes() == C.string_at(C.addressof(c.materials[p.material]), 16)
            end = i + 1
            while end < len(kinds) and kinds[end] == kinds[i]:
                end += 1
            assert d["run_end"] == end, "run_end: one past the maximal run of this kind"
            if p.kind == abi.PRIM_QUAD:
                assert np.array_equal(_bits(d["d"][0:4]), _bits(data[9:13])) and np.array_equal(_bits(d["d"][4:13]), _bits(data[0:9]))
                assert np.array_equal(_bits(d["d"][13:15]), _bits(data[13:15]))
            elif p.kind in (abi.PRIM_SPHERE, abi.PRIM_PLANE):
                assert np.array_equal(_bits(d["d"][0:32]), _bits(data))
            if p.kind == abi.PRIM_MESH:
                root = c.nodes[c.meshes[p.mesh].first_node]
                at = got.nodes[d["node_begin"]]
                assert at["bmin"].tobytes() == bytes(root.bmin) and at["bmax"].tobytes() == bytes(root.bmax)
                assert d["node_begin"] == p.mesh, "level 0 of every mesh comes first"
            else:
                assert d["node_begin"] == 0
    assert kinds_seen == set(range(5))


def _cube_record(data):
    """DevPrim::d of a cube from its primitive data (o2w, w2o column-major), op by op in float32 (rt_prepare.cpp: the matrix-shaped staging,
    cube_normal_table with the device's operation order: three products, two sums, plus zn; squared length, sqrt, one reciprocal, three products)."""
    o2w, w2o = data[0:16], data[16:32]
    zero, one, eps = f32(0.0), f32(1.0), f32(1e-4)
    d = np.zeros(52, np.float32)
    for col in range(4):
        for r in range(3):
            d[3 * col + r] = w2o[4 * col + r]
            d[16 + 3 * col + r] = o2w[4 * col + r]
    zn = [f32(w2o[4 * r + 3] * zero) for r in range(3)]
    for r in range(3):
        d[12 + r] = f32(w2o[12 + r] * zero)
        d[31 + r] = zn[r]
    for k in range(3):
        for sgn in range(2):
            n = [f32(0.0)] * 3
            n[k] = f32(-1.0) if sgn else f32(1.0)
            v = []
            for r in range(3):
                a, b, c = f32(w2o[4 * r + 0] * n[0]), f32(w2o[4 * r + 1] * n[1]), f32(w2o[4 * r + 2] * n[2])
                v.append(f32(f32(f32(a + b) + c) + zn[r]))
            l2 = f32(f32(f32(v[0] * v[0]) + f32(v[1] * v[1])) + f32(v[2] * v[2]))
            ln = f32(np.sqrt(l2))
            if not ln < eps:
                inv = f32(one / ln)
                v = [f32(x * inv) for x in v]
            d[34 + 3 * (2 * k + sgn):34 + 3 * (2 * k + sgn) + 3] = v
    return d


def test_cube_normal_table_bit_for_bit(native, abi):
    from oracle import scene_loader as L
    host, device = native
    ident = [f32(1.0) if k % 5 == 0 else f32(0.0) for k in range(16)]
    q = L.quat_from_euler_yxz_deg(f32(31.0), f32(-112.5), f32(7.25))
    m = L.mat4_from_scale_rotation_translation([f32(0.37), f32(1.9), f32(1.03)], q, [f32(-2.5), f32(0.75), f32(3.125)])
    mats = (abi.Material * 1)()
    mats[0].kind = abi.MAT_LAMBERT_SOLID
    prims = (abi.Primitive * 2)()
    for p, (o2w, w2o) in zip(prims, ((ident, ident), (m, L.mat4_inverse(m)))):
        p.kind, p.material = abi.PRIM_CUBE, 0
        p.data[0:16] = [float(v) for v in o2w]
        p.data[16:32] = [float(v) for v in w2o]
    sc = abi.Scene()
    sc.primitives, sc.n_primitives, sc.materials, sc.n_materials = prims, 2, mats, 1
    got = device.prepare_scene(sc)
    for i in range(2):
        want = _cube_record(np.array(list(prims[i].data), np.float32))
        assert np.array_equal(_bits(got.prims["d"][i]), _bits(want)), (i, got.prims["d"][i][34:52], want[34:52])
    table = got.prims["d"][0][34:52].reshape(6, 3)
    assert np.array_equal(table, np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32))
    lengths = np.linalg.norm(got.prims["d"][1][34:52].reshape(6, 3).astype(np.float64), axis=1)
    assert np.all(np.abs(lengths - 1.0) < 1e-6)


# ---------------------------------------------------------------------------------------------------------------- the variant
def test_shipped_scenes_choose_their_kernels(native, oracle_mod, abi):
    """Before any probe (set_scene may still send veach-mis back to a lockstep kernel when its paths scatter too little)."""
    host, device = native
    for name, variant in (("cornell", 14), ("teapot", 12), ("semesterbild", 13), ("veach", 11)):
        assert device.prepare_scene(shipped(name, oracle_mod, host)).variant == variant, name


def test_inline_steps_follow_the_number_of_mesh_primitives(native, oracle_mod, abi):
    host, device = native
    scenes = [shipped(n, oracle_mod, host) for n in ("cornell", "teapot", "semesterbild", "veach")] + [M._scene(abi, host, fam, M.SEEDS[0]) for fam in M.FAMILIES]
    seen = set()
    for sc in scenes + [fat_leaf_scene(abi, host)]:
        n_mesh = sum(sc.c.primitives[i].kind == abi.PRIM_MESH for i in range(sc.c.n_primitives))
        seen.add(min(n_mesh, 2))
        assert device.prepare_scene(sc).inline_steps == (1 if n_mesh >= 2 else 0), n_mesh
    assert seen == {0, 1, 2}


@pytest.mark.parametrize("fam", list(M.FAMILIES))
def test_forced_variants_follow_the_capability_table(fam, native, abi):
    """Forcing v on the product library keeps v exactly where the table says it accepts the scene (and the library holds it)."""
    host, device = native
    sc = M._scene(abi, host, fam, M.SEEDS[0])
    f = M.planned_features(fam)
    auto = device.prepare_scene(sc).variant
    for v in range(15):
        got = device.prepare_scene(sc, v).variant
        ok = v in M.CAPABILITY and M.accepts(v, f) and M.CAPABILITY[v][1] == "product"
        assert (got == v) == ok, (fam, v, got)
        assert ok or got == auto, "a refused force leaves the automatic choice"
    for v in (-2, 15):
        with pytest.raises(device.RenderError):
            device.prepare_scene(sc, v)


# ---------------------------------------------------------------------------------------------------------------- source and build
def test_the_unit_is_free_of_hip_and_built_once():
    for name in ("rt_prepare.cpp", "rt_prepare.h"):
        assert "#include <hip" not in open(os.path.join(ROOT, "raytracer-rust_amd/csrc/device", name)).read(), name
    build = importlib.import_module("raytracer-rust_amd.build")
    assert [os.path.basename(s) for s in build.DEVICE_SRCS].count("rt_prepare.cpp") == 1
