"""GPU parity: HIP path (through the C ABI) vs the CPU oracle on identical inputs, same RNG mode.

Tolerances (restated in DESIGN.md section 5; tests/parity.py asserts them):
  * scenes whose path uses only + - * / sqrt (cornell, teapot): linear RGB must be BIT-IDENTICAL;
  * scenes with RoughConductor (logf/atanf/sinf/cosf: device libm differs from glibc by ulps, which can
    flip a branch for isolated samples): at most ceil(1e-4 N) of the N pixels with per-pixel L2 > 1e-3,
    at most ceil(1e-3 N) 8-bit pixels that differ, image means within 2e-3.
"""
import numpy as np
import pytest

from conftest import load_for_both
from parity import assert_parity

pytestmark = pytest.mark.gpu

CASES = [  # name, W, H, spp, depth, exact
    ("cornell", 80, 60, 8, 4, True),
    ("cornell", 64, 48, 4, 30, True),
    ("teapot", 64, 48, 4, 16, True),
    ("veach", 96, 54, 8, 16, False),
    ("semesterbild", 80, 60, 8, 30, False),
]


def _compare(gl, ol, gp, op, exact):
    assert_parity(gp, gl, op, ol, exact=exact)


@pytest.mark.parametrize("name,W,H,spp,depth,exact", CASES)
def test_ctr_mode_matches_oracle(name, W, H, spp, depth, exact, native, oracle_mod, abi):
    host, device = native
    sc = load_for_both(name, oracle_mod, host, width=W, height=H, spp=spp, max_depth=depth)
    opt = abi.Options.make(rng_mode=abi.RNG_CTR)
    gp, gl, st = device.render(sc, sc.camera, sc.settings, opt)
    op, ol, cnt = oracle_mod.render(sc, sc.camera, sc.settings, opt)
    assert st.samples == W * H * spp == cnt.samples
    if exact:
        assert st.rays == cnt.rays
    _compare(gl, ol, gp, op, exact)


@pytest.mark.parametrize("name,W,H,spp,depth,exact", [("cornell", 40, 30, 4, 6, True), ("semesterbild", 64, 48, 8, 30, True), ("veach", 64, 36, 8, 16, True)])
def test_ref_mode_replays_reference_stream(name, W, H, spp, depth, exact, native, oracle_mod, abi):
    """MI355RT_RNG_REF: per-row StdRng::seed_from_u64(y) stream (renderer.rs:91), tail-first folding.  In this mode the microfacet
    sampling's ln / atan / sin / cos are evaluated in double and rounded once on BOTH sides (rt_materials.h, oracle SamplerRef), so
    the scenes with rough conductors are bit-identical too, not only the + - * / sqrt ones."""
    host, device = native
    sc = load_for_both(name, oracle_mod, host, width=W, height=H, spp=spp, max_depth=depth)
    opt = abi.Options.make(rng_mode=abi.RNG_REF)
    gp, gl, st = device.render(sc, sc.camera, sc.settings, opt)
    op, ol, cnt = oracle_mod.render(sc, sc.camera, sc.settings, opt)
    _compare(gl, ol, gp, op, exact)


def test_tiling_is_bit_invariant(native, oracle_mod, abi):
    """Any row selection / strip interleave / workspace banding must give the same pixels (RNG keyed by absolute y)."""
    host, device = native
    sc = load_for_both("cornell", oracle_mod, host, width=64, height=48, spp=4, max_depth=8)
    full, full_lin, _ = device.render(sc, sc.camera, sc.settings, abi.Options.make())
    # 3 interleaved parts of 4-row strips
    out = np.zeros_like(full)
    for part in range(3):
        opt = abi.Options.make(strip_rows=4, n_parts=3, part=part)
        p, _, _ = device.render(sc, sc.camera, sc.settings, opt)
        out[abi.rows_selected(48, opt)] = p
    assert np.array_equal(out, full)
    # a row window
    opt = abi.Options.make(row_begin=10, row_end=31)
    p, l, _ = device.render(sc, sc.camera, sc.settings, opt)
    assert np.array_equal(p, full[10:31]) and np.array_equal(l.view(np.uint32), full_lin[10:31].view(np.uint32))
    # tiny workspace -> many bands (one band = 3 pixels)
    opt = abi.Options.make(workspace_bytes=3 * 4 * 12)      # 4 spp x 12 B per sample x 3 pixels
    p, l, st = device.render(sc, sc.camera, sc.settings, opt)
    assert st.bands == (64 * 48 + 2) // 3
    assert np.array_equal(p, full) and np.array_equal(l.view(np.uint32), full_lin.view(np.uint32))


@pytest.mark.parametrize("W,H,spp", [(37, 5, 3), (1, 9, 7), (129, 3, 1), (64, 2, 255), (5, 5, 1000)])
def test_odd_sizes_decode_exactly(W, H, spp, native, oracle_mod, abi):
    """Sample index -> (pixel, sample, row, x) uses magic-number division on the device; widths / spp that are
    not powers of two, single columns and spp > run length must still match the oracle bit-for-bit."""
    host, device = native
    sc = load_for_both("cornell", oracle_mod, host, width=W, height=H, spp=spp, max_depth=5)
    opt = abi.Options.make()
    gp, gl, st = device.render(sc, sc.camera, sc.settings, opt)
    op, ol, cnt = oracle_mod.render(sc, sc.camera, sc.settings, opt)
    assert st.samples == W * H * spp and st.rays == cnt.rays
    assert np.array_equal(gl.view(np.uint32), ol.view(np.uint32)) and np.array_equal(gp, op)


@pytest.fixture
def knobs(native):
    """Diagnostic knobs (mi355rt_debug_set_knob) as process-wide defaults of the product and the reference library, cleared afterwards."""
    _, device = native
    libs = []

    def use(library=None, **kv):
        L = library or device.lib()
        if L not in libs:
            libs.append(L)
        device.clear_knobs(L)
        for k, v in kv.items():
            device.set_knob(k, v, L)
    yield use
    for L in libs:
        device.clear_knobs(L)


@pytest.mark.parametrize("name", ["teapot", "semesterbild"])
def test_mesh_kernels_equal_the_lockstep_walk(name, native, oracle_mod, abi, knobs):
    """Every generation of the mesh path performs the same arithmetic per ray: the product's wavefront kernel (automatic choice), its
    per-lane fallback loop k_render_ctr_mesh, and -- from the tests' reference build (-DMI355RT_REFS), where it was retired to --
    the wave-scheduled state machine (any trav_min, with and without its inline root test) must be bit-identical to each other,
    and identical to the oracle where the path is exact.  (Round 2's LDS walk pool was a fourth reference until round 5: it reported
    a stall once whose cause was never established, and a test that renders again after such a report forgives what nobody can explain;
    the kernel was removed rather than retried -- DESIGN.md 4.1d.)"""
    host, device = native
    R = device.refs()
    assert not device.lib().mi355rt_debug_has_variant(2)                     # retired from the product library
    assert R.mi355rt_debug_has_variant(2) and not R.mi355rt_debug_has_variant(5) and not R.mi355rt_debug_has_variant(6)     # (5 / 6 were the walk pool: in no library)
    sc = load_for_both(name, oracle_mod, host, width=96, height=64, spp=6, max_depth=12)
    ctx = device.Context(0)
    ctx.set_scene(sc, sc.camera, sc.settings)
    # neither scene has a metal: the wavefront kernel without that branch is the automatic choice -- for teapot, whose two meshes are untransformed,
    # in the instantiation that skips mesh_setup's matrix products (12); forcing 10 / 7 on it runs the general forms, which must agree bit for bit
    assert ctx.kernel_variant() == (12 if name == "teapot" else 13)          # (13: the text mesh's tree is small -- 3 351 nodes -- so the instantiation with the shorter WALK rounds)
    ctx.close()
    if name == "semesterbild":                             # its mesh is rotated: the form for untransformed meshes must be refused, not run
        knobs(None, kernel=12)
        ctx = device.Context(0); ctx.set_scene(sc, sc.camera, sc.settings); assert ctx.kernel_variant() == 13; ctx.close()
    outs = []
    for library, kv in ((None, {"kernel": 1}), (None, {}), (None, {"kernel": 7}), (None, {"kernel": 10}), (None, {"kernel": 13}),
                        (R, {"kernel": 1}), (R, {"kernel": 7}),
                        (R, {"kernel": 2, "trav_min": 1}), (R, {"kernel": 2, "trav_min": 64}), (R, {"kernel": 2}), (R, {"kernel": 2, "inline_steps": 0})):
        knobs(library, **kv)
        gp, gl, st = device.render(sc, sc.camera, sc.settings, abi.Options.make(), library=library)     # a kernel watchdog fails the test, once, with its message: no second render
        outs.append((gp, gl, st.rays))
    for i, (gp, gl, rays) in enumerate(outs[1:], 1):
        assert np.array_equal(gl.view(np.uint32), outs[0][1].view(np.uint32)) and np.array_equal(gp, outs[0][0]) and rays == outs[0][2], f"configuration {i}"
    if name == "teapot":
        op, ol, cnt = oracle_mod.render(sc, sc.camera, sc.settings, abi.Options.make())
        assert np.array_equal(outs[0][1].view(np.uint32), ol.view(np.uint32)) and cnt.rays == outs[0][2]


def test_simple_material_kernel_equals_general(native, oracle_mod, abi, knobs):
    """cornell has only Lambertian / Emissive materials, so set_scene picks the instantiation with the other BSDFs
    compiled out.  It must be bit-identical to the general lockstep kernel and to the oracle, and must NOT be
    picked (nor be forceable) for a scene that has any other material."""
    import torch
    host, device = native

    def run(sc):
        ctx = device.Context(0)
        ctx.set_scene(sc, sc.camera, sc.settings)
        n = sc.settings.width * sc.settings.height
        packed = torch.zeros(n, dtype=torch.int32, device="cuda")
        linear = torch.zeros(n * 3, dtype=torch.float32, device="cuda")
        st = ctx.render(packed.data_ptr(), linear.data_ptr(), abi.Options.make(), want_stats=True)
        v = ctx.kernel_variant()
        ctx.close()
        return v, packed.cpu().numpy().view(np.uint32), linear.cpu().numpy(), st.rays

    sc = load_for_both("cornell", oracle_mod, host, width=80, height=48, spp=9, max_depth=12)
    knobs()
    v, gp, gl, rays = run(sc)
    knobs(kernel=0)
    v0, gp0, gl0, rays0 = run(sc)
    knobs(kernel=3)                                       # the Lambert-only kernel for any primitive kinds
    v3, gp3, gl3, rays3 = run(sc)
    assert (v, v0, v3) == (14, 0, 3), "the simple-materials instantiation (pruned to quads and cubes: cornell holds nothing else) was not selected for cornell"
    assert np.array_equal(gl.view(np.uint32), gl0.view(np.uint32)) and np.array_equal(gp, gp0) and rays == rays0
    assert np.array_equal(gl.view(np.uint32), gl3.view(np.uint32)) and np.array_equal(gp, gp3) and rays == rays3
    op, ol, cnt = oracle_mod.render(sc, sc.camera, sc.settings, abi.Options.make())
    assert np.array_equal(gl.view(np.uint32), ol.reshape(-1).view(np.uint32)) and cnt.rays == rays

    # veach-mis has Lambert + Emissive + Beckmann conductors: a mesh-free list whose shading step diverges expensively (rough conductor
    # next to a diffuse material) -> the mesh-free instantiation of the wavefront kernel (11: material-sorted SHADE passes, no metal /
    # dielectric branch).  It must equal the lockstep kernels -- the general one (0) and the one without metal / dielectric (9) -- bit for
    # bit, and the Lambert-only kernel (3) must be refused.
    sv = load_for_both("veach", oracle_mod, host, width=80, height=48, spp=4, max_depth=8)
    knobs()
    vv, vp, vl, vr = run(sv)
    knobs(kernel=3)                                       # refused: the scene has RoughConductor materials
    vv3, _, vl3, _ = run(sv)
    knobs(kernel=0)
    vv0, vp0, vl0, vr0 = run(sv)
    knobs(kernel=9)
    vv9, vp9, vl9, vr9 = run(sv)
    assert (vv, vv3, vv0, vv9) == (11, 11, 0, 9)
    assert np.array_equal(vl.view(np.uint32), vl3.view(np.uint32))
    assert np.array_equal(vl.view(np.uint32), vl0.view(np.uint32)) and np.array_equal(vp, vp0) and vr == vr0
    assert np.array_equal(vl.view(np.uint32), vl9.view(np.uint32)) and np.array_equal(vp, vp9) and vr == vr9
    # a scene with a metal in it is refused by the pruned instantiation
    from fuzz_scenes import random_scene
    sm = random_scene(abi, host, 31, exact_only=True, n_prims=16, only_kinds=[2, 2, 3, 0, 1, 3, 3, 0, 0, 2, 1, 1])
    sm.settings = abi.Settings(40, 30, 3, 6)
    kinds = {sm.c.materials[sm.c.primitives[i].material].kind for i in range(sm.c.n_primitives)}
    assert abi.MAT_METAL in kinds or abi.MAT_DIELECTRIC in kinds
    knobs(kernel=9)
    assert run(sm)[0] == 0
    knobs(kernel=11)
    assert run(sm)[0] == 0
    # ... the instantiation pruned to quads and cubes is refused for a list that holds a sphere (and is not picked for it)
    ss = random_scene(abi, host, 33, exact_only=True, n_prims=9, only_kinds=[2, 3, 0], lambert_only=True)
    ss.settings = abi.Settings(40, 30, 3, 6)
    knobs()
    assert run(ss)[0] == 3
    knobs(kernel=14)
    assert run(ss)[0] == 3
    # ... and a mesh-free wavefront kernel is refused for a list with a mesh
    st = load_for_both("teapot", oracle_mod, host, width=48, height=32, spp=2, max_depth=4)
    knobs(kernel=11)
    assert run(st)[0] == 12                                # (teapot's automatic choice: untransformed meshes)


def test_fixed_wo3_reader_scene_is_bit_identical_to_the_oracle(native, oracle_mod, abi):
    """Opt-in loader fix (4 u32 per WO3 triangle): a different triangle set through the same kernels -- the whole teapot."""
    from oracle import scene_loader
    from conftest import SCENES
    host, device = native
    sc = scene_loader.load_scene(SCENES["teapot"], skip_unknown_primitives=True, wo3_four_index_stride=True, width=80, height=60, spp=4, max_depth=12)
    sc._keep = host.attach_bvh(sc)
    gp, gl, st = device.render(sc, sc.camera, sc.settings, abi.Options.make())
    op, ol, cnt = oracle_mod.render(sc, sc.camera, sc.settings, abi.Options.make())
    assert st.rays == cnt.rays and np.array_equal(gl.view(np.uint32), ol.view(np.uint32)) and np.array_equal(gp, op)


def test_texture_material_scene_matches_the_oracle(native, oracle_mod, abi):
    """TextureMaterial (tungsten/parser.rs:199-243) through the ABI: no loader path of the reference produces it, a host that builds
    its scene in code can.  A textured sphere on a textured quad under the grey sky, GPU against the oracle in counter mode:
    acos / atan2 pick the texel, so isolated samples may land on the neighbouring texel (stated tolerance as for the microfacet BSDFs)."""
    import ctypes as C
    host, device = native
    rng = np.random.default_rng(4)
    rgba = rng.integers(0, 256, (16, 32, 4), dtype=np.uint8)
    small = np.array([[[255, 0, 0, 255], [0, 255, 0, 255]], [[0, 0, 255, 255], [255, 255, 255, 255]]], np.uint8)
    texs = (abi.Texture * 2)(abi.Texture(rgba.ctypes.data_as(C.POINTER(C.c_uint8)), 32, 16), abi.Texture(small.ctypes.data_as(C.POINTER(C.c_uint8)), 2, 2))
    mats = (abi.Material * 2)()
    mats[0].kind = abi.MAT_TEXTURE; mats[0].albedo[:] = (1.0, 0.9, 0.8); mats[0].p0 = 0.25; mats[0].texture = 0
    mats[1].kind = abi.MAT_TEXTURE; mats[1].albedo[:] = (0.7, 0.7, 0.7); mats[1].p0 = 0.0; mats[1].texture = 1
    prims = (abi.Primitive * 2)()
    prims[0].kind = abi.PRIM_SPHERE; prims[0].material = 0; prims[0].data[0:4] = [0.0, 0.0, 0.0, 1.0]
    prims[1].kind = abi.PRIM_SPHERE; prims[1].material = 1; prims[1].data[0:4] = [0.0, -101.0, 0.0, 100.0]
    sc = abi.Scene()
    sc.primitives, sc.n_primitives, sc.materials, sc.n_materials, sc.textures, sc.n_textures = prims, 2, mats, 2, texs, 2
    sc.miss_color[:] = (0.5, 0.5, 0.5)
    cam = abi.Camera()
    cam.position[:] = (0, 0.5, 4); cam.forward[:] = (0, -0.1240, -0.9923); cam.right[:] = (1, 0, 0); cam.true_up[:] = (0, 0.9923, -0.1240)
    cam.half_width, cam.half_height = 0.5, 0.375
    st = abi.Settings(96, 72, 16, 6)
    gp, gl, gs = device.render(sc, cam, st, abi.Options.make())
    op, ol, cnt = oracle_mod.render(sc, cam, st, abi.Options.make())
    assert_parity(gp, gl, op, ol, exact=False, gpu_rays=gs.rays, oracle_rays=cnt.rays)
    # refused: a texture index beyond the table
    mats[1].texture = 5
    with pytest.raises(device.RenderError):
        device.render(sc, cam, st, abi.Options.make())


@pytest.mark.parametrize("kernel", [7, 2, 1])
def test_caller_built_bvh_with_fat_leaves(kernel, native, oracle_mod, abi, knobs):
    """The BVH crosses the ABI in the reference's shape, so a caller may hand over any tree -- also leaves with more triangles than
    the device's 6-bit leaf count holds.  Such a leaf keeps its box test as an inner node in front of a chain of chunk leaves with
    infinite bounds (rt_prepare.cpp, flatten_meshes).  One mesh of 150 triangles under (a) the tree the host builder makes, (b) ONE leaf
    holding all 150, (c) a root over a 100-triangle and a 50-triangle leaf: each must match the oracle walking the SAME tree, bit for
    bit, in every mesh kernel.  (The trees need not agree with each other: a tight child box can reject a grazing hit its parent
    box lets through, reference behaviour that both sides reproduce.)"""
    import ctypes as C
    from fuzz_scenes import random_scene
    host, device = native
    library = device.refs() if kernel == 2 else None                   # the state machine lives in the reference build
    knobs(library, kernel=kernel)
    st = abi.Settings(48, 36, 4, 6)
    keep = []                                                           # ctypes arrays the scene points into

    def scene():
        return random_scene(abi, host, 77, exact_only=True, n_prims=6, mesh_tris=150, only_kinds=[abi.PRIM_MESH, abi.PRIM_QUAD, abi.PRIM_SPHERE])

    def both(sc):
        got = device.render(sc, sc.camera, st, abi.Options.make(), library=library)
        op, ol, cnt = oracle_mod.render(sc, sc.camera, st, abi.Options.make())
        assert np.array_equal(got[1].view(np.uint32), ol.view(np.uint32)) and np.array_equal(got[0], op)
        return got

    base = both(scene())

    def with_tree(make_nodes, idx_of):
        sc = scene()
        c = getattr(sc, "c", sc)
        assert c.n_meshes >= 1
        mesh = c.meshes[0]
        n = mesh.triangle_count
        assert n > 63
        root = c.nodes[mesh.first_node]
        nodes, idx = make_nodes(list(root.bmin), list(root.bmax), n), idx_of(n)
        others_nodes = [c.nodes[i] for i in range(c.n_nodes)]
        others_idx = [c.tri_indices[i] for i in range(c.n_tri_indices)]
        all_nodes = (abi.BvhNode * (len(others_nodes) + len(nodes)))(*others_nodes, *nodes)
        all_idx = (C.c_uint32 * (len(others_idx) + len(idx)))(*others_idx, *idx)
        keep.extend([sc, all_nodes, all_idx])
        c.nodes, c.n_nodes = C.cast(all_nodes, C.POINTER(abi.BvhNode)), len(all_nodes)
        c.tri_indices, c.n_tri_indices = C.cast(all_idx, C.POINTER(C.c_uint32)), len(all_idx)
        mesh.first_node, mesh.node_count, mesh.first_index, mesh.index_count = len(others_nodes), len(nodes), len(others_idx), len(idx)
        return both(sc)

    def node(bmin, bmax, left=0, right=0, first=0, count=0):
        b = abi.BvhNode(); b.bmin[:] = bmin; b.bmax[:] = bmax; b.left, b.right, b.first_index, b.index_count = left, right, first, count
        return b

    one_leaf = with_tree(lambda lo, hi, n: [node(lo, hi, first=0, count=n)], lambda n: list(range(n)))
    two = with_tree(lambda lo, hi, n: [node(lo, hi, left=1, right=2), node(lo, hi, first=0, count=100), node(lo, hi, first=100, count=n - 100)],
                    lambda n: list(range(n)))
    # the mesh is visible at all: the images are not just sky, and the three trees give practically the same picture
    assert np.abs(one_leaf[1] - base[1]).mean() < 1e-3 and np.abs(two[1] - base[1]).mean() < 1e-3


def test_untransformed_mesh_form_and_its_fallback_for_rays_with_zero_components(native, oracle_mod, abi, knobs):
    """k_render_ctr_wf_nometal_ident (variant 12) replaces mesh_setup's matrix products by the ray itself where every mesh of the list is untransformed --
    exact only for rays without a zero or non-finite component (rt_intersect.h ray_nonzero_finite), so a wave that holds such a ray takes the general
    form.  A camera ON the plane x = 0 makes every primary ray start at x == 0 (general form), while the bounced rays take the short form: both forms
    inside one render, and the image must be the oracle's and the general kernel's, bit for bit (mesh_object.rs:264-291)."""
    from oracle import scene_loader as L
    host, device = native
    F = np.float32
    sc = load_for_both("teapot", oracle_mod, host, width=72, height=54, spp=5, max_depth=10)
    sc.camera = L.camera_new((0.0, 2.0, 9.0), (0.0, 1.0, 0.0), (0.0, 1.0, 0.0), F(45.0), F(72 / 54))
    outs = []
    for kv in ({}, {"kernel": 10}, {"kernel": 7}, {"kernel": 1}):
        knobs(None, **kv)
        ctx = device.Context(0); ctx.set_scene(sc, sc.camera, sc.settings)
        assert ctx.kernel_variant() == kv.get("kernel", 12)
        ctx.close()
        outs.append(device.render(sc, sc.camera, sc.settings, abi.Options.make()))
    op, ol, cnt = oracle_mod.render(sc, sc.camera, sc.settings, abi.Options.make())
    assert cnt.rays > 1.2 * cnt.samples                                          # the view does hit the meshes and bounce
    for gp, gl, st in outs:
        assert st.rays == cnt.rays and np.array_equal(gl.view(np.uint32), ol.view(np.uint32)) and np.array_equal(gp, op)
