"""The camera masks of k_render_ctr_simple_qc (csrc/device/rt_prepare.cpp build_camera_masks, through mi355rt_debug_camera_masks): no GPU.

A clear bit makes the kernel's camera pass skip a primitive, so the one property that matters is that a clear bit is never wrong: wherever the
oracle's own hit test accepts a camera ray of a pixel on primitive i alone, bit i of that pixel is set.  The rays are formed as the device forms
them (u = (x + ju) / W in f32, camera_raw's operation order; the oracle's Ray::new normalises twice).  Where the bit is set the property holds
trivially, so the oracle is asked only about pixels whose bit is clear: every such pixel within two pixels of the footprint with all 32 jitter
pairs -- the four corners and edges of the jitter square, 0 / 2^-24 / 0.5 / 1 - 2^-24 in both axes, and 16 random pairs --, every other one with one
random pair.  The second property is that the masks cull at all (the caps of test_cornell_masks_are_not_vacuous)."""
import ctypes as C
import importlib
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_for_both
from fuzz_scenes import random_scene

F = np.float32
EDGE = [0.0, 2.0 ** -24, 0.5, 1.0 - 2.0 ** -24]
_rng = np.random.default_rng(20240611)
JITTER = np.array([(a, b) for a in EDGE for b in EDGE] + [tuple(v) for v in _rng.random((16, 2))], np.float32)       # 32 pairs in [0, 1)


def camera_raw(cam, W, H, x, y, ju, jv):
    """The camera ray's direction before its normalisations, f32 operation by operation as rt_kernels.hip HitStock::camera + rt_materials.h camera_raw."""
    u = (x.astype(F) + ju.astype(F)) / F(W)
    v = (y.astype(F) + jv.astype(F)) / F(H)
    ndc_x = F(2.0) * u - F(1.0)
    ndc_y = F(1.0) - F(2.0) * v
    sx, sy = ndc_x * F(cam.half_width), ndc_y * F(cam.half_height)
    out = np.empty((len(u), 3), F)
    for k in range(3):
        out[:, k] = F(cam.forward[k]) + (F(cam.right[k]) * sx + F(cam.true_up[k]) * sy)
    return out


def one_primitive_scene(abi, sc, i):
    c = getattr(sc, "c", sc)
    one = abi.Scene()
    C.pointer(one)[0] = c
    one.primitives = C.cast(C.addressof(c.primitives[i]), C.POINTER(abi.Primitive))
    one.n_primitives = 1
    return one


def dilate(b, r):
    out = b.copy()
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            s = np.zeros_like(b)
            ys, xs = slice(max(dy, 0), b.shape[0] + min(dy, 0)), slice(max(dx, 0), b.shape[1] + min(dx, 0))
            yd, xd = slice(max(-dy, 0), b.shape[0] + min(-dy, 0)), slice(max(-dx, 0), b.shape[1] + min(-dx, 0))
            s[yd, xd] = b[ys, xs]
            out |= s
    return out


def culled_hits(abi, oracle_mod, sc, cam, W, H, masks, rows=None, all_jitters_everywhere=False):
    """[(primitive, x, y, ju, jv)] of camera rays the oracle accepts on a primitive whose bit is clear in the ray's pixel; how many rays were asked."""
    L = oracle_mod.lib()
    c = getattr(sc, "c", sc)
    origin = np.array(list(cam.position), F)
    out9 = np.zeros(9, F)
    o_ptr, out_ptr = origin.ctypes.data, out9.ctypes.data
    bad, asked = [], 0
    rng = np.random.default_rng(7)
    yy, xx = np.mgrid[0:H, 0:W]
    row_sel = np.ones((H, W), bool) if rows is None else np.isin(yy, list(rows))
    for i in range(c.n_primitives):
        one = one_primitive_scene(abi, sc, i)
        ref = C.byref(one)
        is_set = ((masks >> np.uint32(i)) & np.uint32(1)).astype(bool)
        clear = ~is_set & row_sel
        near = clear if all_jitters_everywhere else (dilate(is_set, 2) & clear)
        far = clear & ~near
        xs = np.concatenate([np.repeat(xx[near], len(JITTER)), xx[far]])
        ys = np.concatenate([np.repeat(yy[near], len(JITTER)), yy[far]])
        j = np.concatenate([np.tile(JITTER, (int(near.sum()), 1)), rng.random((int(far.sum()), 2)).astype(F)]).reshape(-1, 2)
        if len(xs) == 0:
            continue
        d = np.ascontiguousarray(camera_raw(cam, W, H, xs, ys, j[:, 0], j[:, 1]))
        base = d.ctypes.data
        hit = L.oracle_scene_hit
        for k in range(len(xs)):
            rc = hit(ref, o_ptr, base + 12 * k, out_ptr)
            assert rc >= 0
            if rc == 1:
                bad.append((i, int(xs[k]), int(ys[k]), float(j[k, 0]), float(j[k, 1])))
        asked += len(xs)
    return bad, asked


_scenes = {}


def cornell(oracle_mod, host, W, H):
    if (W, H) not in _scenes:
        _scenes[(W, H)] = load_for_both("cornell", oracle_mod, host, width=W, height=H, spp=1, max_depth=3)
    return _scenes[(W, H)]


def test_never_culls_a_hit_cornell_small_every_pixel(native, oracle_mod, abi):
    host, device = native
    sc = cornell(oracle_mod, host, 80, 60)
    masks = device.camera_masks(sc, sc.camera, sc.settings)
    assert masks is not None and masks.shape == (60, 80)
    bad, asked = culled_hits(abi, oracle_mod, sc, sc.camera, 80, 60, masks)
    assert asked > 8 * 2000 and not bad, bad[:10]


def test_never_culls_a_hit_cornell_full_size_rows(native, oracle_mod, abi):
    """800 x 600 on twelve rows: the light's first and last rows and the rows just outside them, each cube's top row and a row through its middle,
    the back wall's first and last rows and the rows just outside (its corners)."""
    host, device = native
    sc = cornell(oracle_mod, host, 800, 600)
    masks = device.camera_masks(sc, sc.camera, sc.settings)
    c = sc.c
    area = [int(((masks >> np.uint32(i)) & 1).sum()) for i in range(c.n_primitives)]
    extent = []
    for i in range(c.n_primitives):
        ys = np.nonzero(((masks >> np.uint32(i)) & 1).any(axis=1))[0]
        extent.append((int(ys[0]), int(ys[-1])))
    quads = [i for i in range(c.n_primitives) if c.primitives[i].kind == abi.PRIM_QUAD]
    cubes = [i for i in range(c.n_primitives) if c.primitives[i].kind == abi.PRIM_CUBE]
    light = [i for i in quads if c.materials[c.primitives[i].material].kind == abi.MAT_EMISSIVE]
    assert len(cubes) == 2 and len(light) == 1
    back = max(quads, key=lambda i: area[i])
    rows = set()
    for i in (light[0], back):
        rows |= {extent[i][0] - 1, extent[i][0], extent[i][1], extent[i][1] + 1}
    for i in cubes:
        rows |= {extent[i][0], (extent[i][0] + extent[i][1]) // 2}
    rows = {y for y in rows if 0 <= y < 600}
    assert len(rows) == 12, sorted(rows)
    bad, asked = culled_hits(abi, oracle_mod, sc, sc.camera, 800, 600, masks, rows=rows)
    assert asked > 8 * 2000 and not bad, bad[:10]


@pytest.mark.parametrize("seed", range(8))
def test_never_culls_a_hit_fuzz_scenes(native, oracle_mod, abi, seed):
    host, device = native
    sc = random_scene(abi, host, 100 + seed, exact_only=True, n_prims=8, only_kinds=[abi.PRIM_QUAD, abi.PRIM_CUBE], lambert_only=True)
    st = abi.Settings(64, 48, 1, 3)
    assert device.prepare_scene(sc).variant == 14
    masks = device.camera_masks(sc, sc.camera, st)
    assert masks is not None and masks.shape == (48, 64)
    bad, asked = culled_hits(abi, oracle_mod, sc, sc.camera, 64, 48, masks)
    assert not bad, bad[:10]
    assert asked > 2000 and int((masks == 0).sum()) > 0                              # (the scenes leave sky around their primitives: something is culled)


# ------------------------------------------------------------------------------------------------------------ hand-made cases
def hand_scene(abi, prims):
    from oracle import scene_loader as L
    sc = L.LoadedScene()
    m = abi.Material(); m.kind = abi.MAT_LAMBERT_SOLID; m.albedo[:] = [0.5, 0.5, 0.5]
    sc.materials, sc.primitives = [m], prims
    sc.finalize()
    return sc


def quad_prim(abi, scale, euler, trans):
    from oracle import scene_loader as L
    m = L.mat4_from_scale_rotation_translation([F(v) for v in scale], L.quat_from_euler_yxz_deg(*[F(v) for v in euler]), [F(v) for v in trans])
    p = abi.Primitive(); p.kind = abi.PRIM_QUAD; p.material = 0
    p.data[0:15] = [float(v) for v in L.quad_from_matrix(m)]
    return p


def cube_prim(abi, scale, euler, trans):
    from oracle import scene_loader as L
    m = L.mat4_from_scale_rotation_translation([F(v) for v in scale], L.quat_from_euler_yxz_deg(*[F(v) for v in euler]), [F(v) for v in trans])
    p = abi.Primitive(); p.kind = abi.PRIM_CUBE; p.material = 0
    with np.errstate(all="ignore"):
        p.data[0:16] = [float(v) for v in m]; p.data[16:32] = [float(v) for v in L.mat4_inverse(m)]
    return p


def hand_camera():
    from oracle import scene_loader as L
    return L.camera_new((0.0, 0.0, 5.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), F(50.0), F(4.0 / 3.0))


HAND_W, HAND_H = 32, 24
# name -> (how the primitive is made, what the whole table must be: "ones" = kept everywhere, "zero" = culled everywhere, None = neither is required)
HAND = {
    "quad_crossing_the_camera_plane": (lambda abi: quad_prim(abi, (4, 1, 12), (0, 0, 0), (0, -1, 3)), "ones"),       # the floor runs from z = -3 to z = 9, under the camera at z = 5
    "camera_inside_a_cube": (lambda abi: cube_prim(abi, (6, 6, 6), (10, 20, 30), (0, 0, 4)), "ones"),
    "quad_seen_edge_on": (lambda abi: quad_prim(abi, (3, 1, 3), (0, 30, 0), (0, 0, 0)), None),                    # its plane y = 0 holds the camera
    "quad_smaller_than_a_pixel": (lambda abi: quad_prim(abi, (0.02, 1, 0.02), (90, 0, 0), (0.3, 0.2, 0)), None),   # (a pixel is 0.19 across there)
    "quad_of_size_1e6": (lambda abi: quad_prim(abi, (1e6, 1, 1e6), (90, 0, 0), (0, 0, -10)), "ones"),                 # it fills the view
    "quad_wholly_behind_the_camera": (lambda abi: quad_prim(abi, (2, 1, 2), (90, 0, 0), (0, 0, 9)), "zero"),
    "cube_wholly_behind_the_camera": (lambda abi: cube_prim(abi, (1, 1, 1), (10, 20, 30), (0, 0, 9)), "zero"),
    "cube_of_zero_scale_on_one_axis": (lambda abi: cube_prim(abi, (1, 0, 1), (10, 20, 30), (0, 0, 0)), "ones"),
    "cube_in_view": (lambda abi: cube_prim(abi, (1, 1.5, 0.7), (10, 20, 30), (0.5, 0.2, 0)), None),
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_never_culls_a_hit_hand_made(native, oracle_mod, abi, name):
    host, device = native
    make, whole = HAND[name]
    sc = hand_scene(abi, [make(abi)])
    cam, st = hand_camera(), abi.Settings(HAND_W, HAND_H, 1, 3)
    assert device.prepare_scene(sc).variant == 14
    masks = device.camera_masks(sc, cam, st)
    assert masks is not None and masks.shape == (HAND_H, HAND_W)
    if whole == "ones":
        assert (masks == 1).all()
    elif whole == "zero":
        assert (masks == 0).all()
    else:
        assert (masks == 0).any()
    bad, asked = culled_hits(abi, oracle_mod, sc, cam, HAND_W, HAND_H, masks, all_jitters_everywhere=True)
    assert not bad, bad[:10]
    if name in ("quad_smaller_than_a_pixel", "cube_in_view", "quad_of_size_1e6"):                  # ... and these are in view: the oracle does hit them where the bit is set
        one = np.zeros_like(masks)
        hits, _ = culled_hits(abi, oracle_mod, sc, cam, HAND_W, HAND_H, one, all_jitters_everywhere=True)
        assert hits and all(masks[y, x] == 1 for _, x, y, _, _ in hits)
    if name == "quad_smaller_than_a_pixel":
        assert 1 <= int(masks.sum()) <= 16                                                            # one or two pixels, dilated by one


def test_a_record_holding_nan_keeps_its_bit_everywhere(native, abi):
    host, device = native
    st = abi.Settings(HAND_W, HAND_H, 1, 3)
    q = quad_prim(abi, (1, 1, 1), (90, 0, 0), (0, 0, 0)); q.data[1] = float("nan")               # the base
    c = cube_prim(abi, (1, 1, 1), (0, 0, 0), (1, 0, 0)); c.data[16 + 5] = float("nan")            # world_to_object
    e = quad_prim(abi, (1, 1, 1), (90, 0, 0), (0, 0, 0)); e.data[13] = float("inf")               # 1 / |e0|^2
    ok = quad_prim(abi, (1, 1, 1), (90, 0, 0), (-1, 0, 0))
    masks = device.camera_masks(hand_scene(abi, [q, ok, c, e]), hand_camera(), st)
    assert masks is not None and ((masks & 0b1101) == 0b1101).all() and ((masks & 0b10) == 0).any()
    cam = hand_camera(); cam.half_width = float("nan")                                            # ... and a camera that is not finite keeps everything
    assert (device.camera_masks(hand_scene(abi, [ok]), cam, st) == 1).all()
    cam = hand_camera(); cam.right[:] = list(cam.forward)                                         # a degenerate basis
    assert (device.camera_masks(hand_scene(abi, [ok]), cam, st) == 1).all()


def test_lists_of_more_than_32_primitives_and_other_kernels_get_no_table(native, oracle_mod, abi):
    host, device = native
    st = abi.Settings(HAND_W, HAND_H, 1, 3)
    prims = [quad_prim(abi, (0.2, 1, 0.2), (90, 0, 0), (0.1 * k - 1.6, 0, 0)) for k in range(33)]
    assert device.prepare_scene(hand_scene(abi, prims)).variant == 14
    assert device.camera_masks(hand_scene(abi, prims), hand_camera(), st) is None
    m32 = device.camera_masks(hand_scene(abi, prims[:32]), hand_camera(), st)
    assert m32 is not None and int(m32.max()) >= 1 << 31                                           # 32 still do, and bit 31 is used
    sc = cornell(oracle_mod, host, 80, 60)
    assert device.camera_masks(sc, sc.camera, sc.settings, forced_variant=3) is None              # k_render_ctr_simple walks without a mask
    veach = load_for_both("veach", oracle_mod, host, width=16, height=12, spp=1, max_depth=3)
    assert device.camera_masks(veach, veach.camera, veach.settings) is None


# ------------------------------------------------------------------------------------------------------------ not vacuous
def test_cornell_masks_are_not_vacuous(native, oracle_mod, abi):
    """The headline view: at most 1.25 primitives per pixel on average out of 8, and at least a fifth of the pixels see nothing at all (the
    construction gives 0.98 and 24 %).  A table of all ones fails both."""
    host, device = native
    sc = cornell(oracle_mod, host, 800, 600)
    masks = device.camera_masks(sc, sc.camera, sc.settings)
    assert masks.shape == (600, 800) and sc.c.n_primitives == 8
    bits = sum(((masks >> np.uint32(i)) & 1).astype(np.int64) for i in range(8))
    mean, empty = float(bits.mean()), float((masks == 0).mean())
    print(f"cornell 800x600: {mean:.4f} mask bits per pixel, {100 * empty:.2f} % of the pixels empty; per primitive "
          + " ".join(f"{100 * float(((masks >> np.uint32(i)) & 1).mean()):.1f}" for i in range(8)))
    assert mean <= 1.25
    assert empty >= 0.20
    assert int(masks.max()) < 256


# ------------------------------------------------------------------------------------------------------------ plumbing
def test_processing_order_table_is_the_gather_of_the_plan_s_rows(native, oracle_mod, abi):
    host, device = native
    sc = cornell(oracle_mod, host, 80, 60)
    masks = device.camera_masks(sc, sc.camera, sc.settings)
    plans = [abi.Options.make(strip_rows=4, n_parts=3, part=1), abi.Options.make(row_begin=7, row_end=31), abi.Options.make(row_begin=59),
             abi.Options.make(row_begin=5, row_end=50, strip_rows=4, n_parts=3, part=2), abi.Options.make()]
    for opt in plans:
        rows = abi.rows_selected(60, opt)
        got = device.camera_masks(sc, sc.camera, sc.settings, options=opt)
        assert got.shape == (len(rows), 80) and np.array_equal(got, masks[rows]), (opt.row_begin, opt.row_end, opt.n_parts)
    assert rows == list(range(60)) and len(abi.rows_selected(60, plans[0])) == 20


# ------------------------------------------------------------------------------------------------------------ memory safety
@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_builder_is_clean_under_asan_and_ubsan(native, oracle_mod, abi, tmp_path):
    """tools/sanitize/camera_masks_main.cpp: a program of its own (rt_prepare.cpp and a main, plain g++) that builds the masks of cornell -- its
    primitives, materials and camera handed over in a file -- at three sizes, gathers its strip plans, and runs the degenerate cases above; built with
    -fsanitize=address,undefined and run directly."""
    host, _ = native
    sc = cornell(oracle_mod, host, 80, 60)
    c = sc.c
    blob = tmp_path / "cornell.bin"
    blob.write_bytes(np.array([c.n_primitives, c.n_materials], np.uint32).tobytes() + C.string_at(c.primitives, c.n_primitives * C.sizeof(abi.Primitive))
                     + C.string_at(c.materials, c.n_materials * C.sizeof(abi.Material)) + bytes(sc.camera))
    device = os.path.join(ROOT, "raytracer-rust_amd", "csrc", "device")
    exe = str(tmp_path / "camera_masks_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-fno-fast-math",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tools", "sanitize", "camera_masks_main.cpp"), os.path.join(device, "rt_prepare.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe, str(blob)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=300)
    assert p.returncode == 0 and "camera masks: all cases behaved" in p.stdout, p.stdout[-4000:]
    assert "AddressSanitizer" not in p.stdout and "runtime error" not in p.stdout, p.stdout[-4000:]
