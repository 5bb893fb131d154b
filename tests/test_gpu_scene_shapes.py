"""The kernels on the scenes of tests/scene_shapes.py: cameras that do not look from +z towards the origin, lists of up to 1000 primitives,
mesh tables in which primitive k does not use mesh k.  Every scene is exact (only + - * / sqrt on the path), so every comparison is bit for
bit: packed pixels, linear f32 words and ray counts against the oracle and between the variants, hit records and occlusion words against
the oracle's per-ray hook.  tests/test_scene_shapes_cpu.py shows that the frames rendered here see what they are meant to see.

One thing pinned here is not written in the source: a quad / cube list of more than 32 primitives gets no mask table, its camera pass runs
k_render_ctr_simple_qc with an all-ones word, and the walk's (pmask >> i) & 1 then shifts by 32 and more -- which the hardware's shift takes
modulo 32 (DESIGN.md 4.1 "Camera masks").  The qc lists of 33 .. 1000 and the run shapes render that pass against the oracle."""
import numpy as np
import pytest

import occlusion_ref as R
import scene_shapes as S
import test_gpu_occlusion as O
import test_gpu_ray_queries as Q
import test_gpu_variant_matrix as M
from parity import assert_parity

pytestmark = pytest.mark.gpu

F = np.float32
GUARD = 64
PACKED_GUARD, LINEAR_GUARD = 0x5A5A5A5A, -7.0
REFS = (2, 4)                                                        # the reference build's variants (test_gpu_variant_matrix.CAPABILITY)


# ---------------------------------------------------------------------------------------------------------------- plumbing
def render(device, abi, sc, cam, st, variant=None, knobs=None, opt=None, chunks=None, launched=None):
    """One render on a fresh context: variant None = the automatic choice, else forced (2: on the reference build); chunks: progressive sample
    counts; launched: the variant whose workgroup size the launch must report (a flag form).  Guard words behind the packed, linear and
    accumulation buffers must stay untouched.  -> (packed, linear, rays), the variant set_scene chose."""
    import torch
    ctx = device.Context(0, library=device.refs() if variant in REFS else device.lib())
    try:
        if variant is not None:
            ctx.set_knob("kernel", variant)
        for name, value in (knobs or {}).items():
            ctx.set_knob(name, value)
        ctx.set_scene(sc, cam, st)
        chosen = ctx.kernel_variant()
        assert variant is None or chosen == variant, (variant, chosen)
        rows = ctx.rows_selected(opt)
        n = rows * st.width
        packed = torch.full((n + GUARD,), PACKED_GUARD, dtype=torch.int32, device="cuda")
        linear = torch.full((3 * n + GUARD,), LINEAR_GUARD, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        if chunks is None:
            stats = [ctx.render(packed.data_ptr(), linear.data_ptr(), opt, want_stats=True)]
        else:
            accum = torch.full((4 * n + GUARD,), LINEAR_GUARD, dtype=torch.float32, device="cuda")
            s, stats = 0, []
            for c in chunks:
                stats.append(ctx.render_progressive(s, s + c, accum.data_ptr(), packed.data_ptr(), linear.data_ptr(), opt, want_stats=True))
                s += c
            assert s == st.samples_per_pixel
        torch.cuda.synchronize()
        ctx.check()
        assert all(x.block_threads == M.block_threads(chosen if launched is None else launched) for x in stats), (chosen, launched, [x.block_threads for x in stats])
        p, l = packed.cpu().numpy(), linear.cpu().numpy()
        assert (p[n:] == PACKED_GUARD).all() and (l[3 * n:] == LINEAR_GUARD).all(), "the render wrote behind its output"
        if chunks is not None:
            assert (accum.cpu().numpy()[4 * n:] == LINEAR_GUARD).all(), "the render wrote behind its sums"
        return (p[:n].view(np.uint32).reshape(rows, st.width).copy(), l[:3 * n].reshape(rows, st.width, 3).copy(), sum(x.rays for x in stats)), chosen
    finally:
        ctx.close()


_oracle = {}


def oracle_frame(oracle_mod, key, sc, cam, st, opt=None):
    if key not in _oracle:
        op, ol, cnt = oracle_mod.render(sc, cam, st, opt)
        op.setflags(write=False); ol.setflags(write=False)
        _oracle[key] = (op, ol, cnt.rays)
    return _oracle[key]


def against_oracle(got, ora, what):
    try:
        assert_parity(got[0], got[1], ora[0], ora[1], exact=True, gpu_rays=got[2], oracle_rays=ora[2])
    except AssertionError as e:
        raise AssertionError(f"{what}: {e}") from None


def every_variant(device, abi, oracle_mod, sc, cam, st, key, what, variants="accepted", opt=None):
    """The automatic variant and the forced ones, each against the oracle and so against each other.  -> the automatic variant."""
    ora = oracle_frame(oracle_mod, key, sc, cam, st, opt)
    auto, chosen = render(device, abi, sc, cam, st, opt=opt)
    against_oracle(auto, ora, f"{what}: the automatic variant {chosen}")
    forced = S.accepted_variants(M, abi, sc) if variants == "accepted" else variants
    for v in forced:
        got, _ = render(device, abi, sc, cam, st, variant=v, opt=opt)
        against_oracle(got, ora, f"{what}: variant {v} forced")
        M._same(got, auto, f"{what}: variant {v} against the automatic {chosen}")
    return chosen


def masked_and_unmasked(device, abi, oracle_mod, sc, cam, W, H, key, what):
    """k_render_ctr_simple_qc at 5 spp (no pass of the camera pass is masked) and at 64 spp (every pass is) with cam_cull 1 and 0."""
    st = abi.Settings(W, H, 5, S.DEPTH)
    got, chosen = render(device, abi, sc, cam, st)
    assert chosen == 14
    against_oracle(got, oracle_frame(oracle_mod, key + (5,), sc, cam, st), f"{what}, 5 spp")
    st = abi.Settings(W, H, 64, S.DEPTH)
    ora = oracle_frame(oracle_mod, key + (64,), sc, cam, st)
    on, chosen = render(device, abi, sc, cam, st, knobs={"cam_cull": 1})
    off, _ = render(device, abi, sc, cam, st, knobs={"cam_cull": 0})
    assert chosen == 14
    M._same(on, off, f"{what}, 64 spp: cam_cull 1 against 0")
    against_oracle(on, ora, f"{what}, 64 spp, cam_cull 1")
    against_oracle(off, ora, f"{what}, 64 spp, cam_cull 0")


def random_rays(seed, n=512, targets=None):
    """Un-normalised rays: from anywhere in the scene's box in any direction, or (targets [k, 3]) aimed near one of the targets from 5 units away."""
    rng = np.random.default_rng(seed)
    if targets is None:
        o = rng.uniform(-4, 4, (n, 3))
        d = rng.normal(size=(n, 3)) * rng.uniform(0.5, 3, (n, 1))
    else:
        at = np.asarray(targets, np.float64)[rng.integers(0, len(targets), n)] + rng.uniform(-0.8, 0.8, (n, 3))
        u = rng.normal(size=(n, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
        o = at + 5.0 * u
        d = (at - o) * rng.uniform(0.2, 2, (n, 1))
    return o.astype(F), d.astype(F)


def queries(device, abi, oracle_mod, sc, key, o, d, what, sizes=()):
    """trace_rays and occluded (test_gpu_occlusion.variants' set of t_max) on o, d and on the degenerate rays; -> the oracle's records of o, d."""
    ora_sc = S.per_ray_scene(abi, sc)
    want = Q.oracle_hits(("scene_shapes rays",) + key, oracle_mod, abi, ora_sc, o, d)
    od, dd = Q.degenerate_rays()
    want_d = Q.oracle_hits(("scene_shapes degenerate",) + key, oracle_mod, abi, ora_sc, od, dd)
    ctx = Q.context_for(device, abi, sc, 16, 12)
    try:
        got = Q.trace(device, abi, ctx, o, d)
        Q.assert_records(got, want, f"{what}: {len(o)} rays")
        Q.assert_records(Q.trace(device, abi, ctx, od, dd), want_d, f"{what}: degenerate rays")
        for n in sizes:
            assert Q.trace(device, abi, ctx, o[:n], d[:n]).tobytes() == got[:n].tobytes(), (what, n)
        O.check_segments(abi, ctx, want, o, d, f"{what}: {len(o)} rays", sizes=sizes)
        O.check_segments(abi, ctx, want_d, od, dd, f"{what}: degenerate rays")
    finally:
        ctx.close()
    return want


# ---------------------------------------------------------------------------------------------------------------- cameras x kernels
@pytest.mark.parametrize("name", list(S.CAMERAS))
def test_camera_on_the_quad_cube_kernel_masked_and_unmasked(name, native, oracle_mod, abi):
    host, device = native
    sc = S.camera_scene(abi, host, "qc")
    W, H = S.frame(name)
    cam = S.camera(name, abi, sc)
    assert (device.camera_masks(sc, cam, abi.Settings(W, H, 64, S.DEPTH)) is not None), "the list has a mask table"
    masked_and_unmasked(device, abi, oracle_mod, sc, cam, W, H, ("camera", "qc", name), f"camera {name} on the quad / cube list")


@pytest.mark.parametrize("which", ["meshfree", "mesh"])
@pytest.mark.parametrize("name", list(S.CAMERAS))
def test_camera_on_every_variant_that_takes_the_scene(name, which, native, oracle_mod, abi):
    """meshfree (no metal, no dielectric): 0 / 9 / 11 and the kernels that also take meshes; mesh (no metal): 1 / 7 / 10 / 13 and the reference
    build's 2."""
    host, device = native
    sc = S.camera_scene(abi, host, which)
    W, H = S.frame(name)
    forced = S.accepted_variants(M, abi, sc)
    assert set(forced) >= ({0, 9, 11} if which == "meshfree" else {1, 2, 7, 10, 13}), forced
    chosen = every_variant(device, abi, oracle_mod, sc, S.camera(name, abi, sc), abi.Settings(W, H, 5, S.DEPTH), ("camera", which, name, 5),
                           f"camera {name} on the {which} scene")
    assert chosen == (9 if which == "meshfree" else 13)


@pytest.mark.parametrize("name", list(S.CAMERAS))
def test_first_hits_under_the_camera(name, native, oracle_mod, abi):
    host, device = native
    W, H = S.frame(name)
    for which in S.CAMERA_SCENES:
        sc = S.camera_scene(abi, host, which)
        cam = S.camera(name, abi, sc)
        want = S.camera_records(oracle_mod, abi, sc, cam, W, H, ("camera", which, name))
        ctx = device.Context(0)
        try:
            ctx.set_scene(sc, cam, abi.Settings(W, H, 1, 1))
            whole = Q.first_hits(device, abi, ctx, W * H)
            Q.assert_records(whole, want, f"first hits, camera {name} on {which}")
            opt = abi.Options.make(row_begin=3, row_end=H - 2, strip_rows=2, n_parts=3, part=1)
            rows = abi.rows_selected(H, opt)
            assert 0 < len(rows) < H
            some = Q.first_hits(device, abi, ctx, len(rows) * W, opt)
            assert some.tobytes() == whole.reshape(H, W)[rows].tobytes(), (name, which)
        finally:
            ctx.close()


def test_ambient_occlusion_on_an_oblique_cameras_first_hits(native, oracle_mod, abi):
    host, device = native
    name = "rolled_oblique"
    W, H = S.frame(name)
    sc = S.camera_scene(abi, host, "mesh")
    cam = S.camera(name, abi, sc)
    want = S.camera_records(oracle_mod, abi, sc, cam, W, H, ("camera", "mesh", name))
    ref = R.AoReference(oracle_mod, S.per_ray_scene(abi, sc))
    ctx = device.Context(0)
    try:
        ctx.set_scene(sc, cam, abi.Settings(W, H, 1, 1))
        hits = O.check_ao(device, abi, ref, ctx, W, H, [(4, 1, np.inf), (4, 1, 0.25)], what=f"camera {name} on the mesh scene")
        Q.assert_records(hits, want, "the records the pass started from")
        assert (hits["primitive"] != abi.NO_HIT).sum() >= 64
    finally:
        ctx.close()


def test_progressive_sequence_under_an_oblique_camera(native, oracle_mod, abi):
    host, device = native
    name = "rolled_oblique"
    W, H = S.frame(name)
    for which in S.CAMERA_SCENES:
        sc = S.camera_scene(abi, host, which)
        cam = S.camera(name, abi, sc)
        st = abi.Settings(W, H, 5, S.DEPTH)
        got, chosen = render(device, abi, sc, cam, st, chunks=(1, 4))
        against_oracle(got, oracle_frame(oracle_mod, ("camera", which, name, 5), sc, cam, st), f"chunks 1 + 4, camera {name} on {which} (variant {chosen})")


# ---------------------------------------------------------------------------------------------------------------- list lengths
LISTS = [(family, n) for family in S.FAMILY_LENGTHS for n in S.FAMILY_LENGTHS[family]]


@pytest.mark.parametrize("family,n", LISTS, ids=[f"{family}-{n}" for family, n in LISTS])
def test_list_of_n_primitives(family, n, native, oracle_mod, abi):
    host, device = native
    sc = S.list_scene(abi, host, family, n)
    W, H = 40, 30
    what = f"{family} list of {n}"
    variants = "accepted" if n in (33, 257) else ()
    chosen = every_variant(device, abi, oracle_mod, sc, sc.camera, abi.Settings(W, H, 5, S.DEPTH), ("list", family, n, 5), what, variants=variants)
    if n in (33, 257):
        assert len(S.accepted_variants(M, abi, sc)) >= 3
    if family == "qc":
        assert chosen == 14 and (device.camera_masks(sc, sc.camera, abi.Settings(W, H, 64, S.DEPTH)) is not None) == (n <= 32)
        masked_and_unmasked(device, abi, oracle_mod, sc, sc.camera, W, H, ("list", family, n), what)


@pytest.mark.parametrize("shape", S.RUN_SHAPES)
def test_run_shapes_of_301(shape, native, oracle_mod, abi):
    host, device = native
    sc = S.run_scene(abi, host, shape)
    masked_and_unmasked(device, abi, oracle_mod, sc, sc.camera, 40, 30, ("run", shape), f"{shape} of {S.RUN_LENGTH}")


@pytest.mark.parametrize("family,n", [("meshfree", 257), ("meshfree", 1000), ("mesh", 257)])
def test_queries_on_long_lists(family, n, native, oracle_mod, abi):
    host, device = native
    sc = S.list_scene(abi, host, family, n)
    o, d = random_rays(n)
    want = queries(device, abi, oracle_mod, sc, ("list", family, n), o, d, f"{family} list of {n}", sizes=(1, 63, 64, 65))
    hit = want["primitive"] != abi.NO_HIT
    who = set(want["primitive"][hit].tolist())
    print(family, n, "hits", int(hit.sum()), "of", len(o), "distinct winners", len(who), "with index >= 32:", sum(i >= 32 for i in who), ">= 256:", sum(i >= 256 for i in who))
    assert sum(i >= 32 for i in who) >= 16 and (n < 1000 or sum(i >= 256 for i in who) >= 16) and (~hit).sum() >= 16


# ---------------------------------------------------------------------------------------------------------------- mesh tables
@pytest.mark.parametrize("shape", S.MESH_TABLES)
def test_mesh_table_on_every_variant_and_the_fixed_aabb_forms(shape, native, oracle_mod, abi):
    host, device = native
    sc = S.table_scene(abi, host, shape)
    st = abi.Settings(40, 30, 5, S.DEPTH)
    forced = S.accepted_variants(M, abi, sc)
    has_mesh = bool(S.mesh_prims(sc))
    assert set(forced) >= ({1, 2, 7, 10, 13} if has_mesh else {0, 1, 2, 7})
    assert (12 in forced) == (shape == "shared_identity")
    every_variant(device, abi, oracle_mod, sc, sc.camera, st, ("table", shape, 5), f"mesh table {shape}")
    # MI355RT_FLAG_FIXED_AABB: the product's form (8 on a list with a mesh) against the reference build's state machine in its form (4), and the oracle
    opt = abi.Options.make(flags=abi.FLAG_FIXED_AABB)
    ora = oracle_frame(oracle_mod, ("table", shape, 5, "fixed aabb"), sc, sc.camera, st, opt)
    base, _ = render(device, abi, sc, sc.camera, st, variant=2, opt=opt, launched=4)
    against_oracle(base, ora, f"mesh table {shape}: fixed AABB, the state machine")
    for v in [None] + [v for v in forced if v not in REFS and has_mesh]:
        got, chosen = render(device, abi, sc, sc.camera, st, variant=v, opt=opt, launched=8 if has_mesh else None)
        M._same(got, base, f"mesh table {shape}: fixed AABB, product variant {chosen} against the state machine")


@pytest.mark.parametrize("shape", S.MESH_TABLES)
def test_mesh_table_queries(shape, native, oracle_mod, abi):
    host, device = native
    sc = S.table_scene(abi, host, shape)
    c = sc.c
    users = S.mesh_prims(sc)
    aim = users if users else S.cubes_of(sc)
    targets = [list(c.primitives[i].data[12:15]) for i in aim]
    o, d = random_rays(7, targets=targets)
    want = queries(device, abi, oracle_mod, sc, ("table", shape), o, d, f"mesh table {shape}")
    wins = np.bincount(want["primitive"][want["primitive"] != abi.NO_HIT].astype(np.int64), minlength=c.n_primitives)
    print(shape, "rays won by each aimed-at primitive", [(i, int(wins[i])) for i in aim], "misses", int((want["primitive"] == abi.NO_HIT).sum()))
    loser = users[1] if shape == "shared_identity" else None
    assert all(wins[i] >= 3 for i in aim if i != loser), wins.tolist()
    # ... and per pixel
    W, H = 40, 30
    records = S.camera_records(oracle_mod, abi, sc, sc.camera, W, H, ("table", shape))
    ctx = device.Context(0)
    try:
        ctx.set_scene(sc, sc.camera, abi.Settings(W, H, 1, 1))
        got = Q.first_hits(device, abi, ctx, W * H)
        Q.assert_records(got, records, f"first hits, mesh table {shape}")
    finally:
        ctx.close()
    if shape == "shared_identity":                                       # coincident users of one mesh: the earlier one in the list wins, as in the oracle
        first, second = users[0], users[1]
        assert bytes(c.primitives[first].data) == bytes(c.primitives[second].data) and c.primitives[first].mesh == c.primitives[second].mesh
        assert wins[second] == 0 and wins[first] >= 3 and not (got["primitive"] == second).any() and (got["primitive"] == first).sum() >= 5
