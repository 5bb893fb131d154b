"""Every counter-mode kernel variant on every scene feature it accepts.

mi355rt_context_set_scene picks one of the render kernels from the scene's material kinds, primitive kinds and meshes (rt_prepare.cpp); the
diagnostic knob "kernel" forces another where the scene allows it.  Each instantiation compiles a different subset of the branches, and several
carry code of their own (run-based list walks, the QC kernel's stocked first hits, the wavefront kernels' sorted SHADE passes, the untransformed
and shallow-tree forms).  The contract is one image: every variant that accepts a scene must render it bit for bit like every other one, and
like the oracle (exactly where only + - * / sqrt are on the path, within the stated tolerance where textures, HDR skies or rough conductors
bring acos / atan2 / ln / sin_cos in).

CAPABILITY below is the table of what set_scene accepts when a variant is forced; the gpu tests pin it to the library, the CPU ledger checks
that the scene families below put every variant on every feature it accepts.
"""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from fuzz_scenes import random_scene
from parity import assert_parity

# material kinds (include/mi355rt.h)
LAMBERT, CHECKER, METAL, DIELECTRIC, EMISSIVE, PLASTIC, GGX, BECKMANN, NULL, TEXTURE = range(10)
SPHERE, PLANE, QUAD, CUBE, MESH = range(5)
MATS_ALL = frozenset(range(10))
MATS_LAMBERT = frozenset({LAMBERT, EMISSIVE, NULL})
MATS_NO_METAL = MATS_ALL - {METAL}
MATS_NO_SPECULAR = MATS_ALL - {METAL, DIELECTRIC}
PRIMS_ALL = frozenset(range(5))
PRIMS_MESH_FREE = PRIMS_ALL - {MESH}
PRIMS_QC = frozenset({QUAD, CUBE})

# variant: (kernel, library, materials, primitive kinds, meshes) -- what set_scene accepts when the variant is forced.
# meshes: "free" = mesh-free lists only; "any"; "identity" = the list has meshes and they are all untransformed.
CAPABILITY = {
    0: ("k_render_ctr_nomesh", "product", MATS_ALL, PRIMS_MESH_FREE, "free"),
    1: ("k_render_ctr_mesh", "product", MATS_ALL, PRIMS_ALL, "any"),
    3: ("k_render_ctr_simple", "product", MATS_LAMBERT, PRIMS_MESH_FREE, "free"),
    7: ("k_render_ctr_wf", "product", MATS_ALL, PRIMS_ALL, "any"),
    9: ("k_render_ctr_nospec", "product", MATS_NO_SPECULAR, PRIMS_MESH_FREE, "free"),
    10: ("k_render_ctr_wf_nometal", "product", MATS_NO_METAL, PRIMS_ALL, "any"),
    11: ("k_render_ctr_wf_meshfree", "product", MATS_NO_SPECULAR, PRIMS_MESH_FREE, "free"),
    12: ("k_render_ctr_wf_nometal_ident", "product", MATS_NO_METAL, PRIMS_ALL, "identity"),
    13: ("k_render_ctr_wf_nometal_shallow", "product", MATS_NO_METAL, PRIMS_ALL, "any"),
    14: ("k_render_ctr_simple_qc", "product", MATS_LAMBERT, PRIMS_QC, "free"),
    2: ("k_render_ctr_sm", "refs", MATS_ALL, PRIMS_ALL, "any"),
}
# Not forceable: the fixed-AABB forms follow options.flags (MI355RT_FLAG_FIXED_AABB) on scenes with a mesh -- 8 for every product variant,
# 4 for the reference build's state machine -- and 5 / 6 were retired (no library holds them).
FLAG_FORMS = {8: ("k_render_ctr_wf_fixaabb", "product", None), 4: ("k_render_ctr_sm_fixaabb", "refs", 2)}
RETIRED = {5, 6}

SEEDS = (0, 1, 2)
# The scene families (tests/fuzz_scenes.random_scene options), smallest first.  sky "alternate": the HDR map on the first two seeds, the flat
# miss colour on the third.
FAMILIES = {
    "lambert_qc": dict(exact_only=True, n_prims=10, only_kinds=[QUAD, CUBE, CUBE, QUAD], lambert_only=True, sky="alternate"),
    "lambert_meshfree_sky": dict(exact_only=True, n_prims=12, only_kinds=[SPHERE, PLANE, QUAD, CUBE], lambert_only=True, sky=True),
    "nospec_textures_rough_sky": dict(exact_only=False, n_prims=14, only_kinds=[SPHERE, PLANE, QUAD, CUBE], no_specular=True, textures=True, sky=True),
    "meshfree_everything": dict(exact_only=True, n_prims=14, only_kinds=[SPHERE, PLANE, QUAD, CUBE, CUBE, QUAD]),
    "mesh_transformed_nometal": dict(exact_only=False, n_prims=14, only_kinds=[MESH, SPHERE, PLANE, QUAD, CUBE, MESH, QUAD], mesh_tris=24, no_metal=True,
                                     textures=True, sky=True),
    "mesh_identity_nometal": dict(exact_only=False, n_prims=14, only_kinds=[MESH, SPHERE, PLANE, QUAD, CUBE, MESH, QUAD], mesh_tris=24, no_metal=True,
                                  textures=True, sky=True, identity_meshes=True),
    "mesh_identity_nometal_large": dict(exact_only=True, n_prims=10, only_kinds=[MESH, QUAD, SPHERE, PLANE, CUBE], mesh_tris=20, no_metal=True,
                                        identity_meshes=True, big_mesh_tris=9000),
    "mesh_everything_large": dict(exact_only=True, n_prims=12, only_kinds=[MESH, SPHERE, PLANE, QUAD, CUBE, MESH], mesh_tris=20, big_mesh_tris=9000),
    "mesh_fixed_aabb": dict(exact_only=True, n_prims=14, only_kinds=[MESH, CUBE, QUAD, SPHERE, PLANE, MESH], mesh_tris=20, textures=True, sky="alternate"),
    "mesh_fixed_aabb_identity_large": dict(exact_only=True, n_prims=10, only_kinds=[MESH, QUAD, SPHERE, PLANE, CUBE], mesh_tris=20, identity_meshes=True,
                                           big_mesh_tris=9000),
    "mesh_fixed_aabb_rough": dict(exact_only=False, n_prims=14, only_kinds=[MESH, CUBE, QUAD, SPHERE, PLANE, MESH], mesh_tris=20),
}
FLAGGED = {"mesh_fixed_aabb", "mesh_fixed_aabb_identity_large", "mesh_fixed_aabb_rough"}    # rendered with MI355RT_FLAG_FIXED_AABB (the oracle too)
# Families checked variant against variant only, not against the oracle.  mesh_fixed_aabb_rough's third seed traces 2 rays more on the GPU than in
# the oracle (2 pixels apart), with and without the flag; the oracle itself traces exactly those 2 rays, at exactly those pixels, when one rough
# conductor's roughness moves by one ulp (test_rough_fixed_aabb_family_moves_with_one_ulp below): the device libm's logf / atanf / sincosf ulps,
# which the ray bound of the fuzz tests does not allow at this frame size.  4 and 8 must still agree bit for bit on it.
VARIANTS_ONLY = {"mesh_fixed_aabb_rough"}
COMMON = dict(every_material=True, coincident=True)
WIDTH, HEIGHT, SPP, DEPTH = 48, 36, 5, 8
RAY_REL = 1e-6                                  # the tolerant fuzz tests' bound (tests/test_fuzz_parity.py)
WF_SHALLOW_NODES = 4096                          # rt_device.h: a "small" tree
LDS_NODE_CAP = 5104


def family_kwargs(family, seed):
    kw = dict(FAMILIES[family], **COMMON)
    if kw.get("sky") == "alternate":
        kw["sky"] = SEEDS.index(seed) < 2
    return kw


def planned_features(family):
    """What the family's scenes hold, from its options alone (random_scene's material list and primitive order)."""
    kw = FAMILIES[family]
    mats = set(MATS_LAMBERT) if kw.get("lambert_only") else {LAMBERT, CHECKER, METAL, DIELECTRIC, EMISSIVE, PLASTIC, NULL}
    if kw.get("no_metal") or kw.get("no_specular"):
        mats.discard(METAL)
    if kw.get("no_specular"):
        mats.discard(DIELECTRIC)
    if not kw["exact_only"]:
        mats |= {GGX, BECKMANN}
    if kw.get("textures"):
        mats.add(TEXTURE)
    prims = set(kw["only_kinds"]) | ({MESH} if kw.get("big_mesh_tris") else set())
    has_mesh = MESH in prims
    sky = {"hdr", "flat"} if kw.get("sky") == "alternate" else {"hdr"} if kw.get("sky") else {"flat"}
    return dict(mats=frozenset(mats), prims=frozenset(prims), sky=frozenset(sky), coincident=True,
                mesh_forms=frozenset({"identity" if kw.get("identity_meshes") else "transformed"} if has_mesh else set()),
                trees=frozenset(({"large"} if kw.get("big_mesh_tris") else set()) | ({"small"} if MESH in set(kw["only_kinds"]) else set())),
                flagged=family in FLAGGED)


def exact(family, seed):
    """Only + - * / sqrt on the path (no rough conductor, texture or HDR sky): bit for bit against the oracle."""
    kw = family_kwargs(family, seed)
    return kw["exact_only"] and not kw.get("textures") and not kw.get("sky")


def accepts(variant, f):
    _, _, mats, prims, meshes = CAPABILITY[variant]
    has_mesh = MESH in f["prims"]
    return (f["mats"] <= mats and f["prims"] <= prims and not (meshes == "free" and has_mesh)
            and not (meshes == "identity" and (not has_mesh or f["mesh_forms"] != {"identity"})))


def runs_of(family):
    """The variants a family renders with: the accepted ones (FIXED_AABB family: the two flag forms)."""
    f = planned_features(family)
    if f["flagged"]:
        return sorted(FLAG_FORMS)
    return sorted(v for v in CAPABILITY if accepts(v, f))


def required_cells(variant):
    """The (feature, value) cells a variant must be planned on: every material kind and primitive kind it accepts, both sky forms,
    coincident geometry, and -- where it takes meshes -- the mesh forms and tree sizes."""
    _, _, mats, prims, meshes = CAPABILITY[variant if variant in CAPABILITY else 7]     # a flag form accepts what the kernel it stands for does
    forms = {"identity"} if meshes == "identity" else {"transformed", "identity"}
    cells = {("mat", m) for m in mats} | {("prim", p) for p in prims} | {("sky", "hdr"), ("sky", "flat"), ("coincident", True)}
    if meshes != "free":
        cells |= {("mesh_form", m) for m in forms} | {("tree", "small"), ("tree", "large")}
    return cells


def cells_of(f):
    return ({("mat", m) for m in f["mats"]} | {("prim", p) for p in f["prims"]} | {("sky", s) for s in f["sky"]} | {("coincident", f["coincident"])}
            | {("mesh_form", m) for m in f["mesh_forms"]} | {("tree", t) for t in f["trees"]})


def _header_int(path, name):
    text = open(os.path.join(ROOT, path)).read()
    return int(re.search(rf"\b{name}\s*=\s*(\d+)", text).group(1))


MATRIX = [(fam, v) for fam in FAMILIES for v in runs_of(fam)]


# ---------------------------------------------------------------------------------------------------------------- the CPU ledger
def test_ledger_plans_every_variant_on_every_feature_it_accepts():
    n_variants = _header_int("raytracer-rust_amd/csrc/device/rt_device.h", "KERNEL_VARIANTS")
    assert _header_int("include/mi355rt.h", "MI355RT_MAT_KIND_COUNT") == len(MATS_ALL), "a new material kind: extend the table and the families"
    assert _header_int("include/mi355rt.h", "MI355RT_PRIM_KIND_COUNT") == len(PRIMS_ALL), "a new primitive kind: extend the table and the families"
    assert set(CAPABILITY) | set(FLAG_FORMS) | RETIRED == set(range(n_variants)), "a variant the table does not declare"
    missing = []
    for v in sorted(set(CAPABILITY) | set(FLAG_FORMS)):
        planned = set()
        for fam in FAMILIES:
            if v in runs_of(fam):
                planned |= cells_of(planned_features(fam))
        missing += [(v, c) for c in sorted(required_cells(v) - planned, key=str)]
    assert not missing, f"(variant, feature) cells no family plans: {missing}"
    # every family runs at least two variants (else nothing is compared); the mesh-free and the mesh kernels each meet the oracle exactly somewhere
    for fam in FAMILIES:
        assert len(runs_of(fam)) >= 2, fam
    for v in sorted(set(CAPABILITY) | set(FLAG_FORMS)):
        assert any(v in runs_of(fam) and exact(fam, s) for fam in FAMILIES for s in SEEDS), v
    assert len(MATRIX) == len(set(MATRIX))


def _source(path):
    return re.sub(r"\s+", " ", open(os.path.join(ROOT, path)).read())


def test_ledger_table_follows_the_librarys_variant_table():
    """The table restated from the library's own description of its variants (rt_device.h VARIANT_TABLE: materials, primitive kinds, the
    untransformed-mesh condition, forceability, the fixed-AABB form, the kernel name and workgroup), the kernel pointers rt_kernels.hip launches
    by it, and set_scene's forced-variant check and the render plan's flag form that read it (rt_prepare.cpp)."""
    import importlib
    dev = _source("raytracer-rust_amd/csrc/device/rt_device.h")
    api = _source("raytracer-rust_amd/csrc/device/rt_api.cpp")
    prep = _source("raytracer-rust_amd/csrc/device/rt_prepare.cpp")
    hip = _source("raytracer-rust_amd/csrc/device/rt_kernels.hip")
    num = {name: int(v) for name, v in re.findall(r"\b(KERNEL_\w+) = (\d+)", dev)}
    kinds = {"MAT_METAL": METAL, "MAT_DIELECTRIC": DIELECTRIC, "MAT_LAMBERT_SOLID": LAMBERT, "MAT_EMISSIVE": EMISSIVE, "MAT_NULL": NULL,
             "PRIM_SPHERE": SPHERE, "PRIM_PLANE": PLANE, "PRIM_QUAD": QUAD, "PRIM_CUBE": CUBE, "PRIM_MESH": MESH}
    assert "constexpr uint32_t MATS_ALL = (1u << MI355RT_MAT_KIND_COUNT) - 1u;" in dev and "constexpr uint32_t PRIMS_ALL = 0xFFFFFFFFu;" in dev

    def kindset(name):                                           # MATS_X / PRIMS_X = [MATS_Y | PRIMS_Y] [| or & ~] MATBIT(...) / (1u << ...) ..., evaluated
        if name in ("0", "MATS_ALL", "PRIMS_ALL"):
            return {"0": frozenset(), "MATS_ALL": MATS_ALL, "PRIMS_ALL": PRIMS_ALL}[name]
        expr = re.search(rf"constexpr uint32_t {name} = ([^;]+);", dev).group(1)
        head = re.match(r"(MATS_\w+|PRIMS_\w+)", expr)
        out = set(kindset(head.group(1))) if head else set()
        bits = {kinds[k] for k in re.findall(r"(?:MATBIT\(|1u << )MI355RT_(\w+?)\)", expr)}
        return frozenset(out - bits if "& ~" in expr else out | bits)

    body = re.search(r"constexpr VariantInfo VARIANT_TABLE\[KERNEL_VARIANTS\] = \{(.*?)\};", dev).group(1)
    rows = re.findall(r"\{(KERNEL_\w+), \"([^\"]+)\", (\w+), (FAMILY_\w+), (\w+), (\w+), (true|false), (true|false), (KERNEL_\w+)\}", body)
    assert [num[r[0]] for r in rows] == list(range(num["KERNEL_VARIANTS"])), "one row per variant, in order"
    table = {num[r[0]]: dict(kernel=r[1], block=_header_int("raytracer-rust_amd/csrc/device/rt_device.h", r[2]) if r[2] != "0" else 0, family=r[3],
                             mats=kindset(r[4]), prims=kindset(r[5]), identity=r[6] == "true", forceable=r[7] == "true", fixed_aabb=num[r[8]]) for r in rows}
    bench = importlib.import_module("bench")
    assert {v: t["kernel"] for v, t in table.items()} == bench.KERNEL_NAMES
    form_of = {of: f for f, (_, _, of) in FLAG_FORMS.items()}    # the variant a flag form stands for -> the form (None: every other one that walks meshes)
    for v, (kernel, _, mats, prims, meshes) in CAPABILITY.items():
        t = table[v]
        assert (t["kernel"], t["mats"], t["prims"], t["forceable"]) == (kernel, mats, prims, True), (v, t)
        assert (MESH not in t["prims"]) == (meshes == "free") and t["identity"] == (meshes == "identity"), (v, t)
        form = v if meshes == "free" else form_of.get(v, form_of[None])
        assert t["fixed_aabb"] == form, (v, t["fixed_aabb"], form)
    for v, (kernel, _, of) in FLAG_FORMS.items():              # a flag form accepts what the kernel it stands for does, and is its own form
        t, base = table[v], CAPABILITY[of if of is not None else 7]
        assert (t["kernel"], t["mats"], t["prims"], t["forceable"], t["identity"], t["fixed_aabb"]) == (kernel, base[2], base[3], False, False, v), (v, t)
    for v in RETIRED:
        t = table[v]
        assert (t["kernel"], t["family"], t["forceable"], t["mats"], t["prims"]) == ("(retired)", "FAMILY_RETIRED", False, frozenset(), frozenset()), (v, t)
    for v in SHAPE_VARIANTS:
        assert table[v]["block"] == block_threads(v), v
    # rt_kernels.hip's kernel pointers, indexed by variant: each row's kernel, the reference build's only under -DMI355RT_REFS, none for the retired
    fns = re.search(r"static const void\* const render_ctr_kernel\[KERNEL_VARIANTS\] = \{(.*?)\};", hip).group(1)
    lib = {v: c[1] for v, c in list(CAPABILITY.items()) + list(FLAG_FORMS.items())}
    expect = ["nullptr" if v in RETIRED else f"{'REFS_' if lib[v] == 'refs' else ''}KFN({t['kernel']})" for v, t in sorted(table.items())]
    assert re.findall(r"(?:REFS_)?KFN\(\w+\)|nullptr", fns) == expect, fns
    # set_scene's forced-variant check and plan_render's flag form read the table
    assert "auto covers = [&](uint32_t variant) { return (scene_mats & ~VARIANT_TABLE[variant].mats) == 0u; };" in prep
    assert "auto kinds_covered = [&](uint32_t variant) { return (scene_prim_kinds & ~VARIANT_TABLE[variant].prims) == 0u; };" in prep
    ok = re.search(r"const bool ok = ([^;]+);", prep).group(1)
    assert ok == ("render_ctr_variant_built(v) && VARIANT_TABLE[v].forceable && covers(v) && kinds_covered(v) && "
                  "!(VARIANT_TABLE[v].identity_meshes && !(has_mesh && all_meshes_identity))"), ok
    assert "if (fixed_aabb && in.has_mesh) variant = VARIANT_TABLE[variant].fixed_aabb;" in prep and "VARIANT_TABLE[variant].fixed_aabb" not in api
    # ... and what it plans (mi355rt_debug_plan_render: the render call's own plan_render, no GPU): the table's form with the flag on a list with a mesh
    device = importlib.import_module("raytracer-rust_amd.device")
    abi = importlib.import_module("raytracer-rust_amd.abi")
    for v, t in table.items():
        for flag, mesh in ((True, True), (True, False), (False, True), (False, False)):
            opt = abi.Options.make(flags=abi.FLAG_FIXED_AABB if flag else 0, row_begin=1, row_end=1)     # (an empty selection: the retired rows have no launch)
            got = device.plan_render(abi.Settings(8, 8, 2, 4), opt, variant=v, has_mesh=mesh).plan.variant
            assert got == (t["fixed_aabb"] if flag and mesh else v), (v, flag, mesh, got)


def test_families_hold_what_the_ledger_plans(native, abi):
    """The planned features are those of the generated scenes (CPU: scene generation and the BVH only)."""
    host, _ = native
    for fam in FAMILIES:
        f = planned_features(fam)
        seen_sky = set()
        for seed in SEEDS:
            sc = random_scene(abi, host, seed, **family_kwargs(fam, seed))
            c = sc.c
            mats = {c.materials[c.primitives[i].material].kind for i in range(c.n_primitives)}
            prims = {c.primitives[i].kind for i in range(c.n_primitives)}
            assert mats == f["mats"] and prims == f["prims"], (fam, seed, mats, prims)
            seen_sky.add("hdr" if c.sky_width else "flat")
            nodes = [c.meshes[m].node_count for m in range(c.n_meshes)]
            if "large" in f["trees"]:
                assert max(nodes) > LDS_NODE_CAP and max(nodes) > WF_SHALLOW_NODES, (fam, nodes)
            if "small" in f["trees"]:
                assert min(nodes) <= WF_SHALLOW_NODES, (fam, nodes)
            kw = family_kwargs(fam, seed)
            ident = [1.0 if (k % 5) == 0 else 0.0 for k in range(16)]
            forms = {"identity" if list(c.primitives[i].data[16:32]) == ident else "transformed" for i in range(c.n_primitives) if c.primitives[i].kind == MESH}
            assert forms == set(f["mesh_forms"]), (fam, forms)
            # coincident geometry: some primitive repeats bit for bit with another material, next to itself
            reps = {c.primitives[i].kind for i in range(c.n_primitives - 1) if bytes(c.primitives[i].data) == bytes(c.primitives[i + 1].data)
                    and c.primitives[i].kind == c.primitives[i + 1].kind and c.primitives[i].material != c.primitives[i + 1].material}
            assert reps == prims, (fam, reps)                               # of every kind in the list
            assert kw.get("textures", False) == (c.n_textures > 0)
        assert seen_sky == set(f["sky"]), fam


def test_rough_fixed_aabb_family_moves_with_one_ulp(native, oracle_mod, abi):
    """Why VARIANTS_ONLY holds mesh_fixed_aabb_rough: in the oracle alone, one ulp more roughness on its Beckmann conductor changes the ray
    count of the third seed's frame (by the 2 rays the GPU traces more, at the 2 pixels where the GPU differs) -- a frame whose ray count
    follows the last bit of a transcendental, which no two libms need to agree on."""
    host, _ = native
    seed = SEEDS[2]
    sc = random_scene(abi, host, seed, **family_kwargs("mesh_fixed_aabb_rough", seed))
    st, opt = abi.Settings(WIDTH, HEIGHT, SPP, DEPTH), _options(abi, "mesh_fixed_aabb_rough")
    _, base, cnt = oracle_mod.render(sc, sc.camera, st, opt)
    beck = [i for i in range(sc.c.n_materials) if sc.c.materials[i].kind == abi.MAT_ROUGH_BECKMANN]
    assert len(beck) == 1
    m = sc.c.materials[beck[0]]
    m.p0 = float(np.nextafter(np.float32(m.p0), np.float32(np.inf)))
    _, nudged, cnt1 = oracle_mod.render(sc, sc.camera, st, opt)
    moved = np.argwhere((nudged.view(np.uint32) != base.view(np.uint32)).any(-1) & (np.sqrt(((nudged.astype(np.float64) - base) ** 2).sum(-1)) > 1e-3))
    assert cnt1.rays - cnt.rays == 2 and moved.tolist() == [[12, 23], [35, 17]], (cnt.rays, cnt1.rays, moved.tolist())
    assert all(fam in FAMILIES and planned_features(fam)["flagged"] for fam in VARIANTS_ONLY)


# ---------------------------------------------------------------------------------------------------------------- on the GPU
_scenes, _baseline, _oracle = {}, {}, {}


def _scene(abi, host, fam, seed):
    if (fam, seed) not in _scenes:
        _scenes[(fam, seed)] = random_scene(abi, host, seed, **family_kwargs(fam, seed))
    return _scenes[(fam, seed)]


def _options(abi, fam, **kw):
    return abi.Options.make(flags=abi.FLAG_FIXED_AABB if fam in FLAGGED else 0, **kw)


def _library(device, v):
    lib = CAPABILITY[v][1] if v in CAPABILITY else FLAG_FORMS[v][1]
    return device.refs() if lib == "refs" else device.lib()


def _forced(v):
    """The knob value that makes the run: the variant itself, or for a flag form the variant whose form it is (None: the automatic choice)."""
    return v if v in CAPABILITY else FLAG_FORMS[v][2]


def block_threads(v):
    """The workgroup size the render launch of variant v reports (rt_device.h VARIANT_TABLE): it tells the kernel families apart, so a
    flagged render that fell back from the state machine's form (4) to the wavefront's (8) is seen."""
    return 1024 if v in (2, 4, 11) else 768 if v in (7, 8, 10, 12, 13) else 256


def render_ctx(device, abi, sc, v, st, opt, progressive=None, forced=-1, knobs=None):
    """One render on a fresh context of variant v's library with v forced (forced: another knob value, None: the automatic choice; knobs: more
    diagnostic knobs); returns (packed [rows, W], linear f32 [rows, W, 3], rays).  progressive: sample chunk sizes summing to
    st.samples_per_pixel (mi355rt_context_render_progressive)."""
    import torch
    ctx = device.Context(0, library=_library(device, v))
    try:
        k = _forced(v) if forced == -1 else forced
        if k is not None:
            ctx.set_knob("kernel", k)
        for name, value in (knobs or {}).items():
            ctx.set_knob(name, value)
        ctx.set_scene(sc, sc.camera, st)
        if k is not None:
            assert ctx.kernel_variant() == k, (v, ctx.kernel_variant())
        elif v == 8:
            assert ctx.kernel_variant() in (7, 10, 12, 13), ctx.kernel_variant()      # a wavefront kernel: its flag form is 8
        rows = ctx.rows_selected(opt)
        n = rows * st.width
        packed = torch.zeros(n, dtype=torch.int32, device="cuda")
        linear = torch.zeros(n * 3, dtype=torch.float32, device="cuda")
        rays = 0
        if progressive is None:
            stats = [ctx.render(packed.data_ptr(), linear.data_ptr(), opt, want_stats=True)]
        else:
            accum = torch.full((n, 4), float("nan"), dtype=torch.float32, device="cuda")
            s, stats = 0, []
            for c in progressive:
                stats.append(ctx.render_progressive(s, s + c, accum.data_ptr(), packed.data_ptr(), linear.data_ptr(), opt, want_stats=True))
                s += c
            assert s == st.samples_per_pixel
        rays = sum(x.rays for x in stats)
        assert all(x.block_threads == block_threads(v) for x in stats), (v, [x.block_threads for x in stats])
        torch.cuda.synchronize()
        return packed.cpu().numpy().view(np.uint32).reshape(rows, st.width), linear.cpu().numpy().reshape(rows, st.width, 3), rays
    finally:
        ctx.close()


def _oracle_of(oracle_mod, abi, fam, seed, sc, st, opt, key):
    if key not in _oracle:
        op, ol, cnt = oracle_mod.render(sc, sc.camera, st, opt)
        _oracle[key] = (op, ol, cnt.rays)
    return _oracle[key]


def _check_oracle(fam, seed, got, ora, rows=None):
    gp, gl, rays = got
    op, ol, orays = ora
    if rows is not None:
        op, ol = op[rows], ol[rows]
    assert_parity(gp, gl, op, ol, exact=exact(fam, seed), rows=rows, gpu_rays=rays, oracle_rays=orays, ray_rel=RAY_REL)


def _same(a, b, what):
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), f"{what}: linear differs in {int((a[1] != b[1]).any(-1).sum())} px"
    assert np.array_equal(a[0], b[0]), f"{what}: packed differs"
    assert a[2] == b[2], f"{what}: rays {a[2]} vs {b[2]}"


@pytest.mark.gpu
@pytest.mark.parametrize("fam", list(FAMILIES))
def test_forced_variants_follow_the_capability_table(fam, native, abi):
    """Forcing v: set_scene keeps v exactly where the table says it accepts the scene, and chooses another kernel elsewhere."""
    host, device = native
    sc = _scene(abi, host, fam, SEEDS[0])
    st = abi.Settings(WIDTH, HEIGHT, SPP, DEPTH)
    f = planned_features(fam)
    for library, variants in ((device.lib(), range(15)), (device.refs(), (2,))):
        for v in variants:
            ctx = device.Context(0, library=library)
            try:
                ctx.set_knob("kernel", v)
                ctx.set_scene(sc, sc.camera, st)
                got = ctx.kernel_variant()
            finally:
                ctx.close()
            ok = v in CAPABILITY and accepts(v, f) and (CAPABILITY[v][1] == "refs") == (library is not device.lib())
            assert (got == v) == ok, (fam, v, got)


@pytest.mark.gpu
@pytest.mark.parametrize("fam,variant", MATRIX, ids=[f"{fam}-v{v}" for fam, v in MATRIX])
def test_variant_renders_the_family_like_every_other_variant_and_the_oracle(fam, variant, native, oracle_mod, abi):
    """The variant's frame of each seed is bit-identical (packed, linear f32, rays) to the baseline's, and matches the oracle.  Baseline: the
    product's automatic choice; under MI355RT_FLAG_FIXED_AABB the reference build's state machine in its flag form (4).  There the row of 8
    renders the product's automatic choice and every product variant the scene accepts, forced (each launches 8), and the row of 4 the state
    machine in its other configurations (one wave per traversal step, no inline root test)."""
    host, device = native
    st = abi.Settings(WIDTH, HEIGHT, SPP, DEPTH)
    flagged = planned_features(fam)["flagged"]
    for seed in SEEDS:
        sc = _scene(abi, host, fam, seed)
        opt = _options(abi, fam)
        if (fam, seed) not in _baseline:
            if flagged:
                _baseline[(fam, seed)] = (*render_ctx(device, abi, sc, 4, st, opt), "the state machine's flag form (4)")
            else:
                ctx = device.Context(0)
                try:
                    ctx.set_scene(sc, sc.camera, st)
                    auto = ctx.kernel_variant()
                finally:
                    ctx.close()
                gp, gl, gs = device.render(sc, sc.camera, st, opt)
                _baseline[(fam, seed)] = (gp, gl, gs.rays, f"the automatic variant {auto}")
        base = _baseline[(fam, seed)]
        if not flagged:
            runs = [(None, {})]
        elif variant == 8:
            runs = [(None, {})] + [(v, {}) for v in (1, 7, 10, 12, 13) if accepts(v, planned_features(fam))]
        else:
            runs = [(2, {"trav_min": 1}), (2, {"inline_steps": 0}), (2, {"trav_min": 64, "inline_steps": 1})]
        for forced, knobs in runs:
            got = (render_ctx(device, abi, sc, variant, st, opt) if forced is None and not flagged
                   else render_ctx(device, abi, sc, variant, st, opt, forced=forced, knobs=knobs))
            _same(got, base[:3], f"{fam} seed {seed}: variant {variant} (kernel knob {forced}, {knobs}) against {base[3]}")
        if fam not in VARIANTS_ONLY:
            _check_oracle(fam, seed, got, _oracle_of(oracle_mod, abi, fam, seed, sc, st, opt, (fam, seed, "frame")))


SHAPE_VARIANTS = sorted(set(CAPABILITY) | set(FLAG_FORMS))


def smallest_family(v):
    return next(fam for fam in FAMILIES if v in runs_of(fam) and fam not in VARIANTS_ONLY)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", SHAPE_VARIANTS, ids=[f"v{v}-{CAPABILITY.get(v, FLAG_FORMS.get(v))[0]}" for v in SHAPE_VARIANTS])
def test_tiny_workloads_per_variant(variant, native, oracle_mod, abi):
    """Work cursors, stocked first hits with fewer than 64 samples and half-empty queues: a 1 x 1 x 1 frame and a 7 x 3 frame at 5 spp
    (the oracle's), bands of 1 and 7 pixels, progressive chunks 1 + 3 + 4, a row window and a strip subset (the variant's own one-shot frame)."""
    host, device = native
    fam = smallest_family(variant)
    seed = SEEDS[0]
    sc = _scene(abi, host, fam, seed)
    for w, h, spp in ((1, 1, 1), (7, 3, 5)):
        st = abi.Settings(w, h, spp, DEPTH)
        opt = _options(abi, fam)
        got = render_ctx(device, abi, sc, variant, st, opt)
        _check_oracle(fam, seed, got, _oracle_of(oracle_mod, abi, fam, seed, sc, st, opt, (fam, seed, w, h, spp)))
    st = abi.Settings(24, 18, 8, DEPTH)
    full = render_ctx(device, abi, sc, variant, st, _options(abi, fam))
    for label, kw in (("bands of 1 pixel", dict(workspace_bytes=8 * 12 * 1)), ("bands of 7 pixels", dict(workspace_bytes=8 * 12 * 7))):
        _same(render_ctx(device, abi, sc, variant, st, _options(abi, fam, **kw)), full, f"variant {variant}, {label}")
    prog = render_ctx(device, abi, sc, variant, st, _options(abi, fam), progressive=(1, 3, 4))
    _same(prog, full, f"variant {variant}, progressive chunks 1 + 3 + 4")
    for label, kw in (("rows 5..13", dict(row_begin=5, row_end=13)), ("strips of 2, part 1 of 3", dict(strip_rows=2, n_parts=3, part=1)),
                      ("rows 3..17, strips of 1, part 0 of 4", dict(row_begin=3, row_end=17, n_parts=4, part=0))):
        opt = _options(abi, fam, **kw)
        rows = abi.rows_selected(st.height, opt)
        gp, gl, _ = render_ctx(device, abi, sc, variant, st, opt)
        assert gp.shape[0] == len(rows) > 0
        assert np.array_equal(gl.view(np.uint32), full[1][rows].view(np.uint32)) and np.array_equal(gp, full[0][rows]), f"variant {variant}, {label}"
