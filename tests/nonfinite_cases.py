"""The poisoned scenes of test_nonfinite_radiance_cpu.py (the conditions, on the oracle alone) and test_gpu_nonfinite_radiance.py (every
kernel variant against the oracle).  A plain module, imported like parity.py.

A case is (poison, base, classes): a poison of fuzz_scenes.POISONS, one of the base scenes below, and the value classes the oracle's image of
it must hold in at least 2 % of its pixels each (beside at least 5 % finite, non-zero pixels) -- measured when the cases were chosen, asserted
by the CPU test.  The bases are scene families of test_gpu_variant_matrix.py (or the same options with a sky map, or without specular
materials) with one seed each, chosen so that the poisoned material is in view.  A base is rendered by every variant that accepts its scene
(variants_of: test_gpu_variant_matrix.accepts on what the generated scene holds; a base rendered with MI355RT_FLAG_FIXED_AABB by the two flag
forms), and every poison family meets every variant that can take it (family_plan, asserted by the CPU test).
"""
import numpy as np

import test_gpu_variant_matrix as vm
from fuzz_scenes import POISONS, random_scene

WIDTH, HEIGHT, SPP, DEPTH = vm.WIDTH, vm.HEIGHT, vm.SPP, vm.DEPTH
SPP_PATHS = 7                                     # the bands / rows / chunks / devices test: progressive chunks 1, 5, rest need a rest
MESHFREE = [vm.SPHERE, vm.PLANE, vm.QUAD, vm.CUBE]

# base -> (random_scene options, seed, rendered with MI355RT_FLAG_FIXED_AABB, exact against the oracle in counter mode)
BASES = {
    "qc": (dict(vm.FAMILIES["lambert_qc"], sky=False, **vm.COMMON), 0, False, True),
    "qc_sky": (dict(vm.FAMILIES["lambert_qc"], sky=True, **vm.COMMON), 0, False, True),                 # the one sky scene variant 14 takes
    "sky": (dict(vm.FAMILIES["lambert_meshfree_sky"], **vm.COMMON), 0, False, True),
    "nospec": (dict(exact_only=True, n_prims=14, only_kinds=MESHFREE, no_specular=True, **vm.COMMON), 1, False, True),     # a checker for 0, 9 and 11
    "mf": (dict(vm.FAMILIES["meshfree_everything"], **vm.COMMON), 1, False, True),                      # metal for the mesh-free variant 0
    "ident": (dict(vm.FAMILIES["mesh_identity_nometal_large"], **vm.COMMON), 0, False, True),
    "ident_sky": (dict(vm.FAMILIES["mesh_identity_nometal_large"], sky=True, **vm.COMMON), 0, False, True),
    "every": (dict(exact_only=True, every_material=True), 1, False, True),       # every primitive and material kind, transformed meshes
    "flagged": (dict(vm.FAMILIES["mesh_fixed_aabb_identity_large"], **vm.COMMON), 0, True, True),
    "flagged_sky": (dict(vm.FAMILIES["mesh_fixed_aabb_identity_large"], sky=True, **vm.COMMON), 0, True, True),
    # rough conductors: the device's libm differs from glibc by ulps in counter mode, so there only the two flag forms (state machine and
    # wavefront) meet each other; the reference-stream mode is bit-identical to the oracle
    "rough": (dict(vm.FAMILIES["mesh_fixed_aabb_rough"], **vm.COMMON), 0, True, False),
}
NAN, PINF, NINF, NEG, DEN = "nan", "+inf", "-inf", "negative", "denormal"
CASES = [
    ("emissive_inf", "qc", {PINF}), ("emissive_mixed", "qc", {NAN, PINF, NINF}), ("emissive_overflow", "qc", {PINF, DEN}), ("emissive_signed", "qc", {NEG, DEN}),
    ("miss_signed", "qc", {NEG, DEN}),
    ("lambert_zero", "qc", set()), ("lambert_gt1", "qc", set()), ("lambert_negative", "qc", {NEG}),
    ("lambert_inf", "qc", {PINF}),                 # 0 * inf at the lights is in 1 % of the pixels here (17 of them); "every" and "sky" hold it in more
    ("sky", "qc_sky", {NAN, PINF, DEN}),
    ("miss_inf", "ident", {PINF}), ("miss_mixed", "ident", {NAN, PINF, NINF}), ("checker_nan", "ident", {NAN}), ("emissive_signed", "ident", {NEG, DEN}),
    ("lambert_negative", "ident", {NEG}),
    ("sky", "ident_sky", {NAN, PINF}),             # (the denormal texels are in view on "qc_sky" and "sky")
    ("lambert_inf", "every", {NAN, PINF}), ("emissive_overflow", "every", {PINF, DEN}), ("metal_inf", "every", {NAN}),
    ("miss_overflow", "every", {PINF, DEN}),
    ("emissive_mixed", "flagged", {NAN, PINF, NINF}), ("metal_inf", "flagged", {NAN, PINF}), ("checker_nan", "flagged", {NAN}), ("lambert_zero", "flagged", set()),
    ("miss_signed", "flagged", {NEG, DEN}),        # (an infinite or NaN miss colour leaves no finite pixel in this frame)
    ("sky", "flagged_sky", {NAN, PINF}),
    ("sky", "sky", {NAN, PINF, DEN}), ("lambert_inf", "sky", {NAN, PINF}),
    ("checker_nan", "nospec", {NAN}), ("metal_inf", "mf", {NAN, PINF}),
    ("rough_inf", "rough", {NAN, PINF}), ("emissive_overflow", "rough", {PINF, DEN}),
]
# reference-stream mode (bit-identical to the oracle also where rough conductors are in view)
REF_CASES = [("rough_inf", "rough"), ("emissive_overflow", "rough"), ("emissive_mixed", "qc")]
# bands, row subsets, progressive chunks and the resident multi-device context: two cases per path (lockstep: "qc"; wavefront: "ident")
PATH_CASES = [("emissive_mixed", "qc"), ("lambert_inf", "qc"), ("miss_mixed", "ident"), ("checker_nan", "ident")]
# The poison families (what POISONS writes into) and the material kind a variant must accept to take one; the miss colour and the sky map
# go with every scene.  Rough conductors are left out of the plan: in counter mode they are checked state machine against wavefront only
# (the "rough" base), and against the oracle in reference-stream mode.
FAMILY_KIND = {"emissive": vm.EMISSIVE, "miss": None, "sky": None, "lambert": vm.LAMBERT, "metal": vm.METAL, "checker": vm.CHECKER}

_scenes = {}


def scene(abi, host, base, poison=None):
    if (base, poison) not in _scenes:
        kw, seed = BASES[base][0], BASES[base][1]
        _scenes[(base, poison)] = random_scene(abi, host, seed, poison=poison, **kw)
    return _scenes[(base, poison)]


def features_of(abi, sc):
    """What test_gpu_variant_matrix.accepts reads, from the generated scene itself."""
    c = sc.c
    ident = [1.0 if (k % 5) == 0 else 0.0 for k in range(16)]
    meshes = [c.primitives[i] for i in range(c.n_primitives) if c.primitives[i].kind == vm.MESH]
    return dict(mats=frozenset(c.materials[c.primitives[i].material].kind for i in range(c.n_primitives)),
                prims=frozenset(c.primitives[i].kind for i in range(c.n_primitives)),
                mesh_forms=frozenset("identity" if list(p.data[16:32]) == ident else "transformed" for p in meshes))


def variants_of(abi, host, base):
    """The variants that render a base: every one that accepts its scene; under MI355RT_FLAG_FIXED_AABB the two flag forms."""
    if BASES[base][2]:
        return sorted(vm.FLAG_FORMS)
    f = features_of(abi, scene(abi, host, base))
    return sorted(v for v in vm.CAPABILITY if vm.accepts(v, f))


def takers(family):
    """Every variant that can take a poison family at all: those whose materials hold the poisoned kind (a flag form: those of the kernel it
    stands for)."""
    kind = FAMILY_KIND[family]
    of = lambda v: vm.CAPABILITY[v if v in vm.CAPABILITY else 7 if vm.FLAG_FORMS[v][2] is None else vm.FLAG_FORMS[v][2]]
    return {v for v in set(vm.CAPABILITY) | set(vm.FLAG_FORMS) if kind is None or kind in of(v)[2]}


def family_plan(abi, host):
    """family -> the variants some case of CASES renders it with."""
    plan = {fam: set() for fam in FAMILY_KIND}
    for poison, base, _ in CASES:
        if POISONS[poison][0] in plan:
            plan[POISONS[poison][0]] |= set(variants_of(abi, host, base))
    return plan


def options(abi, base, **kw):
    return abi.Options.make(flags=abi.FLAG_FIXED_AABB if BASES[base][2] else 0, **kw)


def settings(abi, spp=SPP):
    return abi.Settings(WIDTH, HEIGHT, spp, DEPTH)


def class_shares(linear):
    """Share of the pixels that hold each class in some channel, and of the pixels that are finite and not black."""
    tiny = np.finfo(np.float32).tiny
    px = lambda m: float(m.any(-1).mean())
    return {NAN: px(np.isnan(linear)), PINF: px(linear == np.inf), NINF: px(linear == -np.inf), NEG: px(linear < 0),
            DEN: px((np.abs(linear) < tiny) & (linear != 0)), "finite": float((np.isfinite(linear).all(-1) & (linear != 0).any(-1)).mean())}
