"""Cases for the wave probe of the bounce (csrc/refs/rt_scatter_wave_probe.h): whole waves whose lanes the test chooses, and records at the
edges of every material's decisions.  A plain module like scene_shapes.py; tests/test_scatter_wave_cpu.py checks it on the oracle's side,
tests/test_gpu_scatter_wave.py runs it through every form of the bounce the library launches and through the product's per-record hook.

A record is 16 uint32 words: material index, flags (bit 0 front face, bit 8 live), incoming direction[3], hit point[3], normal[3] as float
bits, then the draw address (k0, k1, x, sample, ray).  The reference of a record is 16 words in the probe's output layout: scattered,
origin[3], direction[3], attenuation[3], emitted[3] from the oracle's Material::scatter (its rejection is the plain sequential loop), then
the accepted unit-ball point[3] (numpy, below) where the event drew one.  An idle lane's reference is all zero.

ADDRESS POOLS.  unit_ball_cooperative is exercised by how many lanes still need a try (owners) and by how deep their first accepted try
lies; neither can be chosen through a scene.  A vectorised numpy pcg4d (pinned to the oracle's generator by the CPU test) searches 2^22
addresses (x, sample) per (key, ray) setting and sorts them by the try at which len2(point) < 1 first holds, in f32 and in the device's
order of additions ((x*x + y*y) + z*z).  pools() holds, per setting: accepted at try 0; try 1; tries 2..3; >= 8; >= 12; >= 16.
"""
import functools

import numpy as np

from oracle.rng_np import block_of, ctr_block, path_base, pcg4d  # noqa: F401  -- re-exported: the tests reach them under these names

f32, u32 = np.float32, np.uint32
EPS = f32(1e-4)
ONES = 0xFFFFFFFF
LIVE, FRONT = 0x100, 1
LAMBERT, CHECKER, METAL, DIELECTRIC, EMISSIVE, PLASTIC, GGX, BECKMANN, NULL, TEXTURE = range(10)
TERMINAL = (EMISSIVE, NULL)

# (key lo, key hi, ray): an ordinary key at ray 1, the all-ones key at ray 30, a key of test_gpu_rng_stepped.PATHS at the last ray
SETTINGS = ((0x1234ABCD, 0x00000007, 1), (ONES, ONES, 30), (0x9E3779B9, 0x7F4A7C15, ONES))
SEARCH_LOG2 = 22
POOL_NAMES = ("t0", "t1", "t23", "ge8", "ge12", "ge16")
N_OWNERS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64)
PLACEMENTS = ("low", "high", "stride", "shuffle")
OTHERS = ("accept0", "idle", "mix")
DEPTHS = ("shallow", "deep8", "deep16", "half12")


# ---- the generator and the unit-ball draw, on uint32 / float32 arrays ---------------------------------------------------------------
def range11(w):
    """rand's random_range(-1.0..1.0) from a u32: (value1_2 - 1) * 2 + -1 with the 23 high bits as the mantissa of a float in [1, 2)."""
    v12 = ((np.asarray(w, u32) >> u32(9)) | u32(0x3F800000)).view(f32)
    return (v12 - f32(1.0)) * f32(2.0) + f32(-1.0)


def u01(w):
    return (np.asarray(w, u32) >> u32(8)).astype(f32) * f32(1.0 / 16777216.0)


def cube_point(block):
    return np.stack([range11(block[1]), range11(block[2]), range11(block[3])], -1)


def vdot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def vnormalized(a):
    """vec3.rs:37-44 on float32 [n, 3]: a * (1 / length), the vector itself below 1e-4."""
    with np.errstate(all="ignore"):
        ln = np.sqrt(vdot(a, a))
        out = a * (f32(1.0) / ln)[..., None]
    return np.where((ln < EPS)[..., None], a, out).astype(f32)


def first_accept(k0, k1, x, s, ray, limit=64):
    """Per address: the first try j whose point lies inside the unit ball, and that point (float32 [n, 3])."""
    k0, k1, x, s, ray = [np.asarray(v, u32) for v in np.broadcast_arrays(k0, k1, x, s, ray)]
    base = path_base(k0, k1, x, s)
    n = x.shape[0]
    first = np.full(n, -1, np.int32)
    point = np.zeros((n, 3), f32)
    todo = np.arange(n)
    for j in range(limit):
        if todo.size == 0:
            break
        p = cube_point(block_of([b[todo] for b in base], ray[todo], j))
        ok = vdot(p, p) < f32(1.0)
        first[todo[ok]] = j
        point[todo[ok]] = p[ok]
        todo = todo[~ok]
    assert todo.size == 0, "an address without an accepted try"
    return first, point


@functools.lru_cache(maxsize=None)
def pools():
    """Per setting: {"k0", "k1", "ray", pool name: dict(x, s, first, point)}; addresses x = i mod 2^11, sample = i >> 11 for i < 2^22."""
    out = []
    i = np.arange(1 << SEARCH_LOG2, dtype=u32)
    x, s = i & u32(2047), i >> u32(11)
    for k0, k1, ray in SETTINGS:
        first, point = first_accept(k0, k1, x, s, ray)
        sel = {"t0": first == 0, "t1": first == 1, "t23": (first == 2) | (first == 3), "ge8": first >= 8, "ge12": first >= 12, "ge16": first >= 16}
        d = {"k0": k0, "k1": k1, "ray": ray, "max_first": int(first.max())}
        for name, m in sel.items():
            idx = np.flatnonzero(m)
            if name in ("t0", "t1", "t23"):
                idx = idx[:4096]                                   # (the shallow pools are half of all addresses: the first few thousand do)
            d[name] = {"x": x[idx], "s": s[idx], "first": first[idx], "point": point[idx]}
        out.append(d)
    return out


# ---- materials --------------------------------------------------------------------------------------------------------------------------
SUB = float(np.float32(2.0) ** -149)
IORS = [1.5, 1.33, 2.4, 1.0, float(np.nextafter(f32(1), f32(2))), float(np.nextafter(f32(1), f32(0))), 0.5, 1e3, 2.0 ** -126, 0.0, -1.5, np.inf, np.nan]
FUZZES = [0.3, 0.05, 0.6, SUB, 2.0 ** -24, 1 - 2.0 ** -24, 1.0, 1.5, -0.0, -0.5, np.inf, np.nan]
INV_SCALES = [1.0, 3.7, 0.25, 0.0, -0.0, -2.7, SUB, 1e9, np.inf, np.nan]
ALBEDOS = [(0.7, 0.6, 0.5), (1.5, 2.0, 1e3), (-0.5, -1.0, 0.25)]
ROUGHS = [0.0, -0.0, np.inf, np.nan]
ETA_K = [((0.2, 1.09, 1.42), (3.91, 2.57, 2.30)), ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)), ((1e20, 1e20, 1e20), (3.91, 2.57, 2.30))]   # copper; eta = k = 0; eta^2 overflows
CRITICAL_IORS = [1.5, 2.4, float(np.nextafter(f32(1), f32(2)))]
CHECK_ON, CHECK_OFF = (0.9, 0.8, 0.7), (0.1, 0.2, 0.3)


@functools.lru_cache(maxsize=None)
def material_table():
    """The one material list every record indexes: a list of dict(kind, albedo, aux, p0, eta, k) and {name: [indices]}."""
    mats, groups = [], {}

    def add(group, kind, albedo=(0.7, 0.6, 0.5), aux=(0, 0, 0), p0=0.0, eta=(0, 0, 0), k=(0, 0, 0)):
        groups.setdefault(group, []).append(len(mats))
        mats.append(dict(kind=kind, albedo=albedo, aux=aux, p0=p0, eta=eta, k=k))

    for a in ALBEDOS:
        add("lambert", LAMBERT, a)
    for v in INV_SCALES:
        add("checker", CHECKER, CHECK_ON, CHECK_OFF, v)
    add("mirror", METAL, (0.8, 0.85, 0.9), p0=0.0)
    add("mirror", METAL, ALBEDOS[1], p0=0.0)
    for v in FUZZES:
        add("fuzzed", METAL, (0.8, 0.85, 0.9), p0=v)
    for v in IORS:
        add("glass", DIELECTRIC, p0=v)
    for v in IORS:
        add("plastic", PLASTIC, (0.3, 0.6, 0.2), p0=v)
    for kind in (GGX, BECKMANN):
        for r in ROUGHS:
            for eta, k in ETA_K:
                add("rough", kind, (0.9, 0.8, 0.7), p0=r, eta=eta, k=k)
    for a in ((0.0, 0.0, 0.0), (1e30, 1e30, 1e30), (4.0, 3.0, 2.0)):
        add("emissive", EMISSIVE, a)
    add("null", NULL)
    add("fuzz1", METAL, (0.8, 0.85, 0.9), p0=1.0)
    add("fuzz09", METAL, (0.8, 0.85, 0.9), p0=0.9)
    for v in CRITICAL_IORS:
        add("critical", DIELECTRIC, p0=v)
    add("checker1", CHECKER, CHECK_ON, CHECK_OFF, 1.0)
    return mats, groups


def materials_ctypes(abi):
    mats, _ = material_table()
    arr = (abi.Material * len(mats))()
    for m, d in zip(arr, mats):
        m.kind = d["kind"]
        m.albedo[:] = d["albedo"]; m.aux[:] = d["aux"]; m.p0 = d["p0"]; m.eta[:] = d["eta"]; m.k[:] = d["k"]
    return arr


def material_field(name):
    mats, _ = material_table()
    with np.errstate(over="ignore"):
        return np.array([m[name] for m in mats], f32 if name != "kind" else u32)


# ---- records ----------------------------------------------------------------------------------------------------------------------------
def pack(material, flags, rd, p, n, k0, k1, x, s, ray):
    m = np.asarray(material, u32)
    rec = np.zeros((m.shape[0], 16), u32)
    rec[:, 0] = m
    rec[:, 1] = flags
    rec[:, 2:5] = np.asarray(rd, f32).view(u32)
    rec[:, 5:8] = np.asarray(p, f32).view(u32)
    rec[:, 8:11] = np.asarray(n, f32).view(u32)
    for c, v in zip(range(11, 16), (k0, k1, x, s, ray)):
        rec[:, c] = np.asarray(v, np.uint64).astype(u32)
    return rec


def unit_vectors(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(f32)


def tangents(rng, n_vec):
    """A unit tangent per normal (float64 arithmetic, rounded once)."""
    n64 = n_vec.astype(np.float64)
    t = rng.normal(size=n64.shape)
    t -= n64 * (t * n64).sum(1, keepdims=True) / (n64 * n64).sum(1, keepdims=True)
    return t / np.linalg.norm(t, axis=1, keepdims=True)


def incoming(n_vec, tang, cos_t, scale=1.0):
    """Directions that meet the normal at cos_t: -(cos * n + sin * t) * scale, in float64 and rounded once."""
    c = np.asarray(cos_t, np.float64)[:, None]
    s = np.sqrt(np.maximum(0.0, 1.0 - c * c))
    return (-(c * n_vec.astype(np.float64) + s * tang) * np.asarray(scale, np.float64).reshape(-1, 1)).astype(f32)


def _from_pool(rng, setting, name, count, distinct=True):
    pl = pools()[setting][name]
    size = pl["x"].shape[0]
    idx = rng.permutation(size)[:count] if distinct and count <= size else rng.integers(0, size, count)
    return pl["x"][idx], pl["s"][idx]


def wave_layout(rng, n_owners, placement, others, depth, try1, setting):
    """One wave of Lambert lanes: (live [64] bool, x [64], s [64]).  An owner is a lane whose first accepted try lies behind the tries its own
    lane makes (try 0, and try 1 where try1 == 1).  Idle lanes carry garbage words: all ones or random."""
    if placement == "low":
        own = np.arange(n_owners)
    elif placement == "high":
        own = np.arange(64 - n_owners, 64)
    elif placement == "stride":
        own = (np.arange(n_owners) * 64) // max(n_owners, 1) + (0 if n_owners in (0, 64) else (63 - ((n_owners - 1) * 64) // n_owners) // 2)
    else:
        own = np.sort(rng.permutation(64)[:n_owners])
    live = np.zeros(64, bool)
    x = np.zeros(64, u32); s = np.zeros(64, u32)
    shallow = ("t23",) if try1 else ("t1", "t23")
    names = np.array([shallow[i % len(shallow)] for i in range(n_owners)], object)
    if depth == "deep8":
        names[:] = "ge8"
    elif depth == "deep16":
        names[rng.permutation(n_owners)[:min(n_owners, 1 + int(rng.integers(0, 4)))]] = "ge16"
    elif depth == "half12":
        names[rng.permutation(n_owners)[:(n_owners + 1) // 2]] = "ge12"
    for name in sorted(set(names)):
        sel = np.flatnonzero(names == name)
        x[own[sel]], s[own[sel]] = _from_pool(rng, setting, name, sel.size)
    live[own] = True
    rest = np.setdiff1d(np.arange(64), own)
    inlane = ("t0", "t1") if try1 else ("t0",)                      # lanes that the in-lane tries serve
    for k, lane in enumerate(rest):
        mode = others if others != "mix" else ("accept0", "idle")[int(rng.integers(0, 2))]
        if others == "idle_try1":
            mode = "accept0" if k % 4 == 0 else "idle"
        if mode == "accept0":
            name = "t1" if (others == "idle_try1" or (try1 and k % 2)) else inlane[0]
            xx, ss = _from_pool(rng, setting, name, 1)
            x[lane], s[lane], live[lane] = xx[0], ss[0], True
        else:
            x[lane], s[lane] = (ONES, ONES) if k % 2 else rng.integers(0, 1 << 32, 2)
    return live, x, s


@functools.lru_cache(maxsize=None)
def lambert_waves(try1):
    """Every owner count x placement x the other lanes x depth mix, Lambert lanes only.  Returns (records [waves * 64, 16], a description per wave)."""
    rng = np.random.default_rng(4100 + try1)
    recs, names = [], []
    w = 0
    for n_owners in N_OWNERS:
        for placement in PLACEMENTS:
            for others in OTHERS + (("idle_try1",) if try1 else ()):
                for depth in DEPTHS:
                    setting = w % len(SETTINGS)
                    recs.append(_lambert_wave(rng, wave_layout(rng, n_owners, placement, others, depth, try1, setting), setting))
                    names.append(f"{n_owners} owners {placement}, others {others}, {depth}, setting {setting}")
                    w += 1
    return np.concatenate(recs), names


def _lambert_wave(rng, layout, setting, material=None, rd=None):
    live, x, s = layout
    st = pools()[setting]
    n = unit_vectors(rng, 64)
    p = rng.uniform(-3, 3, (64, 3)).astype(f32)
    if rd is None:
        rd = (-n + rng.normal(scale=0.4, size=(64, 3))).astype(f32)
    idle = ~live
    k0 = np.where(idle, np.where(np.arange(64) % 2, ONES, rng.integers(0, 1 << 32, 64)), st["k0"])
    k1 = np.where(idle, np.where(np.arange(64) % 2, ONES, rng.integers(0, 1 << 32, 64)), st["k1"])
    mat = np.zeros(64, u32) if material is None else material
    return pack(mat, np.where(live, LIVE | FRONT, 0), rd, p, n, k0, k1, x, s, np.full(64, st["ray"], np.uint64))


@functools.lru_cache(maxsize=None)
def mixed_waves(kinds):
    """The shuffled-placement, mixed-others waves with the lanes' materials drawn from `kinds` (a sorted tuple of material kinds): diffuse
    lanes, fuzzed-metal lanes at a glancing angle (some absorbed after a deep try) and lanes that need no ball, in one wave."""
    _, groups = material_table()
    choice = [groups["lambert"][0], groups["checker"][0], groups["plastic"][0], groups["plastic"][2]]
    if METAL in kinds:
        choice += [groups["fuzz09"][0], groups["fuzz1"][0], groups["fuzzed"][0], groups["mirror"][0]]
    if DIELECTRIC in kinds:
        choice += [groups["glass"][0], groups["glass"][2]]
    choice = np.array(choice, u32)
    kind_of = material_field("kind")
    rng = np.random.default_rng(4200 + len(kinds))
    recs, names = [], []
    w = 0
    for n_owners in N_OWNERS:
        for depth in DEPTHS:
            setting = w % len(SETTINGS)
            layout = wave_layout(rng, n_owners, "shuffle", "mix", depth, 0, setting)
            mat = choice[rng.integers(0, choice.size, 64)]
            n = unit_vectors(rng, 64)
            cos_t = np.where(kind_of[mat] == METAL, rng.uniform(0.002, 0.3, 64), rng.uniform(0.05, 1.0, 64))
            rd = incoming(n, tangents(rng, n), cos_t)
            rec = _lambert_wave(rng, layout, setting, mat, rd)
            rec[:, 8:11] = n.view(u32)
            rec[:, 1] = np.where(layout[0], LIVE | np.where(rng.integers(0, 2, 64) == 1, FRONT, 0), 0)
            recs.append(rec); names.append(f"{n_owners} lanes with deep addresses, {depth}, setting {setting}")
            w += 1
    return np.concatenate(recs), names


# ---- records at the edges ---------------------------------------------------------------------------------------------------------------
VOLUME = 1 << 12
VOLUME_KINDS = ("lambert", "checker", "mirror", "fuzzed", "glass", "plastic")


def _counters(rng, n):
    c = [rng.integers(0, 1 << 32, n, dtype=np.uint64) for _ in range(5)]
    for col in (2, 3, 4):                                          # x, sample, ray at 0 and at their largest values
        pick = rng.integers(0, 8, n)
        c[col] = np.where(pick == 0, 0, np.where(pick == 1, ONES, c[col]))
    return c


def _ulp_step(v, k):
    """The float32 k steps from v (k may be negative), array-wise; v must be finite and the walk must not cross zero."""
    b = np.asarray(v, f32).view(np.int32)
    return np.where(b >= 0, b + k, b - k).astype(np.int32).view(f32)


@functools.lru_cache(maxsize=None)
def edge_records():
    """(records [n, 16] in a seeded shuffle, class [n] as indices into the returned list of class names)."""
    mats, groups = material_table()
    rng = np.random.default_rng(4300)
    recs, cls, names = [], [], []

    def emit(name, mat, flags, rd, p, n, ctr):
        if name not in names:
            names.append(name)
        r = pack(mat, flags, rd, p, n, *ctr)
        recs.append(r); cls.append(np.full(r.shape[0], names.index(name)))

    def normals(m):
        n = unit_vectors(rng, m)
        axes = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, -1]], f32)
        n[::16] = axes[rng.integers(0, 6, n[::16].shape[0])]
        near = unit_vectors(rng, n[1::16].shape[0]).astype(np.float64) * 0.02
        near[:, 2] = np.where(rng.integers(0, 2, near.shape[0]) == 1, 1.0, -1.0)
        n[1::16] = (near / np.linalg.norm(near, axis=1, keepdims=True)).astype(f32)        # |n.z| >= 0.999: to_world's other up vector
        return n

    # volume: per exact kind and per face, every parameter value of the kind in turn
    for kind in VOLUME_KINDS:
        for face in (FRONT, 0):
            m = VOLUME
            n = normals(m)
            ang = rng.uniform(0.0, 89.99, m); ang[::64] = 0.0; ang[1::64] = 89.99
            rd = incoming(n, tangents(rng, n), np.cos(np.radians(ang)), np.where(rng.integers(0, 2, m) == 1, rng.uniform(0.5, 2.0, m), 1.0))
            p = (rng.uniform(-5, 5, (m, 3)) * np.where(rng.integers(0, 4, (m, 1)) == 0, 100.0, 1.0)).astype(f32)
            mat = np.array(groups[kind], u32)[np.arange(m) % len(groups[kind])]
            emit("volume " + kind, mat, LIVE | face, rd, p, n, _counters(rng, m))

    # checker positions: on cell borders, negative cells and -0.0, p * inv_scale at +-2^31 and a step either side, three saturated cells that wrap
    vals = [0.0, -0.0, 1.0, -1.0, 2.0, -2.0, 3.0, 0.5, -0.5, 7.0, -7.0, float(np.nextafter(f32(1), f32(0))), float(np.nextafter(f32(-1), f32(0))), -SUB, SUB]
    big = [2.0 ** 31, -(2.0 ** 31), float(np.nextafter(f32(2.0 ** 31), f32(0))), float(np.nextafter(f32(2.0 ** 31), f32(np.inf))),
           float(np.nextafter(f32(-(2.0 ** 31)), f32(0))), float(np.nextafter(f32(-(2.0 ** 31)), f32(-np.inf))), 3e9, -3e9, 1e30, -1e30]
    m = 1024
    p = np.array(vals, f32)[rng.integers(0, len(vals), (m, 3))]
    sat = np.array(big + vals[:4], f32)[rng.integers(0, len(big) + 4, (m, 3))]
    sat[:64] = f32(3e9); sat[64:128] = f32(-3e9); sat[128:192] = (f32(3e9), f32(3e9), f32(-3e9))
    for name, pos in (("checker borders", p), ("checker saturated", sat)):
        n = normals(m)
        rd = incoming(n, tangents(rng, n), rng.uniform(0.1, 1.0, m))
        emit(name, np.full(m, groups["checker1"][0], u32), LIVE | FRONT, rd, pos, n, _counters(rng, m))

    # critical angle: glass from inside at the critical cosine +- k steps, k <= 64
    for mi in groups["critical"]:
        ior = f32(mats[mi]["p0"])
        c_crit = f32(np.sqrt(1.0 - 1.0 / (np.float64(ior) * np.float64(ior))))
        m = 129 * 8
        k = np.repeat(np.arange(-64, 65), 8)
        n = normals(m)
        rd = incoming(n, tangents(rng, n), _ulp_step(np.full(m, c_crit, f32), k).astype(np.float64))
        emit("critical angle", np.full(m, mi, u32), LIVE, rd, rng.uniform(-2, 2, (m, 3)).astype(f32), n, _counters(rng, m))

    # glancing: mirror metal with dot(rd, n) exactly 0 and +-2^-149
    m = 192
    axis = rng.integers(0, 3, m)
    n = np.zeros((m, 3), f32); n[np.arange(m), axis] = np.where(rng.integers(0, 2, m) == 1, 1, -1)
    rd = unit_vectors(rng, m); rd[np.arange(m), axis] = np.array([0.0, SUB, -SUB], f32)[np.arange(m) % 3]
    emit("glancing", np.full(m, groups["mirror"][0], u32), LIVE | FRONT, rd, rng.uniform(-2, 2, (m, 3)).astype(f32), n, _counters(rng, m))

    # fuzz 1 at 89.9 .. 89.999 degrees over the pools' addresses: dot(raw, n) on both sides of 0
    for si, st in enumerate(pools()):
        m = 256
        n = normals(m)
        rd = incoming(n, tangents(rng, n), np.cos(np.radians(rng.uniform(89.9, 89.999, m))))
        xs = [np.concatenate(v) for v in zip(*[_from_pool(rng, si, nm, c) for nm, c in (("t0", 96), ("t1", 64), ("t23", 32), ("ge8", 48), ("ge12", 8), ("ge16", 8))])]
        emit("fuzz at the surface", np.full(m, groups["fuzz1"][0], u32), LIVE | FRONT, rd, rng.uniform(-2, 2, (m, 3)).astype(f32), n,
             (np.full(m, st["k0"], np.uint64), np.full(m, st["k1"], np.uint64), xs[0], xs[1], np.full(m, st["ray"], np.uint64)))

    # near_zero: n = -normalized(accepted point), and that with one component moved by +-1, 2, 4 ... 64 steps
    for si, st in enumerate(pools()):
        take = {nm: rng.permutation(st[nm]["x"].shape[0])[:c] for nm, c in (("t0", 40), ("t1", 24), ("t23", 16), ("ge8", 16))}
        x = np.concatenate([st[nm]["x"][i] for nm, i in take.items()]); s = np.concatenate([st[nm]["s"][i] for nm, i in take.items()])
        u = vnormalized(np.concatenate([st[nm]["point"][i] for nm, i in take.items()]))
        steps = [0] + [sg * (1 << e) for e in range(7) for sg in (1, -1)]
        for comp in range(3):
            for k in steps if comp == 0 else steps[1:]:
                n = -u
                ok = np.abs(n[:, comp]) > f32(1e-30)
                n[ok, comp] = _ulp_step(n[ok, comp], k)
                m = x.shape[0]
                emit("near zero", np.zeros(m, u32), LIVE | FRONT, (u * f32(-1) + f32(0.1)).astype(f32), rng.uniform(-2, 2, (m, 3)).astype(f32), n,
                     (np.full(m, st["k0"], np.uint64), np.full(m, st["k1"], np.uint64), x, s, np.full(m, st["ray"], np.uint64)))

    # rough conductors where no transcendental result reaches the output: roughness 0, -0.0, +inf, NaN (theta_arg is 0, inf or NaN whatever ln returns)
    m = 16 * len(groups["rough"])
    n = unit_vectors(rng, m)                                       # (no zero component: the half vector's x and y are products with +-0)
    rd = incoming(n, tangents(rng, n), rng.uniform(0.05, 1.0, m))
    emit("rough", np.repeat(np.array(groups["rough"], u32), 16), LIVE | FRONT, rd, rng.uniform(-2, 2, (m, 3)).astype(f32), n, _counters(rng, m))

    # terminal kinds (only the forms whose caller does not finish them, and the product's hook)
    m = 64 * (len(groups["emissive"]) + 1)
    n = unit_vectors(rng, m)
    emit("terminal", np.repeat(np.array(groups["emissive"] + groups["null"], u32), 64), LIVE | FRONT, incoming(n, tangents(rng, n), rng.uniform(0.05, 1.0, m)),
         rng.uniform(-2, 2, (m, 3)).astype(f32), n, _counters(rng, m))

    # non-finite inputs: NaN or inf in rd, p or n, and n = 0
    base_mats = [groups["lambert"][0], groups["checker"][0], groups["mirror"][0], groups["fuzzed"][0], groups["glass"][0], groups["plastic"][0], groups["rough"][0]]
    m = 16
    for mi in base_mats:
        for field in range(3):
            for bad in (np.nan, np.inf, -np.inf):
                n = unit_vectors(rng, m)
                v = [incoming(n, tangents(rng, n), rng.uniform(0.1, 1.0, m)), rng.uniform(-2, 2, (m, 3)).astype(f32), n]
                v[field] = v[field].copy()
                v[field][np.arange(m), rng.integers(0, 3, m)] = bad
                emit("non-finite", np.full(m, mi, u32), LIVE | FRONT, v[0], v[1], v[2], _counters(rng, m))
        n = np.zeros((m, 3), f32)
        emit("non-finite", np.full(m, mi, u32), LIVE | FRONT, unit_vectors(rng, m), rng.uniform(-2, 2, (m, 3)).astype(f32), n, _counters(rng, m))

    recs = np.concatenate(recs); cls = np.concatenate(cls)
    order = np.random.default_rng(4301).permutation(recs.shape[0])
    return recs[order], cls[order], names


# ---- the reference and the comparison ---------------------------------------------------------------------------------------------------
def reference(oracle_mod, mats_c, records):
    """The probe's expected output: the oracle's record, and the accepted unit-ball point where the oracle's event drew tries.  Also returns
    the tries per record (0: no ball) and the generator words drawn."""
    rec = np.ascontiguousarray(records, u32)
    live = (rec[:, 1] & LIVE) != 0
    want = np.zeros((rec.shape[0], 16), u32)
    tries = np.zeros(rec.shape[0], np.int64); words = np.zeros(rec.shape[0], np.int64)
    if live.any():
        o = oracle_mod.scatter_ctr_batch(mats_c, rec[live])
        words[live] = o[:, 13]
        tries[live] = o[:, 13] // 3
        o[:, 13:] = 0
        lt = tries[live]
        has = lt > 0
        if has.any():
            r = rec[live][has]
            blk = ctr_block(r[:, 11], r[:, 12], r[:, 13], r[:, 14], r[:, 15], (lt[has] - 1).astype(u32))
            o[has, 13:16] = cube_point(blk).view(u32)
        want[live] = o
    return want, tries, words


def differing(got, want, words=16):
    """Per record: does any of the first `words` output words differ?  A NaN matches any NaN; everything else is compared as bits."""
    g, w = np.asarray(got, u32)[:, :words], np.asarray(want, u32)[:, :words]
    both_nan = np.isnan(g.view(f32)) & np.isnan(w.view(f32))
    return ((g != w) & ~both_nan).any(1)


def owners_of(tries, try1):
    """Lanes that still need a try after the tries their own lane makes."""
    return tries > (2 if try1 else 1)


def for_form(form, records):
    """The records a form may be fed: kinds in its material set, no terminal kind where its caller finishes those, no texture."""
    kind = material_field("kind")[records[:, 0]]
    ok = ((form["mats"] >> kind) & 1).astype(bool) & (kind != TEXTURE)
    if form["terminal_done"]:
        ok &= ~np.isin(kind, TERMINAL)
    return ok
