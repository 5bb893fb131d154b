"""Cases of the surface probes (mi355rt_context_probe_rays, mi355rt_context_probe_radiance; not a test, not a conftest): the ray maker of
include/mi355rt.h in numpy float32, written from the definition there, one rounding per operation in the order written.

It extends tests/radiance_cases.py: the words of (ray 0, block j) come from oracle.ctr_block, normalized_rows is that module's.  The maker returns
abi.PATH_RAY_DTYPE [n], direction normalised once, x and row the probe's -- what mi355rt_context_probe_rays writes."""
import numpy as np

import radiance_cases as RC
import view_cases as VC

F = np.float32
TRIES = 64
EPS = F(1e-4)
NEAR_ZERO = F(1e-8)

SAMPLES = [1, 5, 17]                         # 17 crosses the sum's 16-sample trip
SEEDS = [0, (1 << 32) - 3]                   # the second carries the key into its high word for rows >= 3
COUNTS = [1, 37, None]                       # probes per call; None = the whole set
DEPTH = 6
SCENES = ["cornell", "teapot"]
W, H = 24, 16                                # the centre view the first-hit probes come from
FREE_SEED = 11                               # numpy seed of the free-space probes

_words = {}


def range11(w):
    """rand's random_range(-1.0..1.0) of a generator word (rt_rng.h u32_to_range11): (w >> 9) * 2^-22 - 1, every step exact."""
    return (np.asarray(w, np.uint32) >> np.uint32(9)).astype(F) * F(2.0 ** -22) - F(1.0)


def block_words(oracle_mod, probes, s, seed, j, rows=None):
    """uint32 [n, 4]: the words of (ray 0, block j) of sample s of the probes `rows` (default: all); ykey = row + seed."""
    idx = np.arange(len(probes)) if rows is None else np.asarray(rows)
    out = np.zeros((len(idx), 4), np.uint32)
    for k, i in enumerate(idx):
        x, row = int(probes["x"][i]), int(probes["row"][i])
        key = (x, row, s, seed, j)
        if key not in _words:
            ykey = (row + seed) & 0xFFFFFFFFFFFFFFFF
            _words[key] = oracle_mod.ctr_block(ykey & 0xFFFFFFFF, ykey >> 32, x, s, 0, j)
        out[k] = _words[key]
    return out


def ball_points(n, block_source, tries=TRIES):
    """(p float32 [n, 3], try number int [n]): rejection in the unit ball.  block_source(j, rows) -> uint32 [len(rows), 4], the words of (ray 0, block j)
    of the probes `rows`; try j takes p = (r(w1), r(w2), r(w3)) and is accepted on (px*px + py*py) + pz*pz < 1; after `tries` rejected tries p = 0 and the
    try number is `tries`."""
    p = np.zeros((n, 3), F)
    tried = np.full(n, tries, np.int64)
    open_ = np.arange(n)
    for j in range(tries):
        if not len(open_):
            break
        w = np.asarray(block_source(j, open_), np.uint32)
        q = np.stack([range11(w[:, 1]), range11(w[:, 2]), range11(w[:, 3])], axis=1)
        assert q.dtype == F
        ok = (q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2] < F(1.0)
        p[open_[ok]], tried[open_[ok]] = q[ok], j
        open_ = open_[~ok]
    return p, tried


def probe_rays(oracle_mod, abi, probes, s, seed=0, block_source=None, want=False):
    """abi.PATH_RAY_DTYPE [n]: the ray of sample s of every probe.  want: also (p, try number, near_zero mask)."""
    n = len(probes)
    src = block_source or (lambda j, rows: block_words(oracle_mod, probes, s, seed, j, rows))
    p, tried = ball_points(n, src)
    N, P = np.ascontiguousarray(probes["normal"], F), np.ascontiguousarray(probes["position"], F)
    d = N + RC.normalized_rows(p)
    nz = (np.abs(d) < NEAR_ZERO).all(axis=1)
    d = np.where(nz[:, None], N, d)
    assert d.dtype == F
    rays = np.zeros(n, abi.PATH_RAY_DTYPE)
    rays["origin"] = P + N * EPS
    rays["direction"] = RC.normalized_rows(d)
    rays["x"], rays["row"] = probes["x"], probes["row"]
    return (rays, p, tried, nz) if want else rays


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------
def first_hit_probes(oracle_mod, abi, sc):
    """Probes at the first hits of the W x H centre view of `sc` through the oracle's scene_hit, misses dropped; built as abi.probes_from_hits builds them."""
    rays = VC.pinhole_rays(oracle_mod, abi, sc.camera, W, H, 0, 0, centre=True)
    hits = np.zeros(W * H, abi.HIT_DTYPE)
    hits["primitive"] = abi.NO_HIT
    for i, r in enumerate(rays):
        hit, h = oracle_mod.scene_hit(sc, r["origin"].copy(), r["direction"].copy())
        if hit:
            hits[i]["position"], hits[i]["normal"], hits[i]["primitive"] = h[0:3], h[3:6], 0
    return abi.probes_from_hits(hits, W)


def free_probes(abi, n=40, seed=FREE_SEED):
    """n free-space points inside the cornell box with random unit normals and scattered 32-bit x / row."""
    rng = np.random.default_rng(seed)
    out = np.zeros(n, abi.PROBE_DTYPE)
    out["position"] = (rng.uniform(-0.6, 0.6, (n, 3)) + np.array([0.0, 1.0, 0.0])).astype(F)
    out["normal"] = RC.normalized_rows(rng.normal(size=(n, 3)).astype(F))
    out["x"] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    out["row"] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    return out


def odd_probes(abi):
    """A normal of length 2 and a zero normal: the normal is used as given."""
    out = np.zeros(2, abi.PROBE_DTYPE)
    out["position"] = [[0.1, 1.0, 0.2], [-0.2, 0.8, 0.1]]
    out["normal"] = [[0.0, 2.0, 0.0], [0.0, 0.0, 0.0]]
    out["x"], out["row"] = [5, 0xFFFFFFFE], [0xFFFFFFFF, 2]
    return out


_sets = {}


def probe_set(oracle_mod, abi, name, sc):
    """The whole set of a scene: its first-hit probes, the free-space probes, the two odd normals.  Built once, read-only."""
    if name not in _sets:
        out = np.concatenate([first_hit_probes(oracle_mod, abi, sc), free_probes(abi), odd_probes(abi)])
        out.setflags(write=False)
        _sets[name] = out
    return _sets[name]


def cancelling_probes(oracle_mod, abi, base, seed, s=0):
    """`base` with every normal set to -normalized(p) of the probe's own accepted try of sample s: d = N + normalized(p) is exactly zero, the
    near_zero branch runs and the ray leaves along N."""
    _, p, tried, _ = probe_rays(oracle_mod, abi, base, s, seed, want=True)
    assert (tried < TRIES).all()
    out = np.array(base, copy=True)
    out["normal"] = -RC.normalized_rows(p)
    return out


def counts(n_all):
    return [n_all if c is None else c for c in COUNTS]
