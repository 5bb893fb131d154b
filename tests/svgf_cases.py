"""Cases of the variance-guided temporal filter (include/mi355rt_svgf.h; not a test, not a conftest): tests/reproject_cases.py's frame pairs -- the
plane seen by two cameras and the records crafted onto the reprojection's decision boundaries -- plus a previous moments buffer and records crafted
onto what this stage adds: the lengths about min_temporal, moments that are not finite in one tap of two, m2 < m1 * m1, a variance of exactly 0,
and misses beside hits.  Every added record lands exactly ON a previous pixel (or exactly between two), as reproject_cases' do."""
import functools

import numpy as np

import reproject_cases as RC
import svgf_ref as SR

F = np.float32
NO_HIT = RC.NO_HIT
GREY = (0.5, 0.5, 0.5)                                  # the colour of the "variance exactly 0" record


@functools.lru_cache(maxsize=None)
def landing(k, size, vertical=False):
    """reproject_cases.landing / landing_b, remembered: the search is the same for every case of a size."""
    return RC.landing(k, size, RC.coord_y if vertical else RC.coord_x)


def grey_lum():
    return SR.lum(np.array([GREY], F))[0]


def random_moments(rng, n):
    """{m1, m2} with m2 >= m1 * m1, and a sprinkle of moments that are not finite."""
    m = np.empty((n, 2), F)
    m[:, 0] = rng.random(n, dtype=F)
    m[:, 1] = m[:, 0] * m[:, 0] + rng.random(n, dtype=F) * F(0.1)
    odd = rng.random(n)
    m[odd < 0.02, 0] = np.nan
    m[(odd > 0.02) & (odd < 0.03), 1] = np.inf
    return m


def items(min_temporal):
    """(name, taps, previous length, previous moments per tap, colour or None).  taps 1: the record lands ON a previous pixel; 2: exactly between two
    (tx = 0.5, ty = 0), both with the same length."""
    l = grey_lum()
    mt = float(min_temporal)
    return [
        ("n == min_temporal - 1", 1, mt - 2.0, [(0.4, 0.2)], None),           # a length below 1 is no history at all (min_temporal <= 2)
        ("n == min_temporal", 1, mt - 1.0, [(0.4, 0.2)], None),
        ("n == min_temporal + 1", 1, mt, [(0.4, 0.2)], None),
        ("m1 +inf in one tap of two", 2, 9.0, [(np.inf, 0.2), (0.4, 0.2)], None),
        ("m2 NaN in one tap of two", 2, 9.0, [(0.4, 0.2), (0.4, np.nan)], None),
        ("m1 -inf in the only tap", 1, 9.0, [(-np.inf, 0.2)], None),
        ("m2 < m1 * m1", 1, 10.0, [(0.5, 0.1)], None),
        ("variance exactly 0", 1, 10.0, [(l, l * l)], GREY),
    ]


def build(abi, cur_size, prev_size, max_history=32, min_temporal=4, seed=0, crafted=True):
    """reproject_cases.build(...)'s dict plus moments_prev, params (an abi.SvgfAccumulateParams with reproject_cases' normal_min and plane_tolerance)
    and `added`: [(name, current pixel, [previous pixels])] of the records above that fitted.  Two current pixels in the last row become misses
    beside hits where the frame has room."""
    case = RC.build(abi, cur_size, prev_size, max_history, seed, crafted)
    (W, H), (Wp, Hp) = cur_size, prev_size
    rng = np.random.default_rng(77 + 1000 * W + 10 * Wp + seed)
    moments = random_moments(rng, Wp * Hp)
    hits_cur, hits_prev, hist, color = case["hits_cur"], case["hits_prev"], case["hist_prev"], case["color_cur"]
    used = {q for _, _, q, _ in case["placed"] if q is not None}
    for q in used:                                                      # reproject_cases' crafted previous pixels carry sound moments: their items decide by the history alone
        moments[q] = (0.4, 0.2)
    j = len(case["placed"])
    added = []

    def record(buf, i, a, b, t):
        r = buf[i:i + 1]
        r["position"], r["t"], r["normal"], r["front_face"], r["primitive"], r["material"] = (a, b, 0.0), t, (0, 0, 1), 1, RC.PRIM, 1

    for name, taps, length, mm, colour in items(min_temporal) if crafted else []:
        if j >= W * H:
            break
        spot = None
        for q in range(Wp * Hp - 1):
            qs = [q] if taps == 1 else [q, q + 1]
            if any(p in used for p in qs) or (taps == 2 and q % Wp == Wp - 1):
                continue
            a = landing(q % Wp + (0.5 if taps == 2 else 0.0), Wp)
            b = landing(q // Wp, Hp, True)
            own = [(landing(p % Wp, Wp), landing(p // Wp, Hp, True)) for p in qs]
            if a is not None and b is not None and all(o[0] is not None and o[1] is not None for o in own):
                spot = (qs, a, b, own)
                break
        if spot is None:
            break
        qs, a, b, own = spot
        used.update(qs)
        record(hits_cur, j, a, b, 2.0)
        if colour is not None:
            color[j] = colour
        for p, (pa, pb), m in zip(qs, own, mm):
            record(hits_prev, p, pa, pb, 1.0)
            hist[p, :3], hist[p, 3] = (0.25, 0.5, 0.75), length
            moments[p] = m
        added.append((name, j, qs))
        j += 1
    if crafted and W * H >= 64:
        for i in (W * H - 2, W * H - 1):                                # misses beside hits (and beside each other)
            m = hits_cur[i:i + 1]
            m["primitive"], m["material"], m["t"] = NO_HIT, NO_HIT, np.inf
    case["moments_prev"] = moments
    case["params"] = abi.SvgfAccumulateParams.make(max_history, RC.NORMAL_MIN, RC.PLANE_TOLERANCE, min_temporal)
    case["reproject_params"] = abi.ReprojectParams.make(max_history, RC.NORMAL_MIN, RC.PLANE_TOLERANCE)
    case["added"] = added
    return case


def reference(case, prev=True):
    """svgf_ref.accumulate of the case: (hist_out, moments_out, variance_out, way)."""
    if not prev:
        return SR.accumulate(case["cur"], None, case["hits_cur"], case["color_cur"], params=case["params"])
    return SR.accumulate(case["cur"], case["prev"], case["hits_cur"], case["color_cur"], case["hits_prev"], case["hist_prev"], case["moments_prev"], case["params"])


# ---- rough guides: what the plane cannot give the geometry weight ------------------------------------------------------------------------------
# The cases above are a plane with one normal and records with the opposite one: nd is +-1 and d is 0, so G(p, q) is 0 or 1 and normal_squarings,
# sigma_plane, t_p and the absolute value never matter.  The two makers below give G thousands of values strictly inside (0, 1)
# (tests/test_svgf_rough_cpu.py measures it).
ROUGH_SEED = 11                                         # of rough(): every size of ROUGH_SIZES meets test_svgf_rough_cpu's conditions with it
BUMPY_SEED = 5
ROUGH_SIZES = [(1, 37), (37, 1), (33, 9), (70, 17), (131, 70)]     # a column, a row, one past the 32 x 8 tile each way, 9 ragged tiles, 45 ragged tiles
BUMPY_SIZES = [((33, 9), (33, 9)), ((70, 17), (70, 17)), ((33, 9), (20, 7))]
_rough = {}


def rough(abi, W, H, seed=ROUGH_SEED):
    """(hist float32 [n, 4], variance float32 [n], hits HIT_DTYPE [n], colour float32 [n, 3]), read-only and computed once: denoise_cases.synthetic's
    colour and records unchanged -- tilted and NaN normals, t = 0 / NaN / inf, coincident positions, runs of misses; negative, denormal and non-finite
    colours -- the history that colour with length 1, and a seeded variance: uniform in [0, 0.05), exactly 0 in the left quarter of the columns, and, at
    a few pixels each chosen as synthetic chooses its own, 1e30, a denormal, negative values, NaN, +inf (e is inf: a = 0) and -inf -- what
    accumulate never writes and the filter's header leaves to the caller."""
    import denoise_cases
    key = (W, H, seed)
    if key not in _rough:
        lin, hits = denoise_cases.synthetic(abi, W, H, seed)
        n = W * H
        colour = lin.reshape(n, 3)
        hist = np.ones((n, 4), F)
        hist[:, :3] = colour
        rng = np.random.default_rng(7919 + seed)
        var = (rng.random(n, dtype=F) * F(0.05)).astype(F)
        var.reshape(H, W)[:, : W // 4] = F(0.0)

        def pick(k):
            return rng.choice(n, size=min(k, n), replace=False)
        if n >= 4:
            few = max(n // 60, 1)
            i = pick(few); var[i] = F(1e30)
            i = pick(few); var[i] = F(1e-40)
            i = pick(max(n // 40, 1)); var[i] = -var[i] - F(0.01)
            i = pick(few); var[i] = F(np.nan)
            i = pick(few); var[i] = F(np.inf)
            i = pick(few); var[i] = F(-np.inf)
        else:
            var[0] = F(-0.25)
        for a in (hist, var):
            a.setflags(write=False)
        _rough[key] = (hist, var, hits, colour)
    return _rough[key]


def bumpy(abi, cur_size, prev_size, max_history=32, min_temporal=4, seed=BUMPY_SEED, flat=None):
    """build(...) with every record that is neither crafted (`placed`, `added`, the two misses) nor a miss perturbed, in both frames: each component of
    the normal + N(0, 0.15), renormalised in float64 and rounded once; position.z + N(0, 0.01).  The crafted records keep their decision boundaries;
    around them the taps' nd and d, and the spatial estimate's G, take values strictly inside their ranges.  flat: build(...)'s dict of the same arguments
    where the caller has it already (it is copied, not changed)."""
    case = build(abi, cur_size, prev_size, max_history, min_temporal) if flat is None else {k: v.copy() if isinstance(v, np.ndarray) else v for k, v in flat.items()}
    rng = np.random.default_rng(seed)
    n_cur = cur_size[0] * cur_size[1]
    kept_cur = {j for _, j, _, _ in case["placed"]} | {j for _, j, _ in case["added"]} | ({n_cur - 2, n_cur - 1} if n_cur >= 64 else set())
    kept_prev = {q for _, _, q, _ in case["placed"] if q is not None} | {q for _, _, qs in case["added"] for q in qs}
    for hits, kept in ((case["hits_cur"], kept_cur), (case["hits_prev"], kept_prev)):
        rough_ones = hits["primitive"] != NO_HIT
        rough_ones[sorted(kept)] = False
        k = int(rough_ones.sum())
        nrm = hits["normal"][rough_ones].astype(np.float64) + rng.normal(0.0, 0.15, (k, 3))
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        pos = hits["position"][rough_ones].astype(np.float64)
        pos[:, 2] += rng.normal(0.0, 0.01, k)
        hits["normal"][rough_ones], hits["position"][rough_ones] = nrm.astype(F), pos.astype(F)
    return case


# ---- the quality case: tests/test_reproject_cpu.py's setting, entirely on the CPU -----------------------------------------------------------
def orbit_frames(oracle_mod, abi, host):
    """cornell at 64 x 48, 8 frames of 1 spp along the 0.5-degree orbit from the oracle (seed = frame number), and the oracle's 256 spp of every
    frame's camera: [(view, hits, raw float32 [n, 3], truth float32 [n, 3])].  The setting, the seeds and the records are test_reproject_cpu's."""
    import test_reproject_cpu as T
    from conftest import SCENES
    from oracle import scene_loader
    from parity import oracle_threads
    sc = host.LoadedScene(SCENES["cornell"], T.Q_W, T.Q_H, 1, T.Q_DEPTH)
    fov = float(np.degrees(2.0 * np.arctan(sc.camera.half_height)))
    aspect = sc.camera.half_width / sc.camera.half_height
    frames = []
    for k in range(T.Q_FRAMES):
        cam = RC.orbit_camera(sc.camera, k, T.Q_STEP_DEG, scene_loader, fov, aspect)
        v = abi.View.make(cam, T.Q_W, T.Q_H, abi.VIEW_PINHOLE, abi.VIEW_CENTRE)
        _, raw, _ = oracle_mod.render(sc, cam, abi.Settings(T.Q_W, T.Q_H, 1, T.Q_DEPTH), abi.Options.make(seed=k), threads=oracle_threads())
        _, want, _ = oracle_mod.render(sc, cam, abi.Settings(T.Q_W, T.Q_H, T.Q_REF_SPP, T.Q_DEPTH), abi.Options.make(seed=1000), threads=oracle_threads())
        frames.append((v, T.oracle_hits(oracle_mod, abi, sc, cam, T.Q_W, T.Q_H), raw.reshape(-1, 3).copy(), want.reshape(-1, 3).copy()))
    return frames


def quality_chain(frames, sigmas):
    """Per frame: (RMSE of the raw frame, of the reprojected image, of the existing route reproject_ref -> denoise_ref at its defaults, {sigma_luminance:
    RMSE of svgf_ref.accumulate -> svgf_ref.filter}), each against that frame's truth.  The plain history is fed back, as the header says."""
    import denoise_ref
    import reproject_ref as RR
    rows = []
    hist = moments = hits_prev = view_prev = rr_hist = None
    for v, hits, raw, truth in frames:
        W, H = v.width, v.height
        rr_hist = RR.reproject(v, view_prev, hits, raw, hits_prev, rr_hist)
        hist, moments, var, _ = SR.accumulate(v, view_prev, hits, raw, hits_prev, hist, moments)
        assert hist.tobytes() == rr_hist.tobytes()
        old = denoise_ref.denoise(rr_hist[:, :3].reshape(H, W, 3).copy(), hits)
        new = {s: SR.filter(hist, var, hits, W, H, sigma_luminance=s) for s in sigmas}
        rows.append((SR.rmse(raw, truth), SR.rmse(hist[:, :3], truth), SR.rmse(old, truth), {s: SR.rmse(new[s], truth) for s in sigmas}))
        hits_prev, view_prev = hits, v
    return rows
