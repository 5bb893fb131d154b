"""The oracle's side of the wave probe's cases (tests/scatter_wave_cases.py; the device's side is tests/test_gpu_scatter_wave.py):

  * the module's numpy generator is the oracle's, word for word, and the pools' first accepted tries and points are what kat_f32's sequential
    loop finds;
  * the address search meets its conditions (>= 64 addresses whose first accepted try is 8 or later, >= 64 at 12 or later, >= 8 at 16 or later,
    per setting);
  * the oracle's batched hook returns what oracle_scatter_ctr returns, and on pool records -- deep tries included -- what kat_f32's
    formulas give, bit for bit;
  * a census of the oracle's answers over the edge records: each side of each decision the records were built to approach occurs at least
    32 times, so the GPU comparison cannot pass vacuously;
  * the forms the probe instantiates cover every kernel of test_gpu_variant_matrix.CAPABILITY with that kernel's material set.
"""
import ctypes as C

import numpy as np

import kat_f32 as K
import scatter_wave_cases as W
import test_gpu_rng_stepped as S
import test_gpu_variant_matrix as V

f32, u32 = np.float32, np.uint32


def test_numpy_generator_is_the_oracles(oracle_mod):
    rng = np.random.default_rng(5)
    a = rng.integers(0, 1 << 32, (64, 6), dtype=np.uint64)
    a[:6, :4] = np.array(S.PATHS, np.uint64)
    a[6:12, 4] = (0, 1, 30, 2 ** 32 - 1, 2 ** 16, 2)
    a[12:18, 5] = (0, 1, 63, 64, 2 ** 24, 2 ** 32 - 1)
    got = np.stack(W.pcg4d(*[a[:, c] for c in range(4)]), -1)
    blk = np.stack(W.ctr_block(*[a[:, c] for c in range(6)]), -1)
    for i, row in enumerate(a):
        r = [int(v) for v in row]
        assert np.array_equal(got[i], oracle_mod.pcg4d(*r[:4])), r
        assert np.array_equal(blk[i], oracle_mod.ctr_block(*r, gen=2)), r
        assert list(blk[i]) == K.ctr_block(*r), r
    w = rng.integers(0, 1 << 32, 4096, dtype=np.uint64).astype(u32)
    L = oracle_mod.lib()
    assert all(W.range11(w)[i] == L.oracle_u32_to_range11(int(w[i])) and W.u01(w)[i] == L.oracle_u32_to_f01(int(w[i])) for i in range(256))
    v = rng.normal(size=(64, 3)).astype(f32)
    v[:4] *= f32(1e-5)
    for a3, b3 in zip(v, W.vnormalized(v)):
        assert np.array_equal(K.normalized(a3).view(u32), b3.view(u32))
    assert (S.PATHS[5][0], S.PATHS[5][1]) == W.SETTINGS[2][:2] and W.SETTINGS[1] == (W.ONES, W.ONES, 30) and W.SETTINGS[2][2] == 2 ** 32 - 1


def test_the_search_meets_its_conditions():
    pools = W.pools()
    assert len(pools) >= 3
    for st in pools:
        sizes = {name: st[name]["x"].shape[0] for name in W.POOL_NAMES}
        assert sizes["ge8"] >= 64 and sizes["ge12"] >= 64 and sizes["ge16"] >= 8, sizes
        assert sizes["t0"] >= 1024 and sizes["t1"] >= 1024 and sizes["t23"] >= 1024, sizes
        assert (st["t0"]["first"] == 0).all() and (st["t1"]["first"] == 1).all() and np.isin(st["t23"]["first"], (2, 3)).all()
        assert (st["ge8"]["first"] >= 8).all() and (st["ge12"]["first"] >= 12).all() and (st["ge16"]["first"] >= 16).all()
        assert st["max_first"] == st["ge16"]["first"].max() >= 16
    assert (1 << W.SEARCH_LOG2) <= 2 ** 22


def test_pool_points_are_the_sequential_loops(oracle_mod):
    """kat_f32's rejection loop (Python integers, float32 scalars) stops at the pool's try with the pool's point -- the deepest addresses included."""
    for st in W.pools():
        for name in W.POOL_NAMES:
            pl = st[name]
            order = np.argsort(-pl["first"], kind="stable")[:6]
            for i in order:
                d = K.CtrDraws(st["k0"], st["k1"], int(pl["x"][i]), int(pl["s"][i]), st["ray"])
                for j in range(int(pl["first"][i])):
                    w = d.block(j)
                    p = K.V(K.range11(w[1]), K.range11(w[2]), K.range11(w[3]))
                    assert not K.dot(p, p) < f32(1.0)
                assert np.array_equal(d.unit_ball().view(u32), pl["point"][i].view(u32))


def _kat(kind, m, rd, p, n, front, draws):
    if kind == W.LAMBERT:
        return K.scatter_lambert(K.V(*m["albedo"]), rd, p, n, draws)
    if kind == W.METAL:
        return K.scatter_metal(K.V(*m["albedo"]), f32(m["p0"]), rd, p, n, draws)
    if kind == W.DIELECTRIC:
        return K.scatter_dielectric(f32(m["p0"]), front, rd, p, n, draws)
    return K.scatter_plastic(K.V(*m["albedo"]), f32(m["p0"]), rd, p, n, draws)


def test_oracle_is_kat_f32_on_pool_records(oracle_mod, abi):
    mats, groups = W.material_table()
    mats_c = W.materials_ctypes(abi)
    rng = np.random.default_rng(6)
    recs = []
    for si, st in enumerate(W.pools()):
        for name in W.POOL_NAMES:
            pl = st[name]
            idx = np.argsort(-pl["first"], kind="stable")[:4]
            for mi in (groups["lambert"][0], groups["lambert"][1], groups["fuzzed"][0], groups["fuzz09"][0], groups["mirror"][0], groups["glass"][0], groups["plastic"][0]):
                m = idx.size
                n = W.unit_vectors(rng, m)
                rd = W.incoming(n, W.tangents(rng, n), rng.uniform(0.02, 1.0, m), rng.uniform(0.5, 2.0, m))
                recs.append(W.pack(np.full(m, mi, u32), W.LIVE | (si & 1), rd, rng.uniform(-2, 2, (m, 3)).astype(f32), n,
                                   np.full(m, st["k0"], np.uint64), np.full(m, st["k1"], np.uint64), pl["x"][idx], pl["s"][idx], np.full(m, st["ray"], np.uint64)))
    recs = np.concatenate(recs)
    want, tries, words = W.reference(oracle_mod, mats_c, recs)
    L = oracle_mod.lib()
    deep = 0
    for r, o, t in zip(recs, want, tries):
        m = mats[int(r[0])]
        rd, p, n = r[2:5].view(f32), r[5:8].view(f32), r[8:11].view(f32)
        ctr = [int(v) for v in r[11:16]]
        draws = K.CtrDraws(*ctr)
        ok, ko, kd, ka = _kat(m["kind"], m, rd, p, n, bool(r[1] & 1), draws)
        assert o[0] == (f32(1.0).view(u32) if ok else 0), (m, ctr)
        if ok:
            assert np.array_equal(np.concatenate([ko, kd, ka]).astype(f32).view(u32), o[1:10]), (m, ctr)
        else:
            assert not o[1:10].any()
        if t:
            assert np.array_equal(draws.unit_ball().view(u32), o[13:16]), (m, ctr)
        deep += t > 12
        single = np.zeros(10, f32)
        z = np.zeros(3, f32)
        assert L.oracle_scatter_ctr(C.byref(mats_c[int(r[0])]), z.ctypes.data, rd.copy().ctypes.data, p.copy().ctypes.data, n.copy().ctypes.data, int(r[1] & 1), *ctr,
                                    single.ctypes.data) == 0
        assert np.array_equal(single.view(u32), o[:10])
    assert deep >= 24                                                 # Lambert and fuzzed-metal lanes whose ball came from try 12 or later


def test_forms_cover_the_variant_table(native):
    host, device = native
    forms = device.scatter_wave_forms()
    by_kernel = {f["kernel"]: f for f in forms}
    assert len(by_kernel) == len(forms) == 13
    for v, (kernel, lib, mats, prims, mesh) in V.CAPABILITY.items():
        f = by_kernel[kernel]
        assert {k for k in range(10) if (f["mats"] >> k) & 1} == set(mats), kernel
        assert f["terminal_done"] == (lib == "product") and f["wide"] == (lib == "product"), kernel
        assert f["try1"] == (1 if mats == V.MATS_LAMBERT else 0), kernel
    assert set(by_kernel) - {c[0] for c in V.CAPABILITY.values()} == {"k_render_sky_simple_qc", "k_render_ctr_wf_fixaabb"}
    assert by_kernel["k_render_ctr_simple_qc"]["in_place"] and not by_kernel["k_render_sky_simple_qc"]["in_place"]
    assert by_kernel["k_render_ctr_simple_qc"]["stepped"] and by_kernel["k_render_sky_simple_qc"]["stepped"]       # MI355RT_STEP_MASK's default
    assert all(by_kernel[k]["fastn"] for k in ("k_render_ctr_simple_qc", "k_render_ctr_simple", "k_render_ctr_nospec", "k_render_ctr_wf_meshfree", "k_render_ctr_nomesh", "k_render_ctr_mesh"))
    assert not any(by_kernel[k]["fastn"] for k in ("k_render_ctr_wf", "k_render_ctr_wf_fixaabb", "k_render_ctr_wf_nometal", "k_render_ctr_wf_nometal_shallow",
                                                   "k_render_ctr_wf_nometal_ident", "k_render_ctr_sm"))


def test_waves_hold_the_owner_counts_and_depths_they_name(oracle_mod, abi):
    mats_c = W.materials_ctypes(abi)
    deepest = 0
    for try1 in (0, 1):
        recs, names = W.lambert_waves(try1)
        want, tries, _ = W.reference(oracle_mod, mats_c, recs)
        own = W.owners_of(tries, try1).reshape(-1, 64).sum(1)
        first = (tries - 1).reshape(-1, 64)
        i = 0
        for n_owners in W.N_OWNERS:
            for placement in W.PLACEMENTS:
                for others in W.OTHERS + (("idle_try1",) if try1 else ()):
                    for depth in W.DEPTHS:
                        assert own[i] == n_owners, names[i]
                        live = (recs[64 * i:64 * i + 64, 1] & W.LIVE) != 0
                        if others == "idle":
                            assert live.sum() == n_owners
                        if others == "accept0":
                            assert live.all()
                        if try1 and others != "idle" and n_owners < 60:
                            assert (first[i][live] == 1).any(), names[i]             # a lane that try 1 serves, in the lane itself
                        if n_owners:
                            f = np.sort(first[i][first[i] > try1])
                            if depth == "deep8":
                                assert f[0] >= 8
                            if depth == "deep16":
                                assert f[-1] >= 16 and (f >= 16).sum() <= 4
                            if depth == "half12":
                                assert (f >= 12).sum() == (n_owners + 1) // 2
                        i += 1
        assert i == len(names)
        deepest = max(deepest, int(first.max()))
    assert deepest >= 16
    lane63 = [n for n in W.lambert_waves(0)[1] if n.startswith("1 owners high, others idle")]
    assert len(lane63) == len(W.DEPTHS)


def _dielectric_state(rec, ior):
    """material.rs:122-162 on float32 arrays, up to the decision: cos_theta, cannot_refract, reflectance, the draw, refract()'s par2."""
    with np.errstate(all="ignore"):
        rd, n = rec[:, 2:5].view(f32), rec[:, 8:11].view(f32)
        front = (rec[:, 1] & 1) != 0
        ratio = np.where(front, f32(1.0) / ior, ior / f32(1.0)).astype(f32)
        unit = W.vnormalized(rd)
        cos = np.minimum(W.vdot(-unit, n), f32(1.0))
        sin2 = f32(1.0) - cos * cos
        cannot = ratio * ratio * sin2 > f32(1.0)
        idx = f32(1.0) / ratio
        r0 = (f32(1.0) - idx) / (f32(1.0) + idx)
        r0 = r0 * r0
        om = f32(1.0) - cos
        refl = r0 + (f32(1.0) - r0) * (om * ((om * om) * (om * om)))
        u = W.u01(W.ctr_block(*[rec[:, c] for c in range(11, 16)], 0)[0])
        perp = (unit + n * cos[:, None]) * ratio[:, None]
        par2 = f32(1.0) - W.vdot(perp, perp)
    return cos, cannot, refl, u, par2


def test_branch_census(oracle_mod, abi):
    """Each side of each decision the edge records approach, counted from the oracle's answers (and from the float32 restatement of the
    dielectric's decision, itself checked against the oracle's draw count and direction).  The par2 < 0 fallback of refract() (material.rs:214)
    is taken where cannot_refract is false by a rounding: the critical-angle class reaches it."""
    mats, groups = W.material_table()
    mats_c = W.materials_ctypes(abi)
    recs, cls, names = W.edge_records()
    want, tries, words = W.reference(oracle_mod, mats_c, recs)
    out = want.view(f32)
    kind, p0 = W.material_field("kind")[recs[:, 0]], W.material_field("p0")[recs[:, 0]]
    scattered = out[:, 0] == 1
    n = recs[:, 8:11].view(f32)
    census = {}
    volume = np.isin(cls, [names.index("volume " + k) for k in W.VOLUME_KINDS])
    assert all((cls == names.index("volume " + k)).sum() == 2 * W.VOLUME for k in W.VOLUME_KINDS)

    # dielectric: the restatement agrees with the oracle (a draw is taken exactly where refraction is possible; the direction's side), then counts
    gl = (kind == W.DIELECTRIC) & (volume | (cls == names.index("critical angle")))
    cos, cannot, refl, u, par2 = _dielectric_state(recs[gl], p0[gl])
    assert np.array_equal(words[gl] == 0, cannot)
    with np.errstate(all="ignore"):
        side = W.vdot(out[gl, 4:7], n[gl])
    reflect_schlick = ~cannot & (refl > u)
    fallback = ~cannot & ~(refl > u) & (par2 < 0)
    refract = ~cannot & ~(refl > u) & ~(par2 < 0)
    clear = np.abs(side) > 1e-3
    assert (side[reflect_schlick & clear] > 0).all() and (side[fallback & clear] > 0).all()
    ordinary = np.isfinite(p0[gl]) & (p0[gl] > 0)
    assert (side[refract & clear & ordinary] < 0).all()
    census["schlick reflect"], census["refract"], census["par2 fallback"] = reflect_schlick.sum(), (refract & ordinary).sum(), fallback.sum()
    crit = cls[gl] == names.index("critical angle")
    ior = p0[gl].astype(np.float64)
    with np.errstate(all="ignore"):
        c_crit = np.sqrt(1.0 - 1.0 / (ior * ior)).astype(f32)
        near = crit & (np.abs(cos.view(np.int32).astype(np.int64) - c_crit.view(np.int32).astype(np.int64)) <= 4)
    census["critical: cannot refract"], census["critical: can refract"] = (near & cannot).sum(), (near & ~cannot).sum()

    metal = kind == W.METAL
    census["mirror scattered"], census["mirror absorbed"] = (metal & (p0 == 0) & scattered).sum(), (metal & (p0 == 0) & ~scattered).sum()
    census["fuzzed scattered"], census["fuzzed absorbed"] = (metal & (p0 > 0) & scattered).sum(), (metal & (p0 > 0) & ~scattered).sum()
    census["fuzzed absorbed after a deep try"] = (metal & (p0 > 0) & ~scattered & (tries > 8)).sum()
    assert (tries[metal & (p0 > 0)] >= 1).all() and (tries[metal & ~(p0 > 0)] == 0).all()

    plastic = kind == W.PLASTIC
    assert np.isin(words[plastic] % 3, (1,)).all()
    census["plastic reflect"], census["plastic diffuse"] = (plastic & (words == 1)).sum(), (plastic & (words >= 4)).sum()

    chk = np.isin(cls, [names.index("checker borders"), names.index("checker saturated"), names.index("volume checker")])
    on, off = np.array(W.CHECK_ON, f32).view(u32), np.array(W.CHECK_OFF, f32).view(u32)
    even, odd = chk & (want[:, 7:10] == on).all(1), chk & (want[:, 7:10] == off).all(1)
    assert (even | odd)[chk].all()
    with np.errstate(all="ignore"):
        cell = np.floor(recs[:, 5:8].view(f32) * p0[:, None])
    saturated = chk & ((np.abs(cell) >= f32(2.0 ** 31)).any(1))
    census["checker odd"], census["checker even"] = odd.sum(), even.sum()
    census["checker saturated"], census["checker not saturated"] = saturated.sum(), (chk & ~saturated).sum()
    census["checker saturated odd"], census["checker saturated even"] = (saturated & odd).sum(), (saturated & even).sum()

    nz = cls == names.index("near zero")
    assert (tries[nz] >= 1).all()
    with np.errstate(all="ignore"):
        d = n[nz] + W.vnormalized(out[nz, 13:16])
    taken = (np.abs(d) < f32(1e-8)).all(1)
    census["near_zero taken"], census["near_zero missed"] = taken.sum(), (~taken).sum()
    # (taken: the direction is the normal's -- after its two normalisations)
    nn = W.vnormalized(W.vnormalized(n[nz]))
    assert (want[nz][taken, 4:7] == nn[taken].view(u32)).all()
    assert (nz.sum() // (3 * 96)) == 43                              # one component moved by 0 and +-1, 2, 4 ... 64 steps

    rough = cls == names.index("rough")
    with np.errstate(all="ignore"):
        census["rough fallback"], census["rough theta 0"] = (rough & ~np.isfinite(p0)).sum(), (rough & (p0 == 0)).sum()
        census["rough scattered"] = (rough & scattered).sum()

    print({k: int(v) for k, v in census.items()})
    assert census["par2 fallback"] >= 1, census
    low = {k: int(v) for k, v in census.items() if v < 32 and k != "par2 fallback"}
    assert not low, (low, census)
    for c in ("glancing", "fuzz at the surface", "terminal", "non-finite"):
        assert (cls == names.index(c)).sum() >= 64
    fz = cls == names.index("fuzz at the surface")
    assert (fz & scattered).sum() >= 32 and (fz & ~scattered).sum() >= 32 and (tries[fz] >= 17).sum() >= 3
    assert np.isnan(out[cls == names.index("non-finite")]).any()
