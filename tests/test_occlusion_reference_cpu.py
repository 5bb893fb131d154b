"""The reference of the occlusion tests (tests/occlusion_ref.py) against the oracle, without a GPU: the numpy pcg4d is the oracle's, the float
mapping is exact, the 16-try fallback is reachable and gives d = N, and the definition of the ambient-occlusion pass behaves like ambient
occlusion on cornell-box (a sanity gate on the DEFINITION; the kernels are compared with it bit for bit in tests/test_gpu_occlusion.py)."""
import numpy as np

import occlusion_ref as R
from conftest import load_for_both, pkg
from test_gpu_ray_queries import camera_dirs, oracle_hits, own_materials

F = np.float32
U = np.uint32


def test_numpy_pcg4d_is_the_oracles(oracle_mod):
    rng = np.random.default_rng(8)
    args = rng.integers(0, 2 ** 32, (300, 4), dtype=np.uint64).astype(U)
    args[:8] = [[0, 0, 0, 0], [0xFFFFFFFF] * 4, [1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1], [799, 599, 255 * 16 + 15, 7], [0x80000000, 1, 2, 3]]
    got = np.stack(R.pcg4d(args[:, 0], args[:, 1], args[:, 2], args[:, 3]), axis=1)
    assert got.dtype == U
    for a, g in zip(args, got):
        assert g.tolist() == oracle_mod.pcg4d(int(a[0]), int(a[1]), int(a[2]), int(a[3])).tolist(), a
    # broadcasting, as ao_directions uses it: scalars against a [samples, tries] counter
    s = np.arange(4, dtype=U)[:, None] * U(16) + np.arange(16, dtype=U)[None, :]
    w = R.pcg4d(U(5), U(7), s, U(9))
    assert w[0].shape == (4, 16) and [int(v[3, 11]) for v in w] == oracle_mod.pcg4d(5, 7, 3 * 16 + 11, 9).tolist()


def test_the_float_mapping_is_exact_and_stays_in_range():
    m = np.concatenate([np.arange(0, 4096), np.arange(2 ** 23 - 2048, 2 ** 23 + 2048), np.arange(2 ** 24 - 4096, 2 ** 24),
                        np.random.default_rng(1).integers(0, 2 ** 24, 20000)]).astype(np.uint64)
    words = ((m << np.uint64(8)) | np.uint64(0xA5)).astype(U)                                  # the low 8 bits are dropped
    c = R.ball_floats(words)
    assert c.dtype == F
    exact = m.astype(np.float64) * 2.0 ** -23 - 1.0                                             # m * 2^-23 - 1, representable for every 24-bit m
    assert (c.astype(np.float64) == exact).all()
    assert c.min() == F(-1.0) and c.max() == F(1.0 - 2.0 ** -23) and (c >= F(-1.0)).all() and (c < F(1.0)).all()
    assert R.ball_floats(np.array([0, 0xFF, 0x80000000, 0xFFFFFFFF], U)).tolist() == [-1.0, -1.0, 0.0, float(F(1.0 - 2.0 ** -23))]


def test_the_fallback_after_sixteen_tries_gives_the_normal():
    corner = U(0xFFFFFF00)                                                                      # c = (1 - 2^-23) three times: l2 > 1
    centre = U(0x80000000)                                                                      # c = 0: l2 = 0
    calls = []

    def stub(x, y, z, w):
        z = np.asarray(z, U)
        calls.append(z.copy())
        sample, j = z // U(16), z % U(16)
        # sample 0 never qualifies, sample 1 qualifies at its last try, sample 2 at its first, sample 3 at try 5 (and again later: the FIRST counts)
        ok = ((sample == 1) & (j == 15)) | ((sample == 2) & (j == 0)) | ((sample == 3) & (j >= 5))
        word = np.where(ok, centre, corner).astype(U)
        return word, np.where(ok & (sample == 3), U(0x80000000) + (j << U(12)), word).astype(U), word, word

    n = np.array([0.25, -0.5, 0.75], F)
    d = R.ao_directions(3, 4, 4, 0, n, words=stub)
    assert calls and calls[0].shape == (4, 16) and calls[0][2, 7] == 2 * 16 + 7
    assert d.dtype == F and d[0].tolist() == n.tolist()                                        # 16 tries failed: v = 0, d = N
    assert d[1].tolist() == n.tolist() and d[2].tolist() == n.tolist()                          # v = (0, 0, 0) drawn, at the last / the first try
    want = n + np.array([0.0, float(R.ball_floats(U(0x80000000 + (5 << 12)))), 0.0], F)
    assert d[3].tolist() == want.tolist()
    # with the real generator the fallback is out of reach for a test (a try fails with probability 1 - pi / 6): every sample of a pixel qualifies early
    real = R.ao_directions(3, 4, 256, 0, n)
    assert (np.linalg.norm((real - n).astype(np.float64), axis=1) < 1.0).all() and len(np.unique(real, axis=0)) == 256


def test_the_definition_darkens_the_floor_along_the_walls(oracle_mod, abi):
    """cornell-box 32 x 24, 16 samples, radius +inf: pixels on the open floor have a strictly larger mean than floor pixels within two pixels of
    a wall-floor edge, and every value is a multiple of 1/16 in [0, 1]."""
    b = pkg("build"); b.build_host()
    host = pkg("host")
    W, H, S = 32, 24, 16
    sc = own_materials(abi, load_for_both("cornell", oracle_mod, host, width=W, height=H, spp=1, max_depth=1))
    dirs = camera_dirs(sc.camera, W, H).reshape(-1, 3)
    origins = np.tile(np.array(list(sc.camera.position), F), (W * H, 1))
    hits = oracle_hits(("occlusion cornell camera", W, H), oracle_mod, abi, sc, origins, dirs)
    ref = R.AoReference(oracle_mod, sc)
    ao = ref.ao(hits, W, list(range(H)), S, 0, np.inf)
    assert ao.dtype == F and ref.calls == int((hits["primitive"] != abi.NO_HIT).sum()) * S
    assert ((ao >= 0) & (ao <= 1)).all() and (ao * S == np.round(ao * S)).all()
    assert (ao[hits["primitive"] == abi.NO_HIT] == 1.0).all() and (hits["primitive"] == abi.NO_HIT).any()
    prim = hits["primitive"].reshape(H, W).astype(np.int64)
    prim[prim == abi.NO_HIT] = -1
    floor = int(prim[H - 1, W // 2])
    assert sc.c.primitives[floor].kind == abi.PRIM_QUAD and abs(hits["normal"].reshape(H, W, 3)[H - 1, W // 2, 1]) == 1.0
    quads = [i for i in range(sc.c.n_primitives) if sc.c.primitives[i].kind == abi.PRIM_QUAD]
    ny = {i: np.abs(hits["normal"][hits["primitive"] == i][:, 1]).max() for i in quads if (hits["primitive"] == i).any()}
    walls = [i for i, v in ny.items() if v < 0.5]                                               # the upright quads: left, right and back wall
    assert len(walls) == 3
    is_wall = np.isin(prim, walls)
    near = np.zeros((H, W), bool)                                                               # within two pixels of a wall pixel
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            sh = np.zeros((H, W), bool)
            ys, yd = slice(max(dy, 0), H + min(dy, 0)), slice(max(-dy, 0), H + min(-dy, 0))
            xs, xd = slice(max(dx, 0), W + min(dx, 0)), slice(max(-dx, 0), W + min(-dx, 0))
            sh[yd, xd] = is_wall[ys, xs]
            near |= sh
    a = ao.reshape(H, W)
    edge, open_floor = a[(prim == floor) & near], a[(prim == floor) & ~near]
    print("floor pixels at an edge", len(edge), "mean", edge.mean(), "open floor", len(open_floor), "mean", open_floor.mean())
    assert len(edge) >= 8 and len(open_floor) >= 8
    assert open_floor.mean() > edge.mean()
