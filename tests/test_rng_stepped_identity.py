"""The identity the stepped draw address rests on (rt_rng.h, RngCtrT<true>), stated in numpy and checked without a GPU.

pcg4d starts with one LCG step per word, v -> v * A + C mod 2^32.  The step is linear, so for a word that moves by a counter

    (v + j) * A + C  ==  (v * A + C) + j * A        (mod 2^32, for every 32-bit v and j)

and a path's draws, pcg4d(base.x, base.y, base.z + r, base.w + j), are pcg4d_stepped(W0, W1, W2 + r * A, W3 + j * A) with W = the stepped
base: the device takes the step once per path, advances W2 by A per event and adds j * A per try.  The cooperative rejection reaches try j by
the owner's running word (start at try 1, + (A << lg) per failed round) plus a worker's sub * A from a 24-bit multiply, sub < 64.  Each of
these is restated here and compared with the plain form on 10^5 random (words, r, j) and on the edge values where a product or a sum wraps;
a handful of addresses also go through the oracle's own generator."""
import numpy as np

A, C = np.uint32(1664525), np.uint32(1013904223)
U = np.uint32

RAYS = [0, 1, 2, 29, 30, 31, 2 ** 16, 2 ** 32 - 1]
TRIES = [0, 1, 2, 3, 63, 64, 65, 2 ** 24 - 1, 2 ** 24, 2 ** 32 - 1]
WORDS = [0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF]


def step(v):
    return v * A + C


def rounds(x, y, z, w):
    """pcg4d after its LCG step (rt_rng.h pcg4d_stepped), on uint32 arrays (numpy wraps mod 2^32)."""
    x = x + y * w; y = y + z * x; z = z + x * y; w = w + y * z
    x = x ^ (x >> U(16)); y = y ^ (y >> U(16)); z = z ^ (z >> U(16)); w = w ^ (w >> U(16))
    x = x + y * w; y = y + z * x; z = z + x * y; w = w + y * z
    return np.stack([x, y, z, w])


def pcg4d(x, y, z, w):
    return rounds(step(x), step(y), step(z), step(w))


def inputs():
    rng = np.random.default_rng(20250)
    n = 100_000
    base = rng.integers(0, 2 ** 32, (4, n), dtype=np.uint64)
    r = rng.integers(0, 2 ** 32, n, dtype=np.uint64)
    j = rng.integers(0, 2 ** 32, n, dtype=np.uint64)
    small = rng.integers(0, 64, n, dtype=np.uint64)                       # most rays and tries of a render are small
    r[: n // 2] = small[: n // 2]; j[n // 4: 3 * n // 4] = small[n // 4: 3 * n // 4]
    edge = np.array([(a, b, c, d, rr, jj) for a in WORDS for b in (0, 0xFFFFFFFF) for c in WORDS for d in WORDS for rr in RAYS for jj in TRIES], np.uint64).T
    cols = np.concatenate([np.concatenate([base, r[None], j[None]]), edge], axis=1)
    return [c.astype(np.uint32) for c in cols]


def test_the_lcg_step_is_linear_in_a_counter():
    x, y, z, w, r, j = inputs()
    with np.errstate(over="ignore"):
        assert np.array_equal(step(z + r), step(z) + r * A)
        assert np.array_equal(step(w + j), step(w) + j * A)


def test_stepped_form_draws_what_the_plain_form_draws():
    x, y, z, w, r, j = inputs()
    with np.errstate(over="ignore"):
        plain = pcg4d(x, y, z + r, w + j)
        W0, W1, W2, W3 = step(x), step(y), step(z), step(w)               # start(): once per path
        W2r = W2 + r * A                                                  # set_ray(r)
        assert np.array_equal(rounds(W0, W1, W2r, W3 + j * A), plain)    # block(a, j)
        # next_event(): r single steps of A (r small enough to walk)
        walk = r < 64
        acc = W2.copy()
        for k in range(64):
            acc = np.where(walk & (k < r), acc + A, acc)
        assert np.array_equal(acc[walk], W2r[walk])


def test_running_word_of_the_cooperative_rejection():
    """The owner starts at try jbase (1, or 2 after an in-lane try 1) and advances by A << lg per failed round of 2^lg tries; worker sub of the
    round adds sub * A, exact in a 24-bit multiply because A < 2^24 and sub < 64.  After `failed` rounds of possibly different sizes the
    try number is jbase + (the tries passed) + sub, and the word is W3 + that * A."""
    rng = np.random.default_rng(7)
    n = 20_000
    w3 = step(rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32))
    assert int(A) < 2 ** 24
    for jbase in (1, 2):
        with np.errstate(over="ignore"):
            wnext = w3 + U(jbase) * A
            j = np.full(n, jbase, np.uint64)
            for _ in range(12):                                           # twelve rounds, each with its own group size (the number of owners changes)
                lg = rng.integers(0, 7, n).astype(np.uint32)
                sub = (rng.integers(0, 64, n).astype(np.uint32)) & ((U(1) << lg) - U(1))
                prod24 = ((sub & U(0xFFFFFF)).astype(np.uint64) * np.uint64(int(A) & 0xFFFFFF))
                assert (prod24 < 2 ** 32).all()                           # v_mul_u32_u24 returns the low 32 bits: nothing is lost
                got = wnext + prod24.astype(np.uint32)
                want = w3 + ((j + sub) & np.uint64(0xFFFFFFFF)).astype(np.uint32) * A
                assert np.array_equal(got, want)
                wnext = wnext + (A << lg)
                j = j + (np.uint64(1) << lg.astype(np.uint64))


def test_restatement_is_the_oracles_generator(oracle_mod):
    """The numpy pcg4d above against the oracle's, and the stepped addressing against the oracle's ctr_block, at the edge rays and tries."""
    with np.errstate(over="ignore"):
        for args in [(0, 0, 0, 0), (1, 2, 3, 4), (0xFFFFFFFF,) * 4, (0x80000000, 0, 0xFFFFFFFF, 1)]:
            mine = pcg4d(*[np.array([a], np.uint32) for a in args])[:, 0]
            assert mine.tolist() == oracle_mod.pcg4d(*args).tolist()
        for k0, k1, x, s in [(0, 0, 0, 0), (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF), (0x9E3779B9, 7, 799, 255)]:
            b = pcg4d(*[np.array([a], np.uint32) for a in (x, s, k0, k1)])[:, 0]
            W = [step(v) for v in b]
            for r in RAYS:
                for j in TRIES:
                    got = rounds(W[0], W[1], W[2] + U(r) * A, W[3] + U(j) * A)
                    assert [int(v) for v in got] == oracle_mod.ctr_block(k0, k1, x, s, r, j, gen=2).tolist(), (k0, k1, x, s, r, j)
