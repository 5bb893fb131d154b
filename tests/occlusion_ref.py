"""Reference for the occlusion queries (not a test): a numpy float32 restatement of mi355rt.h's definitions.

  pcg4d           oracle/rng_np.py's, re-exported: the generator of rt_rng.h on uint32 arrays (the oracle exposes the scalar one as oracle.pcg4d)
  ball_floats     c_k = (float)(w_k >> 8) * 2^-24 * 2 - 1
  ao_directions   the directions N + v of the samples of one pixel (16 tries per sample, then v = 0); not normalised: the ray is
                  {P, d} and Ray::new -- in the oracle's hook as on the device -- normalises it once
  occluded        the rule (hit && t < t_max, strict, f32) on top of oracle.scene_hit
  AoReference     the pass over a buffer of first-hit records; it keeps the oracle's answer of every (pixel, sample, seed) ray -- a sample's
                  ray does not depend on `samples` or `radius` -- so that the cases of a test share their oracle calls."""
import numpy as np

from oracle.rng_np import pcg4d  # noqa: F401  -- re-exported: tests/test_occlusion_reference_cpu.py pins it under this name

F = np.float32
U = np.uint32
NO_HIT = 0xFFFFFFFF
TRIES = 16


def ball_floats(words):
    """(float)(w >> 8) * 2^-24 * 2 - 1, every step exact."""
    f = (np.asarray(words).astype(U) >> U(8)).astype(F)
    out = f * F(2.0 ** -24) * F(2.0) - F(1.0)
    assert out.dtype == F
    return out


def ao_directions(x, y, samples, seed, normal, words=pcg4d):
    """float32 [samples, 3]: d = N + v of sample 0 .. samples-1 of pixel (x, y); `words` is the generator (a test stubs it)."""
    s = np.arange(samples, dtype=U)[:, None]
    j = np.arange(TRIES, dtype=U)[None, :]
    w0, w1, w2, _ = words(U(x), U(y), s * U(TRIES) + j, U(seed))
    c = np.stack([ball_floats(w0), ball_floats(w1), ball_floats(w2)], axis=-1)                 # [samples, tries, 3]
    l2 = (c[..., 0] * c[..., 0] + c[..., 1] * c[..., 1]) + c[..., 2] * c[..., 2]
    assert l2.dtype == F
    ok = l2 < F(1.0)
    first = np.argmax(ok, axis=1)
    v = c[np.arange(samples), first]
    v[~ok.any(axis=1)] = F(0.0)
    d = np.asarray(normal, F)[None, :] + v
    assert d.dtype == F
    return d


def occluded(oracle_mod, sc, origin, direction, t_max):
    hit, r = oracle_mod.scene_hit(sc, origin, direction)
    return 1 if (hit and bool(F(r[6]) < F(t_max))) else 0


def occluded_from_t(hit, t, t_max):
    """The rule on recorded oracle answers: arrays of hit flags and t (NaN t: 0; NaN t_max: 0)."""
    with np.errstate(invalid="ignore"):
        return (np.asarray(hit, bool) & (np.asarray(t, F) < np.asarray(t_max, F))).astype(U)


class AoReference:
    def __init__(self, oracle_mod, sc):
        self.oracle, self.sc = oracle_mod, sc
        self._t = {}                                       # (x, y, seed) -> float32 [samples so far]: the closest t of each sample's ray, +inf for a miss... NaN kept
        self.calls = 0

    def _sample_t(self, x, y, seed, samples, p, n):
        key = (int(x), int(y), int(seed), p.tobytes(), n.tobytes())
        have = self._t.get(key, np.zeros(0, F))
        if len(have) < samples:
            d = ao_directions(x, y, samples, seed, n)
            more = np.zeros(samples, F)
            more[:len(have)] = have
            for s in range(len(have), samples):
                hit, r = self.oracle.scene_hit(self.sc, p, d[s])
                self.calls += 1
                more[s] = F(r[6]) if hit else F(np.inf)    # a miss is below no radius, like +inf
            self._t[key] = have = more
        return have[:samples]

    def ao(self, hits, width, rows, samples, seed, radius):
        """hits: abi.HIT_DTYPE [len(rows) * width] (what first_hits wrote for `rows`, absolute image rows) -> float32 [len(rows) * width]."""
        out = np.ones(len(hits), F)
        for i, h in enumerate(hits):
            if h["primitive"] == NO_HIT:
                continue
            x, y = i % width, rows[i // width]
            t = self._sample_t(x, y, seed, samples, np.array(h["position"], F), np.array(h["normal"], F))
            with np.errstate(invalid="ignore"):
                count = int((t < F(radius)).sum())
            out[i] = F(1.0) - F(count) / F(samples)
        return out
