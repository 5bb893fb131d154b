"""The reduction tree of mi355rt_noise_device_evaluate's mean_error (include/mi355rt.h, "the same estimate on the device") restated in
numpy float64 -- written from the header's description, not from csrc/device/rt_noise.hip.  A plain module, imported like noise_ref.py.

Every `a + b` below is one elementwise float64 addition of two arrays (one rounding each, nothing pairwise: np.sum is never used), so the
order of the additions is the one the header writes."""
import numpy as np

TILE = 256          # consecutive pixels per tile
WAVE = 64


def _tree(v):
    """TREE over the last axis (256 entries): every run of 64 halved six times, then (s0 + s1) + (s2 + s3)."""
    x = v.reshape(v.shape[:-1] + (TILE // WAVE, WAVE))
    h = WAVE // 2
    while h >= 1:
        x = x[..., :h] + x[..., h:2 * h]
        h //= 2
    s = x[..., 0]
    return (s[..., 0] + s[..., 1]) + (s[..., 2] + s[..., 3])


def tree_sum(e):
    """e: the per-pixel terms in pixel order, float64, +0.0 where a pixel is not counted."""
    e = np.asarray(e, np.float64).reshape(-1)
    n_tiles = (e.size + TILE - 1) // TILE
    padded = np.zeros(n_tiles * TILE, np.float64)
    padded[:e.size] = e
    with np.errstate(all="ignore"):
        S = _tree(padded.reshape(n_tiles, TILE))                     # one sum per tile
        rounds = (n_tiles + TILE - 1) // TILE
        Sp = np.zeros(rounds * TILE, np.float64)
        Sp[:n_tiles] = S
        Sp = Sp.reshape(rounds, TILE)
        a = np.zeros(TILE, np.float64)
        for r in range(rounds):                                      # tile sums 256 apart, in ascending order
            a = a + Sp[r]
        return float(_tree(a))


def mean_error(err):
    """err: float64 per pixel in pixel order, NaN where the pixel is not counted.  The header's mean_error."""
    err = np.asarray(err, np.float64).reshape(-1)
    bad = np.isnan(err)
    counted = err.size - int(bad.sum())
    if counted == 0:
        return 0.0
    with np.errstate(all="ignore"):
        return float(np.float64(tree_sum(np.where(bad, 0.0, err))) / np.float64(counted))


def error_float64(ref, floor):
    """The float64 err of noise_ref.NoiseRef's state (its evaluate returns the map rounded to float32), NaN where not counted."""
    N = np.float64(ref.N)
    with np.errstate(all="ignore"):
        m = ref.T / N
        err = ref.standard_error() / (np.where(m > 0, m, 0.0) + np.float64(floor))
    bad = ~(np.isfinite(ref.T) & np.isfinite(ref.Q)) | np.isnan(err)
    return np.where(bad, np.nan, err)
