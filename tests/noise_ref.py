"""The noise estimate of include/mi355rt.h (mi355rt_noise_*) restated in numpy float64, operation by operation and in the header's order --
written from the header's definition, not from csrc/host/noise_estimate.cpp.  A plain module, imported like denoise_ref.py.

numpy's elementwise float64 operations round once each and nothing is fused, which is what the definition asks; the one sum over pixels
(mean_error) is taken with cumsum, which adds strictly in order (np.sum adds pairwise)."""
import numpy as np

DEFAULTS = dict(threshold=0.02, floor=0.01, min_chunks=4, allowed_above=0)


class NoiseRef:
    def __init__(self, width, rows):
        self.width, self.rows = width, rows
        self.reset()

    def reset(self):
        n = self.width * self.rows
        self.prev = np.zeros((n, 3), np.float32)
        self.T = np.zeros(n, np.float64)
        self.Q = np.zeros(n, np.float64)
        self.K = 0
        self.N = 0

    def update(self, accum, samples_total):
        assert samples_total > self.N
        a = np.asarray(accum, np.float32).reshape(-1, 4)
        n = np.float64(samples_total - self.N)
        with np.errstate(all="ignore"):
            d = a[:, :3].astype(np.float64) - self.prev.astype(np.float64)
            y = (np.float64(0.2126) * d[:, 0] + np.float64(0.7152) * d[:, 1]) + np.float64(0.0722) * d[:, 2]
            self.T = self.T + y
            self.Q = self.Q + (y * y) / n
        self.prev = a[:, :3].copy()
        self.K += 1
        self.N = samples_total

    def standard_error(self):
        """se per pixel (float64), the intermediate the calibration tests look at."""
        N = np.float64(self.N)
        with np.errstate(all="ignore"):
            ss = self.Q - (self.T * self.T) / N
            var = np.where(ss > 0, ss, 0.0) / np.float64(self.K - 1)
            return np.sqrt(var / N)

    def evaluate(self, threshold=0.02, floor=0.01, min_chunks=4, allowed_above=0):
        """(error map float32 [rows, width], dict of the summary fields)."""
        assert self.K >= 2
        N = np.float64(self.N)
        with np.errstate(all="ignore"):
            m = self.T / N
            se = self.standard_error()
            err = se / (np.where(m > 0, m, 0.0) + np.float64(floor))
        bad = ~(np.isfinite(self.T) & np.isfinite(self.Q)) | np.isnan(err)
        err = np.where(bad, np.nan, err)                       # one NaN, whatever sign the arithmetic gave it
        good = err[~bad]
        above = int((good > threshold).sum())
        summary = dict(chunks=self.K, samples=self.N, pixels=err.size, above=above, nonfinite=int(bad.sum()),
                       max_error=float(good.max()) if good.size else 0.0,
                       mean_error=float(np.cumsum(good)[-1] / np.float64(good.size)) if good.size else 0.0,
                       converged=int(self.K >= min_chunks and above <= allowed_above), _pad=0)
        with np.errstate(all="ignore"):
            return err.astype(np.float32).reshape(self.rows, self.width), summary
