"""The parity contract between the HIP path and the CPU oracle, as one assertion the tests share (DESIGN.md
section 5).  A plain module, imported like conftest.

  * exact scenes (only + - * / sqrt on the path, or the reference-stream mode): linear f32 bit for bit, packed equal, ray counts equal;
  * scenes with logf / atanf / sincosf / acosf / atan2f, where the device libm and glibc differ by ulps and an ulp can flip a branch for
    an isolated sample -- counted, not fractions, so that a small image stays meaningful (a 96x54 image may carry one outlier):
      - at most ceil(1e-4 N) pixels with per-pixel linear-RGB L2 > 1e-3 (a non-finite pixel is always an outlier),
      - at most ceil(1e-3 N) 8-bit pixels that differ,
      - image means within 2e-3 relative,
      - |delta rays| <= ray_rel * oracle rays.
A failure names the offending pixels by absolute (row, x) and the rows that hold most of them, so a band, work-shard or strip bug
shows up as the rows where it sits.  Measured (profiles/fullsize_parity.txt): veach-mis 1280x720x1024, the worst image, has 13 of the 93
allowed L2 outliers, 11 of the 922 allowed 8-bit differences and 166 rays in 2.34 G; the other images of that file none, rays within 7e-8.
"""
import math
import os

import numpy as np

L2_TOL = 1e-3              # per-pixel linear-RGB distance that counts as "the same pixel"
L2_OUTLIERS = 1e-4         # share of N: pixels allowed beyond L2_TOL
BYTE_DIFFS = 1e-3          # share of N: 8-bit pixels allowed to differ (the contract: >= 99.9 % identical)
MEAN_REL = 2e-3            # image-mean relative difference


def oracle_threads():
    """Threads for an oracle render of a large image.  oracle.render(threads=0) takes std::thread::hardware_concurrency(), the whole
    machine, which can be many times the CPUs this process may use: at most 16, at most the affinity mask, at most OMP_NUM_THREADS."""
    n = min(16, len(os.sched_getaffinity(0)))
    try:
        omp = int(os.environ.get("OMP_NUM_THREADS", "0"))
    except ValueError:
        omp = 0
    if omp > 0:
        n = min(n, omp)
    return max(1, n)


def allowed(n_pixels):
    """(L2 outliers, differing 8-bit pixels) the tolerant contract allows in an image of n_pixels."""
    return math.ceil(L2_OUTLIERS * n_pixels), math.ceil(BYTE_DIFFS * n_pixels)


def _where(bad, rows):
    """Description of the pixels where `bad` [rows, W] is set: how many, the first ten as absolute (row, x), the rows holding most."""
    ys, xs = np.nonzero(bad)
    ab = np.asarray(rows, np.int64)[ys] if rows is not None else ys
    first = ", ".join(f"({int(y)}, {int(x)})" for y, x in zip(ab[:10], xs[:10]))
    u, c = np.unique(ab, return_counts=True)
    top = np.argsort(-c, kind="stable")[:8]
    worst = ", ".join(f"{int(u[i])} ({int(c[i])})" for i in top)
    return f"{len(ys)} px; first (row, x): {first}; rows with most (row (count)): {worst}"


def assert_parity(gpu_packed, gpu_linear, ora_packed, ora_linear, *, exact, rows=None, gpu_rays=None, oracle_rays=None, ray_rel=0.0):
    """gpu_* / ora_*: packed u32 [R, W] and linear f32 [R, W, 3] of the same R rows.  `rows` maps each of the R rows to its absolute image
    row (a row subset or window); None: row i is image row i.  Ray counts are checked when both are given."""
    gp, op = np.asarray(gpu_packed), np.asarray(ora_packed)
    gl, ol = np.asarray(gpu_linear, np.float32), np.asarray(ora_linear, np.float32)
    assert gp.shape == op.shape and gl.shape == ol.shape and gl.shape[:2] == gp.shape, (gp.shape, op.shape, gl.shape, ol.shape)
    if rows is not None:
        assert len(rows) == gp.shape[0], (len(rows), gp.shape)
    n = gp.size
    have_rays = gpu_rays is not None and oracle_rays is not None
    rays = f"rays gpu {gpu_rays} oracle {oracle_rays}"
    l2 = np.sqrt(((gl.astype(np.float64) - ol.astype(np.float64)) ** 2).sum(-1))
    l2_max = np.nanmax(l2) if np.isfinite(l2).any() else float("nan")
    if exact:
        bits = (gl.view(np.uint32) != ol.view(np.uint32)).any(-1) | (gp != op)
        assert not bits.any(), f"not bit-identical to the oracle: {_where(bits, rows)}; max L2 {l2_max:.3e}; {rays}"
        if have_rays:
            assert int(gpu_rays) == int(oracle_rays), f"ray counts differ: {rays}"
        return
    far = ~(l2 <= L2_TOL)                                       # NaN / inf count as outliers
    byte = gp != op
    max_far, max_byte = allowed(n)
    msg = (f"{int(far.sum())} of {n} px beyond L2 {L2_TOL:g} (allowed {max_far}), {int(byte.sum())} 8-bit px differ (allowed {max_byte}); "
           f"max L2 {l2_max:.3e}; {rays}")
    assert far.sum() <= max_far, f"{msg}\n  L2 outliers: {_where(far, rows)}"
    assert byte.sum() <= max_byte, f"{msg}\n  8-bit differences: {_where(byte, rows)}"
    gm, om = float(gl.mean(dtype=np.float64)), float(ol.mean(dtype=np.float64))
    assert abs(gm - om) <= MEAN_REL * max(om, 1e-6), f"image means differ: gpu {gm} oracle {om}; {msg}"
    if have_rays:
        assert abs(int(gpu_rays) - int(oracle_rays)) <= ray_rel * int(oracle_rays), f"ray counts differ by more than {ray_rel:g}: {rays}"


NAN_WORD = np.uint32(0x7FC00000)


def nan_folded_bits(a):
    """The f32 words of `a` with every NaN as one word: x86 and gfx950 give a default NaN different signs, and which payload an operation
    on two NaNs keeps is not part of the contract.  Everything else -- the sign of a zero or an infinity, a denormal -- stays what it is."""
    a = np.ascontiguousarray(a, np.float32)
    return np.where(np.isnan(a), NAN_WORD, a.view(np.uint32))


def assert_same_bits_nan_folded(got, want, what=""):
    """got == want word for word, every NaN being one value: a NaN is equal to a NaN only, so a NaN paired with a number (an infinity
    included) fails like any other difference.  Names the first differing elements."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, f"{what}: shapes {got.shape} vs {want.shape}"
    g, w = nan_folded_bits(got), nan_folded_bits(want)
    bad = g != w
    if bad.any():
        idx = np.argwhere(bad)
        first = "; ".join(f"{tuple(int(v) for v in i)}: got {got[tuple(i)]!r} ({int(g[tuple(i)]):#010x}) want {want[tuple(i)]!r} ({int(w[tuple(i)]):#010x})"
                          for i in idx[:6])
        nan_vs_number = int((bad & (np.isnan(got) != np.isnan(want))).sum())
        raise AssertionError(f"{what}: {len(idx)} of {g.size} words differ ({nan_vs_number} pair a NaN with a number); first: {first}")
