"""mi355rt_noise_device_*: the noise estimate on device memory against BOTH the C estimator of the host library (host.NoiseState) and the numpy
restatement (noise_ref.NoiseRef), fed the same sums.  The error map, the counts, max_error and the verdict must be the same words; mean_error
must be, word for word, the header's reduction tree (noise_device_ref.py) and within (pixels + 64) * 2^-53, relative, of the host's sum in pixel
order.  Device buffers are torch tensors; nothing here provokes a fault -- every buffer is as large as the header asks.

One case the definition cannot reach with float inputs: T * T never overflows a double (|Y| stays below 2^129 per chunk), so "huge" sums are
tested for what they do reach -- Q and ss of the order 1e76, and the float map overflowing to +inf."""
import ctypes as C

import numpy as np
import pytest

from conftest import SCENES
from converge_cases import five_kinds_scene
from noise_device_ref import TILE, error_float64, mean_error
from noise_ref import NoiseRef

gpu = pytest.mark.gpu
u32 = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
u64 = lambda x: int(np.float64(x).view(np.uint64))
SUMMARY_BYTES = 56
FIELDS = ("chunks", "samples", "pixels", "above", "nonfinite", "converged", "_pad")
# (width, rows): 1, around a wave, around the tile of 256, an odd image, more tiles than k_noise_finish has threads (257), and that plus one tile plus one pixel
SHAPES = [(1, 1), (63, 1), (64, 1), (65, 1), (255, 1), (256, 1), (257, 1), (33, 17), (257, TILE), (257, 257)]
PARAM_SETS = (dict(), dict(floor=0.0), dict(threshold=0.5, allowed_above=7, min_chunks=12))


def synthetic_sums(n, updates, seed):
    """[(running sums float32 [n, 4], samples_total)] for `updates` chunks of unequal size.  Ordinary pixels grow by positive increments; pixels drawn
    at random are denormal, -0, negative, huge, constant (0 / 0 with floor 0), +-inf or NaN in a channel.  The fourth word of every pixel is a NaN
    whose payload depends on the seed and the chunk: it must never be read."""
    rng = np.random.default_rng(seed)
    kind = rng.integers(0, 24, n)                                     # 0 .. 7 special, the rest ordinary
    if n >= 16:
        kind[:8] = np.arange(8)                                       # every special at least once
    acc = np.zeros((n, 3), np.float32)
    out, total = [], 0
    for k in range(updates):
        chunk = int(rng.integers(1, 40))
        total += chunk
        inc = (rng.random((n, 3)) ** 3 * chunk).astype(np.float32)
        with np.errstate(all="ignore"):
            acc = (acc + inc).astype(np.float32)
            a = acc.copy()
            a[kind == 0] = (rng.random((int((kind == 0).sum()), 3)) * 1e-40).astype(np.float32)       # float denormals
            a[kind == 1] = np.float32(-0.0) if k % 2 else np.float32(0.0)                              # -0 against +0
            a[kind == 2] = -acc[kind == 2]                                                             # negative sums
            a[kind == 3] = (acc[kind == 3] * np.float32(1e37)).astype(np.float32)                      # huge, some channels overflow to +inf
            a[kind == 4] = np.float32(0.0)                                                             # never changes: 0 / 0 with floor 0
            a[kind == 5, k % 3] = np.float32(np.inf) if k else np.float32(1.0)
            a[kind == 6, (k + 1) % 3] = np.float32(-np.inf) if k == updates - 1 else a[kind == 6, (k + 1) % 3]
            a[kind == 7, 2] = np.float32(np.nan) if k >= 1 else np.float32(2.0)
        full = np.empty((n, 4), np.float32)
        full[:, :3] = a
        full[:, 3].view(np.uint32)[:] = 0x7FC00000 | ((seed * 977 + k * 131 + np.arange(n)) & 0x3FFFFF)
        out.append((full, total))
    return out


def check_same(got_map, got, host_pair, ref, params, n):
    """One device result against the host's and the restatement's, as the header promises."""
    host_map, hs = host_pair
    ref_map, rs = ref.evaluate(**{**dict(threshold=0.02, floor=0.01, min_chunks=4, allowed_above=0), **params})
    if got_map is not None:
        assert np.array_equal(u32(got_map), u32(host_map)) and np.array_equal(u32(got_map), u32(ref_map))
    for f in FIELDS:
        assert getattr(got, f) == getattr(hs, f) == rs[f], (f, getattr(got, f), getattr(hs, f), rs[f])
    assert u64(got.max_error) == u64(hs.max_error) == u64(rs["max_error"]), (got.max_error, hs.max_error)
    tree = mean_error(error_float64(ref, params.get("floor", 0.01)))
    print(f"pixels {n} chunks {got.chunks}: mean_error device {got.mean_error!r} tree {tree!r} host {hs.mean_error!r}")
    assert u64(got.mean_error) == u64(tree), (got.mean_error, tree)
    if np.isfinite(hs.mean_error):
        assert abs(got.mean_error - hs.mean_error) <= (n + 64) * 2.0 ** -53 * hs.mean_error, (got.mean_error, hs.mean_error)
    else:
        assert u64(got.mean_error) == u64(hs.mean_error)


class Trio:
    """The device object, the C estimator and the numpy restatement, fed the same sums."""

    def __init__(self, native, w, h):
        import torch
        self.torch = torch
        host, device = native
        self.w, self.h, self.n = w, h, w * h
        self.dev, self.host, self.ref = device.NoiseDevice(w, h), host.NoiseState(w, h), NoiseRef(w, h)
        self.keep = []

    def update(self, accum, total, stream=None):
        t = self.torch.from_numpy(accum).cuda()
        self.torch.cuda.synchronize()
        self.keep.append(t)
        self.dev.update(t.data_ptr(), total, stream)
        self.host.update(accum, total)
        self.ref.update(accum, total)

    def check(self, abi, params):
        got_map, got = self.dev.evaluate(abi.NoiseParams.make(**params) if params else None)
        check_same(got_map, got, self.host.evaluate(abi.NoiseParams.make(**params) if params else None), self.ref, params, self.n)
        return got_map, got

    def close(self):
        self.torch.cuda.synchronize()
        self.dev.free(); self.host.close()


@gpu
@pytest.mark.parametrize("w,h,updates", [(w, h, 2 + (3 * i + 1) % 8) for i, (w, h) in enumerate(SHAPES)])      # 2 .. 9 updates, spread over the shapes
def test_synthetic_sums_at_every_shape(native, abi, w, h, updates):
    n = w * h
    t = Trio(native, w, h)
    try:
        sums = synthetic_sums(n, updates, seed=n)
        interior = max(2, updates // 2)
        for k, (a, total) in enumerate(sums, 1):
            t.update(a, total)
            if k == interior or k == updates:
                for params in PARAM_SETS:
                    _, got = t.check(abi, params)
                if n >= 16:
                    assert got.nonfinite > 0 and got.pixels == n
    finally:
        t.close()


@gpu
def test_object_refusals_change_nothing(native, abi):
    import torch
    _, device = native
    L = device.lib()
    err = lambda: L.mi355rt_last_error().decode()
    t = Trio(native, 9, 5)
    try:
        sums = synthetic_sums(45, 3, seed=5)
        d = torch.zeros(45 * 4 + 4, dtype=torch.float32, device="cuda")
        out = torch.zeros(64, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        h = t.dev._h
        assert L.mi355rt_noise_device_evaluate(h, None, None, out.data_ptr(), None) == abi.ERR_INVALID and "needs at least 2 chunks" in err()
        t.update(*sums[0])
        assert L.mi355rt_noise_device_evaluate(h, None, None, out.data_ptr(), None) == abi.ERR_INVALID and "needs at least 2 chunks" in err()
        total = sums[0][1]
        for bad in (0, total - 1, total):
            assert L.mi355rt_noise_device_update(h, d.data_ptr(), bad, None) == abi.ERR_INVALID
            assert err() == f"noise_device_update: samples_total ({bad}) must exceed the {total} samples already seen"
        assert L.mi355rt_noise_device_update(h, d.data_ptr() + 4, total + 1, None) == abi.ERR_INVALID and "16-byte aligned" in err()
        t.update(*sums[1])
        assert L.mi355rt_noise_device_evaluate(h, None, out.data_ptr() + 2, out.data_ptr(), None) == abi.ERR_INVALID and "d_out_error must be 4-byte aligned" in err()
        assert L.mi355rt_noise_device_evaluate(h, None, None, out.data_ptr() + 4, None) == abi.ERR_INVALID and "8-byte aligned" in err()
        t.check(abi, {})                                              # K, N and the sums are what the accepted calls left
        t.update(*sums[2])
        t.check(abi, dict(floor=0.0))
    finally:
        t.close()


@gpu
def test_double_division_and_square_root_are_the_hosts(native, abi):
    """2048 one-pixel states across the exponent range: max_error is the pixel's err, a chain of five divisions and one square root in double.
    One word of difference from the host's correctly rounded arithmetic fails here."""
    import torch
    host, device = native
    draws = 2048
    rng = np.random.default_rng(2024)
    e1 = rng.integers(-140, 120, (draws, 1))
    a1 = (rng.uniform(0.5, 1.0, (draws, 3)) * 2.0 ** (e1 + rng.integers(-3, 4, (draws, 3)))).astype(np.float32)
    with np.errstate(all="ignore"):
        a2 = (a1 * rng.uniform(1.0, 3.0, (draws, 3)) * 2.0 ** rng.integers(0, 3, (draws, 1))).astype(np.float32)
    a2[::7] = (a1[::7] * np.float32(1.0000001)).astype(np.float32)    # nearly equal chunks: ss cancels to a few bits or below 0
    n1 = rng.integers(1, 1000, draws); n2 = n1 + rng.integers(1, 1000, draws)
    floors = np.where(np.arange(draws) % 3 == 0, 0.0, np.where(np.arange(draws) % 3 == 1, 0.01, 2.0 ** rng.integers(-160, 100, draws).astype(np.float64)))
    acc = np.zeros((draws, 2, 4), np.float32)
    acc[:, 0, :3], acc[:, 1, :3] = a1, a2
    d_acc = torch.from_numpy(acc).cuda()
    d_sum = torch.zeros(draws * SUMMARY_BYTES, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    dev, hs = device.NoiseDevice(1, 1), host.NoiseState(1, 1)
    want = []
    try:
        for i in range(draws):
            prm = abi.NoiseParams.make(floor=float(floors[i]), min_chunks=2)
            dev.reset()
            dev.update(d_acc.data_ptr() + i * 32, int(n1[i]))
            dev.update(d_acc.data_ptr() + i * 32 + 16, int(n2[i]))
            dev.evaluate_into(None, d_sum.data_ptr() + i * SUMMARY_BYTES, prm)
            hs.reset(); hs.update(acc[i, 0], int(n1[i])); hs.update(acc[i, 1], int(n2[i]))
            want.append(hs.evaluate(prm, want_map=False)[1])
        torch.cuda.synchronize()
        got = d_sum.cpu().numpy().reshape(draws, SUMMARY_BYTES)
        bad, positive = [], []
        for i in range(draws):
            g = abi.NoiseSummary.from_buffer_copy(got[i].tobytes())
            w = want[i]
            if (u64(g.max_error), g.nonfinite, g.above, u64(g.mean_error)) != (u64(w.max_error), w.nonfinite, w.above, u64(w.mean_error)):
                bad.append((i, g.max_error, w.max_error, acc[i].tolist(), int(n1[i]), int(n2[i]), float(floors[i])))
            elif np.isfinite(w.max_error) and w.max_error > 1e-300 and w.nonfinite == 0:
                positive.append(i)
        print(f"{draws} draws, {len(positive)} with a finite positive err, {len(bad)} differ")
        assert not bad, bad[:5]
        assert len(positive) > draws // 2
        # the comparison with the threshold is strict: err > err is false, err > the next double below it is true
        d_two = torch.zeros(2 * SUMMARY_BYTES, dtype=torch.uint8, device="cuda")
        for i in positive[::37]:
            e = want[i].max_error
            dev.reset()
            dev.update(d_acc.data_ptr() + i * 32, int(n1[i]))
            dev.update(d_acc.data_ptr() + i * 32 + 16, int(n2[i]))
            dev.evaluate_into(None, d_two.data_ptr(), abi.NoiseParams.make(threshold=e, floor=float(floors[i]), min_chunks=2))
            dev.evaluate_into(None, d_two.data_ptr() + SUMMARY_BYTES, abi.NoiseParams.make(threshold=float(np.nextafter(e, 0.0)), floor=float(floors[i]), min_chunks=2))
            torch.cuda.synchronize()
            two = d_two.cpu().numpy().reshape(2, SUMMARY_BYTES)
            at, below = (abi.NoiseSummary.from_buffer_copy(two[j].tobytes()) for j in range(2))
            assert (at.above, at.converged, below.above, below.converged) == (0, 1, 1, 0), (i, e)
    finally:
        torch.cuda.synchronize()
        dev.free(); hs.close()


@gpu
@pytest.mark.parametrize("w,h", [(33, 17), (257, 1)])
def test_every_word_is_written_and_nothing_beyond(native, abi, w, h):
    import torch
    n, pad = w * h, 256
    t = Trio(native, w, h)
    try:
        for a, total in synthetic_sums(n, 3, seed=77):
            t.update(a, total)
        want_map, want = t.host.evaluate(None)
        results = []
        for fill in (0xA5, 0x5A):
            d_err = torch.full((pad + n * 4 + pad,), fill, dtype=torch.uint8, device="cuda")
            d_sum = torch.full((pad + SUMMARY_BYTES + pad,), fill, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            t.dev.evaluate_into(d_err.data_ptr() + pad, d_sum.data_ptr() + pad, None)
            torch.cuda.synchronize()
            e, s = d_err.cpu().numpy(), d_sum.cpu().numpy()
            assert (e[:pad] == fill).all() and (e[pad + n * 4:] == fill).all() and (s[:pad] == fill).all() and (s[pad + SUMMARY_BYTES:] == fill).all()
            results.append((e[pad:pad + n * 4].tobytes(), s[pad:pad + SUMMARY_BYTES].tobytes()))
        assert results[0] == results[1]                               # no byte of the two outputs is left as it was
        got = abi.NoiseSummary.from_buffer_copy(results[0][1])
        check_same(np.frombuffer(results[0][0], np.float32).reshape(h, w), got, (want_map, want), t.ref, {}, n)
        # without a map only the summary is written
        d_err = torch.full((n * 4,), 0xA5, dtype=torch.uint8, device="cuda")
        d_sum = torch.full((pad + SUMMARY_BYTES + pad,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        t.dev.evaluate_into(None, d_sum.data_ptr() + pad, None)
        torch.cuda.synchronize()
        s = d_sum.cpu().numpy()
        assert (d_err.cpu().numpy() == 0xA5).all() and (s[:pad] == 0xA5).all() and (s[pad + SUMMARY_BYTES:] == 0xA5).all()
        assert s[pad:pad + SUMMARY_BYTES].tobytes() == results[0][1]
    finally:
        t.close()


def _sequence(device, torch, w, h, d_sums, totals, stream, dev=None):
    """update + evaluate of every chunk from the second on, enqueued back to back on `stream` with no host synchronisation between them; the
    results land in one slot per chunk.  Returns (maps uint8 tensor, summaries uint8 tensor, the object)."""
    n = w * h
    dev = dev or device.NoiseDevice(w, h)
    maps = torch.zeros((len(totals), n * 4), dtype=torch.uint8, device="cuda")
    sums = torch.zeros((len(totals), 64), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s = stream.cuda_stream
    for k, total in enumerate(totals):
        dev.update(d_sums[k].data_ptr(), total, s)
        if k >= 1:
            dev.evaluate_into(maps[k].data_ptr(), sums[k].data_ptr(), None, s)
    return maps, sums, dev


@gpu
def test_stream_order_and_determinism(native, abi):
    import torch
    host, device = native
    w, h = 61, 23
    n = w * h
    chunks = synthetic_sums(n, 4, seed=3)
    totals = [t for _, t in chunks]
    d_sums = [torch.from_numpy(a).cuda() for a, _ in chunks]
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    maps, sums, dev = _sequence(device, torch, w, h, d_sums, totals, stream)      # one first update, then three chunks of update + evaluate
    stream.synchronize()
    got_maps, got_sums = maps.cpu().numpy(), sums.cpu().numpy()
    hs, ref = host.NoiseState(w, h), NoiseRef(w, h)
    try:
        for k, (a, total) in enumerate(chunks):
            hs.update(a, total); ref.update(a, total)
            if k >= 1:
                got = abi.NoiseSummary.from_buffer_copy(got_sums[k, :SUMMARY_BYTES].tobytes())
                check_same(got_maps[k].view(np.float32).reshape(h, w), got, hs.evaluate(None), ref, {}, n)
        # the same sequence again: in a second object created separately, and in the first one after reset
        maps2, sums2, dev2 = _sequence(device, torch, w, h, d_sums, totals, stream)
        dev.reset(stream.cuda_stream)
        maps3, sums3, _ = _sequence(device, torch, w, h, d_sums, totals, stream, dev)
        stream.synchronize()
        for m, s in ((maps2, sums2), (maps3, sums3)):
            assert np.array_equal(m.cpu().numpy(), got_maps) and np.array_equal(s.cpu().numpy(), got_sums)
        dev2.free()
    finally:
        torch.cuda.synchronize()
        dev.free(); hs.close()


@gpu
@pytest.mark.parametrize("scene", ["cornell", "five_kinds"])
def test_real_sums_are_estimated_where_they_are(native, abi, tmp_path, scene):
    """Context.render_progressive chunk by chunk, counter mode: the device estimate reads d_accum itself, the host estimate a copy of it."""
    import torch
    host, device = native
    path, w, h = (SCENES["cornell"], 40, 30) if scene == "cornell" else (five_kinds_scene(tmp_path), 33, 17)
    n, depth = w * h, 6
    sc = host.LoadedScene(path, w, h, 4, depth)
    ctx = device.Context(0)
    dev, hs, ref = device.NoiseDevice(w, h), host.NoiseState(w, h), NoiseRef(w, h)
    try:
        ctx.set_scene(sc, sc.camera, sc.settings)
        accum = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
        packed = torch.zeros(n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        s = 0
        for k, chunk in enumerate((4, 3, 5, 4, 6), 1):               # unequal chunks
            ctx.render_progressive(s, s + chunk, accum.data_ptr(), packed.data_ptr(), None, abi.Options.make())
            s += chunk
            dev.update(accum.data_ptr(), s)                           # the same (null) stream: behind the render, no copy
            torch.cuda.synchronize()
            a = accum.cpu().numpy()
            hs.update(a, s); ref.update(a, s)
            if k >= 2:
                for params in (dict(), dict(floor=0.0, min_chunks=2, threshold=0.3, allowed_above=n // 10)):
                    prm = abi.NoiseParams.make(**params)
                    got_map, got = dev.evaluate(prm)
                    check_same(got_map, got, hs.evaluate(prm), ref, params, n)
        ctx.check()
    finally:
        torch.cuda.synchronize()
        ctx.close(); dev.free(); hs.close(); sc.close()
