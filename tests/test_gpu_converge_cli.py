"""rt_render --noise-target: the converging loop of the CLI against a REPLAY -- the same chunks rendered with Context.render_progressive, the sums
copied back after every chunk and fed to a host.NoiseState.  The CLI must stop where the replay's verdict first holds, report the replay's
figures, write the replay's error map word for word, and every image it writes must be the one-shot render of the samples it stopped at, bit
for bit (the speculative chunk it had in flight leaves no trace).  Every CLI run is a child process under a timeout."""
import math

import numpy as np
import pytest

from conftest import SCENES
from converge_cases import five_kinds_scene, infinite_emitter_scene, parse_noise_line, pick_threshold, read_pfm
from test_rt_render_cli import _cli

gpu = pytest.mark.gpu
W, H, DEPTH, CHUNK = 48, 36, 6, 4


def _size(w=W, h=H, depth=DEPTH):
    return ["--width", str(w), "--height", str(h), "--max-depth", str(depth)]


def _replay(native, abi, path, w, h, depth, chunk, n_chunks, max_spp=None):
    """{k: sums after chunk k} as float32 [h * w, 4] for k = 1 .. n_chunks, chunk k ending at min(k * chunk, max_spp)."""
    import torch
    host, device = native
    sc = host.LoadedScene(path, w, h, chunk, depth)
    ctx = device.Context(0)
    sums = {}
    try:
        ctx.set_scene(sc, sc.camera, sc.settings)
        accum = torch.zeros((h * w, 4), dtype=torch.float32, device="cuda")
        packed = torch.zeros(h * w, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        s = 0
        for k in range(1, n_chunks + 1):
            e = min(k * chunk, max_spp or k * chunk)
            ctx.render_progressive(s, e, accum.data_ptr(), packed.data_ptr(), None, abi.Options.make())
            torch.cuda.synchronize()
            sums[k] = (accum.cpu().numpy().copy(), e)
            s = e
        ctx.check()
    finally:
        ctx.close()
    return sums


def _estimates(host, abi, sums, w, h, **params):
    """{k: (error map, summary)} for k = 2 .., the NoiseState fed chunk by chunk."""
    st = host.NoiseState(w, h)
    out = {}
    for k in sorted(sums):
        st.update(*sums[k])
        if k >= 2:
            out[k] = st.evaluate(abi.NoiseParams.make(**params))
    st.close()
    return out


def _want_files(native, abi, path, w, h, depth, spp, tmp_path, tag):
    """PNG and PFM bytes of the one-shot render (mi355rt_render) at `spp` samples."""
    host, device = native
    sc = host.LoadedScene(path, w, h, spp, depth)
    gp, gl, _ = device.render(sc, sc.camera, sc.settings, abi.Options.make())
    png, pfm = str(tmp_path / f"{tag}_want.png"), str(tmp_path / f"{tag}_want.pfm")
    host.write_png(png, gp, w, h)
    host.write_pfm(pfm, gl, w, h)
    return open(png, "rb").read(), open(pfm, "rb").read(), gl


def _run(path, tmp_path, tag, *args, size=None):
    out = {e: str(tmp_path / f"{tag}.{e}") for e in ("png", "pfm")}
    r = _cli(path, *(size or _size()), "-o", out["png"], "--pfm", out["pfm"], *args)
    return parse_noise_line(r.stdout), open(out["png"], "rb").read(), open(out["pfm"], "rb").read(), r


@gpu
def test_a_huge_target_stops_at_min_chunks_on_an_odd_chunk(native, abi, tmp_path):
    n, png, pfm, _ = _run(SCENES["cornell"], tmp_path, "odd", "--noise-target", "1e9", "--chunk", str(CHUNK), "--min-chunks", "3", "--max-spp", "64")
    assert (n["samples"], n["chunks"], n["converged"], n["above"], n["rendered"]) == (12, 3, 1, 0, 16)       # k = 3; chunk 4 was in flight
    want_png, want_pfm, _ = _want_files(native, abi, SCENES["cornell"], W, H, DEPTH, 12, tmp_path, "odd")
    assert png == want_png and pfm == want_pfm


@gpu
def test_target_zero_runs_to_max_spp_with_a_short_last_chunk(native, abi, tmp_path):
    n, png, pfm, r = _run(SCENES["cornell"], tmp_path, "full", "--noise-target", "0", "--chunk", str(CHUNK), "--max-spp", "22")
    assert (n["samples"], n["chunks"], n["converged"], n["rendered"]) == (22, 6, 0, 22)                       # 4, 8, 12, 16, 20, 22: nothing speculative
    assert n["above"] > 0 and "22 / 22 samples per pixel" in r.stdout
    want_png, want_pfm, _ = _want_files(native, abi, SCENES["cornell"], W, H, DEPTH, 22, tmp_path, "full")
    assert png == want_png and pfm == want_pfm


def _interior_stop(native, abi, tmp_path, path, w, h, depth, tag, k_stop=6):
    """Picks, from the replay, a threshold and an allowance that first hold at chunk k_stop (even: the other output pair than the tests above),
    and asks the CLI for them."""
    host, _ = native
    sums = _replay(native, abi, path, w, h, depth, CHUNK, k_stop + 1)
    maps = {k: m for k, (m, _) in _estimates(host, abi, sums, w, h, min_chunks=2).items() if k <= k_stop}
    t, frac, allowed = pick_threshold(maps, k_stop)
    est = _estimates(host, abi, sums, w, h, threshold=t, min_chunks=2, allowed_above=allowed)
    verdicts = [est[k][1].converged for k in range(2, k_stop + 2)]
    print(f"{tag}: threshold {t!r}, allowance {frac} ({allowed} pixels), above by chunk {[int(est[k][1].above) for k in sorted(est)]}")
    assert verdicts[:k_stop - 1] == [0] * (k_stop - 2) + [1], verdicts                     # first at k_stop
    want_map, want = est[k_stop]
    map_path = str(tmp_path / f"{tag}_noise.pfm")
    n, png, pfm, r = _run(path, tmp_path, tag, "--noise-target", repr(t), "--noise-allow", repr(frac), "--min-chunks", "2", "--chunk", str(CHUNK),
                          "--max-spp", "64", "--noise-out", map_path, size=_size(w, h, depth))
    assert math.floor(frac * w * h) == allowed
    assert (n["samples"], n["chunks"], n["converged"], n["rendered"]) == (k_stop * CHUNK, k_stop, 1, (k_stop + 1) * CHUNK)
    assert (n["above"], n["nonfinite"]) == (want.above, want.nonfinite)
    assert n["max"] == pytest.approx(want.max_error, rel=1e-8) and n["mean"] == pytest.approx(want.mean_error, rel=1e-8)    # (printed with 9 digits)
    got_map = read_pfm(map_path)
    for c in range(3):                                                                    # grey: the map in every channel, word for word
        assert np.array_equal(got_map[..., c].view(np.uint32), want_map.view(np.uint32)), c
    want_png, want_pfm, _ = _want_files(native, abi, path, w, h, depth, k_stop * CHUNK, tmp_path, tag)
    assert png == want_png and pfm == want_pfm
    return n, want_map


@gpu
def test_an_interior_stop_on_an_even_chunk_is_the_replays(native, abi, tmp_path):
    _interior_stop(native, abi, tmp_path, SCENES["cornell"], W, H, DEPTH, "interior")


@gpu
def test_all_five_primitive_kinds_and_a_mesh_at_an_odd_size(native, abi, tmp_path):
    _interior_stop(native, abi, tmp_path, five_kinds_scene(tmp_path), 33, 17, DEPTH, "five_kinds")


@gpu
def test_an_infinite_emitter_is_reported_and_does_not_block(native, abi, tmp_path):
    host, _ = native
    path = infinite_emitter_scene(tmp_path)
    w, h = 40, 30
    sums = _replay(native, abi, path, w, h, DEPTH, CHUNK, 4)
    want_map, want = _estimates(host, abi, sums, w, h, threshold=1e9, min_chunks=4)[4]
    assert want.nonfinite > 0 and want.converged == 1 and np.isnan(want_map).sum() == want.nonfinite < w * h // 2
    map_path = str(tmp_path / "inf_noise.pfm")
    n, png, pfm, _ = _run(path, tmp_path, "inf", "--noise-target", "1e9", "--min-chunks", "4", "--chunk", str(CHUNK), "--max-spp", "64", "--noise-out", map_path,
                          size=_size(w, h))
    assert (n["samples"], n["chunks"], n["converged"], n["above"], n["nonfinite"]) == (16, 4, 1, 0, want.nonfinite)
    got = read_pfm(map_path)
    assert np.array_equal(np.isnan(got[..., 0]), np.isnan(want_map)) and np.array_equal(got[..., 1].view(np.uint32), want_map.view(np.uint32))
    want_png, want_pfm, gl = _want_files(native, abi, path, w, h, DEPTH, 16, tmp_path, "inf")
    assert png == want_png and pfm == want_pfm and np.isinf(gl).any()


@gpu
def test_denoise_out_is_the_denoised_image_of_the_samples_it_stopped_at(native, abi, tmp_path):
    import torch
    host, device = native
    denoised = str(tmp_path / "denoised.png")
    n, png, _, r = _run(SCENES["cornell"], tmp_path, "dn", "--noise-target", "1e9", "--chunk", str(CHUNK), "--min-chunks", "2", "--max-spp", "64", "--denoise-out", denoised)
    assert (n["samples"], n["chunks"], n["rendered"]) == (8, 2, 12) and f"Denoised image saved as '{denoised}'" in r.stdout
    sc = host.LoadedScene(SCENES["cornell"], W, H, 8, DEPTH)
    ctx = device.Context(0)
    try:
        ctx.set_scene(sc, sc.camera, sc.settings)
        packed = torch.zeros((H, W), dtype=torch.int32, device="cuda")
        linear = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
        hits = torch.zeros((W * H * 48,), dtype=torch.uint8, device="cuda")
        scratch = torch.zeros((device.denoise_scratch_bytes(W, H),), dtype=torch.uint8, device="cuda")
        out = torch.zeros((H, W), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.render(packed.data_ptr(), linear.data_ptr(), abi.Options.make())
        ctx.first_hits(hits.data_ptr())
        ctx.denoise(W, H, linear.data_ptr(), hits.data_ptr(), scratch.data_ptr(), None, out.data_ptr())
        torch.cuda.synchronize()
        ctx.check()
    finally:
        ctx.close()
    want_plain, want = str(tmp_path / "want_plain.png"), str(tmp_path / "want.png")
    host.write_png(want_plain, packed.cpu().numpy().view(np.uint32), W, H)
    host.write_png(want, out.cpu().numpy().view(np.uint32), W, H)
    assert png == open(want_plain, "rb").read()
    assert open(denoised, "rb").read() == open(want, "rb").read() != png


def test_usage_errors_exit_2(native, tmp_path):
    """Decided before the scene is loaded and before any device is looked for: no GPU needed."""
    s = SCENES["cornell"]
    for args, text in ((("--noise-target", "0.1", "--gpus", "2"), "--gpus or --devices"), (("--noise-target", "0.1", "--gpus", "1"), "--gpus or --devices"),
                       (("--noise-target", "0.1", "--devices", "0"), "--gpus or --devices"), (("--noise-target", "0.1", "--rng", "ref"), "--rng ref"),
                       (("--rng", "ref", "--noise-target", "0.1"), "--rng ref"), (("--noise-out", str(tmp_path / "m.pfm")), "--noise-out needs --noise-target"),
                       (("--noise-target", "-1"), "--noise-target wants"), (("--noise-target", "nan"), "--noise-target wants"),
                       (("--noise-target", "0.1", "--min-chunks", "1"), "--min-chunks wants"), (("--noise-target", "0.1", "--noise-floor", "-1"), "--noise-floor wants"),
                       (("--noise-target", "0.1", "--noise-allow", "1.5"), "--noise-allow wants"), (("--max-spp", "8"), "go with --noise-target")):
        r = _cli(s, *args, expect=2)
        assert r.stderr.startswith("usage:") and text in r.stderr, (args, r.stderr[-300:])
        assert "Attempting to load" not in r.stdout
