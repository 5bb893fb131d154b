#!/usr/bin/env python3
"""Times the camera views (mi355rt_context_render_view) on the GPU and writes profiles/view_bench.txt.

  python tools/view_bench.py [--out profiles/view_bench.txt] [--seconds 1.0]

Cornell-box, 800 x 600, 16 samples per call at max_depth 30: 7.68 M paths per call.  Timed loops, each a batch of calls enqueued back to back
between a pair of device events, after a warm-up batch, INTERLEAVED: a round takes one batch of every line below, rounds repeat until every line
has at least --seconds of timed kernel work.  Per line: the median ms per call over the rounds and their spread ((max - min) / median).
  view pinhole           render_view, the scene's own camera, jittered (the render's image, bit for bit -- checked here against context_render)
  view pinhole centre    the same with MI355RT_VIEW_CENTRE: the rays of the next line, made in the refill instead of loaded
  query, resident rays   mi355rt_context_trace_radiance with K = 8 along resident pixel-centre rays (tools/radiance_bench.py's figure; the rays are view_rays')
  view thin lens         the other model, jittered, from the same pose
  render                 mi355rt_context_render of the same frame, timing pool (path-tracing kernel + resolve kernel)
The host-made route to the same jittered image is timed on the host, once: per sample index, the rays in numpy (pcg4d twice per pixel, vectorised;
checked word for word against mi355rt_context_view_rays), their upload, and one trace_radiance call [s, s + 1) -- wall time for 16 samples, against
the wall time of one render_view call for the same 16.
The file records build.kernel_hash() and the registers, spills and code size of the k_view* kernels.  Without a GPU the tool fails."""
import argparse
import os
import statistics
import time

import numpy as np
import torch  # noqa: F401  -- before the HIP library (tests/conftest.py: one HIP runtime in the process)

import stage_bench
from oracle.rng_np import pcg4d
from stage_bench import ROOT

W, H, SAMPLES, DEPTH = 800, 600, 16, 30
BATCH = 8
F = np.float32
U = np.uint32


def host_rays(abi, cam, s, seed=0):
    """The jittered pinhole rays of sample s, as a host without the views makes them: abi.PATH_RAY_DTYPE [H * W], normalised once."""
    x = np.tile(np.arange(W, dtype=U), H)
    y = np.repeat(np.arange(H, dtype=U), W)
    ykey = y.astype(np.uint64) + np.uint64(seed)
    base = pcg4d(x, np.full_like(x, s), (ykey & np.uint64(0xFFFFFFFF)).astype(U), (ykey >> np.uint64(32)).astype(U))
    w = pcg4d(*base)                                                        # (ray 0, block 0)
    ju, jv = ((a >> U(8)).astype(F) * F(1.0 / 16777216.0) for a in w[:2])
    u, v = (x.astype(F) + ju) / F(W), (y.astype(F) + jv) / F(H)
    ax = (F(2.0) * u - F(1.0)) * F(cam.half_width)
    ay = (F(1.0) - F(2.0) * v) * F(cam.half_height)
    right, up, fwd = (np.array(list(a), F) for a in (cam.right, cam.true_up, cam.forward))
    raw = fwd[None, :] + (right[None, :] * ax[:, None] + up[None, :] * ay[:, None])
    l = np.sqrt((raw[:, 0] * raw[:, 0] + raw[:, 1] * raw[:, 1]) + raw[:, 2] * raw[:, 2])
    rays = np.zeros(H * W, abi.PATH_RAY_DTYPE)
    rays["origin"] = np.array(list(cam.position), F)[None, :]
    rays["direction"] = raw * (F(1.0) / l)[:, None]
    rays["x"], rays["row"] = x, y
    return rays


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "view_bench.txt"))
    ap.add_argument("--seconds", type=float, default=1.0, help="timed kernel work per line, at least")
    args = ap.parse_args(argv)
    stage_bench.require_gpu("view_bench")
    abi, build, host, device = stage_bench.packages("abi", "build", "host", "device")

    sc = host.LoadedScene(os.path.join(ROOT, "data/scenes/tungsten/cornell-box/scene.json"), W, H, SAMPLES, DEPTH)
    cam = sc.camera
    n = W * H
    dist = float(np.linalg.norm(np.array(list(cam.position))))
    views = {"view pinhole": abi.View.make(cam, W, H), "view pinhole centre": abi.View.make(cam, W, H, flags=abi.VIEW_CENTRE),
             "view thin lens": abi.View.make(cam, W, H, abi.VIEW_THIN_LENS, 0, 0.02 * dist, 0.8 * dist)}
    ctx = device.Context(0)
    try:
        ctx.set_scene(sc, cam, sc.settings)
        d_rays = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")        # the resident pixel-centre rays of the query: view_rays' own
        ctx.view_rays(views["view pinhole centre"], 0, d_rays.data_ptr())
        d_accum = torch.zeros(n * 4, dtype=torch.float32, device="cuda")
        d_linear = torch.zeros(n * 3, dtype=torch.float32, device="cuda")
        d_scratch = torch.zeros(device.view_scratch_bytes(views["view pinhole"], SAMPLES), dtype=torch.uint8, device="cuda")
        d_packed = torch.zeros(n, dtype=torch.int32, device="cuda")
        d_render = torch.zeros(n, dtype=torch.int32, device="cuda")
        stream = torch.cuda.current_stream()
        s = stream.cuda_stream
        prm = abi.RadianceParams.make(0, SAMPLES, DEPTH, 0)

        calls = {name: (lambda v=v: ctx.render_view(v, prm, d_accum.data_ptr(), d_scratch.data_ptr(), d_linear.data_ptr(), d_packed.data_ptr(), s)) for name, v in views.items()}
        calls["query, resident rays"] = lambda: ctx.trace_radiance(prm, d_rays.data_ptr(), n, d_accum.data_ptr(), d_scratch.data_ptr(), d_linear.data_ptr(), s)
        order = ["view pinhole", "view pinhole centre", "query, resident rays", "view thin lens"]
        calls = {name: calls[name] for name in order}
        ctx.set_timing(True)
        means, kept, r_ms, v_ms = {}, {}, [], []
        stage_bench.render_kernel_batch(ctx, d_render, s, BATCH)             # the render's warm-up, and its image

        def warmed(name):                                                   # what each line computes
            means[name] = float(d_linear.cpu().numpy().mean())
            if name == "view pinhole":
                assert d_render.cpu().numpy().tobytes() == d_packed.cpu().numpy().tobytes(), "the pinhole view is not the render's image"
            if name == "view pinhole centre":
                kept["centre_sums"] = d_accum.cpu().numpy().tobytes()
            if name == "query, resident rays":
                assert d_accum.cpu().numpy().tobytes() == kept["centre_sums"], "the centre view and the query along centre rays differ"

        def render_batch():
            r, v = stage_bench.render_kernel_batch(ctx, d_render, s, BATCH)
            r_ms.append(r); v_ms.append(v)

        ms = stage_bench.interleaved_rounds(calls, args.seconds, BATCH, after_round=render_batch, warmed=warmed)
        ctx.check()

        # the host-made route to the jittered image, wall time: rays in numpy, upload, one call per sample index
        d_one = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
        ctx.view_rays(views["view pinhole"], 3, d_one.data_ptr(), 0, s)
        torch.cuda.synchronize()
        assert host_rays(abi, cam, 3).tobytes() == d_one.cpu().numpy().tobytes(), "the host-made rays are not view_rays'"
        make_s = upload_s = 0.0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for si in range(SAMPLES):
            t = time.perf_counter()
            rays = host_rays(abi, cam, si)
            make_s += time.perf_counter() - t
            t = time.perf_counter()
            d_one.copy_(torch.from_numpy(rays.view(np.uint8).reshape(-1)))
            torch.cuda.synchronize()
            upload_s += time.perf_counter() - t
            ctx.trace_radiance(abi.RadianceParams.make(si, si + 1, DEPTH, 0), d_one.data_ptr(), n, d_accum.data_ptr(), d_scratch.data_ptr(), d_linear.data_ptr(), s)
        torch.cuda.synchronize()
        host_route_s = time.perf_counter() - t0
        host_packed_ok = d_linear.cpu().numpy().tobytes()
        t0 = time.perf_counter()
        calls["view pinhole"]()
        torch.cuda.synchronize()
        view_wall_s = time.perf_counter() - t0
        assert d_linear.cpu().numpy().tobytes() == host_packed_ok, "the host-made route and the view differ"
        variant = ctx.kernel_variant()
    finally:
        ctx.close()

    rk, vk = statistics.median(r_ms), statistics.median(v_ms)
    med, spread = stage_bench.summary(ms)
    q = "query, resident rays"
    lines = [stage_bench.header("view_bench", f"--seconds {args.seconds:g}"), "# k_view* kernels of the measured library (tools/isa_stats.py):"]
    lines += stage_bench.kernel_table(build.DEVICE_SO, lambda k: "k_view" in k or "k_radiance" in k, 28)[0]
    lines += ["", f"## cornell-box, {W} x {H}, samples [0, {SAMPLES}) per call, max_depth {DEPTH}: {n * SAMPLES} paths per call (paths kernel + sum kernel), K = 8 (the default)",
              f"##     ms = median over the rounds of (device events around {BATCH} calls back to back) / {BATCH}; spread = (max - min) / median of the rounds; rounds interleave every line and the render",
              f"{'':>22s} {'ms per call':>11s} {'(min)':>8s} {'(max)':>8s} {'spread':>7s} {'rounds':>6s} {'Msamples/s':>10s} {'/ query':>8s} {'/ render kernels':>16s} {'image mean':>10s}"]
    for name in order:
        lines.append(f"{name:>22s} {med[name]:11.4f} {min(ms[name]):8.4f} {max(ms[name]):8.4f} {spread[name] * 100:6.2f}% {len(ms[name]):6d} "
                     f"{n * SAMPLES / (med[name] * 1e-3) / 1e6:10.1f} {med[name] / med[q]:8.3f} {med[name] / (rk + vk):16.2f} {means[name]:10.6f}")
    lines += ["", f"## mi355rt_context_render of the same frame ({W} x {H} x {SAMPLES}, max_depth {DEPTH}; variant {variant}), timing pool, same rounds: its packed image is the pinhole view's, word for word",
              f"{'render kernel ms':>18s} {'resolve kernel ms':>17s} {'both':>8s} {'rounds':>6s} {'Msamples/s':>10s}",
              f"{rk:18.4f} {vk:17.4f} {rk + vk:8.4f} {len(r_ms):6d} {n * SAMPLES / ((rk + vk) * 1e-3) / 1e6:10.1f}",
              "", f"## the same rays made or loaded: view pinhole centre {med['view pinhole centre']:.4f} ms, query {med[q]:.4f} ms: "
                  f"{100 * (med['view pinhole centre'] - med[q]) / med[q]:+.2f} % against a spread of {100 * max(spread['view pinhole centre'], spread[q]):.2f} %",
              f"## the jittered pinhole view {med['view pinhole']:.4f} ms: {100 * (med['view pinhole'] - med[q]) / med[q]:+.2f} % against the query (other rays: every sample its own), "
              f"spread {100 * max(spread['view pinhole'], spread[q]):.2f} %",
              "", f"## the host-made route to the jittered image, wall time on the host for {SAMPLES} sample indices (one run; the same linear image, word for word):",
              f"##     rays in numpy {make_s * 1e3:.1f} ms + upload of {SAMPLES} x {n * 32 / 1e6:.2f} MB {upload_s * 1e3:.1f} ms + {SAMPLES} calls = {host_route_s * 1e3:.1f} ms in all;",
              f"##     one render_view call for the same {SAMPLES} samples, enqueue to synchronize: {view_wall_s * 1e3:.3f} ms: {host_route_s / view_wall_s:.0f} x"]
    stage_bench.write_report(lines, args.out)


if __name__ == "__main__":
    main()
