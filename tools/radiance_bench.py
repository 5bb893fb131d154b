#!/usr/bin/env python3
"""Times the radiance query (mi355rt_context_trace_radiance) on the GPU and writes profiles/radiance_bench.txt.

  python tools/radiance_bench.py [--out profiles/radiance_bench.txt] [--seconds 1.0]

Cornell-box, the camera rays of an 800 x 600 image (through the pixel centres, made on the host once, in numpy), 16 samples per call at
max_depth 30: 7.68 M paths per call.  The items a lane of k_radiance_paths owns, K (diagnostic knob "radiance_items"), runs over {1, 2, 4, 8, 16}:
every K has its own timed loop -- batches of calls enqueued back to back between a pair of device events -- after a warm-up batch, and the loops
are interleaved: a round takes one batch of every K and one batch of the yardstick, rounds repeat until every K has at least --seconds of timed
kernel work.  Printed per K: the median ms per call over the rounds, the spread of the rounds ((max - min) / median), and Msamples/s.
The yardstick is the render's own kernel time for the same frame: mi355rt_context_render of 800 x 600 x 16 at depth 30 with the timing pool
(path-tracing kernel and resolve kernel), in the same process and the same rounds.  The query's time includes its k_radiance_sum.
The two do not compute the same image -- the render jitters every sample's camera ray, the query follows ONE ray per pixel 16 times -- but the
same number of paths through the same scene from the same camera.
The file records build.kernel_hash() and the registers, spills and code size of the k_radiance* kernels (tools/isa_stats.py).  Without a GPU the
tool fails; it measures nothing on the CPU."""
import argparse
import os
import statistics

import numpy as np
import torch  # noqa: F401  -- before the HIP library (tests/conftest.py: one HIP runtime in the process)

import stage_bench
from stage_bench import ROOT

W, H, SAMPLES, DEPTH = 800, 600, 16, 30
KS = (1, 2, 4, 8, 16)
BATCH = 8
F = np.float32


def centre_rays(abi, cam):
    """abi.PATH_RAY_DTYPE [H * W]: Camera::get_ray (camera.rs:33-42) through every pixel centre, normalised once; x = column, row = image row."""
    x = np.tile(np.arange(W, dtype=np.uint32), H)
    y = np.repeat(np.arange(H, dtype=np.uint32), W)
    u, v = (x.astype(F) + F(0.5)) / F(W), (y.astype(F) + F(0.5)) / F(H)
    ax = (F(2.0) * u - F(1.0)) * F(cam.half_width)
    ay = (F(1.0) - F(2.0) * v) * F(cam.half_height)
    right, up, fwd = (np.array(list(a), F) for a in (cam.right, cam.true_up, cam.forward))
    raw = fwd[None, :] + (right[None, :] * ax[:, None] + up[None, :] * ay[:, None])
    raw = raw / np.sqrt((raw * raw).sum(-1, keepdims=True, dtype=F))
    rays = np.zeros(H * W, abi.PATH_RAY_DTYPE)
    rays["origin"] = np.array(list(cam.position), F)[None, :]
    rays["direction"] = raw.astype(F)
    rays["x"], rays["row"] = x, y
    return rays


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "radiance_bench.txt"))
    ap.add_argument("--seconds", type=float, default=1.0, help="timed kernel work per K, at least")
    args = ap.parse_args(argv)
    stage_bench.require_gpu("radiance_bench")
    abi, build, host, device = stage_bench.packages("abi", "build", "host", "device")

    sc = host.LoadedScene(os.path.join(ROOT, "data/scenes/tungsten/cornell-box/scene.json"), W, H, SAMPLES, DEPTH)
    n = W * H
    ctx = device.Context(0)
    try:
        ctx.set_scene(sc, sc.camera, sc.settings)
        d_rays = torch.from_numpy(centre_rays(abi, sc.camera).view(np.uint8).reshape(-1).copy()).cuda()
        d_accum = torch.zeros(n * 4, dtype=torch.float32, device="cuda")
        d_linear = torch.zeros(n * 3, dtype=torch.float32, device="cuda")
        d_scratch = torch.zeros(device.radiance_scratch_bytes(n, SAMPLES), dtype=torch.uint8, device="cuda")
        d_packed = torch.zeros(n, dtype=torch.int32, device="cuda")
        stream = torch.cuda.current_stream()
        s = stream.cuda_stream
        prm = abi.RadianceParams.make(0, SAMPLES, DEPTH, 0)

        def query_batch(k):
            ctx.set_knob("radiance_items", k)
            return stage_bench.timed_batch(stream, lambda: ctx.trace_radiance(prm, d_rays.data_ptr(), n, d_accum.data_ptr(), d_scratch.data_ptr(), d_linear.data_ptr(), s), BATCH)

        def render_batch():
            r, v = stage_bench.render_kernel_batch(ctx, d_packed, s, BATCH)
            r_ms.append(r); v_ms.append(v)

        ctx.set_timing(True)
        words, r_ms, v_ms = {}, [], []
        stage_bench.render_kernel_batch(ctx, d_packed, s, BATCH)           # the yardstick's warm-up

        def warmed(k):                                                     # K does not change a word
            words[k] = d_accum.cpu().numpy().tobytes()
            assert words[k] == words[KS[0]], "the sums depend on K"

        ms = stage_bench.interleaved_rounds({k: k for k in KS}, args.seconds, BATCH, query_batch, render_batch, warmed)
        ctx.set_knob("radiance_items", 0)
        ctx.check()
        mean = float(d_linear.cpu().numpy().mean())
        variant = ctx.kernel_variant()
    finally:
        ctx.close()

    rk, vk = statistics.median(r_ms), statistics.median(v_ms)
    med, spread = stage_bench.summary(ms)
    best = min(KS, key=lambda k: med[k])
    lines = [stage_bench.header("radiance_bench", f"--seconds {args.seconds:g}"), "# k_radiance* kernels of the measured library (tools/isa_stats.py):"]
    lines += stage_bench.kernel_table(build.DEVICE_SO, lambda k: "k_radiance" in k, 22)[0]
    lines += ["", f"## cornell-box, {W} x {H} = {n} camera rays (pixel centres), samples [0, {SAMPLES}) per call, max_depth {DEPTH}: {n * SAMPLES} paths per call "
                  f"(k_radiance_paths + k_radiance_sum); image mean {mean:.6f}",
              f"##     ms = median over the rounds of (device events around {BATCH} calls back to back) / {BATCH}; spread = (max - min) / median of the rounds; rounds interleave every K and the yardstick",
              f"{'K (items per lane)':>18s} {'ms per call':>11s} {'(min)':>8s} {'(max)':>8s} {'spread':>7s} {'rounds':>6s} {'Msamples/s':>10s} {'/ K = 1':>8s} {'/ render kernels':>16s}"]
    for k in KS:
        lines.append(f"{k:18d} {med[k]:11.4f} {min(ms[k]):8.4f} {max(ms[k]):8.4f} {spread[k] * 100:6.2f}% {len(ms[k]):6d} {n * SAMPLES / (med[k] * 1e-3) / 1e6:10.1f} "
                     f"{med[k] / med[1]:8.3f} {med[k] / (rk + vk):16.2f}")
    lines += ["", f"## the yardstick: mi355rt_context_render of the same frame ({W} x {H} x {SAMPLES}, max_depth {DEPTH}; variant {variant}), timing pool, same rounds",
              f"{'render kernel ms':>18s} {'resolve kernel ms':>17s} {'both':>8s} {'rounds':>6s} {'Msamples/s':>10s}",
              f"{rk:18.4f} {vk:17.4f} {rk + vk:8.4f} {len(r_ms):6d} {n * SAMPLES / ((rk + vk) * 1e-3) / 1e6:10.1f}",
              "", f"## fastest K: {best} ({med[best]:.4f} ms; K = 1: {med[1]:.4f} ms, {100 * (med[1] - med[best]) / med[1]:+.2f} % against a spread of "
                  f"{100 * max(spread[1], spread[best]):.2f} %); the query takes {med[best] / (rk + vk):.2f} x the render's kernels for the same number of paths"]
    stage_bench.write_report(lines, args.out)


if __name__ == "__main__":
    main()
