#!/usr/bin/env python3
"""Times the temporal reprojection (mi355rt_post_reproject, libmi355rt_post.so) in a frame loop on the GPU, measures what it buys, and writes
profiles/reproject_bench.txt.

  python tools/reproject_bench.py [--out profiles/reproject_bench.txt] [--seconds 0.5] [--frames 8] [--step-deg 0.5]

Cornell-box at 800 x 600 along a small orbit: the scene's camera swung about the point it looks at, --step-deg a frame.  A frame is
  first hits     mi355rt_context_view_rays(MI355RT_VIEW_CENTRE) + mi355rt_context_trace_rays
  render_view    2 samples per pixel, max_depth 30, params.seed = the frame number
  reproject      this frame's colour and hits, the previous frame's hits and history (ping-pong), d_out_linear and d_out_packed both asked for
  denoise        mi355rt_context_denoise with the defaults (5 levels) on the reprojected image, guided by this frame's hits
(a) ms per stage: each line is a batch of calls enqueued back to back between a pair of device events, after a warm-up batch, INTERLEAVED: a round
    takes one batch of every line, rounds repeat until every line has at least --seconds of timed work.  Median over the rounds and the spread
    ((max - min) / median).  The yardstick of the new kernel is mi355rt_context_denoise with levels = 1 on the same buffers in the same rounds:
    code of the parent commit, 25 taps (a prepass and one staged level) against 4 gathered ones.
(b) RMSE of every frame against a 1024-spp mi355rt_context_render_view of that frame's camera (another seed), for the raw 2-spp frame, the
    reprojected one, the denoised raw one and the denoised reprojected one.
The file records the registers, spills and code size of k_post_reproject.  Without a GPU the tool fails."""
import argparse
import os

import numpy as np
import torch  # noqa: F401  -- before the HIP libraries (tests/conftest.py: one HIP runtime in the process)

import stage_bench
from stage_bench import ROOT

W, H, SPP, DEPTH = 800, 600, 2, 30
REF_SPP, REF_CHUNK, REF_SEED = 1024, 64, 1 << 20
BATCH = 20
F = np.float32


def orbit_camera(abi, cam, frame, step_deg):
    """The camera `cam` swung about the point it looks at (its distance from the origin ahead of it) by frame * step_deg about the y axis: a look-at
    camera as src/camera.rs builds one, in float64, rounded once."""
    pos, fwd = (np.array(list(a), np.float64) for a in (cam.position, cam.forward))
    dist = float(np.linalg.norm(pos)) or 1.0
    target = pos + fwd * dist
    ang = np.radians(step_deg * frame)
    rel = pos - target
    eye = target + np.array([rel[0] * np.cos(ang) + rel[2] * np.sin(ang), rel[1], -rel[0] * np.sin(ang) + rel[2] * np.cos(ang)])
    f = target - eye
    f /= np.linalg.norm(f)
    right = np.cross(f, (0.0, 1.0, 0.0))
    right /= np.linalg.norm(right)
    up = np.cross(right, f)
    out = abi.Camera()
    for name, val in (("position", eye), ("forward", f), ("right", right), ("true_up", up)):
        for i in range(3):
            getattr(out, name)[i] = float(F(val[i]))
    out.half_width, out.half_height = cam.half_width, cam.half_height
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reproject_bench.txt"))
    ap.add_argument("--seconds", type=float, default=0.5, help="timed work per line, at least")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--step-deg", type=float, default=0.5)
    args = ap.parse_args(argv)
    stage_bench.require_gpu("reproject_bench")
    abi, build, host, device, post = stage_bench.packages("abi", "build", "host", "device", "post")

    sc = host.LoadedScene(os.path.join(ROOT, "data/scenes/tungsten/cornell-box/scene.json"), W, H, SPP, DEPTH)
    n = W * H
    stream = torch.cuda.current_stream()
    s = stream.cuda_stream
    u8 = lambda size: torch.zeros(size, dtype=torch.uint8, device="cuda")
    f32 = lambda count: torch.zeros(count, dtype=torch.float32, device="cuda")
    ctx = device.Context(0)
    try:
        ctx.set_scene(sc, sc.camera, sc.settings)
        cams = [orbit_camera(abi, sc.camera, k, args.step_deg) for k in range(args.frames)]
        centre = [abi.View.make(c, W, H, abi.VIEW_PINHOLE, abi.VIEW_CENTRE) for c in cams]
        jittered = [abi.View.make(c, W, H, abi.VIEW_PINHOLE) for c in cams]
        d_rays, d_accum, d_packed = u8(n * 32), f32(n * 4), torch.zeros(n, dtype=torch.int32, device="cuda")
        d_scratch = u8(max(device.view_scratch_bytes(jittered[0], REF_CHUNK), device.denoise_scratch_bytes(W, H)))
        d_hits, d_hist = [u8(n * 48), u8(n * 48)], [f32(n * 4), f32(n * 4)]
        d_raw, d_rep, d_dn_raw, d_dn_rep, d_ref = f32(n * 3), f32(n * 3), f32(n * 3), f32(n * 3), f32(n * 3)

        def first_hits(k, me):
            ctx.view_rays(centre[k], 0, d_rays.data_ptr(), 0, s)
            ctx.trace_rays(d_rays.data_ptr(), n, d_hits[me].data_ptr(), s)

        def colour(k):
            ctx.render_view(jittered[k], abi.RadianceParams.make(0, SPP, DEPTH, seed=k), d_accum.data_ptr(), d_scratch.data_ptr(), d_raw.data_ptr(), None, s)

        def reproject(k, me):
            other = me ^ 1
            post.reproject(centre[k], centre[k - 1] if k else None, d_hits[me].data_ptr(), d_raw.data_ptr(), d_hits[other].data_ptr() if k else None,
                           d_hist[other].data_ptr() if k else None, d_hist[me].data_ptr(), d_rep.data_ptr(), d_packed.data_ptr(), None, 0, s)

        def denoise(src, dst, me, params=None):
            ctx.denoise(W, H, src.data_ptr(), d_hits[me].data_ptr(), d_scratch.data_ptr(), dst.data_ptr(), None, params, s)

        rmse = lambda a: float(torch.sqrt(torch.mean((a.double() - d_ref.double()) ** 2)).item())
        # (b) the chain, once: what each frame's images are worth
        quality = []
        for k in range(args.frames):
            me = k & 1
            for begin in range(0, REF_SPP, REF_CHUNK):
                ctx.render_view(jittered[k], abi.RadianceParams.make(begin, begin + REF_CHUNK, DEPTH, seed=REF_SEED), d_accum.data_ptr(), d_scratch.data_ptr(), d_ref.data_ptr(), None, s)
            first_hits(k, me); colour(k); reproject(k, me)
            denoise(d_raw, d_dn_raw, me); denoise(d_rep, d_dn_rep, me)
            torch.cuda.synchronize()
            ctx.check()
            length = d_hist[me].view(-1, 4)[:, 3]
            quality.append((rmse(d_raw), rmse(d_rep), rmse(d_dn_raw), rmse(d_dn_rep), float(length.mean().item()), float((length == 1).float().mean().item())))

        # (a) the stages on the last frame's buffers (its previous frame's hits and history stay where the chain left them)
        k = args.frames - 1
        me = k & 1
        one_level = abi.DenoiseParams.make(levels=1)
        calls = {"first hits (view_rays + trace_rays)": lambda: first_hits(k, me), f"render_view {SPP} spp": lambda: colour(k),
                 "reproject": lambda: reproject(k, me), "denoise, defaults (5 levels)": lambda: denoise(d_rep, d_dn_rep, me),
                 "denoise, levels = 1 (yardstick)": lambda: denoise(d_rep, d_dn_rep, me, one_level)}

        hist_before = d_hist[me].clone()
        ms = stage_bench.interleaved_rounds(calls, args.seconds, BATCH)
        ctx.check()
        assert torch.equal(hist_before.view(torch.int32), d_hist[me].view(torch.int32)), "the timed calls did not reproduce the chain's history"
    finally:
        ctx.close()

    med, spread = stage_bench.summary(ms)
    lines = [stage_bench.header("reproject_bench", f"--seconds {args.seconds:g} --frames {args.frames} --step-deg {args.step_deg:g}"),
             "# k_post_reproject of the measured library (tools/isa_stats.py):"] + stage_bench.kernel_table(build.POST_SO, None, 28)[0]
    y = "denoise, levels = 1 (yardstick)"
    lines += ["", f"## (a) cornell-box, {W} x {H}, frame {k} of the orbit ({args.step_deg:g} degrees a frame): ms per call",
              f"##     ms = median over the rounds of (device events around {BATCH} calls back to back) / {BATCH}; spread = (max - min) / median of the rounds; rounds interleave every line",
              f"{'':>38s} {'ms per call':>11s} {'(min)':>8s} {'(max)':>8s} {'spread':>7s} {'rounds':>6s} {'/ yardstick':>11s}"]
    for name in calls:
        lines.append(f"{name:>38s} {med[name]:11.4f} {min(ms[name]):8.4f} {max(ms[name]):8.4f} {spread[name] * 100:6.2f}% {len(ms[name]):6d} {med[name] / med[y]:11.3f}")
    verdict = "not slower than" if med["reproject"] <= med[y] else "SLOWER than"
    lines += [f"## reproject {med['reproject']:.4f} ms is {verdict} the yardstick {med[y]:.4f} ms ({med['reproject'] / med[y]:.3f} x; spreads {spread['reproject'] * 100:.2f} % and {spread[y] * 100:.2f} %)",
              f"## the frame's four stages: {sum(med[name] for name in list(calls)[:4]):.4f} ms, of which reproject {100 * med['reproject'] / sum(med[name] for name in list(calls)[:4]):.1f} %",
              "", f"## (b) RMSE (linear RGB) against {REF_SPP} spp of the same camera (render_view, seed {REF_SEED}), {SPP} spp a frame, seed = frame number; reproject and denoise with their defaults",
              f"{'frame':>5s} {'raw':>9s} {'reprojected':>11s} {'denoised raw':>12s} {'denoised reprojected':>20s} {'mean length':>11s} {'restarted':>9s}"]
    for i, q in enumerate(quality):
        lines.append(f"{i:5d} {q[0]:9.5f} {q[1]:11.5f} {q[2]:12.5f} {q[3]:20.5f} {q[4]:11.2f} {q[5] * 100:8.2f}%")
    stage_bench.write_report(lines, args.out)


if __name__ == "__main__":
    main()
