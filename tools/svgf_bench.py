#!/usr/bin/env python3
"""Times the variance-guided temporal filter (mi355rt_svgf_accumulate, mi355rt_svgf_filter; libmi355rt_svgf.so) in a frame loop on the GPU beside the
stages it extends, measures what it buys, and writes profiles/svgf_bench.txt.

  python tools/svgf_bench.py [--out profiles/svgf_bench.txt] [--seconds 0.5] [--frames 8] [--step-deg 0.5]

Cornell-box at 800 x 600 along tools/reproject_bench.py's orbit, 2 samples per pixel a frame.  A frame of the new route is
  first hits -> render_view -> svgf accumulate (history, moments, variance; ping-pong) -> svgf filter (defaults)
and of the existing one   first hits -> render_view -> reproject -> denoise (defaults).  Both chains run on the same colour and records.
(a) ms per call on the last frame's buffers: batches of calls between a pair of device events, after a warm-up batch, INTERLEAVED round by round
    (tools/stage_bench.py); median over the rounds and the spread ((max - min) / median).  accumulate against mi355rt_post_reproject, filter at 1 and 5
    levels against mi355rt_context_denoise at 1 and 5 levels, each staged form against its gathers (MI355RT_SVGF_GATHERS_ONLY).
(b) RMSE of every frame against a 1024-spp mi355rt_context_render_view of that frame's camera (another seed): raw, reprojected, the existing route, the new one.
The file records the registers, spills, code size and LDS of the library's kernels.  Without a GPU the tool fails."""
import argparse
import os

import torch  # noqa: F401  -- before the HIP libraries (tests/conftest.py: one HIP runtime in the process)

import stage_bench
from reproject_bench import BATCH, DEPTH, REF_CHUNK, REF_SEED, REF_SPP, SPP, H, W, orbit_camera
from stage_bench import ROOT


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "svgf_bench.txt"))
    ap.add_argument("--seconds", type=float, default=0.5, help="timed work per line, at least")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--step-deg", type=float, default=0.5)
    args = ap.parse_args(argv)
    stage_bench.require_gpu("svgf_bench")
    abi, build, host, device, post, svgf = stage_bench.packages("abi", "build", "host", "device", "post", "svgf")

    sc = host.LoadedScene(os.path.join(ROOT, "data/scenes/tungsten/cornell-box/scene.json"), W, H, SPP, DEPTH)
    n = W * H
    s = torch.cuda.current_stream().cuda_stream
    u8 = lambda size: torch.zeros(size, dtype=torch.uint8, device="cuda")
    f32 = lambda count: torch.zeros(count, dtype=torch.float32, device="cuda")
    ctx = device.Context(0)
    try:
        ctx.set_scene(sc, sc.camera, sc.settings)
        cams = [orbit_camera(abi, sc.camera, k, args.step_deg) for k in range(args.frames)]
        centre = [abi.View.make(c, W, H, abi.VIEW_PINHOLE, abi.VIEW_CENTRE) for c in cams]
        jittered = [abi.View.make(c, W, H, abi.VIEW_PINHOLE) for c in cams]
        d_rays, d_accum = u8(n * 32), f32(n * 4)
        d_scratch = u8(max(device.view_scratch_bytes(jittered[0], REF_CHUNK), device.denoise_scratch_bytes(W, H), svgf.scratch_bytes(W, H)))
        d_hits, d_hist, d_moments, d_rep_hist = [u8(n * 48), u8(n * 48)], [f32(n * 4), f32(n * 4)], [f32(n * 2), f32(n * 2)], [f32(n * 4), f32(n * 4)]
        d_var, d_raw, d_rep, d_old, d_new, d_ref = f32(n), f32(n * 3), f32(n * 3), f32(n * 3), f32(n * 3), f32(n * 3)
        p = lambda t: t.data_ptr()

        def first_hits(k, me):
            ctx.view_rays(centre[k], 0, p(d_rays), 0, s)
            ctx.trace_rays(p(d_rays), n, p(d_hits[me]), s)

        def colour(k):
            ctx.render_view(jittered[k], abi.RadianceParams.make(0, SPP, DEPTH, seed=k), p(d_accum), p(d_scratch), p(d_raw), None, s)

        def reproject(k, me):
            o = me ^ 1
            post.reproject(centre[k], centre[k - 1] if k else None, p(d_hits[me]), p(d_raw), p(d_hits[o]) if k else None, p(d_rep_hist[o]) if k else None,
                           p(d_rep_hist[me]), p(d_rep), None, None, 0, s)

        def accumulate(k, me, prev=True):
            o, prev = me ^ 1, prev and k > 0
            svgf.accumulate(centre[k], centre[k - 1] if prev else None, p(d_hits[me]), p(d_raw), p(d_hits[o]) if prev else None, p(d_hist[o]) if prev else None,
                            p(d_moments[o]) if prev else None, p(d_hist[me]), p(d_moments[me]), p(d_var), None, 0, s)

        def denoise(src, dst, me, params=None):
            ctx.denoise(W, H, p(src), p(d_hits[me]), p(d_scratch), p(dst), None, params, s)

        def svgf_filter(me, params=None):
            svgf.filter(W, H, p(d_hist[me]), p(d_var), p(d_hits[me]), p(d_scratch), p(d_new), None, params, 0, s)

        rmse = lambda a: float(torch.sqrt(torch.mean((a.double() - d_ref.double()) ** 2)).item())
        # (b) both chains, once: what each frame's images are worth
        quality = []
        for k in range(args.frames):
            me = k & 1
            for begin in range(0, REF_SPP, REF_CHUNK):
                ctx.render_view(jittered[k], abi.RadianceParams.make(begin, begin + REF_CHUNK, DEPTH, seed=REF_SEED), p(d_accum), p(d_scratch), p(d_ref), None, s)
            first_hits(k, me); colour(k); reproject(k, me); accumulate(k, me)
            denoise(d_rep, d_old, me); svgf_filter(me)
            torch.cuda.synchronize()
            ctx.check()
            assert torch.equal(d_hist[me].view(torch.int32), d_rep_hist[me].view(torch.int32)), "accumulate's history is not the reprojection's"
            spatial = float((d_hist[me].view(-1, 4)[:, 3] < 4).float().mean().item())      # (an upper bound of the estimated pixels but for moment restarts: the default min_temporal is 4)
            quality.append((rmse(d_raw), rmse(d_rep), rmse(d_old), rmse(d_new), float(d_var.mean().item()), spatial))

        # (a) the stages on the last frame's buffers (its previous frame's hits, history and moments stay where the chain left them)
        k = args.frames - 1
        me = k & 1
        dn = lambda levels: abi.DenoiseParams.make(levels=levels)
        fp = lambda levels, flags=0: abi.SvgfFilterParams.make(levels=levels, flags=flags)
        G = abi.SVGF_GATHERS_ONLY
        calls = {"reproject": lambda: reproject(k, me), "svgf accumulate": lambda: accumulate(k, me),
                 "svgf accumulate, no previous frame": lambda: accumulate(k, me, prev=False),
                 "denoise, levels = 1": lambda: denoise(d_rep, d_old, me, dn(1)), "svgf filter, levels = 1": lambda: svgf_filter(me, fp(1)),
                 "svgf filter, levels = 1, gathers": lambda: svgf_filter(me, fp(1, G)),
                 "denoise, levels = 2": lambda: denoise(d_rep, d_old, me, dn(2)), "svgf filter, levels = 2": lambda: svgf_filter(me, fp(2)),
                 "svgf filter, levels = 2, gathers": lambda: svgf_filter(me, fp(2, G)),
                 "denoise, levels = 5": lambda: denoise(d_rep, d_old, me, dn(5)), "svgf filter, levels = 5": lambda: svgf_filter(me, fp(5)),
                 "svgf filter, levels = 5, gathers": lambda: svgf_filter(me, fp(5, G))}
        ms = stage_bench.interleaved_rounds(calls, args.seconds, BATCH)
        accumulate(k, me)                                                 # (the line without a previous frame was the last to write the frame's buffers)
        torch.cuda.synchronize()
        ctx.check()
        assert torch.equal(d_hist[me].view(torch.int32), d_rep_hist[me].view(torch.int32)), "the timed calls did not reproduce the chain's history"
    finally:
        ctx.close()

    med, spread = stage_bench.summary(ms)
    table, _ = stage_bench.kernel_table(build.SVGF_SO, None, 24)
    post_table, _ = stage_bench.kernel_table(build.POST_SO, None, 24)
    lines = [stage_bench.header("svgf_bench", f"--seconds {args.seconds:g} --frames {args.frames} --step-deg {args.step_deg:g}"),
             "# the kernels of the measured library (tools/isa_stats.py), and the reprojection's beside them:"] + table + post_table[1:]
    lines += ["", f"## (a) cornell-box, {W} x {H}, frame {k} of the orbit ({args.step_deg:g} degrees a frame): ms per call",
              f"##     ms = median over the rounds of (device events around {BATCH} calls back to back) / {BATCH}; spread = (max - min) / median of the rounds; rounds interleave every line",
              f"{'':>38s} {'ms per call':>11s} {'(min)':>8s} {'(max)':>8s} {'spread':>7s} {'rounds':>6s}"]
    for name in calls:
        lines.append(f"{name:>38s} {med[name]:11.4f} {min(ms[name]):8.4f} {max(ms[name]):8.4f} {spread[name] * 100:6.2f}% {len(ms[name]):6d}")
    ratio = lambda a, b: f"{a} / {b} = {med[a] / med[b]:.3f}"
    lines += ["## " + ratio("svgf accumulate", "reproject") + "   (expected within 1.5)",
              "## " + ratio("svgf accumulate, no previous frame", "reproject") + "   (every pixel takes the 7 x 7 estimate)"]
    lines += ["## " + ratio(f"svgf filter, levels = {lv}", f"denoise, levels = {lv}") + ("   (expected within 1.3)" if lv != 2 else "") for lv in (1, 2, 5)]
    lines += ["## staged / gathers: " + ratio(f"svgf filter, levels = {lv}", f"svgf filter, levels = {lv}, gathers") for lv in (1, 2, 5)]
    lines += ["", f"## (b) RMSE (linear RGB) against {REF_SPP} spp of the same camera (render_view, seed {REF_SEED}), {SPP} spp a frame, seed = frame number; every stage with its defaults",
              f"{'frame':>5s} {'raw':>9s} {'reprojected':>11s} {'reproject -> denoise':>20s} {'accumulate -> filter':>20s} {'mean variance':>13s} {'length < 4':>10s}"]
    for i, q in enumerate(quality):
        lines.append(f"{i:5d} {q[0]:9.5f} {q[1]:11.5f} {q[2]:20.5f} {q[3]:20.5f} {q[4]:13.5f} {q[5] * 100:9.2f}%")
    stage_bench.write_report(lines, args.out)


if __name__ == "__main__":
    main()
