#!/usr/bin/env python3
"""Times the denoiser (mi355rt_context_denoise) on the GPU and writes profiles/denoise.txt.

  python tools/denoise_bench.py [--out profiles/denoise.txt] [--seconds 0.3] [--step-timeout 240]

For cornell-box and teapot at 800 x 600 and 1920 x 1080: the frame is rendered at 4 samples per pixel, its first hits are taken, and then
  - mi355rt_context_denoise with the defaults (5 levels): ms per call, device events around each call;
  - the same call with levels = 0 .. 5: the increments are the kernels (levels 0 is k_denoise_copy alone; levels 1 is k_denoise_prepass and
    the step-1 level; every further level adds one launch with the next step);
  - the A/B behind the kernels' form: levels = 1, 2 and 5 once more with the step-1 and step-2 levels gathering from global memory like the
    later ones (diagnostic knob denoise_staged = 0) instead of reading their tile and halo from LDS (the product);
  - for comparison mi355rt_context_first_hits (events around each launch) and mi355rt_context_render of the same frame at 4 samples per
    pixel (mi355rt_context_set_timing: path tracing + resolve kernel) -- the cheapest other way to a lower-noise preview is more samples.
Calls are enqueued back to back in batches, the figures alternate batch by batch, each until it has --seconds of timed kernel work behind a
warm-up batch; the median is reported.  Every (scene, size) step runs in a process of its own under --step-timeout, and the first step that
fails ends the tool.  The file records build.kernel_hash() and the registers, code bytes and LDS of the k_denoise* kernels (tools/isa_stats.py).
Without a GPU the tool fails; it measures nothing on the CPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import stage_bench
from stage_bench import ROOT

SCENES = {"cornell-box": ("data/scenes/tungsten/cornell-box/scene.json", False), "teapot": ("data/scenes/tungsten/teapot/scene.json", True)}
SIZES = [(800, 600), (1920, 1080)]
SPP = 4
BATCH = 50


def step(name, W, H, seconds):
    """One (scene, size): runs in a child process, prints one JSON line."""
    import torch
    abi, host, device = stage_bench.packages("abi", "host", "device")
    path, skip = SCENES[name]
    sc = host.LoadedScene(os.path.join(ROOT, path), W, H, SPP, 0, skip_unknown_primitives=skip)           # max_depth 0: the scene file's own
    ctx = device.Context(0)
    try:
        ctx.set_scene(sc, sc.camera, sc.settings)
        n = W * H
        packed = torch.zeros(n, dtype=torch.int32, device="cuda")
        linear = torch.zeros(n * 3, dtype=torch.float32, device="cuda")
        hits = torch.zeros(n * 12, dtype=torch.int32, device="cuda")
        scratch = torch.zeros(device.denoise_scratch_bytes(W, H), dtype=torch.uint8, device="cuda")
        out_packed = torch.zeros(n, dtype=torch.int32, device="cuda")
        out_linear = torch.zeros(n * 3, dtype=torch.float32, device="cuda")
        stream = torch.cuda.current_stream()
        s = stream.cuda_stream
        ctx.render(packed.data_ptr(), linear.data_ptr(), None, s)
        ctx.first_hits(hits.data_ptr(), None, s)
        torch.cuda.synchronize()

        timed = lambda call: stage_bench.timed_launches(stream, call, BATCH)

        def denoise(levels):
            p = abi.DenoiseParams.make(levels=levels)
            return lambda: ctx.denoise(W, H, linear.data_ptr(), hits.data_ptr(), scratch.data_ptr(), out_linear.data_ptr(), out_packed.data_ptr(), p, s)

        def render_batch():
            for _ in range(BATCH):
                ctx.render(packed.data_ptr(), None, None, s)
            torch.cuda.synchronize()
            r, v, launches = ctx.read_timing()
            assert launches == BATCH, launches
            return (r + v) / BATCH

        def gathers(levels):                                             # the A/B: the same call with the first two levels gathering too
            call = denoise(levels)

            def both():
                ctx.set_knob("denoise_staged", 0); call(); ctx.set_knob("denoise_staged", 1)
            return both

        figures = {f"levels{k}": denoise(k) for k in range(6)}
        figures.update({f"gathers{k}": gathers(k) for k in (1, 2, 5)})
        figures["first_hits"] = lambda: ctx.first_hits(hits.data_ptr(), None, s)
        ctx.set_timing(True)
        for call in figures.values():
            timed(call)
        render_batch()                                                   # warm-up: code objects, the row tables, the workspace
        ms = {k: [] for k in figures}
        render_ms = []
        while min(sum(v) for v in ms.values()) < seconds * 1e3 or sum(render_ms) * BATCH < seconds * 1e3:
            for k, call in figures.items():
                if sum(ms[k]) < seconds * 1e3:
                    ms[k] += timed(call)
            if sum(render_ms) * BATCH < seconds * 1e3:
                render_ms.append(render_batch())
        ctx.check()
        res = {"scene": name, "W": W, "H": H, "variant": ctx.kernel_variant(), "render_ms": statistics.median(render_ms), "render_launches": len(render_ms) * BATCH}
        for k, v in ms.items():
            res[k] = statistics.median(v); res[k + "_min"] = min(v); res[k + "_n"] = len(v)
        print("RESULT " + json.dumps(res), flush=True)
    finally:
        ctx.close()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise.txt"))
    ap.add_argument("--seconds", type=float, default=0.3, help="timed kernel work per figure, at least")
    ap.add_argument("--step-timeout", type=float, default=240.0, help="seconds one (scene, size) step may take")
    ap.add_argument("--step", nargs=3, metavar=("SCENE", "W", "H"), help="run one step in this process (what the tool starts for every step)")
    args = ap.parse_args(argv)
    import torch  # noqa: F401  -- before the HIP library (tests/conftest.py: one HIP runtime in the process)
    if args.step:
        stage_bench.require_gpu("denoise_bench")
        return step(args.step[0], int(args.step[1]), int(args.step[2]), args.seconds)
    build, = stage_bench.packages("build")
    lines = [stage_bench.header("denoise_bench", f"--seconds {args.seconds:g}", device_name=False), "# k_denoise* kernels of the measured library (tools/isa_stats.py):"]
    lines += stage_bench.kernel_table(build.DEVICE_SO, lambda k: "k_denoise" in k, 24, insts=False)[0]
    lines += ["", f"## mi355rt_context_denoise with the defaults (levels 5) on a {SPP}-spp frame, beside mi355rt_context_first_hits and a {SPP}-spp mi355rt_context_render of the same frame",
              f"##   ms = median per call, device events around each call (render: path tracing + resolve kernel by mi355rt_context_set_timing); batches of {BATCH} back to back, alternating",
              f"{'scene':12s} {'size':>10s} {'variant':>7s} {'denoise ms':>10s} {'(min)':>8s} {'calls':>6s} {'first_hits ms':>13s} {'render 4spp ms':>14s} {'launches':>8s} {'denoise / render':>16s}"]
    per_kernel = ["", "## the same call with levels 0 .. 5: ms per call and what each level adds (levels 0: k_denoise_copy; 1: k_denoise_prepass + the step-1 level;",
                  "##   every further level: one more launch; steps 1 and 2 are the staged kernels)",
                  f"{'scene':12s} {'size':>10s} " + " ".join(f"{'levels ' + str(k):>9s}" for k in range(6)) + "   " + " ".join(f"{'+step ' + str(1 << k):>9s}" for k in range(1, 5))]
    ab = ["", "## A/B: the levels with step 1 and 2 with their tile and halo staged in LDS (the product) against the same levels as global gathers (diagnostic knob",
          "##   denoise_staged = 0): ms per call of levels = 1, 2 and 5, same batches, same process; ratio = staged / gathers",
          f"{'scene':12s} {'size':>10s} " + " ".join(f"{'gathers L' + str(k):>10s} {'staged L' + str(k):>10s} {'ratio':>6s}" for k in (1, 2, 5))]
    for name in SCENES:
        for W, H in SIZES:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--seconds", str(args.seconds), "--step", name, str(W), str(H)],
                               capture_output=True, text=True, timeout=args.step_timeout)
            got = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
            if r.returncode != 0 or not got:
                sys.exit(f"denoise_bench: step {name} {W}x{H} failed ({r.returncode}); nothing more is run\n{r.stdout}\n{r.stderr}")
            v = json.loads(got[0][7:])
            lines.append(f"{name:12s} {f'{W}x{H}':>10s} {v['variant']:7d} {v['levels5']:10.4f} {v['levels5_min']:8.4f} {v['levels5_n']:6d} {v['first_hits']:13.4f} "
                         f"{v['render_ms']:14.4f} {v['render_launches']:8d} {v['levels5'] / v['render_ms']:16.3f}")
            per_kernel.append(f"{name:12s} {f'{W}x{H}':>10s} " + " ".join(f"{v['levels' + str(k)]:9.4f}" for k in range(6)) + "   " +
                              " ".join(f"{v['levels' + str(k + 1)] - v['levels' + str(k)]:9.4f}" for k in range(1, 5)))
            ab.append(f"{name:12s} {f'{W}x{H}':>10s} " + " ".join(f"{v['gathers' + str(k)]:10.4f} {v['levels' + str(k)]:10.4f} {v['levels' + str(k)] / v['gathers' + str(k)]:6.3f}" for k in (1, 2, 5)))
            print(lines[-1], flush=True)
            print(per_kernel[-1], flush=True)
            print(ab[-1], flush=True)
    stage_bench.write_report(lines + per_kernel + ab, args.out, echo=False)


if __name__ == "__main__":
    main()
