#!/usr/bin/env python3
"""Times rt_render --noise-target (the converging loop) against a fixed-spp chunked render and writes profiles/converge.txt.

  python tools/converge_bench.py [--out profiles/converge.txt] [--repeats 3] [--step-timeout 120] [--chunk 64] [--stop-chunks 4] [--noise-device] [--append]

cornell-box at 800 x 600, max depth 30, chunks of 64 samples:
  1. a probe run (--noise-target 0 --max-spp 256 --noise-out): the error map after 4 chunks; the target is set just above the error that
     --noise-allow 0.05 of the pixels exceed, so that the verdict holds at chunk 4 (--min-chunks 4 keeps it from holding earlier);
  2. the converging run with that target and --max-spp 1024: it must stop at 256 samples with one speculative chunk behind it (rendered = 320);
     wall_ms, kernel_ms and the host's time per mi355rt_noise_update / mi355rt_noise_evaluate are what the tool prints;
  3. the fixed run `--chunk 64 --spp 256` of the same binary (mi355rt_render_progressive: the code path this feature leaves as it was).
--noise-device adds, alternating with the others, the same converging run with the estimate taken on the device (rt_render --noise-device:
`noise device: pass_ms=`, the device time of update + evaluate per chunk) and writes profiles/converge_device.txt unless --out says otherwise;
--chunk N and --stop-chunks K set the samples per chunk and the chunk the verdict holds at (small chunks: where the host pass falls behind).
Every step is one rt_render process under its own `timeout -k 10`; the steps of a phase are chained with `&&`, so nothing is started after a
step that failed, hung or was killed, and the tool stops there.  Without a GPU the first step fails; nothing is measured on the CPU."""
import argparse
import os
import re
import shlex
import statistics
import subprocess
import sys
import tempfile

import stage_bench
from stage_bench import ROOT

SCENE = os.path.join(ROOT, "data/scenes/tungsten/cornell-box/scene.json")
W, H, DEPTH, ALLOW = 800, 600, 30, 0.05

NOISE = re.compile(r"^noise: samples=(\d+) chunks=(\d+) rendered=(\d+) above=(\d+) nonfinite=(\d+) max=(\S+) mean=(\S+) converged=([01]) wall_ms=(\S+) kernel_ms=(\S+)$", re.M)
HOST = re.compile(r"^noise host: update_ms=(\S+) evaluate_ms=(\S+) per chunk", re.M)
DEVICE = re.compile(r"^noise device: pass_ms=(\S+) per chunk", re.M)
FIXED = re.compile(r"^Rendered in (\S+) seconds \(.*kernels (\S+) ms path tracing \+ (\S+) ms resolve", re.M)


def chain(steps, timeout_s):
    """steps: [(argv, log path)].  One shell line: every step under its own time limit, joined with &&."""
    line = " && ".join(f"timeout -k 10 {timeout_s:g} {' '.join(shlex.quote(a) for a in argv)} > {shlex.quote(log)} 2>&1" for argv, log in steps)
    rc = subprocess.run(["bash", "-c", line]).returncode
    if rc != 0:
        last = [log for _, log in steps if os.path.exists(log)][-1:]
        tail = open(last[0]).read()[-2000:] if last else ""
        sys.exit(f"converge_bench: a step failed ({rc}; 124 / 137: its time limit); nothing more is run\n{tail}")
    return [open(log).read() for _, log in steps]


def read_pfm_grey(path):
    import numpy as np
    raw = open(path, "rb").read()
    m = re.match(rb"PF\n(\d+) (\d+)\n-1.0\n", raw)
    return np.frombuffer(raw[m.end():], "<f4").reshape(int(m.group(2)), int(m.group(1)), 3)[..., 0]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="profiles/converge.txt, or profiles/converge_device.txt with --noise-device")
    ap.add_argument("--chunk", type=int, default=64, help="samples per chunk")
    ap.add_argument("--stop-chunks", type=int, default=4, help="the chunk the verdict holds at (--min-chunks)")
    ap.add_argument("--noise-device", action="store_true", help="also time the loop with the estimate on the device")
    ap.add_argument("--append", action="store_true", help="add this configuration to --out instead of replacing the file")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--step-timeout", type=float, default=120.0, help="seconds one rt_render process may take")
    args = ap.parse_args(argv)
    if args.chunk < 1 or args.stop_chunks < 2:
        sys.exit("converge_bench: --chunk wants at least 1 sample and --stop-chunks at least 2 chunks")
    CHUNK, KSTOP = args.chunk, args.stop_chunks
    STOP = CHUNK * KSTOP
    args.out = args.out or os.path.join(ROOT, "profiles", "converge_device.txt" if args.noise_device else "converge.txt")
    import numpy as np
    build, = stage_bench.packages("build")
    exe = build.CLI
    if not os.path.exists(exe):
        sys.exit(f"converge_bench: {exe} is missing: build first")
    with tempfile.TemporaryDirectory() as tmp:
        size = ["--width", str(W), "--height", str(H), "--max-depth", str(DEPTH)]
        png = os.path.join(tmp, "out.png")
        probe_map = os.path.join(tmp, "probe.pfm")
        probe = [exe, SCENE, *size, "-o", png, "--chunk", str(CHUNK), "--noise-target", "0", "--max-spp", str(STOP), "--noise-out", probe_map]
        chain([(probe, os.path.join(tmp, "probe.log"))], args.step_timeout)
        err = read_pfm_grey(probe_map).reshape(-1).astype(np.float64)
        err = np.sort(err[~np.isnan(err)])[::-1]
        allowed = int(np.floor(ALLOW * W * H))
        target = float(err[allowed]) * 1.0001                               # above(target) <= allowed at chunk KSTOP
        conv = [exe, SCENE, *size, "-o", png, "--chunk", str(CHUNK), "--noise-target", repr(target), "--noise-allow", repr(ALLOW), "--min-chunks", str(KSTOP),
                "--max-spp", str(4 * STOP)]
        fixed = [exe, SCENE, *size, "-o", png, "--chunk", str(CHUNK), "--spp", str(STOP)]
        kinds = ["conv"] + (["dev"] if args.noise_device else []) + ["fixed"]
        argv_of = {"conv": conv, "dev": conv + ["--noise-device"], "fixed": fixed}
        steps = []
        for i in range(args.repeats):                                       # alternating, so that all see the same machine
            steps += [(argv_of[kind], os.path.join(tmp, f"{kind}{i}.log")) for kind in kinds]
        logs = chain(steps, args.step_timeout)
    rows_c, rows_d, rows_f = [], [], []
    for j, text in enumerate(logs):
        kind = kinds[j % len(kinds)]
        if kind == "fixed":
            m = FIXED.search(text)
            rows_f.append((float(m.group(1)) * 1e3, float(m.group(2)) + float(m.group(3))))
            continue
        n, h = NOISE.search(text), (HOST if kind == "conv" else DEVICE).search(text)
        if not n or not h or (int(n.group(1)), int(n.group(3)), int(n.group(8))) != (STOP, STOP + CHUNK, 1):
            sys.exit(f"converge_bench: the converging run did not stop at {STOP} samples with one speculative chunk\n{text[-1500:]}")
        if kind == "conv":
            rows_c.append((float(n.group(9)), float(n.group(10)), float(h.group(1)), float(h.group(2)), int(n.group(4)), float(n.group(6)), float(n.group(7))))
        else:
            rows_d.append((float(n.group(9)), float(n.group(10)), float(h.group(1)), int(n.group(4)), float(n.group(6)), float(n.group(7))))
    med = lambda rows, i: statistics.median(r[i] for r in rows)
    flags = (f" --chunk {CHUNK}" if CHUNK != 64 else "") + (f" --stop-chunks {KSTOP}" if KSTOP != 4 else "") + (" --noise-device" if args.noise_device else "")
    lines = [stage_bench.header("converge_bench", f"--repeats {args.repeats}{flags}", device_name=False),
             f"# cornell-box {W}x{H}, max depth {DEPTH}, chunks of {CHUNK} samples; target {target!r} with --noise-allow {ALLOW} ({allowed} pixels), --min-chunks {KSTOP}: stops at {STOP} samples",
             "# wall_ms: context, scene upload, buffers, every chunk, the copy back (no file written inside it); kernel_ms: path tracing + resolve kernels, device events",
             f"# converging: kernel_ms covers the samples the device traced (rendered), the speculative chunk included; fixed: rt_render --chunk {CHUNK} --spp {STOP} (mi355rt_render_progressive)",
             "", f"{'run':12s} {'samples':>7s} {'rendered':>8s} {'wall_ms':>10s} {'kernel_ms':>10s} {'update_ms/chunk':>15s} {'evaluate_ms/chunk':>17s}"]
    for r in rows_c:
        lines.append(f"{'converging':12s} {STOP:7d} {STOP + CHUNK:8d} {r[0]:10.3f} {r[1]:10.3f} {r[2]:15.3f} {r[3]:17.3f}")
    for r in rows_d:
        lines.append(f"{'on device':12s} {STOP:7d} {STOP + CHUNK:8d} {r[0]:10.3f} {r[1]:10.3f} {'pass_ms/chunk':>15s} {r[2]:17.3f}")
    for r in rows_f:
        lines.append(f"{'fixed':12s} {STOP:7d} {STOP:8d} {r[0]:10.3f} {r[1]:10.3f}")
    kc, kf = med(rows_c, 1), med(rows_f, 1)
    per_chunk = kf / KSTOP
    lines += ["", f"median converging: wall {med(rows_c, 0):.3f} ms, kernels {kc:.3f} ms; median fixed: wall {med(rows_f, 0):.3f} ms, kernels {kf:.3f} ms",
              f"kernel time of one chunk (fixed / {KSTOP}): {per_chunk:.3f} ms; converging / fixed kernels: {kc / kf:.3f} (one speculative chunk of {KSTOP + 1}: {(STOP + CHUNK) / STOP:.3f})",
              f"host pass per chunk: update {med(rows_c, 2):.3f} ms + evaluate {med(rows_c, 3):.3f} ms = {med(rows_c, 2) + med(rows_c, 3):.3f} ms"
              f" ({'shorter' if med(rows_c, 2) + med(rows_c, 3) < per_chunk else 'LONGER'} than a chunk's kernels)",
              f"at the stop: above {rows_c[0][4]} of {W * H} pixels, max error {rows_c[0][5]:.6g}, mean error {rows_c[0][6]:.6g}"]
    if rows_d:
        wc, wd = sorted(r[0] for r in rows_c), sorted(r[0] for r in rows_d)
        host_pass, dev_pass = med(rows_c, 2) + med(rows_c, 3), med(rows_d, 2)
        lines += ["", f"estimate on the device: median wall {med(rows_d, 0):.3f} ms (runs {wd[0]:.3f} .. {wd[-1]:.3f}), kernels {med(rows_d, 1):.3f} ms;"
                      f" on the host: median wall {med(rows_c, 0):.3f} ms (runs {wc[0]:.3f} .. {wc[-1]:.3f})",
                  f"device wall - host wall: {med(rows_d, 0) - med(rows_c, 0):+.3f} ms; run-to-run spread of the host loop {wc[-1] - wc[0]:.3f} ms, of the device loop {wd[-1] - wd[0]:.3f} ms",
                  f"device pass per chunk (update + evaluate + finish, device events): {dev_pass:.3f} ms = {host_pass / dev_pass:.1f} x shorter than the host pass of {host_pass:.3f} ms;"
                  f" 100 bytes per pixel moved (update 80, evaluate 20): {W * H * 100 / (dev_pass * 1e-3) / 1e9:.1f} GB/s over the pass",
                  f"at the stop (device): above {rows_d[0][3]} of {W * H} pixels, max error {rows_d[0][4]:.6g}, mean error {rows_d[0][5]:.6g}"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        f.write(("\n" if args.append else "") + "\n".join(lines) + "\n")
    print("\n".join(lines))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
