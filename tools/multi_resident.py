#!/usr/bin/env python3
"""One-call multi-GPU render (mi355rt_render_multi) against the resident multi-device context (mi355rt_multi_context_*), same frame,
same devices, one process -- prints ONE JSON line.

  python tools/multi_resident.py --devices 0,0 --workload cornell-box-800x600x256-d30 --calls 10

render_multi: wall ms of its first and second call (it creates, uploads and probes on every device and copies to host memory each time).
multi context: wall ms of create + set_scene; then wall ms of resident renders -- host clock around a call that ends in a device
synchronise -- first call, second call and the median of --calls; one more call with stats gives the kernel ms of every part.
image_checksum: sum of the packed image as int64, what bench.py prints as `image_checksum` for the same workload; the line also says
whether the resident image equals render_multi's, packed and linear bit for bit.
A device listed several times is a rehearsal on one GPU (every part renders on the same device): not a scaling figure.

  python tools/multi_resident.py --devices 0,0 --workload cornell-box-800x600x256-d30 --chunk 64

--chunk K prints another line instead: the frame rendered in chunks of K samples on the resident multi context
(mi355rt_multi_context_render_progressive; the last chunk may be shorter) against one resident full-frame call.  Wall ms per chunk (host clock
around a call that ends in a device synchronise) of a timed sequence after a warm-up sequence: the first chunk on its own and the median;
the sequence's total against the median of --calls full-frame calls; the median chunk again when the gathered sums are asked for too
(d_accum: one more peer copy per part and k_gather_accum); and whether the final image equals the full-frame one, packed and linear, bit
for bit.
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import torch  # noqa: F401  -- before the HIP library (tests/conftest.py: one HIP runtime in the process)

import stage_bench
from stage_bench import ROOT


def main(argv=None):
    bench = importlib.import_module("bench")
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--devices", default="0", help="comma-separated HIP devices; the first holds the image (a device may repeat)")
    ap.add_argument("--workload", default="cornell-box-800x600x256-d30", choices=sorted(bench.WORKLOADS))
    ap.add_argument("--calls", type=int, default=10, help="resident renders timed (the median is reported)")
    ap.add_argument("--strip-rows", type=int, default=0, help="rows per strip dealt round-robin over the parts (0 -> 4)")
    ap.add_argument("--chunk", type=int, default=0, help="samples per progressive chunk: time the chunked frame instead (0: off)")
    args = ap.parse_args(argv)
    devices = [int(d) for d in args.devices.split(",") if d.strip()]
    abi, host, device = stage_bench.packages("abi", "host", "device")
    path, W, H, spp, depth, skip_unknown = bench.WORKLOADS[args.workload]
    sc = host.LoadedScene(os.path.join(ROOT, path), W, H, spp, depth, skip_unknown_primitives=skip_unknown)
    opt = abi.Options.make(strip_rows=args.strip_rows)
    dev0 = torch.device(f"cuda:{devices[0]}")
    if args.chunk > 0:
        return chunked(args, devices, sc, opt, dev0, device, W, H, spp)

    one_call_ms = []
    for _ in range(2):
        t0 = time.perf_counter()
        rp, rl, _ = device.render_multi(sc, sc.camera, sc.settings, devices, opt)
        one_call_ms.append((time.perf_counter() - t0) * 1e3)

    packed = torch.zeros((H, W), dtype=torch.int32, device=dev0)
    linear = torch.zeros((H, W, 3), dtype=torch.float32, device=dev0)
    torch.cuda.synchronize(dev0)
    t0 = time.perf_counter()
    m = device.MultiContext(devices)
    m.set_scene(sc, sc.camera, sc.settings)
    create_ms = (time.perf_counter() - t0) * 1e3
    try:
        wall = []
        for _ in range(max(2, args.calls)):
            t0 = time.perf_counter()
            m.render(packed, linear, opt)
            torch.cuda.synchronize(dev0)
            wall.append((time.perf_counter() - t0) * 1e3)
        m.check()
        st = m.render(packed, linear, opt, want_stats=True)
        parts_ms = m.part_kernel_ms()
        torch.cuda.synchronize(dev0)
        img = packed.cpu().numpy().view("uint32")
        lin = linear.cpu().numpy()
    finally:
        m.close()
    median = statistics.median(wall)
    line = {
        "tool": "multi_resident", "workload": args.workload, "devices": devices, "strip_rows": args.strip_rows or 4,
        "gpus_used": len(set(devices)),
        "render_multi_ms": {"first_call": round(one_call_ms[0], 3), "second_call": round(one_call_ms[1], 3)},
        "multi_context_create_set_scene_ms": round(create_ms, 3),
        "resident_render_ms": {"first_call": round(wall[0], 3), "second_call": round(wall[1], 3), "median": round(median, 3), "calls": len(wall)},
        "resident_over_render_multi_second_call": round(median / one_call_ms[1], 4),
        "part_kernel_ms": [round(x, 3) for x in parts_ms],
        "stats": {"render_kernel_ms_max": round(st.render_kernel_ms, 3), "resolve_kernel_ms_max": round(st.resolve_kernel_ms, 3),
                  "total_ms": round(st.total_ms, 3), "samples": st.samples, "rays": st.rays, "rows": st.rows_rendered, "bands": st.bands},
        "msamples_per_s": round(st.samples / (median * 1e3), 1),
        "image_checksum": int(img.astype("int64").sum()),
        "equals_render_multi": bool((img == rp).all() and (lin.view("uint32") == rl.view("uint32")).all()),
        "note": "wall ms = host clock around a call that ends in a device synchronise; a device listed more than once renders every part "
                "on the same GPU (a rehearsal of the protocol, not a scaling figure)",
    }
    print(json.dumps(line), flush=True)
    return 0 if line["equals_render_multi"] else 1


def chunked(args, devices, sc, opt, dev0, device, W, H, spp):
    """--chunk K: the chunked frame on the resident multi context against one resident full-frame call."""
    bounds = [(s, min(s + args.chunk, spp)) for s in range(0, spp, args.chunk)]
    packed = torch.zeros((H, W), dtype=torch.int32, device=dev0)
    linear = torch.zeros((H, W, 3), dtype=torch.float32, device=dev0)
    full_packed, full_linear = torch.zeros_like(packed), torch.zeros_like(linear)
    accum = torch.zeros((H, W, 4), dtype=torch.float32, device=dev0)
    m = device.MultiContext(devices)
    m.set_scene(sc, sc.camera, sc.settings)

    def timed(call):
        torch.cuda.synchronize(dev0)
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize(dev0)
        return (time.perf_counter() - t0) * 1e3

    try:
        full = [timed(lambda: m.render(full_packed, full_linear, opt)) for _ in range(max(2, args.calls) + 1)][1:]   # (the first call warms up)
        sequences = []
        for acc in (None, None, accum):                                # warm-up, timed, timed with the gathered sums
            sequences.append([timed(lambda b=b: m.render_progressive(b[0], b[1], packed, linear, acc, opt)) for b in bounds])
        m.check()
        img, lin = packed.cpu().numpy().view("uint32"), linear.cpu().numpy()
        equal = bool((img == full_packed.cpu().numpy().view("uint32")).all() and (lin.view("uint32") == full_linear.cpu().numpy().view("uint32")).all())
    finally:
        m.close()
    seq, seq_accum = sequences[1], sequences[2]
    full_median = statistics.median(full)
    line = {
        "tool": "multi_resident", "mode": "chunked", "workload": args.workload, "devices": devices, "strip_rows": args.strip_rows or 4,
        "gpus_used": len(set(devices)), "chunk_spp": args.chunk, "chunks": len(bounds),
        "chunk_ms": {"first": round(seq[0], 3), "median": round(statistics.median(seq), 3), "all": [round(x, 3) for x in seq]},
        "chunked_total_ms": round(sum(seq), 3),
        "full_frame_ms": {"median": round(full_median, 3), "calls": len(full)},
        "chunked_over_full_frame": round(sum(seq) / full_median, 4),
        "chunk_ms_with_gathered_sums": {"median": round(statistics.median(seq_accum), 3), "total": round(sum(seq_accum), 3)},
        "image_checksum": int(img.astype("int64").sum()),
        "final_equals_full_frame": equal,
        "note": "wall ms = host clock around a call that ends in a device synchronise; a chunk = every part renders its strips for the chunk's "
                "samples and resolves them, then the peer copies and the gather; a device listed more than once renders every part on the same "
                "GPU (a rehearsal of the protocol, not a scaling figure)",
    }
    print(json.dumps(line), flush=True)
    return 0 if equal else 1


if __name__ == "__main__":
    sys.exit(main())
