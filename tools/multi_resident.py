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
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import torch  # noqa: F401  -- before the HIP library (tests/conftest.py: one HIP runtime in the process)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    bench = importlib.import_module("bench")
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--devices", default="0", help="comma-separated HIP devices; the first holds the image (a device may repeat)")
    ap.add_argument("--workload", default="cornell-box-800x600x256-d30", choices=sorted(bench.WORKLOADS))
    ap.add_argument("--calls", type=int, default=10, help="resident renders timed (the median is reported)")
    ap.add_argument("--strip-rows", type=int, default=0, help="rows per strip dealt round-robin over the parts (0 -> 4)")
    args = ap.parse_args(argv)
    devices = [int(d) for d in args.devices.split(",") if d.strip()]
    abi = importlib.import_module("raytracer-rust_amd.abi")
    host = importlib.import_module("raytracer-rust_amd.host")
    device = importlib.import_module("raytracer-rust_amd.device")
    path, W, H, spp, depth, skip_unknown = bench.WORKLOADS[args.workload]
    sc = host.LoadedScene(os.path.join(ROOT, path), W, H, spp, depth, skip_unknown_primitives=skip_unknown)
    opt = abi.Options.make(strip_rows=args.strip_rows)
    dev0 = torch.device(f"cuda:{devices[0]}")

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


if __name__ == "__main__":
    sys.exit(main())
