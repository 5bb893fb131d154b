#!/usr/bin/env python3
"""Times the ray queries (mi355rt_context_first_hits, mi355rt_context_trace_rays) on the GPU and writes profiles/ray_queries.txt.

  python tools/query_bench.py [--out profiles/ray_queries.txt] [--seconds 0.5]

(a) First-hit pass at 800 x 600 on cornell-box, teapot and semesterbild: ms per launch and rays/s of mi355rt_context_first_hits, beside the
    same library's cheapest other way to reach first hits, in the same process: mi355rt_context_render at 1 sample per pixel, max_depth 1
    (path-tracing kernel + resolve kernel: the persistent render kernel with its generator, workspace store and resolve).
    Both are timed per launch with device events around the kernels -- the render through mi355rt_context_set_timing, the query with an
    event pair of its own --, launches enqueued back to back in batches, batches alternating between the two, until each has at least
    --seconds of timed kernel work after a warm-up batch.  The back-to-back figure (events around a whole batch of queries: launch gaps
    included) is printed too.
(b) Incoherent rays: 2^20 random rays on teapot (origins on a sphere around the scene's bounds, aimed at random points inside them) through
    mi355rt_context_trace_rays (device buffers, device events), beside the parent's only per-ray path, the test hook mi355rt_debug_hit, named
    for what it is: per-call allocation, pageable host copies, 64-lane workgroups on the NULL stream; host clock around the blocking call.
    The ratio has no threshold.  The two results are compared word for word.
The file records build.kernel_hash() and the registers, spills and scratch of the k_query_* kernels (tools/isa_stats.py).  Without a GPU the
tool fails; it measures nothing on the CPU."""
import argparse
import ctypes as C
import os
import statistics
import time

import numpy as np
import torch  # noqa: F401  -- before the HIP library (tests/conftest.py: one HIP runtime in the process)

import stage_bench
from stage_bench import ROOT

SCENES = [("cornell-box", "data/scenes/tungsten/cornell-box/scene.json", False), ("teapot", "data/scenes/tungsten/teapot/scene.json", True),
          ("semesterbild", "data/scenes/semesterbild.json", False)]
W, H = 800, 600
BATCH = 100


def first_hit_pass(abi, host, device, name, path, skip_unknown, seconds):
    sc = host.LoadedScene(os.path.join(ROOT, path), W, H, 1, 1, skip_unknown_primitives=skip_unknown)        # 1 sample per pixel, max_depth 1
    ctx = device.Context(0)
    try:
        ctx.set_scene(sc, sc.camera, sc.settings)
        n = W * H
        hits = torch.zeros(n * 12, dtype=torch.int32, device="cuda")
        packed = torch.zeros(n, dtype=torch.int32, device="cuda")
        stream = torch.cuda.current_stream()
        s = stream.cuda_stream

        query_batch = lambda: stage_bench.timed_launches(stream, lambda: ctx.first_hits(hits.data_ptr(), None, s), BATCH)

        def render_batch():
            for _ in range(BATCH):
                ctx.render(packed.data_ptr(), None, None, s)
            torch.cuda.synchronize()
            r, v, launches = ctx.read_timing()
            assert launches == BATCH, launches
            return (r + v) / BATCH, r / BATCH

        ctx.set_timing(True)
        query_batch(); render_batch()                                        # warm-up: code objects, the row tables, the workspace
        q_ms, r_ms, r_trace_ms = [], [], []
        while sum(q_ms) < seconds * 1e3 or sum(r_ms) * BATCH < seconds * 1e3:
            q_ms += query_batch()
            both, trace = render_batch()
            r_ms.append(both); r_trace_ms.append(trace)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        reps = max(BATCH, int(seconds * 1e3 / max(statistics.median(q_ms), 1e-3)))
        e0.record(stream)
        for _ in range(reps):
            ctx.first_hits(hits.data_ptr(), None, s)
        e1.record(stream); torch.cuda.synchronize()
        ctx.check()
        rec = np.frombuffer(hits.cpu().numpy().tobytes(), abi.HIT_DTYPE)
        q, r = statistics.median(q_ms), statistics.median(r_ms)
        return {"scene": name, "variant": ctx.kernel_variant(), "query_ms": q, "query_ms_min": min(q_ms), "query_launches": len(q_ms),
                "query_back_to_back_ms": e0.elapsed_time(e1) / reps, "render1_ms": r, "render1_trace_ms": statistics.median(r_trace_ms),
                "render1_launches": len(r_ms) * BATCH, "rays_per_s": n / (q * 1e-3), "misses": int((rec["primitive"] == abi.NO_HIT).sum())}
    finally:
        ctx.close()


def incoherent(abi, host, device, seconds):
    name, path, skip_unknown = SCENES[1]
    sc = host.LoadedScene(os.path.join(ROOT, path), W, H, 1, 1, skip_unknown_primitives=skip_unknown)
    c = sc.c if hasattr(sc, "c") else sc
    tri = np.ctypeslib.as_array(C.cast(c.triangles, C.POINTER(C.c_float)), shape=(c.n_triangles, 12))[:, :9].reshape(-1, 3)    # teapot's meshes are untransformed
    lo, hi = tri.min(axis=0).astype(np.float64), tri.max(axis=0).astype(np.float64)
    centre, radius = (lo + hi) / 2, float(np.linalg.norm(hi - lo))            # a sphere of twice the bounds' half diagonal
    n = 1 << 20
    rng = np.random.default_rng(20)
    p = rng.normal(size=(n, 3)); p = centre + radius * p / np.linalg.norm(p, axis=1, keepdims=True)
    d = rng.uniform(lo, hi, (n, 3)) - p
    rays = np.zeros((n, 8), np.float32); rays[:, 0:3], rays[:, 4:7] = p, d
    rays6 = np.ascontiguousarray(np.concatenate([rays[:, 0:3], rays[:, 4:7]], axis=1))
    ctx = device.Context(0)
    try:
        ctx.set_scene(sc, sc.camera, sc.settings)
        d_rays, d_hits = torch.from_numpy(rays).cuda(), torch.zeros(n * 12, dtype=torch.int32, device="cuda")
        stream = torch.cuda.current_stream()
        torch.cuda.synchronize()

        batch = lambda k: stage_bench.timed_launches(stream, lambda: ctx.trace_rays(d_rays.data_ptr(), n, d_hits.data_ptr(), stream.cuda_stream), k)

        batch(3)
        q_ms = []
        while sum(q_ms) < seconds * 1e3:
            q_ms += batch(20)
        L = device.lib()
        out = np.zeros((n, 12), np.float32)
        call = lambda: device._check(L.mi355rt_debug_hit(ctx._h, C.c_void_p(rays6.ctypes.data), n, C.c_void_p(out.ctypes.data)), "mi355rt_debug_hit")
        call()
        hook_ms = []
        while sum(hook_ms) < seconds * 1e3:
            t0 = time.perf_counter(); call(); hook_ms.append((time.perf_counter() - t0) * 1e3)
        ctx.check()
        rec = np.frombuffer(d_hits.cpu().numpy().tobytes(), abi.HIT_DTYPE)
        hit = rec["primitive"] != abi.NO_HIT
        same = (hit == (out[:, 9] == 1.0)).all() and (rec["position"][hit].view(np.uint32) == out[hit, 0:3].view(np.uint32)).all() and \
            (rec["t"][hit].view(np.uint32) == out[hit, 6].view(np.uint32)).all() and (rec["normal"][hit].view(np.uint32) == out[hit, 3:6].view(np.uint32)).all()
        q, hk = statistics.median(q_ms), statistics.median(hook_ms)
        return {"scene": name, "rays": n, "misses": int((~hit).sum()), "query_ms": q, "query_launches": len(q_ms), "rays_per_s": n / (q * 1e-3),
                "hook_ms": hk, "hook_calls": len(hook_ms), "hook_rays_per_s": n / (hk * 1e-3), "ratio": hk / q, "same_as_hook": bool(same)}
    finally:
        ctx.close()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ray_queries.txt"))
    ap.add_argument("--seconds", type=float, default=0.5, help="timed kernel work per figure, at least")
    args = ap.parse_args(argv)
    stage_bench.require_gpu("query_bench")
    abi, build, host, device = stage_bench.packages("abi", "build", "host", "device")
    lines = [stage_bench.header("query_bench", f"--seconds {args.seconds:g}"), "# k_query_* kernels of the measured library (tools/isa_stats.py):"]
    lines += stage_bench.kernel_table(build.DEVICE_SO, lambda k: "k_query" in k, 22)[0]
    lines += ["", f"## (a) first-hit pass, {W} x {H} = {W * H} camera rays: mi355rt_context_first_hits against mi355rt_context_render at 1 spp, max_depth 1 (render + resolve kernel)",
              "##     ms = median per launch, device events around the kernels; launches back to back in alternating batches of %d" % BATCH,
              f"{'scene':14s} {'render variant':>14s} {'misses':>7s} {'first_hits ms':>13s} {'(min)':>8s} {'launches':>8s} {'Mrays/s':>9s} {'back-to-back ms':>15s} "
              f"{'render 1spp ms':>14s} {'(trace only)':>12s} {'launches':>8s} {'render / first_hits':>19s}"]
    for name, path, skip in SCENES:
        r = first_hit_pass(abi, host, device, name, path, skip, args.seconds)
        lines.append(f"{r['scene']:14s} {r['variant']:14d} {r['misses']:7d} {r['query_ms']:13.4f} {r['query_ms_min']:8.4f} {r['query_launches']:8d} {r['rays_per_s'] / 1e6:9.1f} "
                     f"{r['query_back_to_back_ms']:15.4f} {r['render1_ms']:14.4f} {r['render1_trace_ms']:12.4f} {r['render1_launches']:8d} {r['render1_ms'] / r['query_ms']:19.2f}")
        print(lines[-1], flush=True)
    b = incoherent(abi, host, device, args.seconds)
    lines += ["", "## (b) incoherent rays on teapot: 2^20 rays from a sphere around the scene's bounds to random points inside them",
              "##     mi355rt_context_trace_rays: device buffers, median ms per launch by device events",
              "##     mi355rt_debug_hit (the parent's test hook: per-call allocation, pageable host copies, 64-lane workgroups, NULL stream): median wall ms per blocking call",
              f"{'scene':14s} {'rays':>8s} {'misses':>7s} {'trace_rays ms':>13s} {'launches':>8s} {'Mrays/s':>9s} {'debug_hit ms':>12s} {'calls':>6s} {'Mrays/s':>9s} {'debug_hit / trace_rays':>22s} {'same records':>12s}",
              f"{b['scene']:14s} {b['rays']:8d} {b['misses']:7d} {b['query_ms']:13.4f} {b['query_launches']:8d} {b['rays_per_s'] / 1e6:9.1f} {b['hook_ms']:12.3f} {b['hook_calls']:6d} "
              f"{b['hook_rays_per_s'] / 1e6:9.1f} {b['ratio']:22.1f} {str(b['same_as_hook']):>12s}"]
    print(lines[-1], flush=True)
    stage_bench.write_report(lines, args.out, echo=False)


if __name__ == "__main__":
    main()
