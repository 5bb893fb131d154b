#!/usr/bin/env python3
"""Times the occlusion queries (mi355rt_context_occluded, mi355rt_context_ambient_occlusion) on the GPU and writes profiles/occlusion.txt.

  python tools/occlusion_bench.py [--out profiles/occlusion.txt] [--seconds 0.5]

Baselines are the only other way of the same library to the same answers: mi355rt_context_trace_rays on the same rays in a device buffer
(a segment has the layout of a ray), whose 48-byte records the caller would then compare with t_max and count.  Neither the generation of
the rays nor that reduction is charged to the baseline.
(a) mi355rt_context_occluded against mi355rt_context_trace_rays:
      teapot    2^20 incoherent segments (origins on a sphere around the scene's bounds, aimed at random points inside them, t_max = the
                distance to that point: "is the point visible from there?"), the rays of tools/query_bench.py (b);
      cornell   shadow-style segments from the first-hit point of every pixel of an 800 x 600 view that hits something to a point just below the light.
(b) mi355rt_context_ambient_occlusion at 800 x 600 x 16 samples, radius +inf, on cornell-box, teapot and semesterbild -- both forms of
    dealing (pixel, sample) pairs to lanes (diagnostic knob "ao_form": 0 = a pixel's samples across the lanes of a wave, 1 = a pixel per lane)
    -- against trace_rays over the same sample rays (made here with the definition of mi355rt.h: the generator's words by oracle/rng_np.py, the rest in torch; only the rays
    of pixels that hit something, which are the rays the pass traces).  The pass's floats are compared with the reduction of the baseline's records.
Every figure: ms per launch by device events around the launch, launches back to back in batches, batches alternating between the
contenders, until each has at least --seconds of timed kernel work after a warm-up batch; medians.  The file records build.kernel_hash()
and the registers of the kernels (tools/isa_stats.py).  Without a GPU the tool fails; it measures nothing on the CPU."""
import argparse
import ctypes as C
import os
import statistics

import numpy as np
import torch  # noqa: F401  -- before the HIP library (tests/conftest.py: one HIP runtime in the process)

import stage_bench
from oracle.rng_np import pcg4d
from stage_bench import ROOT

SCENES = [("cornell-box", "data/scenes/tungsten/cornell-box/scene.json", False), ("teapot", "data/scenes/tungsten/teapot/scene.json", True),
          ("semesterbild", "data/scenes/semesterbild.json", False)]
W, H, SAMPLES = 800, 600, 16
BATCH = 10


def alternate(contenders, seconds):
    """contenders: {name: launch()} -> {name: [ms per launch]}; batches of BATCH launches alternate until every contender has `seconds` of timed work."""
    stream = torch.cuda.current_stream()
    batch = lambda launch: stage_bench.timed_launches(stream, launch, BATCH)
    for launch in contenders.values():
        batch(launch)                                                    # warm-up: code objects, row tables
    ms = {k: [] for k in contenders}
    while any(sum(v) < seconds * 1e3 for v in ms.values()):
        for k, launch in contenders.items():
            ms[k] += batch(launch)
    return ms


def ao_rays(hits_f, hit_pixels, seed):
    """The sample rays of mi355rt.h's definition for the pixels `hit_pixels` (indices into the 800 x 600 image): float32 [n, SAMPLES, 8] on the device."""
    px = hit_pixels.cpu().numpy()
    x, y = (px % W).astype(np.uint32)[:, None], (px // W).astype(np.uint32)[:, None]
    s = np.arange(SAMPLES, dtype=np.uint32)[None, :]
    v = torch.zeros((len(hit_pixels), SAMPLES, 3), dtype=torch.float32, device="cuda")
    found = torch.zeros((len(hit_pixels), SAMPLES), dtype=torch.bool, device="cuda")
    for j in range(16):
        words = pcg4d(x, y, s * np.uint32(16) + np.uint32(j), np.uint32(seed))[:3]                 # on the host; the float mapping on the device
        c = torch.stack([torch.from_numpy((w >> np.uint32(8)).astype(np.float32)).cuda() * (2.0 ** -24) * 2.0 - 1.0 for w in words], dim=-1)
        l2 = (c[..., 0] * c[..., 0] + c[..., 1] * c[..., 1]) + c[..., 2] * c[..., 2]
        take = (l2 < 1.0) & ~found
        v[take] = c[take]
        found |= take
    rays = torch.zeros((len(hit_pixels), SAMPLES, 8), dtype=torch.float32, device="cuda")
    rays[..., 0:3] = hits_f[hit_pixels, 0:3][:, None, :]
    rays[..., 4:7] = hits_f[hit_pixels, 4:7][:, None, :] + v
    rays[..., 7] = float("inf")
    return rays


def load(host, name, path, skip):
    return host.LoadedScene(os.path.join(ROOT, path), W, H, 1, 1, skip_unknown_primitives=skip)


def first_hits(ctx):
    hits = torch.zeros(W * H * 12, dtype=torch.int32, device="cuda")
    ctx.first_hits(hits.data_ptr(), None, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return hits


def occluded_case(abi, ctx, what, seg, seconds):
    """seg: float32 [n, 8] on the device.  occluded against trace_rays on the same buffer; the words are checked against the records."""
    n = len(seg)
    s = torch.cuda.current_stream().cuda_stream
    words = torch.zeros(n, dtype=torch.int32, device="cuda")
    recs = torch.zeros(n * 12, dtype=torch.int32, device="cuda")
    ms = alternate({"occluded": lambda: ctx.occluded(seg.data_ptr(), n, words.data_ptr(), s),
                    "trace_rays": lambda: ctx.trace_rays(seg.data_ptr(), n, recs.data_ptr(), s)}, seconds)
    ctx.check()
    r, rf = recs.view(n, 12), recs.view(torch.float32).view(n, 12)
    want = (r[:, 8] != -1) & (rf[:, 3] < seg[:, 7])
    same = bool(torch.equal(want.to(torch.int32), words))
    o, t = statistics.median(ms["occluded"]), statistics.median(ms["trace_rays"])
    return {"what": what, "n": n, "ones": int(words.sum()), "occluded_ms": o, "occluded_launches": len(ms["occluded"]), "trace_ms": t,
            "trace_launches": len(ms["trace_rays"]), "ratio": t / o, "same": same}


def incoherent_segments(sc):
    c = sc.c if hasattr(sc, "c") else sc
    tri = np.ctypeslib.as_array(C.cast(c.triangles, C.POINTER(C.c_float)), shape=(c.n_triangles, 12))[:, :9].reshape(-1, 3)    # teapot's meshes are untransformed
    lo, hi = tri.min(axis=0).astype(np.float64), tri.max(axis=0).astype(np.float64)
    centre, radius = (lo + hi) / 2, float(np.linalg.norm(hi - lo))
    n = 1 << 20
    rng = np.random.default_rng(20)
    p = rng.normal(size=(n, 3)); p = centre + radius * p / np.linalg.norm(p, axis=1, keepdims=True)
    d = rng.uniform(lo, hi, (n, 3)) - p
    seg = np.zeros((n, 8), np.float32); seg[:, 0:3], seg[:, 4:7] = p, d
    seg[:, 7] = np.linalg.norm(seg[:, 4:7].astype(np.float64), axis=1)          # up to the point aimed at
    return torch.from_numpy(seg).cuda()


def shadow_segments(hits):
    h = hits.view(W * H, 12)
    hf = h.view(torch.float32)
    lit = (h[:, 8] != -1).nonzero().flatten()
    light = torch.tensor([0.0, 1.97, 0.0], device="cuda")                       # just below cornell-box's light quad
    seg = torch.zeros((len(lit), 8), dtype=torch.float32, device="cuda")
    seg[:, 0:3] = hf[lit, 0:3]
    seg[:, 4:7] = light[None, :] - hf[lit, 0:3]
    seg[:, 7] = torch.linalg.norm(seg[:, 4:7], dim=1) - 1e-3
    return seg


def ao_case(abi, device, sc, name, seconds):
    s = torch.cuda.current_stream().cuda_stream
    ctxs = {}
    try:
        for form in (0, 1):
            ctxs[form] = device.Context(0)
            ctxs[form].set_knob("ao_form", form)
            ctxs[form].set_scene(sc, sc.camera, sc.settings)
        hits = first_hits(ctxs[0])
        h = hits.view(W * H, 12)
        hit_pixels = (h[:, 8] != -1).nonzero().flatten()
        rays = ao_rays(h.view(torch.float32), hit_pixels, 0).view(-1, 8)
        n_rays = len(rays)
        recs = torch.zeros(n_rays * 12, dtype=torch.int32, device="cuda")
        out = {form: torch.zeros(W * H, dtype=torch.float32, device="cuda") for form in (0, 1)}
        prm = abi.AoParams.make(SAMPLES, 0, float("inf"))
        ms = alternate({"spread": lambda: ctxs[0].ambient_occlusion(hits.data_ptr(), out[0].data_ptr(), prm, None, s),
                        "lane": lambda: ctxs[1].ambient_occlusion(hits.data_ptr(), out[1].data_ptr(), prm, None, s),
                        "trace_rays": lambda: ctxs[0].trace_rays(rays.data_ptr(), n_rays, recs.data_ptr(), s)}, seconds)
        ctxs[0].check(); ctxs[1].check()
        r, rf = recs.view(len(hit_pixels), SAMPLES, 12), recs.view(torch.float32).view(len(hit_pixels), SAMPLES, 12)
        count = ((r[..., 8] != -1) & (rf[..., 3] < float("inf"))).sum(dim=1)
        want = torch.ones(W * H, dtype=torch.float32, device="cuda")
        want[hit_pixels] = 1.0 - count.to(torch.float32) / float(SAMPLES)
        same = bool(torch.equal(want.view(torch.int32), out[0].view(torch.int32)) and torch.equal(out[0].view(torch.int32), out[1].view(torch.int32)))
        med = {k: statistics.median(v) for k, v in ms.items()}
        return {"scene": name, "hit_pixels": len(hit_pixels), "rays": n_rays, "mean": float(out[0].mean()), "spread_ms": med["spread"], "lane_ms": med["lane"],
                "trace_ms": med["trace_rays"], "launches": {k: len(v) for k, v in ms.items()}, "same": same}
    finally:
        for c in ctxs.values():
            c.close()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "occlusion.txt"))
    ap.add_argument("--seconds", type=float, default=0.5, help="timed kernel work per figure, at least")
    args = ap.parse_args(argv)
    stage_bench.require_gpu("occlusion_bench")
    abi, build, host, device = stage_bench.packages("abi", "build", "host", "device")
    lines = [stage_bench.header("occlusion_bench", f"--seconds {args.seconds:g}"), "# occlusion kernels of the measured library and the baseline's (tools/isa_stats.py):"]
    lines += stage_bench.kernel_table(build.DEVICE_SO, lambda k: k.startswith(("k_occluded", "k_ao_", "k_query_rays")), 22)[0]
    scenes = {name: load(host, name, path, skip) for name, path, skip in SCENES}
    lines += ["", "## (a) mi355rt_context_occluded against mi355rt_context_trace_rays on the same buffer: median ms per launch, device events, alternating batches of %d" % BATCH,
              f"{'segments':44s} {'n':>8s} {'occluded':>8s} {'occluded ms':>11s} {'launches':>8s} {'Msegments/s':>11s} {'trace_rays ms':>13s} {'launches':>8s} {'trace_rays / occluded':>21s} {'same answers':>12s}"]
    for what, name in (("teapot, 2^20 incoherent, t_max = the target", "teapot"), ("cornell-box, first hits to the light", "cornell-box")):
        ctx = device.Context(0)
        try:
            ctx.set_scene(scenes[name], scenes[name].camera, scenes[name].settings)
            seg = incoherent_segments(scenes[name]) if name == "teapot" else shadow_segments(first_hits(ctx))
            r = occluded_case(abi, ctx, what, seg, args.seconds)
        finally:
            ctx.close()
        lines.append(f"{r['what']:44s} {r['n']:8d} {r['ones']:8d} {r['occluded_ms']:11.4f} {r['occluded_launches']:8d} {r['n'] / r['occluded_ms'] / 1e3:11.1f} "
                     f"{r['trace_ms']:13.4f} {r['trace_launches']:8d} {r['ratio']:21.2f} {str(r['same']):>12s}")
        print(lines[-1], flush=True)
    lines += ["", f"## (b) mi355rt_context_ambient_occlusion, {W} x {H} x {SAMPLES} samples, radius +inf, seed 0: the two forms (knob ao_form) against trace_rays over the same sample rays",
              "##     (the rays of the pixels that hit something: the rays the pass traces; generation and reduction are not charged to trace_rays)",
              f"{'scene':14s} {'hit pixels':>10s} {'rays':>9s} {'mean AO':>8s} {'spread ms':>10s} {'Mrays/s':>8s} {'pixel-per-lane ms':>17s} {'trace_rays ms':>13s} {'trace_rays / spread':>19s} {'lane / spread':>13s} {'launches':>14s} {'same floats':>11s}"]
    for name, _, _ in SCENES:
        r = ao_case(abi, device, scenes[name], name, args.seconds)
        L = r["launches"]
        lines.append(f"{r['scene']:14s} {r['hit_pixels']:10d} {r['rays']:9d} {r['mean']:8.4f} {r['spread_ms']:10.4f} {r['rays'] / r['spread_ms'] / 1e3:8.1f} {r['lane_ms']:17.4f} "
                     f"{r['trace_ms']:13.4f} {r['trace_ms'] / r['spread_ms']:19.2f} {r['lane_ms'] / r['spread_ms']:13.2f} {L['spread']:4d}/{L['lane']:4d}/{L['trace_rays']:4d} {str(r['same']):>11s}")
        print(lines[-1], flush=True)
    stage_bench.write_report(lines, args.out, echo=False)


if __name__ == "__main__":
    main()
