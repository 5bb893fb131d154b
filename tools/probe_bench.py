#!/usr/bin/env python3
"""Times the surface probes (mi355rt_context_probe_radiance) on the GPU and writes profiles/probe_bench.txt.

  python tools/probe_bench.py [--out profiles/probe_bench.txt] [--seconds 1.0]

Cornell-box: a probe at the first hit of every pixel-centre ray of the 800 x 600 view (mi355rt_context_first_hits -> abi.probes_from_hits, misses
dropped), 16 samples per call at max_depth 30, K = 8 (the default).  Timed loops, each a batch of calls enqueued back to back between a pair of
device events, after a warm-up batch, INTERLEAVED: a round takes one batch of every line below, rounds repeat until every line has at least
--seconds of timed kernel work.  Per line: the median ms per call over the rounds and their spread ((max - min) / median).
  probe_radiance            the rays made in the refill of the path loop, one call [0, 16)
  query, rays of sample 0   mi355rt_context_trace_radiance, one call [0, 16) along the resident rays mi355rt_context_probe_rays wrote for sample 0: the
                            same origins, the same distribution of directions, as many paths and launches -- but sample s > 0 continues sample 0's ray, so these
                            are not the paths of the line above
  query, one ray per path   one call [0, 1) along ALL the resident rays probe_rays wrote for the samples 0 .. 15 (16 rays per probe, probe-major): as many
                            paths, every path with a first ray of its own as in the first line, the rays loaded -- other paths again (every ray draws from sample
                            0's stream), 16 times the ray reads, and a sum kernel over 16 n rows of one sample
  query, 16 x one sample    16 calls [s, s + 1) along the resident rays probe_rays wrote for each s: THE SAME PATHS as the first line (the sums are
                            compared word for word here), at 16 launches of each kernel instead of one
The host-made route to the same sums is timed on the host, once: per sample index, the rays in numpy (pcg4d per try, vectorised; checked word for
word against mi355rt_context_probe_rays), their upload, and one trace_radiance call [s, s + 1) -- wall time for 16 samples, against the wall time of
one probe_radiance call for the same 16.
The file records build.kernel_hash() and the registers, spills, code size and instruction counts of the k_probe* kernels beside k_radiance*.
Without a GPU the tool fails."""
import argparse
import os
import time

import numpy as np
import torch  # noqa: F401  -- before the HIP library (tests/conftest.py: one HIP runtime in the process)

import stage_bench
from oracle.rng_np import pcg4d
from stage_bench import ROOT

W, H, SAMPLES, DEPTH = 800, 600, 16, 30
BATCH = 8
TRIES = 64
F = np.float32
U = np.uint32


def normalized_rows(a):
    l = np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])
    inv = F(1.0) / np.where(l < F(1e-4), F(1.0), l)
    return np.where((l < F(1e-4))[:, None], a, a * inv[:, None]).astype(F)


def host_rays(abi, probes, s, seed=0):
    """The probe rays of sample s, as a host without the probes makes them (include/mi355rt.h's definition): abi.PATH_RAY_DTYPE [n], normalised once."""
    n = len(probes)
    ykey = probes["row"].astype(np.uint64) + np.uint64(seed)
    base = pcg4d(probes["x"].astype(U), np.full(n, s, U), (ykey & np.uint64(0xFFFFFFFF)).astype(U), (ykey >> np.uint64(32)).astype(U))
    p = np.zeros((n, 3), F)
    open_ = np.arange(n)
    for j in range(TRIES):
        if not len(open_):
            break
        with np.errstate(over="ignore"):
            w = pcg4d(base[0][open_], base[1][open_], base[2][open_], base[3][open_] + U(j))      # (ray 0, block j)
        q = np.stack([(a >> U(9)).astype(F) * F(2.0 ** -22) - F(1.0) for a in w[1:]], axis=1)
        ok = (q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2] < F(1.0)
        p[open_[ok]] = q[ok]
        open_ = open_[~ok]
    N = probes["normal"]
    d = N + normalized_rows(p)
    d = np.where((np.abs(d) < F(1e-8)).all(axis=1)[:, None], N, d)
    rays = np.zeros(n, abi.PATH_RAY_DTYPE)
    rays["origin"] = probes["position"] + N * F(1e-4)
    rays["direction"] = normalized_rows(d)
    rays["x"], rays["row"] = probes["x"], probes["row"]
    return rays


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "probe_bench.txt"))
    ap.add_argument("--seconds", type=float, default=1.0, help="timed kernel work per line, at least")
    args = ap.parse_args(argv)
    stage_bench.require_gpu("probe_bench")
    abi, build, host, device = stage_bench.packages("abi", "build", "host", "device")

    sc = host.LoadedScene(os.path.join(ROOT, "data/scenes/tungsten/cornell-box/scene.json"), W, H, SAMPLES, DEPTH)
    ctx = device.Context(0)
    try:
        ctx.set_scene(sc, sc.camera, sc.settings)
        d_hits = torch.zeros(W * H * 48, dtype=torch.uint8, device="cuda")
        ctx.first_hits(d_hits.data_ptr())
        torch.cuda.synchronize()
        probes = abi.probes_from_hits(d_hits.cpu().numpy().view(abi.HIT_DTYPE), W)       # the lightmap recipe of INTEGRATION.md
        n = len(probes)
        d_probes = torch.from_numpy(probes.view(np.uint8).reshape(-1).copy()).cuda()
        d_rays = torch.zeros(SAMPLES * n * 32, dtype=torch.uint8, device="cuda")          # the resident rays of every sample: probe_rays' own
        for si in range(SAMPLES):
            ctx.probe_rays(d_probes.data_ptr(), n, si, d_rays.data_ptr() + si * n * 32)
        torch.cuda.synchronize()
        d_rays_pm = d_rays.view(SAMPLES, n, 32).transpose(0, 1).contiguous()              # probe-major: ray i * 16 + s, the order of probe_radiance's items
        d_accum_pm = torch.zeros(SAMPLES * n * 4, dtype=torch.float32, device="cuda")
        d_linear_pm = torch.zeros(SAMPLES * n * 3, dtype=torch.float32, device="cuda")
        d_accum = torch.zeros(n * 4, dtype=torch.float32, device="cuda")
        d_linear = torch.zeros(n * 3, dtype=torch.float32, device="cuda")
        d_scratch = torch.zeros(device.radiance_scratch_bytes(n, SAMPLES), dtype=torch.uint8, device="cuda")
        stream = torch.cuda.current_stream()
        s = stream.cuda_stream
        prm = abi.RadianceParams.make(0, SAMPLES, DEPTH, 0)
        one = [abi.RadianceParams.make(si, si + 1, DEPTH, 0) for si in range(SAMPLES)]

        def per_sample():
            for si in range(SAMPLES):
                ctx.trace_radiance(one[si], d_rays.data_ptr() + si * n * 32, n, d_accum.data_ptr(), d_scratch.data_ptr(), d_linear.data_ptr(), s)

        P, Q0, Q1, Q16 = "probe_radiance", "query, rays of sample 0", "query, one ray per path", "query, 16 x one sample"
        calls = {P: lambda: ctx.probe_radiance(prm, d_probes.data_ptr(), n, d_accum.data_ptr(), d_scratch.data_ptr(), d_linear.data_ptr(), s),
                 Q0: lambda: ctx.trace_radiance(prm, d_rays.data_ptr(), n, d_accum.data_ptr(), d_scratch.data_ptr(), d_linear.data_ptr(), s),
                 Q1: lambda: ctx.trace_radiance(one[0], d_rays_pm.data_ptr(), SAMPLES * n, d_accum_pm.data_ptr(), d_scratch.data_ptr(), d_linear_pm.data_ptr(), s),
                 Q16: per_sample}
        order = [P, Q0, Q1, Q16]
        means, sums = {}, {}

        def warmed(name):                                                   # what each line computes
            means[name] = float((d_linear_pm if name == Q1 else d_linear).cpu().numpy().mean())
            sums[name] = d_accum.cpu().numpy().tobytes()
            if name == Q16:
                assert sums[P] == sums[Q16], "probe_radiance and the query along probe_rays' rays, sample by sample, differ"

        ms = stage_bench.interleaved_rounds(calls, args.seconds, BATCH, warmed=warmed)
        ctx.check()

        # the host-made route, wall time: rays in numpy, upload, one call per sample index
        d_one = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
        assert host_rays(abi, probes, 3).tobytes() == d_rays[3 * n * 32:4 * n * 32].cpu().numpy().tobytes(), "the host-made rays are not probe_rays'"
        make_s = upload_s = 0.0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for si in range(SAMPLES):
            t = time.perf_counter()
            rays = host_rays(abi, probes, si)
            make_s += time.perf_counter() - t
            t = time.perf_counter()
            d_one.copy_(torch.from_numpy(rays.view(np.uint8).reshape(-1)))
            torch.cuda.synchronize()
            upload_s += time.perf_counter() - t
            ctx.trace_radiance(one[si], d_one.data_ptr(), n, d_accum.data_ptr(), d_scratch.data_ptr(), d_linear.data_ptr(), s)
        torch.cuda.synchronize()
        host_route_s = time.perf_counter() - t0
        assert d_accum.cpu().numpy().tobytes() == sums[P], "the host-made route and probe_radiance differ"
        t0 = time.perf_counter()
        calls[P]()
        torch.cuda.synchronize()
        probe_wall_s = time.perf_counter() - t0
    finally:
        ctx.close()

    med, spread = stage_bench.summary(ms)
    table, stats = stage_bench.kernel_table(build.DEVICE_SO, lambda k: "k_probe" in k or "k_radiance" in k, 28)
    insts = {k: st.get("insts", 0) for k, st in stats.items()}
    lines = [stage_bench.header("probe_bench", f"--seconds {args.seconds:g}"), "# k_probe* and k_radiance* kernels of the measured library (tools/isa_stats.py):"] + table
    lines += [f"# static instructions: k_probe_paths {insts['k_probe_paths']} against k_radiance_paths {insts['k_radiance_paths']} (+{insts['k_probe_paths'] - insts['k_radiance_paths']}), "
              f"k_probe_paths_mesh {insts['k_probe_paths_mesh']} against k_radiance_paths_mesh {insts['k_radiance_paths_mesh']} (+{insts['k_probe_paths_mesh'] - insts['k_radiance_paths_mesh']})",
              "", f"## cornell-box, {n} probes at the first hits of the {W} x {H} centre rays ({W * H - n} misses dropped), samples [0, {SAMPLES}) per call, max_depth {DEPTH}: "
                  f"{n * SAMPLES} paths per call (paths kernel + sum kernel), K = 8 (the default)",
              f"##     ms = median over the rounds of (device events around {BATCH} calls back to back) / {BATCH}; spread = (max - min) / median of the rounds; rounds interleave every line",
              f"{'':>24s} {'ms per call':>11s} {'(min)':>8s} {'(max)':>8s} {'spread':>7s} {'rounds':>6s} {'Msamples/s':>10s} {'/ query 0':>9s} {'mean':>10s}"]
    for name in order:
        lines.append(f"{name:>24s} {med[name]:11.4f} {min(ms[name]):8.4f} {max(ms[name]):8.4f} {spread[name] * 100:6.2f}% {len(ms[name]):6d} "
                     f"{n * SAMPLES / (med[name] * 1e-3) / 1e6:10.1f} {med[name] / med[Q0]:9.3f} {means[name]:10.6f}")
    lines += ["", f"## rays made or loaded: probe_radiance {med[P]:.4f} ms against the query along the rays of sample 0 {med[Q0]:.4f} ms: "
                  f"{100 * (med[P] - med[Q0]) / med[Q0]:+.2f} % against a spread of {100 * max(spread[P], spread[Q0]):.2f} % (as many paths from the same origins, not the same paths)",
              f"## every path a loaded first ray of its own: {med[Q1]:.4f} ms: probe_radiance is {100 * (med[P] - med[Q1]) / med[Q1]:+.2f} % against it, spread "
              f"{100 * max(spread[P], spread[Q1]):.2f} % (as many paths, not the same paths; {SAMPLES} x the ray reads and a sum over {SAMPLES} x the rows)",
              f"## the same paths in {SAMPLES} calls of one sample each: {med[Q16]:.4f} ms ({med[Q16] / med[P]:.2f} x probe_radiance), the sums word for word probe_radiance's",
              "", f"## the host-made route to the same sums, wall time on the host for {SAMPLES} sample indices (one run; the same sums, word for word):",
              f"##     rays in numpy {make_s * 1e3:.1f} ms + upload of {SAMPLES} x {n * 32 / 1e6:.2f} MB {upload_s * 1e3:.1f} ms + {SAMPLES} calls = {host_route_s * 1e3:.1f} ms in all;",
              f"##     one probe_radiance call for the same {SAMPLES} samples, enqueue to synchronize: {probe_wall_s * 1e3:.3f} ms: {host_route_s / probe_wall_s:.0f} x"]
    stage_bench.write_report(lines, args.out)


if __name__ == "__main__":
    main()
