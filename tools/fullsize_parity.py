"""Parity at the BASELINE sizes: HIP path vs oracle, counter-mode RNG, the oracle on tests/parity.py's oracle_threads().
Every pixel of cornell, teapot, veach-mis (1024 spp) and semesterbild 800x600; config 5 (semesterbild 1920x1080x4096, 4 bands) on
the rows tests/test_gpu_fullsize.py compares; and the ray counts of the rough-conductor fuzz scenes of tests/test_fuzz_parity.py.
Run on a GPU box; the output is profiles/fullsize_parity.txt.

usage: python tools/fullsize_parity.py [--out FILE] [--head GIT_HEAD]"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  -- before the HIP library (tests/conftest.py)
from conftest import SCENES, pkg  # noqa: E402
from fuzz_scenes import random_scene  # noqa: E402
from parity import allowed, assert_parity, oracle_threads  # noqa: E402
from test_gpu_fullsize import _band_plan, _config5_rows, _oracle_rows, _windows  # noqa: E402
import oracle  # noqa: E402

CASES = [("cornell", 800, 600, 256, 30, True), ("teapot", 800, 600, 256, 64, True), ("veach", 1280, 720, 1024, 16, False),
         ("semesterbild", 800, 600, 256, 30, False), ("semesterbild", 1920, 1080, 4096, 30, False)]


def verdict(gp, gl, op, ol, exact, rows, gpu_rays, ora_rays):
    try:
        assert_parity(gp, gl, op, ol, exact=exact, rows=rows, gpu_rays=gpu_rays, oracle_rays=ora_rays, ray_rel=0.0 if exact else 1e-6)
        return "pass"
    except AssertionError as e:
        return "FAIL: " + str(e).replace("\n", " | ")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--head", default=None, help="git head of the tree (the GPU box receives a snapshot without .git)")
    a = ap.parse_args()
    abi, host, device, build = pkg("abi"), pkg("host"), pkg("device"), pkg("build")
    oracle.build()
    head = a.head
    if head is None:
        try:
            head = subprocess.check_output(["git", "rev-parse", "--short=12", "HEAD"], cwd=ROOT, text=True).strip()
        except (OSError, subprocess.CalledProcessError):
            head = "unknown"
    lines = [f"# kernel_hash {build.kernel_hash()}  git head {head}  oracle threads {oracle_threads()}",
             "# contract (tests/parity.py): exact = bit-identical + equal rays; tolerant = L2 > 1e-3 on <= ceil(1e-4 N) px, "
             "8-bit differences <= ceil(1e-3 N) px, means within 2e-3, |d rays| <= 1e-6 rays"]

    def out(s):
        print(s, flush=True)
        lines.append(s)

    for line in lines:
        print(line, flush=True)
    for name, W, H, spp, depth, exact in CASES:
        sc = host.LoadedScene(SCENES[name], W, H, spp, depth, skip_unknown_primitives=(name == "teapot"))
        gp, gl, st = device.render(sc, sc.camera, sc.settings, abi.Options.make())
        rows = None
        t = time.time()
        if H == 1080:
            rows = _config5_rows()
            op, ol, ora_rays = _oracle_rows(oracle, abi, sc, rows)
            dt = time.time() - t
            gpu_rays = sum(int(device.render(sc, sc.camera, sc.settings, abi.Options.make(row_begin=b, row_end=e), want_linear=False)[2].rays)
                           for b, e in _windows(rows))
            gp, gl = gp[rows], gl[rows]
        else:
            op, ol, cnt = oracle.render(sc, sc.camera, sc.settings, abi.Options.make(), threads=oracle_threads())
            ora_rays, gpu_rays = int(cnt.rays), int(st.rays)
            dt = time.time() - t
        n = gp.size
        same_f32 = (gl.view(np.uint32) == ol.view(np.uint32)).all(-1)
        l2 = np.sqrt(((gl.astype(np.float64) - ol) ** 2).sum(-1))
        far, byte = int((~(l2 <= 1e-3)).sum()), int((gp != op).sum())
        what = f"{len(rows)} rows {rows}" if rows else "every pixel"
        if rows:
            what += f"; band-boundary rows {_band_plan(W, H, spp)[1]}, shard-boundary rows {_band_plan(W, H, spp)[2]}, bands {st.bands}"
        out(f"{name} {W}x{H}x{spp} d{depth} ({what}; {'exact' if exact else 'tolerant'}):\n"
            f"  bit-identical (f32 linear) {same_f32.mean() * 100:.4f} %  8-bit identical {(gp == op).mean() * 100:.4f} %  "
            f"L2 > 1e-3: {far} px (allowed {allowed(n)[0]})  8-bit differing: {byte} px (allowed {allowed(n)[1]})  max L2 {l2.max():.3e}\n"
            f"  rays gpu {gpu_rays} oracle {ora_rays} (|d| {abs(gpu_rays - ora_rays)}, {abs(gpu_rays - ora_rays) / ora_rays:.2e})  "
            f"oracle {dt:.1f} s  gpu kernel {st.render_kernel_ms:.1f} ms  contract: {verdict(gp, gl, op, ol, exact, rows, gpu_rays, ora_rays)}")
    out("fuzz scenes with rough conductors (tests/test_fuzz_parity.py, 64x48x6 d8, counter mode):")
    for seed in (11, 12, 13):
        sc = random_scene(abi, host, seed, exact_only=False)
        st_ = abi.Settings(64, 48, 6, 8)
        gp, gl, gs = device.render(sc, sc.camera, st_, abi.Options.make())
        op, ol, cnt = oracle.render(sc, sc.camera, st_, abi.Options.make())
        l2 = np.sqrt(((gl.astype(np.float64) - ol) ** 2).sum(-1))
        out(f"  seed {seed}: rays gpu {gs.rays} oracle {cnt.rays} (|d| {abs(int(gs.rays) - int(cnt.rays))})  "
            f"bit-identical {(gl.view(np.uint32) == ol.view(np.uint32)).all(-1).mean() * 100:.2f} %  L2 > 1e-3: {int((~(l2 <= 1e-3)).sum())} px  "
            f"8-bit differing: {int((gp != op).sum())} px  max L2 {l2.max():.3e}")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
