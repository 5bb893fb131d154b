#!/usr/bin/env python3
"""Scans sigma_luminance of the variance-guided filter (include/mi355rt_svgf.h) on the CPU and writes profiles/svgf_quality.txt.

  python tools/svgf_quality.py [--out profiles/svgf_quality.txt]

The chain is tests/test_svgf_cpu.py's quality case: cornell at 64 x 48, 8 frames of 1 spp along the 0.5-degree orbit from the oracle, truth = the
oracle's 256 spp of each frame's camera; tests/svgf_ref.py's accumulate -> filter at sigma_luminance 1, 2, 4 and 8 beside the existing route
tests/reproject_ref.py -> tests/denoise_ref.py at its defaults, on the same frames.  No GPU is involved: both routes are the numpy restatements.

The recipe DEPENDS ON TEST MODULES: it imports tests/conftest.py (outside pytest: for the package's modules) and tests/svgf_cases.py, which takes the
setting's constants and the oracle's first-hit records from tests/test_reproject_cpu.py -- so that the file and the test's assertion come from one
chain.  Those shared pieces would sit better in tests/reproject_cases.py; they stay where the earlier change put them."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tests"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

SIGMAS = (1.0, 2.0, 4.0, 8.0)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "svgf_quality.txt"))
    args = ap.parse_args(argv)
    import conftest
    import oracle
    import svgf_cases as SC
    oracle.build()
    build = conftest.pkg("build")
    build.build_host()
    rows = SC.quality_chain(SC.orbit_frames(oracle, conftest.pkg("abi"), conftest.pkg("host")), SIGMAS)
    last = rows[-1]
    best = min(SIGMAS, key=lambda s: last[3][s])
    lines = ["# python tools/svgf_quality.py   (numpy restatements only: tests/svgf_ref.py, tests/reproject_ref.py, tests/denoise_ref.py)",
             "## RMSE (linear RGB) against the oracle's 256 spp of the same camera; cornell 64 x 48, 1 spp a frame, 0.5 degrees a frame, seed = frame number",
             "## existing route: reproject -> denoise at its defaults; new route: svgf accumulate -> filter (5 levels) at each sigma_luminance",
             f"{'frame':>5s} {'raw':>9s} {'reprojected':>11s} {'existing route':>14s} " + " ".join(f"{'svgf s=' + format(s, 'g'):>10s}" for s in SIGMAS)]
    for k, (raw, rep, old, new) in enumerate(rows):
        lines.append(f"{k:5d} {raw:9.5f} {rep:11.5f} {old:14.5f} " + " ".join(f"{new[s]:10.5f}" for s in SIGMAS))
    lines.append(f"## lowest last-frame RMSE of the new route: sigma_luminance = {best:g} ({last[3][best]:.5f}); existing route {last[2]:.5f}, reprojected {last[1]:.5f}")
    print("\n".join(lines))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
