#!/usr/bin/env python3
"""profiles/scatter_wave_probe.txt: what tests/test_gpu_scatter_wave.py runs, in figures -- per form of the bounce the waves and records
run through the reference build's probe on the GPU, the owner-count and first-accepted-try histograms of the waves, and how many records
differ from the oracle.

usage: python tools/scatter_wave_report.py [out.txt]      (needs an MI355X; default: stdout)"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def hist(values):
    v, c = np.unique(values, return_counts=True)
    return " ".join(f"{int(a)}:{int(b)}" for a, b in zip(v, c))


def main():
    import oracle
    import scatter_wave_cases as W
    import test_gpu_scatter_wave as T
    abi = importlib.import_module("raytracer-rust_amd.abi")
    device = importlib.import_module("raytracer-rust_amd.device")
    oracle.build()
    mats_c = W.materials_ctypes(abi)
    lines = ["# python tools/scatter_wave_report.py: the wave probe of the bounce (csrc/refs/rt_scatter_wave_probe.h) against the oracle, on the GPU.",
             "# owners: lanes of a wave that still need a try behind the tries of their own lane; first accept: the try a live lane's point came from.",
             "# pools (2^22 addresses per setting): " + "; ".join(
                 f"key {st['k0']:#x}/{st['k1']:#x} ray {st['ray']}: >=8 {st['ge8']['x'].size}, >=12 {st['ge12']['x'].size}, >=16 {st['ge16']['x'].size}, max {st['max_first']}"
                 for st in W.pools())]
    total = differ = 0
    edge, cls, names = W.edge_records()
    edge_want, edge_tries, _ = T.reference_of("edge", oracle, mats_c, edge)
    for form_no, form, kernels in T.distinct_forms(device):
        lines.append("")
        lines.append(f"form {form_no}: {' / '.join(kernels)}   " + " ".join(f"{k}={form[k]:#x}" if k == "mats" else f"{k}={int(form[k])}" for k in
                                                                            ("mats", "wide", "fastn", "try1", "terminal_done", "stepped", "in_place")))
        recs, wnames, want, tries, got, bad = T.run_lambert_waves(device, oracle, mats_c, form_no, form, kernels)
        live = (recs[:, 1] & W.LIVE) != 0
        owners = W.owners_of(tries, form["try1"]).reshape(-1, 64).sum(1)
        lines.append(f"  lambert waves: {len(wnames)} waves, {recs.shape[0]} lane records ({int(live.sum())} live), differing {int(bad.sum())}")
        lines.append(f"    waves by owner count: {hist(owners)}")
        lines.append(f"    live lanes by first accept: {hist(tries[live] - 1)}")
        total += recs.shape[0]; differ += int(bad.sum())
        kinds = tuple(k for k in range(10) if (form["mats"] >> k) & 1)
        if W.CHECKER in kinds:
            recs, wnames = W.mixed_waves(kinds)
            want, tries, _ = T.reference_of(("mixed", kinds), oracle, mats_c, recs)
            bad = W.differing(device.debug_scatter_wave(form_no, mats_c, recs), want)
            used = tries > 0
            lines.append(f"  mixed-material waves: {len(wnames)} waves, {recs.shape[0]} lane records, {int(used.sum())} with a ball, "
                         f"{int((((recs[:, 1] & W.LIVE) != 0) & ~used).sum())} live without, differing {int(bad.sum())}")
            lines.append(f"    ball lanes by first accept: {hist(tries[used] - 1)}")
            total += recs.shape[0]; differ += int(bad.sum())
        ok = W.for_form(form, edge)
        bad = W.differing(device.debug_scatter_wave(form_no, mats_c, edge[ok]), edge_want[ok])
        lines.append(f"  edge records: {int(ok.sum())}, differing {int(bad.sum())}   by class: " +
                     ", ".join(f"{names[c]} {int((cls[ok] == c).sum())}" for c in np.unique(cls[ok])))
        total += int(ok.sum()); differ += int(bad.sum())
    bad = W.differing(T.products_hook(device, mats_c, edge), edge_want, 13)
    lines += ["", f"product hook (k_debug_scatter, sequential rejection): {edge.shape[0]} edge records, differing {int(bad.sum())}",
              f"  ball records by first accept: {hist(edge_tries[edge_tries > 0] - 1)}"]
    total += edge.shape[0]; differ += int(bad.sum())
    lines += ["", f"total: {total} lane records, {differ} differing"]
    text = "\n".join(lines) + "\n"
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text)
    sys.stdout.write(text)
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
