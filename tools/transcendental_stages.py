#!/usr/bin/env python3
"""Runs the sweeps of tests/test_gpu_transcendental_stages.py on the GPU and writes what they counted: per stage and domain, the elements,
the device / oracle differences per output word, the device's and glibc's largest distance from the float64 value (f32 steps), and the
differences no transcendental accounts for.  A failing assertion is reported, not raised, so the counts of a failing build are kept too.

usage: python tools/transcendental_stages.py [--out profiles/transcendental_stages.txt]"""
import argparse
import inspect
import os
import sys
import time
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402,F401  -- before the HIP library, as tests/conftest.py does

import test_gpu_transcendental_stages as T  # noqa: E402

WORD_NAMES = {"lattice": ("ln", "theta_arg", "theta", "sin_t", "cos_t", "sin_p", "cos_p", "phi"),
              "half": ("l.x", "l.y", "l.z", "at.r", "at.g", "at.b", "ok", "sig"), "acos": ("acos",), "atan2": ("atan2",),
              "tex": ("r", "g", "b", "acos", "atan2", "fmod"), "sky": ("r", "g", "b", "acos", "atan2"), "fmod": ("mismatch",), "atan2x": ("mismatch",)}


def _calls():
    for name, fn in inspect.getmembers(T, inspect.isfunction):
        if not name.startswith("test_"):
            continue
        marks = {m.name: m for m in getattr(fn, "pytestmark", [])}
        if "parametrize" in marks:
            argnames, values = marks["parametrize"].args[:2]
            argnames = [a.strip() for a in argnames.split(",")] if isinstance(argnames, str) else list(argnames)
            for v in values:
                v = v if isinstance(v, tuple) and len(argnames) > 1 else (v,)
                yield f"{name}{list(v)}", fn, dict(zip(argnames, v))
        else:
            yield name, fn, {}


def _merged(rows):
    """TEX and SKY: one line per kind of input (pseudo-random / special) summed over the image sizes and offsets; the rest as recorded."""
    import numpy as np
    out, groups = [], {}
    for stage, domain, form, n, res in rows:
        if stage not in ("tex", "sky"):
            out.append((stage, domain, form, n, res))
            continue
        key = (stage, form, domain.endswith("special"))
        if key not in groups:
            groups[key] = [stage, 0, 0, form, np.zeros(64)]
            out.append(key)
        g = groups[key]
        g[1] += 1; g[2] += n
        for w in range(8):
            g[4][4 * w] += res[4 * w]; g[4][4 * w + 1] = max(g[4][4 * w + 1], res[4 * w + 1]); g[4][4 * w + 2] = max(g[4][4 * w + 2], res[4 * w + 2])
        g[4][32] += res[32]; g[4][34] += res[34]
    merged = []
    for r in out:
        if len(r) == 3:                                                   # a (stage, form, special) key
            stage, images, n, form, res = groups[r]
            merged.append((stage, f"{'special inputs' if r[2] else 'pseudo-random directions'}, {images} images x offsets", form, n, res))
        else:
            merged.append(r)
    return merged


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transcendental_stages.txt"))
    args = ap.parse_args()
    lines, outcomes = [], []
    t_all = time.time()
    for name, fn, kw in _calls():
        t0 = time.time()
        try:
            fn(**kw)
            outcomes.append(f"# pass  {time.time() - t0:6.1f} s  {name}")
        except AssertionError as e:
            outcomes.append(f"# FAIL  {time.time() - t0:6.1f} s  {name}: {str(e)[:300]}")
        except Exception:
            outcomes.append(f"# ERROR {time.time() - t0:6.1f} s  {name}: {traceback.format_exc(limit=2)[-300:]}")
        print(outcomes[-1], flush=True)
    lines.append(f"# tests/test_gpu_transcendental_stages.py sweeps, {time.time() - t_all:.0f} s in all; form: CTR = counter mode, REF = reference-stream mode")
    lines.append("# per word: differences device vs oracle / device's max f32 steps from float64 / glibc's (oracle's) max; 'unattr' = elements whose final")
    lines.append("# words differ while every transcendental word agrees (must be 0); 'final' = elements whose final words differ")
    lines += outcomes
    for stage, domain, form, n, res in _merged(T.record()):
        names = WORD_NAMES[stage]
        words = "  ".join(f"{nm} {int(res[4 * w])}/{int(res[4 * w + 1])}/{int(res[4 * w + 2])}" for w, nm in enumerate(names))
        tail = "" if stage in ("acos", "atan2", "fmod", "atan2x") else f"  final {int(res[34])} unattr {int(res[32])}"
        lines.append(f"{stage:7s} {'REF' if form else 'CTR'}  n={n:<11d} {domain:52s} {words}{tail}")
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {args.out}: {len(lines)} lines")


if __name__ == "__main__":
    main()
