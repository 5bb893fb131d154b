"""The support modules the GPU tests and the stage benches share, without a GPU: tests/device_buffers.py on torch's cpu device and
tools/stage_bench.py's round loop and kernel table (the built library is cross-compiled; its table needs no GPU)."""
import functools
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT, pkg
from device_buffers import PATTERN, Guarded, packed_of

sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_stats  # noqa: E402
import stage_bench  # noqa: E402

_kernel_stats = functools.lru_cache(maxsize=None)(isa_stats.kernel_stats)     # the library is read once for the three table cases


def test_guarded_reads_its_payload_and_tells_a_damaged_guard():
    import torch
    data = np.arange(24, dtype=np.float32)
    g = Guarded(96, data, guard=32, device="cpu")
    assert g.read(np.float32, "a call").tobytes() == data.tobytes() and len(g.t) == 128 and g.ptr == g.t.data_ptr()
    assert not g.untouched()
    fresh = Guarded(96, device="cpu")
    assert fresh.untouched() and (fresh.read(np.uint8, "fresh") == PATTERN).all()
    fresh.t[5] = 0
    assert not fresh.untouched()                                              # one payload byte changed
    fresh.fill_nan_f32()
    assert np.isnan(fresh.read(np.float32, "sums")).all()
    fresh.upload(data)
    assert fresh.read(np.float32, "uploaded").tobytes() == data.tobytes()
    for at in (96, 96 + 63):                                                  # the first and the last byte of the guard
        g = Guarded(96, data, device="cpu")
        g.t[at] = 0
        with pytest.raises(AssertionError, match="the call that did it"):
            g.read(np.float32, "the call that did it")
    g = Guarded(96, data, device="cpu")
    g.t = torch.full((96 + 60,), PATTERN, dtype=torch.uint8)                 # a tail of the wrong length
    with pytest.raises(AssertionError, match="short tail"):
        g.read(np.float32, "short tail")
    with pytest.raises(AssertionError):
        Guarded(96, data[:23], device="cpu")


def test_packed_of_clamps_and_truncates():
    F = np.float32
    lin = np.array([[0.25, 0.25, 0.25], [np.nan, -1.0, 4.0], [1.0, 0.0, -0.0], [np.inf, -np.inf, 1e-30], [0.5, 0.9999, 2.0 ** -16]], F)
    got = packed_of(lin)
    assert got.dtype == np.uint32
    assert got.tolist() == [0x7F7F7F, 0x0000FF, 0xFF0000, 0xFF0000, (int(F(np.sqrt(F(0.5))) * F(255)) << 16) | (254 << 8) | 0]
    assert packed_of(lin.reshape(5, 1, 3)).shape == (5, 1)


def test_interleaved_rounds_warms_every_line_then_rounds_until_each_has_its_seconds():
    ms_of = {"a": 30.0, "b": 10.0, "c": 20.0}                               # ms per call; a batch of 4 calls is 120, 40 and 80 ms of timed work
    log = []

    def timed(line):
        log.append(line)
        return ms_of[line]

    ms = stage_bench.interleaved_rounds({k: k for k in ms_of}, 0.1, 4, timed, after_round=lambda: log.append("round"), warmed=lambda line: log.append("warmed " + line))
    # b needs 3 rounds to reach 100 ms (40, 80, 120); the loop stops at the first round after which every line has reached it
    assert log == ["a", "warmed a", "b", "warmed b", "c", "warmed c"] + ["a", "b", "c", "round"] * 3
    assert ms == {"a": [30.0] * 3, "b": [10.0] * 3, "c": [20.0] * 3}
    med, spread = stage_bench.summary({"a": [1.0, 2.0, 4.0], "b": [3.0]})
    assert med == {"a": 2.0, "b": 3.0} and spread == {"a": 1.5, "b": 0.0}


def _table_of(report):
    """The table's header line and its rows in a committed report."""
    lines = open(os.path.join(ROOT, "profiles", report)).read().splitlines()
    at = next(i for i, ln in enumerate(lines) if ln.startswith("# kernel "))
    rows = [ln for ln in lines[at + 1:at + 40] if re.match(r"# k_\w+ +\d", ln)]
    return lines[at], rows


@pytest.mark.parametrize("report,kernels,width,insts", [("radiance_bench.txt", ("k_radiance",), 22, True), ("probe_bench.txt", ("k_probe", "k_radiance"), 28, True),
                                                        ("denoise.txt", ("k_denoise",), 24, False)])
def test_kernel_table_has_the_committed_reports_layout(report, kernels, width, insts, monkeypatch):
    """The tool's own selection and width: the header line is the committed report's, character for character, and every row has its rows' fields."""
    monkeypatch.setattr(isa_stats, "kernel_stats", _kernel_stats)
    lines, stats = stage_bench.kernel_table(pkg("build").build_device(), lambda k: any(sub in k for sub in kernels), width, insts)
    want_header, want_rows = _table_of(report)
    assert lines[0] == want_header
    assert len(lines) == 1 + len(stats) >= 4 and all(any(sub in k for sub in kernels) for k in stats) and (" insts " in lines[0]) == insts
    widths = lambda row: [len(f) for f in re.findall(r" +\S+", row[2 + width:])]
    for row in lines[1:]:
        assert row.startswith("# k_") and len(row) == len(want_header) and widths(row) == widths(want_rows[0]), row
        assert row[:2 + width].rstrip()[2:] in stats
    assert all(len(r) == len(want_header) and widths(r) == widths(want_rows[0]) for r in want_rows)
