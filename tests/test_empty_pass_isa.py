"""The two switches of "nothing for pixels that see nothing" (rt_kernels.hip: MI355RT_QC_EMPTY_PASS, the fourth bit of k_render_ctr_simple_qc's FORM,
and MI355RT_RESOLVE_SKIP in k_resolve), read from built gfx950 code objects (no GPU needed).

With both at 0 (build.build_empty_pass_off) the library is the one before the change: k_render_ctr_simple_qc holds exactly the 100 v_mov_b32 of the
listing tests/test_state_in_place_isa.py caps, spills 8 scalar registers through 10 v_readlane and 8 v_writelane (tests/test_nosky_budget.py), and
k_resolve is inside its budget.  The instruction-for-instruction comparison with the parent's library is profiles/isa_diff_empty_pass_vs_parent.txt.
The shipped library -- both at 1 -- must keep the same figures in the render kernel: the shortcut guards the pass's camera() call and its walk by one
wave-uniform flag and adds no edge to the loop, so the allocation of the loop does not move (profiles/isa_diff_empty_pass_vs_parent.txt lists the
forms that did move it)."""
import importlib
import os
import sys

import test_nosky_budget as nosky
import test_state_in_place_isa as in_place

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

RESOLVE_VGPRS, RESOLVE_CODE_BYTES = 16, 2048          # k_resolve's budget: enough waves in flight to keep the read stream busy


def _figures(so):
    isa_stats = importlib.import_module("isa_stats")
    stats = {isa_stats.short(k): v for k, v in isa_stats.kernel_stats(so).items()}
    ops = {isa_stats.short(k): [line.split()[0] for line in v] for k, v in isa_stats.kernel_isa(so).items()}
    return stats, ops


def _render_kernel(stats, ops):
    st, op = stats["k_render_ctr_simple_qc"], ops["k_render_ctr_simple_qc"]
    count = lambda prefix: sum(o.startswith(prefix) for o in op)
    return count("v_mov_b32"), (st["sgpr_spill_count"], count("v_readlane"), count("v_writelane"))


def _resolve_in_budget(stats):
    st = stats["k_resolve"]
    return (st["vgpr_count"] <= RESOLVE_VGPRS and st["vgpr_spill_count"] == 0 and st["sgpr_spill_count"] == 0 and st.get("scratch_insts", 0) == 0
            and st.get("private_segment_fixed_size", 0) == 0 and st["code_bytes"] <= RESOLVE_CODE_BYTES and st["group_segment_fixed_size"] == 0)


def test_both_switches_off_build_the_library_before(native):
    build = importlib.import_module("raytracer-rust_amd.build")
    assert sorted(build.EMPTY_PASS_OFF_DEFINES) == ["MI355RT_QC_EMPTY_PASS=0", "MI355RT_RESOLVE_SKIP=0"]
    stats, ops = _figures(build.build_empty_pass_off())
    v_mov, triple = _render_kernel(stats, ops)
    assert v_mov == in_place.SHIPPED_V_MOV == 100, v_mov
    assert triple == (nosky.SGPR_SPILLS, nosky.V_READLANE, nosky.V_WRITELANE) == (8, 10, 8), triple
    assert _resolve_in_budget(stats), stats["k_resolve"]


def test_the_shipped_library_keeps_the_render_kernels_figures(native):
    build = importlib.import_module("raytracer-rust_amd.build")
    stats, ops = _figures(build.DEVICE_SO)
    off_stats, off_ops = _figures(build.build_empty_pass_off())
    assert _render_kernel(stats, ops) == _render_kernel(off_stats, off_ops) == (100, (8, 10, 8))
    assert _resolve_in_budget(stats), stats["k_resolve"]
    # the two switches reach these two kernels and nothing else
    assert sorted(ops) == sorted(off_ops)
    assert sorted(k for k in ops if ops[k] != off_ops[k]) == ["k_render_ctr_simple_qc", "k_resolve"]


def test_the_form_0_library_is_built_without_the_shortcut():
    build = importlib.import_module("raytracer-rust_amd.build")
    assert "MI355RT_QC_EMPTY_PASS=0" in build.QC_FORM0_DEFINES
