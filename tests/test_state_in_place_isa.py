"""The register copies of k_render_ctr_simple_qc, read from the built gfx950 code object (no GPU needed).

The kernel carries a path's state in place (rt_kernels.hip, FORM_HIT_IN_PLACE and FORM_STATE_IN_PLACE): the block of v_mov_b32 at the bottom of every
bounce iteration and the copy of the whole hit in front of the deal are gone from its listing.  Before, the listing held 117 v_mov_b32
(profiles/isa_diff_state_in_place_vs_parent.txt); the shipped one holds 100, and a change that brings copies back shows here before it costs time on
the GPU.  k_render_sky_simple_qc, the twin with the sky lookup, is compiled from the same body with the steps off and keeps the count it had."""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

PARENT_V_MOV = 117                          # k_render_ctr_simple_qc before the steps (every step's define at 0 builds it again)
SHIPPED_V_MOV = 100                         # the shipped listing's own count
TWIN_V_MOV = 138                            # k_render_sky_simple_qc, then and now


def _v_mov(so):
    isa_stats = importlib.import_module("isa_stats")
    return {isa_stats.short(k): sum(line.split()[0].startswith("v_mov_b32") for line in v) for k, v in isa_stats.kernel_isa(so).items()}


def test_fewer_register_copies_than_the_form_before(native):
    build = importlib.import_module("raytracer-rust_amd.build")
    count = _v_mov(build.DEVICE_SO)
    assert SHIPPED_V_MOV < PARENT_V_MOV
    assert count["k_render_ctr_simple_qc"] <= SHIPPED_V_MOV, count["k_render_ctr_simple_qc"]
    assert count["k_render_sky_simple_qc"] == TWIN_V_MOV, count["k_render_sky_simple_qc"]


def test_the_steps_at_zero_build_the_form_before(native):
    build = importlib.import_module("raytracer-rust_amd.build")
    count = _v_mov(build.build_qc_form0())
    assert (count["k_render_ctr_simple_qc"], count["k_render_sky_simple_qc"]) == (PARENT_V_MOV, TWIN_V_MOV), count
