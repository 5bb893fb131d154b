"""Variant 14's two entry points, read from the built gfx950 code object and from the host half (no GPU needed).

k_render_ctr_simple_qc is compiled without the HDR sky lookup and for 8 waves per SIMD: 64 VGPRs, and 16 KB of LDS per workgroup so that eight
workgroups of 256 threads fit in a CU's 160 KB (the refill pass parks the paths' rays inside the empty ring).  k_render_sky_simple_qc is the body
with the lookup, for scenes that carry a sky texture, and stays inside the line tests/test_isa_budget.py drew for k_render_ctr_simple_qc when that
kernel held the lookup: 7 waves per SIMD."""
import importlib
import os
import sys

import test_gpu_variant_matrix as vm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

LDS_PER_CU = 163840
PARENT_CODE_BYTES = 9756                    # k_render_ctr_simple_qc with the lookup compiled in
# The shipped form's own counts, from the listing of the product library (tools/isa_stats.py; profiles/isa_diff_nosky_eight_waves_vs_parent.txt):
# at 8 waves per SIMD a wave may hold 80 scalar registers (96 at 7), and the kernel spills 8 of them into lanes of one vector register.
SGPR_SPILLS, V_READLANE, V_WRITELANE = 8, 10, 8


def _library():
    isa_stats = importlib.import_module("isa_stats")
    build = importlib.import_module("raytracer-rust_amd.build")
    stats = {isa_stats.short(k): v for k, v in isa_stats.kernel_stats(build.DEVICE_SO).items()}
    isa = {isa_stats.short(k): [line.split()[0] for line in v] for k, v in isa_stats.kernel_isa(build.DEVICE_SO).items()}
    return stats, isa


def test_the_twin_keeps_the_line_of_the_kernel_with_the_lookup(native):
    stats, _ = _library()
    st = stats["k_render_sky_simple_qc"]
    assert st["vgpr_count"] <= 72 and st["vgpr_spill_count"] <= 1 and st["code_bytes"] <= 10 * 1024 and st.get("scratch_insts", 0) <= 1, st
    assert 0 < 7 * st["group_segment_fixed_size"] <= LDS_PER_CU, st


def test_the_kernel_without_the_lookup(native):
    stats, isa = _library()
    st, ops = stats["k_render_ctr_simple_qc"], isa["k_render_ctr_simple_qc"]
    count = lambda prefix: sum(op.startswith(prefix) for op in ops)
    assert count("flat_load") == 0                                    # a miss reads no texel and selects no pointer
    assert st["code_bytes"] <= PARENT_CODE_BYTES, st
    assert (st["sgpr_spill_count"], count("v_readlane"), count("v_writelane")) == (SGPR_SPILLS, V_READLANE, V_WRITELANE), st
    # eight waves per SIMD: 512 VGPRs / 8, nothing spilled, eight workgroups in the CU's LDS -- and the ring of first hits is there
    assert st["vgpr_count"] <= 64 and st["vgpr_spill_count"] == 0 and st.get("scratch_insts", 0) == 0, st
    assert 4 * 64 * 64 <= st["group_segment_fixed_size"] <= 20480 and 8 * st["group_segment_fixed_size"] <= LDS_PER_CU, st


def test_the_launch_follows_the_sky(native, abi):
    """Host only: a prepared list of quads and cubes with Lambert materials is variant 14 with and without a sky texture, launched on the kernel
    without the lookup in one case and on the twin in the other; every other variant has one kernel for both."""
    host, device = native
    fam = "lambert_qc"
    seen = set()
    for seed in vm.SEEDS:
        sc = vm._scene(abi, host, fam, seed)
        has_sky = sc.c.sky_width != 0
        variant = device.prepare_scene(sc).variant
        assert variant == 14, (seed, variant)
        assert device.entry_kernel(variant, has_sky) == ("k_render_sky_simple_qc" if has_sky else "k_render_ctr_simple_qc")
        seen.add(has_sky)
    assert seen == {False, True}
    for v, (kernel, library, _, _, _) in vm.CAPABILITY.items():
        if v != 14:
            assert device.entry_kernel(v, False) == device.entry_kernel(v, True) == kernel, v
    assert device.entry_kernel(15, False) is None
