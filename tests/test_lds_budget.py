"""The LDS of the lockstep kernels, read from the built gfx950 code object (no GPU needed).  k_render_ctr_simple_qc keeps its camera rays' first
hits in stock (HitStock: 64 entries of 64 bytes and 1.5 KB of parked rays per wave, rt_kernels.hip); it runs 7 waves per SIMD, i.e. 7 workgroups of
256 threads per CU, and all 7 must fit in the CU's 160 KB of LDS or the occupancy the kernel was tuned for is lost."""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

LDS_PER_CU = 163840
WORKGROUPS_PER_CU = {"k_render_ctr_simple_qc": 7, "k_render_ctr_simple": 7, "k_render_ctr_nospec": 7, "k_render_ctr_nomesh": 6}


def test_lockstep_kernels_fit_their_workgroups_in_lds(native):
    isa_stats = importlib.import_module("isa_stats")
    build = importlib.import_module("raytracer-rust_amd.build")
    stats = {isa_stats.short(k): v for k, v in isa_stats.kernel_stats(build.DEVICE_SO).items()}
    for name, wgs in WORKGROUPS_PER_CU.items():
        lds = stats[name]["group_segment_fixed_size"]
        assert 0 < lds <= LDS_PER_CU // wgs, (name, lds, wgs)
    assert stats["k_render_ctr_simple_qc"]["group_segment_fixed_size"] >= 4 * 64 * 64     # the ring of first hits is there (4 waves x 64 x 64 B)
