"""What mi355rt_debug_plan_render plans is what mi355rt_context_render launches: the bands, the largest grid, the workgroup size and the row
tables of a render equal the hook's for the same inputs (both call rt_prepare.cpp's plan_render, render_band and row_tables; the CPU side is
tests/test_render_plan.py).  At these sizes a band has fewer runs than any device has wave slots, so the grid is bounded by the run count and the
hook needs no number of the device at hand."""
import numpy as np
import pytest
import torch

from conftest import SCENES

pytestmark = pytest.mark.gpu

CASES = {
    "cornell_strips_banded": ("cornell", 33, 35, 3, 6, dict(strip_rows=2, n_parts=3, part=0, workspace_bytes=33 * 4 * 3 * 12), 1, False),
    "cornell_strips_banded_share_4": ("cornell", 33, 35, 3, 6, dict(strip_rows=2, n_parts=3, part=0, workspace_bytes=33 * 4 * 3 * 12), 4, False),
    "teapot_fixed_aabb": ("teapot", 64, 48, 4, 16, dict(), 1, True),
}


@pytest.mark.parametrize("case", list(CASES))
def test_a_render_launches_what_the_hook_plans(case, native, abi):
    host, device = native
    name, W, H, spp, depth, opt_kw, share, fixed = CASES[case]
    sc = host.LoadedScene(SCENES[name], W, H, spp, depth, skip_unknown_primitives=(name == "teapot"))
    opt = abi.Options.make(flags=abi.FLAG_FIXED_AABB if fixed else 0, **opt_kw)
    has_mesh = any(sc.c.primitives[i].kind == abi.PRIM_MESH for i in range(sc.c.n_primitives))
    assert has_mesh == fixed
    ctx = device.Context(0)
    try:
        ctx.set_scene(sc, sc.camera, sc.settings)
        ctx.set_share(share)
        out = torch.zeros((H, W), dtype=torch.int32, device="cuda")
        st = ctx.render(out.data_ptr(), None, opt, None, want_stats=True)
        want = device.plan_render(sc.settings, opt, variant=ctx.kernel_variant(), has_mesh=has_mesh, n_prims=sc.c.n_primitives, block_slots=256,
                                  grid_div=share)
        natural, processing, out_row, _ = ctx.row_tables()
    finally:
        ctx.close()
    assert want.plan.variant == (8 if fixed else 14) and want.plan.n_bands > (0 if fixed else 1)
    assert int(want.bands["grid"].max()) < 256 // share                                        # bounded by the runs, not by the slots
    assert (st.bands, st.grid_blocks, st.block_threads) == (want.plan.n_bands, int(want.bands["grid"].max()), want.plan.block_threads)
    assert st.rows_rendered == len(want.natural) and st.samples == want.plan.total_pixels * spp
    assert np.array_equal(natural, want.natural) and np.array_equal(processing, want.processing) and np.array_equal(out_row, want.out_row)
