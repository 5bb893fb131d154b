"""k_render_ctr_simple_qc's range arithmetic (rt_math.h, "Range arithmetic": the closed-form second normalisation, the ranged first one, the quad's
division and the cube's reciprocals without a fix-up).  Each form is the guarded form's bits on the range it tests for, and a wave with a lane outside
it takes the guarded form -- so no image may move a bit.

  * tools/verify/range_arithmetic.hip enumerates every claim on the shipped functions (all 2^32 floats; 8 x 2^17 x 2^23 pairs of significands for the
    division; a table of special values for the quad's predicate) and is run here with a time limit.
  * The whole kernel: cornell-box at 32 x 24, 64 samples per pixel, depth 30 (one masked refill pass per pixel pair) and at 4 samples (unmasked passes of
    sixteen pixels) with the product library and with the library built with every step's define at 0 (build.build_range_off).  Radiance words, packed
    pixels and ray counts are the same from both, and the oracle's.
  * (no GPU work) The all-off library differs from the product library in k_render_ctr_simple_qc only -- and not at all when no step ships at 1."""
import importlib
import os
import subprocess
import sys

import pytest

import test_gpu_nosky as ns
import test_gpu_variant_matrix as vm
from conftest import ROOT, load_for_both, pkg
from parity import assert_parity

pytestmark = pytest.mark.gpu

W, H = 32, 24


def _render(device, abi, sc, library):
    ctx = device.Context(0, library=library)
    try:
        ctx.set_knob("kernel", 14)
        ctx.set_scene(sc, sc.camera, sc.settings)
        assert ctx.kernel_variant() == 14 and ctx.kernel_entry()[0] == ns.PLAIN
        return ns._render_on(ctx, abi, sc.settings, abi.Options.make(rng_mode=abi.RNG_CTR))
    finally:
        ctx.close()


def test_range_forms_equal_the_guarded_forms_on_every_operand():
    exe = pkg("build").build_verify_range()
    r = subprocess.run([exe, "8"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    out = r.stdout
    assert "recip_nofix: 0 differences among the normal numbers below 2^126 and NaN" in out
    assert "recip3_nofix: 0 differences over all x below 2^126, zeros, infinities, NaN (want 0), 0 with FIRST" in out
    assert "renorm_scale: 3073 of 2^32 x pass the guard (want 3073), 0 differences" in out and "0 floats of [1 - 2^-13, 1 + 2^-13] refused" in out
    assert "normalized_ranged: 1056964609 of 2^32 x pass the range test (want 1056964609), 0 differences" in out and "0 floats of the range refused" in out
    assert "vectors: 0 differences of normalized_ranged, 0 of ray_direction with both forms, 0 with the closed form alone" in out
    assert "div_bounded_nofix: 0 differences over 8 x 2^17" in out and "div_bounded_nofix: 0 differences in the quad's predicate or accepted t" in out
    assert "all checks passed" in out


@pytest.mark.parametrize("spp", [64, 4])
def test_cornell_with_and_without_the_range_forms(spp, native, oracle_mod, abi):
    host, device = native
    sc = load_for_both("cornell", oracle_mod, host, width=W, height=H, spp=spp, max_depth=30)
    opt = abi.Options.make(rng_mode=abi.RNG_CTR)
    op, ol, cnt = oracle_mod.render(sc, sc.camera, sc.settings, opt)
    got = _render(device, abi, sc, device.lib())
    off = _render(device, abi, sc, device.load(pkg("build").build_range_off()))
    vm._same(got, off, f"cornell {W} x {H} x {spp}: the range forms against the guarded forms")
    assert cnt.samples == W * H * spp and cnt.rays > 2 * cnt.samples
    assert_parity(got[0], got[1], op, ol, exact=True, gpu_rays=got[2], oracle_rays=cnt.rays)
    assert_parity(off[0], off[1], op, ol, exact=True, gpu_rays=off[2], oracle_rays=cnt.rays)


def test_the_two_libraries_differ_in_this_kernel_only(native):
    """(no GPU work: the code objects)"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    isa_stats = importlib.import_module("isa_stats")
    build = pkg("build")
    a = {isa_stats.short(k): v for k, v in isa_stats.kernel_isa(build.DEVICE_SO).items()}
    b = {isa_stats.short(k): v for k, v in isa_stats.kernel_isa(build.build_range_off()).items()}
    assert sorted(a) == sorted(b)
    assert [k for k in a if a[k] != b[k]] in (["k_render_ctr_simple_qc"], [])
