"""The denoiser's definition (include/mi355rt.h), checked on its numpy restatement tests/denoise_ref.py with the oracle's images and guides: no
GPU, no product code.  What the filter promises -- zero levels copy, a geometric edge between exact colours stays exact, non-finite pixels
pass through and contaminate nothing -- and the quality gate: on the oracle's 4-spp cornell-box the defaults bring the error against the
oracle's 1024-spp image to at most 0.60 of the noisy image's (measured 0.476)."""
import numpy as np

import denoise_cases as cases
import denoise_ref as ref

F = np.float32


def two_halves(abi, W=24, H=16):
    """Left half: colour exactly 0 on a floor (normal +y); right half: colour exactly 1 on a wall (normal +x): perpendicular guides."""
    lin = np.zeros((H, W, 3), F)
    lin[:, W // 2:] = F(1.0)
    hits = np.zeros((H, W), abi.HIT_DTYPE)
    yy, xx = np.mgrid[0:H, 0:W]
    hits["position"][..., 0], hits["position"][..., 2] = xx * F(0.1), yy * F(0.1)
    hits["normal"][:, : W // 2] = [0.0, 1.0, 0.0]
    hits["normal"][:, W // 2:] = [1.0, 0.0, 0.0]
    hits["position"][:, W // 2:, 0] = F(W // 2 * 0.1)                  # the wall is a plane x = const: its pixels differ in y and z only
    hits["position"][:, W // 2:, 1] = (xx[:, W // 2:] * F(0.1)).astype(F)
    hits["t"], hits["front_face"], hits["primitive"] = F(3.0), 1, 0
    return lin, hits.reshape(-1)


def test_zero_levels_is_the_identity(abi):
    lin, hits = cases.synthetic(abi, 37, 11, 5)
    out = ref.denoise(lin, hits, levels=0)
    assert out.view(np.uint32).tobytes() == lin.view(np.uint32).tobytes()


def test_a_perpendicular_edge_between_exact_colours_stays_exact(abi):
    lin, hits = two_halves(abi)
    out = ref.denoise(lin, hits, levels=5, normal_squarings=5, sigma_color=2.0, sigma_plane=0.05)
    assert out.view(np.uint32).tobytes() == lin.view(np.uint32).tobytes()       # 0 / ws and ws / ws are exact
    # ... and without the geometry weight the same image does blur: the edge is kept by the guides, not by the colour weight at sigma 2
    same = hits.copy(); same["normal"] = [0.0, 1.0, 0.0]; same["position"][:, 1] = 0
    blurred = ref.denoise(lin, same, levels=5, normal_squarings=5, sigma_color=2.0, sigma_plane=1e9)
    assert ((blurred > 0) & (blurred < 1)).any()


def test_inf_and_nan_pixels_pass_through_and_contaminate_nothing(abi):
    rng = np.random.default_rng(11)
    H, W = 20, 28
    lin = rng.uniform(0.2, 0.8, (H, W, 3)).astype(F)
    hits = np.zeros(H * W, abi.HIT_DTYPE)
    hits["normal"], hits["t"], hits["primitive"] = [0.0, 1.0, 0.0], F(2.0), 3
    yy, xx = np.divmod(np.arange(H * W), W)
    hits["position"][:, 0], hits["position"][:, 2] = xx * F(0.05), yy * F(0.05)
    lin[7, 9] = [np.inf, 0.5, 0.5]
    lin[12, 20] = [0.5, np.nan, 0.5]
    lin[3, 3] = [-np.inf, np.nan, np.inf]
    out = ref.denoise(lin, hits, **ref.DEFAULTS)
    special = np.zeros((H, W), bool)
    for y, x in ((7, 9), (12, 20), (3, 3)):
        special[y, x] = True
        assert out[y, x].view(np.uint32).tobytes() == lin[y, x].view(np.uint32).tobytes(), (y, x)
    assert np.isfinite(out[~special]).all()
    assert (out[~special] != lin[~special]).any()                       # the rest was filtered


def test_quality_gate_on_the_oracles_cornell_box(native, oracle_mod, abi):
    host, _ = native
    noisy = cases.gate_oracle_image(oracle_mod, abi, host, cases.GATE_SPP)
    clean = cases.gate_oracle_image(oracle_mod, abi, host, cases.GATE_REF_SPP)
    guides = cases.gate_oracle_guides(oracle_mod, abi, host)
    out = ref.denoise(noisy, guides, **ref.DEFAULTS)
    e_noisy, e_out = ref.rmse(noisy, clean), ref.rmse(out, clean)
    print(f"RMSE noisy {e_noisy:.4f} denoised {e_out:.4f} ratio {e_out / e_noisy:.4f}")
    assert e_out / e_noisy <= cases.GATE_LIMIT, (e_out, e_noisy)
