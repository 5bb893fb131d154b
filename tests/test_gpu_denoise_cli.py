"""rt_render --denoise-out: the PNG it writes holds the packed output of the context path (Context.render, Context.first_hits,
Context.denoise with the defaults) for the same frame, and the -o image is the one written without the flag."""
import numpy as np
import pytest

from conftest import SCENES
from test_rt_render_cli import _cli

pytestmark = pytest.mark.gpu

W, H, SPP, DEPTH = 64, 48, 4, 6


def test_denoise_out_is_the_context_path_and_leaves_the_plain_image_alone(native, abi, tmp_path):
    import torch
    host, device = native
    size = ["--width", str(W), "--height", str(H), "--spp", str(SPP), "--max-depth", str(DEPTH)]
    plain, with_flag, denoised = (str(tmp_path / n) for n in ("plain.png", "with_flag.png", "denoised.png"))
    _cli(SCENES["cornell"], *size, "-o", plain)
    r = _cli(SCENES["cornell"], *size, "-o", with_flag, "--denoise-out", denoised)
    assert f"Denoised image saved as '{denoised}'" in r.stdout
    assert open(with_flag, "rb").read() == open(plain, "rb").read()
    sc = host.LoadedScene(SCENES["cornell"], W, H, SPP, DEPTH)
    ctx = device.Context(0)
    try:
        ctx.set_scene(sc, sc.camera, sc.settings)
        packed = torch.zeros((H, W), dtype=torch.int32, device="cuda")
        linear = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
        hits = torch.zeros((W * H * 48,), dtype=torch.uint8, device="cuda")
        scratch = torch.zeros((device.denoise_scratch_bytes(W, H),), dtype=torch.uint8, device="cuda")
        out = torch.zeros((H, W), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.render(packed.data_ptr(), linear.data_ptr(), abi.Options.make())
        ctx.first_hits(hits.data_ptr())
        ctx.denoise(W, H, linear.data_ptr(), hits.data_ptr(), scratch.data_ptr(), None, out.data_ptr())
        torch.cuda.synchronize()
        ctx.check()
    finally:
        ctx.close()
    want_plain, want = str(tmp_path / "want_plain.png"), str(tmp_path / "want.png")
    host.write_png(want_plain, packed.cpu().numpy().view(np.uint32), W, H)
    host.write_png(want, out.cpu().numpy().view(np.uint32), W, H)
    assert open(plain, "rb").read() == open(want_plain, "rb").read()
    assert open(denoised, "rb").read() == open(want, "rb").read()                 # equal files: equal pixels
    assert open(denoised, "rb").read() != open(plain, "rb").read()
