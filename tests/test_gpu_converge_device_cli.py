"""rt_render --noise-target --noise-device: the converging loop with the estimate taken on the device, against the SAME command line without
the flag (the host loop, which tests/test_gpu_converge_cli.py holds against a replay).  Every image file and the error map must be the same
bytes, the `noise:` line the same figures -- mean alone may differ by the rounding of another order of summation, within the header's bound
widened by the 9 digits it is printed with.  Every CLI run is a child process under a timeout."""
import pytest

from conftest import SCENES
from converge_cases import five_kinds_scene, infinite_emitter_scene, parse_noise_line
from test_rt_render_cli import _cli

gpu = pytest.mark.gpu
W, H, DEPTH, CHUNK = 48, 36, 6, 4
SAME = ("samples", "chunks", "rendered", "above", "nonfinite", "max", "converged")


def _pair(path, tmp_path, tag, *args, w=W, h=H, noise_out=True, denoise=False):
    """The command line once without and once with --noise-device; returns the two parsed `noise:` lines after comparing every file."""
    got = {}
    for mode in ("host", "device"):
        out = {e: str(tmp_path / f"{tag}_{mode}.{e}") for e in ("png", "pfm", "map.pfm", "dn.png")}
        extra = (["--noise-out", out["map.pfm"]] if noise_out else []) + (["--denoise-out", out["dn.png"]] if denoise else []) + (["--noise-device"] if mode == "device" else [])
        r = _cli(path, "--width", str(w), "--height", str(h), "--max-depth", str(DEPTH), "-o", out["png"], "--pfm", out["pfm"], "--chunk", str(CHUNK), *args, *extra)
        files = {e: open(p, "rb").read() for e, p in out.items() if (e != "map.pfm" or noise_out) and (e != "dn.png" or denoise)}
        got[mode] = (parse_noise_line(r.stdout), files, r.stdout)
    (nh, fh, oh), (nd, fd, od) = got["host"], got["device"]
    assert fh.keys() == fd.keys() and len(fh) == 2 + noise_out + denoise
    for e in fh:
        assert fh[e] == fd[e], e                                      # -o, --pfm, --noise-out, --denoise-out: byte for byte
    for f in SAME:
        assert nh[f] == nd[f], (f, nh, nd)
    # (pixels + 64) * 2^-53 relative, and each of the two figures is printed with 9 significant digits
    assert abs(nh["mean"] - nd["mean"]) <= ((w * h + 64) * 2.0 ** -53 + 1e-8) * nh["mean"], (nh["mean"], nd["mean"])
    assert "noise host: update_ms=" in oh and "noise device:" not in oh
    assert "noise device: pass_ms=" in od and "noise host:" not in od
    progress = lambda o: [l for l in o.splitlines() if l.startswith("  ") and "samples per pixel" in l]
    assert [l.split(" mean=")[0] for l in progress(oh)] == [l.split(" mean=")[0] for l in progress(od)]      # the same verdict after every chunk
    return nh, nd


@gpu
def test_an_odd_interior_stop(tmp_path):
    nh, _ = _pair(SCENES["cornell"], tmp_path, "odd", "--noise-target", "1e9", "--min-chunks", "3", "--max-spp", "64")
    assert (nh["samples"], nh["chunks"], nh["converged"], nh["rendered"]) == (12, 3, 1, 16)


@gpu
def test_an_even_interior_stop_on_the_estimate(tmp_path):
    """An even chunk (the other output pair and summary slot than the odd stop), and a threshold the estimate itself decides on the five-kinds
    scene at an odd size: wherever the host loop stops, the device loop does."""
    nh, _ = _pair(SCENES["cornell"], tmp_path, "even", "--noise-target", "1e9", "--min-chunks", "6", "--max-spp", "64")
    assert (nh["samples"], nh["chunks"], nh["converged"], nh["rendered"]) == (24, 6, 1, 28)
    nh, _ = _pair(five_kinds_scene(tmp_path), tmp_path, "five", "--noise-target", "0.35", "--noise-allow", "0.2", "--min-chunks", "2", "--max-spp", "40", w=33, h=17)
    assert nh["chunks"] >= 2


@gpu
def test_target_zero_runs_to_max_spp_with_a_short_last_chunk(tmp_path):
    nh, _ = _pair(SCENES["cornell"], tmp_path, "full", "--noise-target", "0", "--max-spp", "22")
    assert (nh["samples"], nh["chunks"], nh["converged"], nh["rendered"]) == (22, 6, 0, 22) and nh["above"] > 0


@gpu
def test_the_infinite_emitter(tmp_path):
    nh, _ = _pair(infinite_emitter_scene(tmp_path), tmp_path, "inf", "--noise-target", "1e9", "--min-chunks", "4", "--max-spp", "64", w=40, h=30)
    assert (nh["samples"], nh["chunks"], nh["converged"], nh["above"]) == (16, 4, 1, 0) and nh["nonfinite"] > 0


@gpu
def test_denoise_out(tmp_path):
    nh, _ = _pair(SCENES["cornell"], tmp_path, "dn", "--noise-target", "1e9", "--min-chunks", "2", "--max-spp", "64", noise_out=False, denoise=True)
    assert (nh["samples"], nh["chunks"], nh["rendered"]) == (8, 2, 12)


def test_noise_device_alone_is_a_usage_error(native, tmp_path):
    """Decided before the scene is loaded and before any device is looked for: no GPU needed."""
    for args in (("--noise-device",), ("--noise-device", "--chunk", "4"), ("--spp", "4", "--noise-device")):
        r = _cli(SCENES["cornell"], *args, expect=2)
        assert r.stderr.startswith("usage:") and "--noise-device needs --noise-target" in r.stderr and "[--noise-device]" in r.stderr
        assert "Attempting to load" not in r.stdout
    r = _cli(SCENES["cornell"], "--noise-device", "--noise-target", "0.1", "--gpus", "2", expect=2)     # the flag does not lift the one-GPU rule
    assert "--gpus or --devices" in r.stderr
