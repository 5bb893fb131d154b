"""CPU half of tests/test_gpu_transcendental_stages.py: the ledger of transcendental call sites, and the oracle's stage entry
(oracle_debug_stages) against the oracle's render-path hooks, so that what the GPU module compares with is the render's own code."""
import ctypes as C
import os
import re
import sys
from collections import Counter

import numpy as np
import pytest

from conftest import ROOT, pkg

sys.path.insert(0, os.path.join(ROOT, "tests"))
import kat_f32 as K  # noqa: E402
from parity import oracle_threads  # noqa: E402

# Every transcendental call of the render path, and the stage of tests/test_gpu_transcendental_stages.py that enumerates it:
# (file, function called, calls, stage, where)
STAGE_TABLE = [
    ("raytracer-rust_amd/csrc/device/rt_materials.h", "acosf", 2, "TEX, SKY, ACOS", "texture_lookup :66, miss_colour :240"),
    ("raytracer-rust_amd/csrc/device/rt_materials.h", "atan2f", 2, "TEX, SKY, ATAN2, ATAN2_EXACT", "texture_lookup :67, miss_colour :241"),
    ("raytracer-rust_amd/csrc/device/rt_materials.h", "fmodf", 1, "TEX, FMOD_EXACT", "texture_lookup :70"),
    ("raytracer-rust_amd/csrc/device/rt_materials.h", "logf", 1, "LATTICE, HALF (CTR)", "scatter_pre, rough conductor"),
    ("raytracer-rust_amd/csrc/device/rt_materials.h", "log", 1, "LATTICE, HALF (REF)", "scatter_pre, rough conductor"),
    ("raytracer-rust_amd/csrc/device/rt_materials.h", "atanf", 1, "LATTICE, HALF (CTR)", "scatter_pre, theta"),
    ("raytracer-rust_amd/csrc/device/rt_materials.h", "atan", 1, "LATTICE, HALF (REF)", "scatter_pre, theta"),
    ("raytracer-rust_amd/csrc/device/rt_materials.h", "sincosf", 2, "LATTICE, HALF (CTR)", "scatter_pre, theta and phi"),
    ("raytracer-rust_amd/csrc/device/rt_materials.h", "sin", 2, "LATTICE, HALF (REF)", "scatter_pre, theta and phi"),
    ("raytracer-rust_amd/csrc/device/rt_materials.h", "cos", 2, "LATTICE, HALF (REF)", "scatter_pre, theta and phi"),
    ("oracle/rt_oracle.cpp", "log", 2, "LATTICE, HALF", "MicrofacetLibm::ln, both forms"),
    ("oracle/rt_oracle.cpp", "atan", 2, "LATTICE, HALF", "MicrofacetLibm::at"),
    ("oracle/rt_oracle.cpp", "sin", 2, "LATTICE, HALF", "MicrofacetLibm::sn"),
    ("oracle/rt_oracle.cpp", "cos", 2, "LATTICE, HALF", "MicrofacetLibm::cs"),
    ("oracle/rt_oracle.cpp", "acos", 2, "TEX, SKY, ACOS", "texture_texel, sky_lookup"),
    ("oracle/rt_oracle.cpp", "atan2", 2, "TEX, SKY, ATAN2", "texture_texel, sky_lookup"),
    ("oracle/rt_oracle.cpp", "fmod", 1, "TEX, FMOD_EXACT", "texture_texel"),
]
_CALL = re.compile(r"(?<![\w:.])(?:std::)?(acosf|atan2f|logf|atanf|sincosf|fmodf|log|atan|sin|cos|acos|atan2|fmod)\s*\(")
_STAGES_MARK = "// ===================="          # rt_oracle.cpp: oracle_debug_stages and its float64 references start at this rule


def _render_path_sources():
    dev = os.path.join(ROOT, "raytracer-rust_amd", "csrc", "device")
    files = sorted(os.path.join(dev, f) for f in os.listdir(dev) if f.endswith((".h", ".hip", ".cpp")))
    yield from files
    yield os.path.join(ROOT, "oracle", "rt_oracle.cpp")


def test_every_transcendental_call_of_the_render_path_is_enumerated():
    """A source scan of the device code and the oracle's render path finds every call of acosf / atan2f / logf / atanf / sincosf / fmodf and of
    log / atan / sin / cos / acos / atan2 / fmod; each (file, function) must be a row of STAGE_TABLE with that many calls.  A new
    transcendental on the hot path fails here until a stage enumerates it."""
    build = pkg("build")
    found = Counter()
    for path in _render_path_sources():
        text = open(path, encoding="utf-8").read()
        if path.endswith("rt_oracle.cpp"):
            assert text.count(_STAGES_MARK) >= 1
            text = text[:text.index(_STAGES_MARK)]
        for name in _CALL.findall(build._code_only(text)):
            found[(os.path.relpath(path, ROOT), name)] += 1
    table = Counter({(f, name): n for f, name, n, _, _ in STAGE_TABLE})
    assert found == table, {"not in the table": dict(found - table), "no longer in the code": dict(table - found)}


def _stage_args(stage, **kw):
    device = pkg("device")
    a = device.StageArgs()
    a.stage, a.stride = device.STAGES[stage], 1
    for k, v in kw.items():
        if k in ("n", "rd"):
            getattr(a, k)[:3] = v
        else:
            setattr(a, k, v)
    return a


def _f32_normalized(v):
    v = np.asarray(v, np.float32)
    n = np.float32(np.sqrt(np.float32(np.float32(v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])))
    return v if n < np.float32(1e-4) else v * np.float32(np.float32(1.0) / n)


def test_rough_conductor_stage_is_the_oracles_scatter(oracle_mod, abi):
    """oracle_debug_stages' HALF on the draws that oracle_scatter_ctr's counter-mode generator makes (u1, u2 = block 0, words 0 and 1)
    returns the direction (before Ray::new) and attenuation of the render's Material::scatter, for 300 events of both rough kinds."""
    L = oracle_mod.lib()
    rng = np.random.default_rng(7)
    n_scattered = 0
    for i in range(300):
        ggx = i % 2 == 0
        rough = np.float32(rng.choice([0.01, 0.05, 0.1, 0.25, 0.5, 1.0]))
        m = abi.Material()
        m.kind = abi.MAT_ROUGH_GGX if ggx else abi.MAT_ROUGH_BECKMANN
        m.albedo[:] = (0.9, 0.8, 0.7); m.p0 = float(rough); m.eta[:] = (0.2, 1.09, 1.42); m.k[:] = (3.91, 2.57, 2.30)
        n = _f32_normalized(rng.normal(size=3)) if i % 3 else np.array([0, 0, 1], np.float32)
        rd = np.asarray(-n + rng.normal(scale=0.6, size=3), np.float32)
        ctr = tuple(int(x) for x in rng.integers(0, 2 ** 31, 5))
        out = np.zeros(10, np.float32)
        assert L.oracle_scatter_ctr(C.byref(m), np.zeros(3, np.float32).ctypes.data, rd.ctypes.data, np.zeros(3, np.float32).ctypes.data,
                                    n.ctypes.data, 1, *ctr, out.ctypes.data) == 0
        w = oracle_mod.ctr_block(*ctr, 0)
        in4 = np.array([[oracle_mod.lib().oracle_u32_to_f01(int(w[0])), oracle_mod.lib().oracle_u32_to_f01(int(w[1])), 0, 0]], np.float32)
        a = _stage_args("half", ggx=int(ggx), rough=float(rough), n=n, rd=rd)
        _, words = oracle_mod.debug_stages(a, 1, in4=in4, mat=m, want_words=True)
        f = words[0].view(np.float32)
        assert (f[6] == 1.0) == (out[0] == 1.0), i
        if out[0] == 1.0:
            n_scattered += 1
            assert np.array_equal(f[3:6].view(np.uint32), out[7:10].view(np.uint32)), i
            assert np.array_equal(_f32_normalized(_f32_normalized(f[0:3])).view(np.uint32), out[4:7].view(np.uint32)), i
    assert n_scattered > 100


def test_texture_stage_is_the_oracles_texture_material(oracle_mod, abi):
    """oracle_debug_stages' TEX returns the texel the render's TextureMaterial picks (oracle_scatter_ctr's attenuation with albedo 1), on a
    texture whose texels encode their own (x, y): random normals, the seam and the poles, three sizes and offsets."""
    L = oracle_mod.lib()
    L.oracle_set_textures.argtypes = [C.POINTER(abi.Texture), C.c_uint32]
    rng = np.random.default_rng(11)
    try:
        for w, h, hoff in ((8, 4, 0.3), (255, 256, 0.0), (1, 1, 0.999999)):
            texels = np.ascontiguousarray((np.arange(w, dtype=np.uint32)[None, :] | (np.arange(h, dtype=np.uint32)[:, None] << 8)))
            tex = abi.Texture(texels.ctypes.data_as(C.POINTER(C.c_uint8)), w, h)
            textures = (abi.Texture * 1)(tex)
            L.oracle_set_textures(textures, 1)
            m = abi.Material(); m.kind = abi.MAT_TEXTURE; m.albedo[:] = (1, 1, 1); m.p0 = hoff; m.texture = 0
            normals = [_f32_normalized(rng.normal(size=3)) for _ in range(100)]
            normals += [np.array(v, np.float32) for v in ((-1, 0.3, 0.0), (-1, 0.3, -0.0), (0, 1, 0), (0, -1, 0), (1, 0, 0))]
            in4 = np.zeros((len(normals), 4), np.float32)
            in4[:, :3] = normals
            _, words = oracle_mod.debug_stages(_stage_args("tex", img_w=w, img_h=h, h_offset=hoff), len(normals), in4=in4, tex=tex, want_words=True)
            for i, n in enumerate(normals):
                out = np.zeros(10, np.float32)
                rd = np.asarray(-n, np.float32)
                assert L.oracle_scatter_ctr(C.byref(m), np.zeros(3, np.float32).ctypes.data, rd.ctypes.data, np.zeros(3, np.float32).ctypes.data,
                                            n.ctypes.data, 1, 1, 2, i, 3, 1, out.ctypes.data) == 0
                assert np.array_equal(words[i, :3], out[7:10].view(np.uint32)), (w, h, hoff, n)
    finally:
        L.oracle_set_textures(None, 0)


def test_oracle_fmod_stage_is_exact_on_a_stride_of_every_u(oracle_mod):
    """The oracle's side of FMOD_EXACT on every 97th f32 in [0, 1] (the GPU module runs every one): std::fmod(u + h, 1) == a - floor(a)."""
    for hoff in (0.0, 0.3, 0.999999, 1.0 - 2.0 ** -24):
        a = _stage_args("fmod_exact", h_offset=hoff)
        a.stride = 97
        res, _ = oracle_mod.debug_stages(a, 0x3F800001 // 97 + 1, threads=oracle_threads())
        assert res[0] == 0, (hoff, res[1])


def test_stage_args_layouts_agree():
    """device.StageArgs mirrors the 96-byte record both native sides read."""
    assert C.sizeof(pkg("device").StageArgs) == 96
