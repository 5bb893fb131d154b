"""Progressive rendering on the resident multi-device context (mi355rt_multi_context_render_progressive, mi355rt_render_progressive_multi;
added within ABI version 5) without a GPU: both are declared and exported, they check their arguments before they look for a device, the
one-shot refuses to run on the CPU, and the ABI number did not move."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

NEW = ("mi355rt_multi_context_render_progressive", "mi355rt_render_progressive_multi")


def _settings(abi):
    return abi.Settings(16, 8, 4, 3)


def test_declared_and_exported(native):
    _, device = native
    header = open(os.path.join(ROOT, "include", "mi355rt.h")).read()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert hasattr(device.lib(), name)
        assert name in device.EXPORTS


def test_abi_version_is_still_5(native, abi):
    _, device = native
    assert device.lib().mi355rt_abi_version() == abi.ABI_VERSION == 5


def test_multi_context_render_progressive_checks_before_the_device(native, abi):
    _, device = native
    L = device.lib()
    assert L.mi355rt_multi_context_render_progressive(None, None, 0, 4, None, None, None, None, None) == abi.ERR_INVALID
    assert b"multi context is null" in L.mi355rt_last_error()
    for begin, end in ((4, 4), (5, 2)):
        assert L.mi355rt_multi_context_render_progressive(None, None, begin, end, None, None, None, None, None) == abi.ERR_INVALID


def _one_shot(L, abi, devices, chunk, settings=None, packed=True):
    sc, cam = abi.Scene(), abi.Camera()
    st = settings if settings is not None else _settings(abi)
    out = (C.c_uint32 * (16 * 8))()
    devs = (C.c_int * max(len(devices), 1))(*devices)
    return L.mi355rt_render_progressive_multi(C.byref(sc), C.byref(cam), C.byref(st), None, devs, len(devices), chunk,
                                              abi.ProgressFn(), None, out if packed else None, None, None)


def test_render_progressive_multi_checks_before_the_device(native, abi):
    _, device = native
    L = device.lib()
    assert _one_shot(L, abi, [0, 0], 0) == abi.ERR_INVALID
    assert b"chunk_spp" in L.mi355rt_last_error()
    assert _one_shot(L, abi, [], 2) == abi.ERR_INVALID
    assert b"empty" in L.mi355rt_last_error()
    assert _one_shot(L, abi, [0], 2, packed=False) == abi.ERR_INVALID
    assert _one_shot(L, abi, [0], 2, settings=abi.Settings(0, 8, 4, 3)) == abi.ERR_INVALID
    opt = abi.Options.make(n_parts=2, part=1)
    sc, cam, st = abi.Scene(), abi.Camera(), _settings(abi)
    out = (C.c_uint32 * (16 * 8))()
    devs = (C.c_int * 2)(0, 0)
    assert L.mi355rt_render_progressive_multi(C.byref(sc), C.byref(cam), C.byref(st), C.byref(opt), devs, 2, 2, abi.ProgressFn(), None,
                                              out, None, None) == abi.ERR_INVALID
    assert b"deals the strips itself" in L.mi355rt_last_error()
    ref = abi.Options.make(rng_mode=abi.RNG_REF)
    assert L.mi355rt_render_progressive_multi(C.byref(sc), C.byref(cam), C.byref(st), C.byref(ref), devs, 2, 2, abi.ProgressFn(), None,
                                              out, None, None) == abi.ERR_INVALID
    assert b"MI355RT_RNG_CTR" in L.mi355rt_last_error()


def test_render_progressive_multi_has_no_cpu_path(native, abi):
    _, device = native
    L = device.lib()
    h = C.c_void_p()
    devs = (C.c_int * 1)(0)
    if L.mi355rt_multi_context_create(devs, 1, C.byref(h)) == 0:
        L.mi355rt_multi_context_destroy(h)
        pytest.skip("a GPU is visible here")
    assert _one_shot(L, abi, [0, 0], 2) == abi.ERR_NO_DEVICE
    assert b"no CPU path" in L.mi355rt_last_error()
    with pytest.raises(device.RenderError) as e:
        device.render_progressive_multi(abi.Scene(), abi.Camera(), _settings(abi), [0, 0], 2, on_chunk=lambda *a: 0)
    assert e.value.rc == abi.ERR_NO_DEVICE
