"""The resident multi-device context (mi355rt_multi_context_*, ABI version 5) without a GPU: it refuses to run on the CPU, checks its
arguments before it looks for a device, and ABI-5 libraries still accept the options of version 4 (no struct changed)."""
import ctypes as C

import pytest


def test_multi_context_has_no_cpu_path(native, abi):
    _, device = native
    L = device.lib()
    h = C.c_void_p()
    devs = (C.c_int * 2)(0, 0)
    rc = L.mi355rt_multi_context_create(devs, 2, C.byref(h))
    if rc == 0:
        L.mi355rt_multi_context_destroy(h)
        pytest.skip("a GPU is visible here")
    assert rc == abi.ERR_NO_DEVICE
    assert b"no CPU path" in L.mi355rt_last_error()
    assert not h.value
    L.mi355rt_multi_context_destroy(None)                                # (a null context is ignored)


def test_multi_context_checks_its_arguments_before_the_device(native, abi):
    _, device = native
    L = device.lib()
    with pytest.raises(device.RenderError, match="empty") as e:
        device.MultiContext([])
    assert e.value.rc == abi.ERR_INVALID
    devs = (C.c_int * 1)(0)
    assert L.mi355rt_multi_context_create(devs, 1, None) == abi.ERR_INVALID
    assert L.mi355rt_multi_context_render(None, None, None, None, None, None) == abi.ERR_INVALID
    assert L.mi355rt_multi_context_check(None) == abi.ERR_INVALID
    assert L.mi355rt_multi_context_set_scene(None, None, None, None) == abi.ERR_INVALID


@pytest.mark.parametrize("version,ok", [(4, True), (5, True), (7, False), (3, False)])
def test_options_of_abi_version_4_and_5_are_accepted(version, ok, native, abi):
    _, device = native
    L = device.lib()
    assert L.mi355rt_abi_version() == abi.ABI_VERSION == 5
    st = abi.Settings(8, 10, 1, 1)
    opt = abi.Options.make(strip_rows=2, n_parts=3, part=1)
    opt.abi_version = version
    n = C.c_uint32()
    rc = L.mi355rt_rows_selected(C.byref(st), C.byref(opt), C.byref(n))
    if ok:
        assert rc == 0 and n.value == 4
    else:
        assert rc == abi.ERR_INVALID and b"abi_version" in L.mi355rt_last_error()
