"""ctypes binding of libmi355rt_post.so -- the image-space post stages on device buffers (include/mi355rt_post.h).

A library of its own beside libmi355rt.so: a stage needs no scene and no context, only a device and a stream.  There is no CPU fallback: `lib()`
raises if the library has not been built, and `reproject` raises if no GPU is visible.  torch is NOT needed here; callers that hold torch
tensors pass `tensor.data_ptr()` and `torch.cuda.current_stream().cuda_stream`.
"""
import ctypes as C
import os

from . import abi, build

EXPORTS = ["mi355rt_post_last_error", "mi355rt_post_abi_version", "mi355rt_post_reproject"]

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(build.POST_SO):
            raise RuntimeError(f"{build.POST_SO} is missing: the HIP extension must be built (__graft_entry__.build()); there is no CPU fallback")
        L = C.CDLL(build.POST_SO)
        L.mi355rt_post_last_error.restype = C.c_char_p
        L.mi355rt_post_abi_version.restype = C.c_uint32
        L.mi355rt_post_reproject.restype = C.c_int
        L.mi355rt_post_reproject.argtypes = [C.c_int, C.POINTER(abi.View), C.POINTER(abi.View), C.POINTER(abi.ReprojectParams)] + [C.c_void_p] * 8
        if L.mi355rt_post_abi_version() != abi.POST_ABI_VERSION:
            raise RuntimeError("libmi355rt_post.so ABI version does not match abi.py")
        _lib = L
    return _lib


class RenderError(RuntimeError):
    def __init__(self, what, rc):
        super().__init__(f"{what} failed ({rc}): {lib().mi355rt_post_last_error().decode()}")
        self.rc = rc


def _check(rc, what):
    if rc != 0:
        raise RenderError(what, rc)


def reproject(cur, prev, d_hits_cur, d_color_cur, d_hits_prev, d_hist_prev, d_hist_out, d_out_linear=None, d_out_packed=None, params=None,
              hip_device=0, stream=None):
    """mi355rt_post_reproject: this frame's history {r, g, b, length} from this frame's colour and the previous frame's history, enqueued on
    `stream` of `hip_device`.  cur, prev: abi.View (prev None: no previous frame, every pixel starts at length 1).  Integer device addresses:
    d_hits_cur cur.width * cur.height abi.Hit records and d_color_cur as many * 3 floats; d_hits_prev / d_hist_prev the previous view's records and
    float4 history (None without prev); d_hist_out cur.width * cur.height float4 (never d_hist_prev); d_out_linear (may be d_color_cur) and
    d_out_packed (0x00RRGGBB words) or None.  params: abi.ReprojectParams or None for the defaults."""
    p = lambda a: C.c_void_p(a) if a else None
    ref = lambda s: C.byref(s) if s is not None else None
    _check(lib().mi355rt_post_reproject(int(hip_device), ref(cur), ref(prev), ref(params), p(d_hits_cur), p(d_color_cur), p(d_hits_prev), p(d_hist_prev),
                                        p(d_hist_out), p(d_out_linear), p(d_out_packed), p(stream)), "mi355rt_post_reproject")
