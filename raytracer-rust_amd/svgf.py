"""ctypes binding of libmi355rt_svgf.so -- the variance-guided temporal filter on device buffers (include/mi355rt_svgf.h).

A library of its own beside libmi355rt.so and libmi355rt_post.so: a stage needs no scene and no context, only a device and a stream.  There is no
CPU fallback: `lib()` raises if the library has not been built, and the calls raise if no GPU is visible.  torch is NOT needed here; callers that
hold torch tensors pass `tensor.data_ptr()` and `torch.cuda.current_stream().cuda_stream`.

The module's own functions (lib, scratch_bytes, accumulate, filter) are those of the product library, build.SVGF_SO.  `open_library(path)` binds
another file with the same exports -- a variant of build.build_svgf_variant -- to the same call wrappers; which file a call goes to is decided by
the object it is called on, never by the environment.
"""
import ctypes as C
import os

from . import abi, build

EXPORTS = ["mi355rt_svgf_last_error", "mi355rt_svgf_abi_version", "mi355rt_svgf_scratch_bytes", "mi355rt_svgf_accumulate", "mi355rt_svgf_filter"]


class RenderError(RuntimeError):
    def __init__(self, what, rc, text):
        super().__init__(f"{what} failed ({rc}): {text}")
        self.rc = rc


_p = lambda a: C.c_void_p(a) if a else None
_ref = lambda s: C.byref(s) if s is not None else None


class Library:
    """One library file with the exports of include/mi355rt_svgf.h, loaded at the first call."""
    RenderError = RenderError

    def __init__(self, path):
        self.path = path
        self._lib = None

    def lib(self):
        if self._lib is None:
            if not os.path.exists(self.path):
                raise RuntimeError(f"{self.path} is missing: the HIP extension must be built (__graft_entry__.build()); there is no CPU fallback")
            L = C.CDLL(self.path)
            L.mi355rt_svgf_last_error.restype = C.c_char_p
            L.mi355rt_svgf_abi_version.restype = C.c_uint32
            L.mi355rt_svgf_scratch_bytes.restype = C.c_int
            L.mi355rt_svgf_scratch_bytes.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]
            L.mi355rt_svgf_accumulate.restype = C.c_int
            L.mi355rt_svgf_accumulate.argtypes = [C.c_int, C.POINTER(abi.View), C.POINTER(abi.View), C.POINTER(abi.SvgfAccumulateParams)] + [C.c_void_p] * 9
            L.mi355rt_svgf_filter.restype = C.c_int
            L.mi355rt_svgf_filter.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.POINTER(abi.SvgfFilterParams)] + [C.c_void_p] * 7
            if L.mi355rt_svgf_abi_version() != abi.SVGF_ABI_VERSION:
                raise RuntimeError(f"{os.path.basename(self.path)} ABI version does not match abi.py")
            self._lib = L
        return self._lib

    def _check(self, rc, what):
        if rc != 0:
            raise RenderError(what, rc, self.lib().mi355rt_svgf_last_error().decode())

    def scratch_bytes(self, width, height):
        """mi355rt_svgf_scratch_bytes: the bytes of filter's d_scratch for a frame of width x height pixels."""
        out = C.c_uint64()
        self._check(self.lib().mi355rt_svgf_scratch_bytes(int(width), int(height), C.byref(out)), "mi355rt_svgf_scratch_bytes")
        return out.value

    def accumulate(self, cur, prev, d_hits_cur, d_color_cur, d_hits_prev, d_hist_prev, d_moments_prev, d_hist_out, d_moments_out, d_variance_out, params=None,
                   hip_device=0, stream=None):
        """mi355rt_svgf_accumulate: this frame's history {r, g, b, length}, luminance moments {m1, m2} and variance from this frame's colour and the previous
        frame's history and moments, enqueued on `stream` of `hip_device`.  cur, prev: abi.View (prev None: no previous frame).  Integer device addresses:
        d_hits_cur cur.width * cur.height abi.Hit records and d_color_cur as many * 3 floats; d_hits_prev / d_hist_prev / d_moments_prev the previous view's
        records, float4 history and float2 moments (None without prev); d_hist_out float4, d_moments_out float2 (neither the previous frame's buffer),
        d_variance_out float, per pixel of cur.  params: abi.SvgfAccumulateParams or None for the defaults."""
        self._check(self.lib().mi355rt_svgf_accumulate(int(hip_device), _ref(cur), _ref(prev), _ref(params), _p(d_hits_cur), _p(d_color_cur), _p(d_hits_prev), _p(d_hist_prev),
                                                       _p(d_moments_prev), _p(d_hist_out), _p(d_moments_out), _p(d_variance_out), _p(stream)), "mi355rt_svgf_accumulate")

    def filter(self, width, height, d_hist_in, d_variance_in, d_hits, d_scratch, d_out_linear=None, d_out_packed=None, params=None, hip_device=0, stream=None):
        """mi355rt_svgf_filter: the a-trous filter whose colour weight follows the variance, enqueued on `stream` of `hip_device`.  Integer device
        addresses: d_hist_in width * height float4 (accumulate's d_hist_out), d_variance_in as many floats, d_hits this frame's abi.Hit records, d_scratch
        scratch_bytes(width, height) bytes; d_out_linear (width * height * 3 floats) and / or d_out_packed (0x00RRGGBB words).  params: abi.SvgfFilterParams
        or None for the defaults."""
        self._check(self.lib().mi355rt_svgf_filter(int(hip_device), int(width), int(height), _ref(params), _p(d_hist_in), _p(d_variance_in), _p(d_hits), _p(d_scratch),
                                                   _p(d_out_linear), _p(d_out_packed), _p(stream)), "mi355rt_svgf_filter")


def open_library(path):
    """The call wrappers bound to the library file `path` (lib, scratch_bytes, accumulate, filter, RenderError, as this module's)."""
    return Library(path)


_product = Library(build.SVGF_SO)
lib, scratch_bytes, accumulate, filter = _product.lib, _product.scratch_bytes, _product.accumulate, _product.filter
