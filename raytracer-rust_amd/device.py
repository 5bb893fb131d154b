"""ctypes binding of libmi355rt.so -- the HIP path behind the C ABI (include/mi355rt.h).

There is no CPU fallback: `lib()` raises if the HIP library has not been built, and every render call
raises if no GPU is visible.  torch is NOT needed here; callers that hold torch tensors pass
`tensor.data_ptr()` and `torch.cuda.current_stream().cuda_stream`.
"""
import collections
import ctypes as C
import os

import numpy as np

from . import abi, build

EXPORTS = ["mi355rt_render", "mi355rt_render_multi", "mi355rt_render_progressive", "mi355rt_context_create", "mi355rt_context_destroy", "mi355rt_context_set_scene",
           "mi355rt_rows_selected", "mi355rt_context_render", "mi355rt_context_render_progressive", "mi355rt_context_set_timing", "mi355rt_context_read_timing",
           "mi355rt_context_check", "mi355rt_context_set_share", "mi355rt_last_error", "mi355rt_abi_version",
           "mi355rt_multi_context_create", "mi355rt_multi_context_destroy", "mi355rt_multi_context_set_scene", "mi355rt_multi_context_render",
           "mi355rt_multi_context_check", "mi355rt_multi_context_render_progressive", "mi355rt_render_progressive_multi",
           "mi355rt_context_trace_rays", "mi355rt_context_first_hits", "mi355rt_trace_rays",
           "mi355rt_denoise_scratch_bytes", "mi355rt_context_denoise", "mi355rt_denoise",
           "mi355rt_context_occluded", "mi355rt_occluded", "mi355rt_context_ambient_occlusion",
           "mi355rt_radiance_scratch_bytes", "mi355rt_context_trace_radiance", "mi355rt_trace_radiance",
           "mi355rt_view_scratch_bytes", "mi355rt_context_view_rays", "mi355rt_context_render_view",
           "mi355rt_context_probe_rays", "mi355rt_context_probe_radiance",
           "mi355rt_noise_device_create", "mi355rt_noise_device_destroy", "mi355rt_noise_device_reset", "mi355rt_noise_device_update",
           "mi355rt_noise_device_evaluate"]

_lib = None
_extra = {}


def load(so):
    """Bind another build of the device library (diagnostic / reference builds; the product path uses lib())."""
    so = os.path.abspath(so)
    if so not in _extra:
        _extra[so] = _bind(so)
    return _extra[so]


def refs():
    """The tests' reference build: the product sources plus the retired mesh kernel (the state machine), mi355rt_debug_stages and the
    resolve / gather probe (mi355rt_debug_resolve, mi355rt_debug_gather) and the generator probe (mi355rt_debug_rng_block) and the wave probe of the bounce (mi355rt_debug_scatter_wave), -DMI355RT_REFS."""
    L = load(build.build_device_variant("refs", ["MI355RT_REFS"]))
    L.mi355rt_debug_stages.restype = C.c_int
    L.mi355rt_debug_stages.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.mi355rt_debug_resolve.restype = C.c_int
    L.mi355rt_debug_resolve.argtypes = [C.c_void_p]
    L.mi355rt_debug_resolve_masked.restype = C.c_int
    L.mi355rt_debug_resolve_masked.argtypes = [C.c_void_p]
    L.mi355rt_debug_gather.restype = C.c_int
    L.mi355rt_debug_gather.argtypes = [C.c_void_p]
    L.mi355rt_debug_rng_block.restype = C.c_int
    L.mi355rt_debug_rng_block.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_int]
    L.mi355rt_debug_scatter_wave.restype = C.c_int
    L.mi355rt_debug_scatter_wave.argtypes = [C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int]
    L.mi355rt_debug_range_wave.restype = C.c_int
    L.mi355rt_debug_range_wave.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint32), C.c_int]
    L.mi355rt_debug_scatter_wave_form.restype = C.c_int
    L.mi355rt_debug_scatter_wave_form.argtypes = [C.c_uint32, C.c_void_p, C.POINTER(C.c_char_p)]
    return L


# mi355rt_debug_resolve / mi355rt_debug_gather (csrc/refs/rt_resolve_probe.hip): the shipped launch_resolve, launch_gather_strips and
# launch_gather_accum on the caller's device buffers.  Every pointer is a device address of the current device (torch: tensor.data_ptr()),
# 0 = null; the caller sizes the buffers.
class ResolveProbeArgs(C.Structure):
    _fields_ = [("radiance", C.c_uint64), ("out_packed", C.c_uint64), ("out_linear", C.c_uint64), ("accum", C.c_uint64), ("out_row", C.c_uint64),
                ("accum_load", C.c_uint32), ("band_pixel0", C.c_uint32), ("band_pixels", C.c_uint32), ("spp", C.c_uint32),
                ("inv_spp", C.c_float), ("width", C.c_uint32)]


class ResolveMaskedProbeArgs(C.Structure):
    _fields_ = [("plain", ResolveProbeArgs), ("cam_mask", C.c_uint64), ("miss", C.c_float * 3), ("pad", C.c_uint32)]


class GatherProbeArgs(C.Structure):
    _fields_ = [("src_row", C.c_uint64), ("src_packed", C.c_uint64), ("dst_packed", C.c_uint64), ("src_linear", C.c_uint64), ("dst_linear", C.c_uint64),
                ("accum_src", C.c_uint64), ("accum_dst", C.c_uint64), ("n_rows", C.c_uint32), ("width", C.c_uint32)]


def debug_resolve(radiance, out_packed, spp, inv_spp, band_pixels, band_pixel0=0, out_linear=0, accum=0, accum_load=False, out_row=0, width=0):
    """Diagnostic (reference build): one k_resolve launch through launch_resolve, waited for.  radiance: 3 * spp * band_pixels floats, the
    band's samples; the outputs are indexed by band_pixel0 + p, or through out_row (processing row -> output row of an image `width` wide)."""
    a = ResolveProbeArgs(int(radiance), int(out_packed), int(out_linear), int(accum), int(out_row), 1 if accum_load else 0,
                         int(band_pixel0), int(band_pixels), int(spp), float(inv_spp), int(width))
    L = refs()
    _check(L.mi355rt_debug_resolve(C.addressof(a)), "mi355rt_debug_resolve", L)


def debug_resolve_masked(radiance, out_packed, spp, inv_spp, band_pixels, cam_mask, miss, band_pixel0=0, out_linear=0, accum=0, accum_load=False,
                         out_row=0, width=0):
    """Diagnostic (reference build): debug_resolve with the band's camera-mask words (cam_mask: band_pixels uint32 on the device, 0 = no
    table) and the miss colour (three floats): a pixel whose word is 0 is resolved from `miss` and its samples are not read."""
    a = ResolveMaskedProbeArgs(ResolveProbeArgs(int(radiance), int(out_packed), int(out_linear), int(accum), int(out_row), 1 if accum_load else 0,
                                                int(band_pixel0), int(band_pixels), int(spp), float(inv_spp), int(width)),
                               int(cam_mask), (C.c_float * 3)(*[float(m) for m in miss]), 0)
    L = refs()
    _check(L.mi355rt_debug_resolve_masked(C.addressof(a)), "mi355rt_debug_resolve_masked", L)


def debug_gather(src_row, n_rows, width, src_packed=0, dst_packed=0, src_linear=0, dst_linear=0, accum_src=0, accum_dst=0):
    """Diagnostic (reference build): k_gather_strips (src_packed given) and / or k_gather_accum (accum_src given) through their launchers,
    waited for.  Output row r is staging row src_row[r]."""
    a = GatherProbeArgs(int(src_row), int(src_packed), int(dst_packed), int(src_linear), int(dst_linear), int(accum_src), int(accum_dst),
                        int(n_rows), int(width))
    L = refs()
    _check(L.mi355rt_debug_gather(C.addressof(a)), "mi355rt_debug_gather", L)


def debug_rng_block(records, hip_device=0):
    """Diagnostic (reference build, csrc/refs/rt_rng_probe.hip): one block of the counter-mode generator per record.  records: uint32 [n, 6] =
    (key lo, key hi, x, sample, ray, try).  Returns uint32 [n, 3, 4]: the block through the plain draw address, through the stepped one
    (set_ray + next_event, the full multiply for the try) and through the stepped form's running word (unit_ball_cooperative's arithmetic)."""
    L = refs()
    rec = np.ascontiguousarray(records, np.uint32).reshape(-1, 6)
    out = np.zeros((rec.shape[0], 3, 4), np.uint32)
    _check(L.mi355rt_debug_rng_block(rec.ctypes.data, rec.shape[0], out.ctypes.data, hip_device), "mi355rt_debug_rng_block", L)
    return out


WAVE_LIVE = 0x100            # flags word of a wave-probe record: bit 0 front face, bit 8 live (csrc/refs/rt_scatter_wave_probe.h)


def scatter_wave_forms():
    """Diagnostic (reference build, csrc/refs/rt_scatter_wave_probe.h): the forms of the bounce the library launches, in the probe's order.
    A list of dicts: kernel (the kernel the form belongs to), mats (bit k: material kind k), wide, fastn, try1, terminal_done, stepped, in_place.
    Needs no GPU."""
    L = refs()
    forms, count, i = [], 1, 0
    while i < count:
        w = np.zeros(8, np.uint32)
        name = C.c_char_p()
        _check(L.mi355rt_debug_scatter_wave_form(i, w.ctypes.data, C.byref(name)), "mi355rt_debug_scatter_wave_form", L)
        count = int(w[7])
        forms.append(dict(kernel=name.value.decode(), mats=int(w[0]), wide=bool(w[1]), fastn=bool(w[2]), try1=int(w[3]), terminal_done=bool(w[4]),
                          stepped=bool(w[5]), in_place=bool(w[6])))
        i += 1
    return forms


def debug_scatter_wave(form, materials, records, hip_device=0):
    """Diagnostic (reference build): one scatter event per lane through the shipped pieces of the bounce -- scatter_pre, unit_ball_cooperative,
    ball_finish, scatter_origin, ray_direction -- with the template arguments of form `form` (scatter_wave_forms()).  materials: ctypes array
    of abi.Material; records: uint32 [n, 16] = (material, flags, direction[3], position[3], normal[3] as float bits, k0, k1, x, sample, ray),
    64 to a wave in the order given; an idle lane (flags without WAVE_LIVE) passes false to the cooperative draw and its generator words are
    the record's (k0, k1, x, sample).  Returns uint32 [n, 16]: the float bits of scattered, origin[3], direction[3], attenuation[3],
    emitted[3] and the accepted unit-ball point[3]; what a lane did not produce is +0."""
    L = refs()
    rec = np.ascontiguousarray(records, np.uint32).reshape(-1, 16)
    out = np.zeros((rec.shape[0], 16), np.uint32)
    _check(L.mi355rt_debug_scatter_wave(int(form), materials, len(materials), rec.ctypes.data, rec.shape[0], out.ctypes.data, hip_device),
           "mi355rt_debug_scatter_wave", L)
    return out


def debug_range_wave(selector, quad_d, cube_d, records, hip_device=0):
    """Diagnostic (reference build): k_render_ctr_simple_qc's range arithmetic on caller-chosen waves (csrc/refs/rt_range_wave_probe.h).  selector 0:
    the guarded forms, 1: the RANGE bits the library ships, 2: all four steps.  quad_d: float32 [16], cube_d: float32 [28] (the words of DevPrim::d the
    two hit tests read); records: uint32 [n, 16] = (raw direction[3], origin[3] as float bits, flags: bit 0 active), 64 to a wave.  Returns (uint32
    [n, 16]: the float bits of normalized_ranged[3], ray_direction[3], quad hit, quad t, cube hit, cube t, cube po[3], then quad idx, cube idx, 0;
    the RANGE bits behind the selector)."""
    L = refs()
    q, c = np.ascontiguousarray(quad_d, np.float32), np.ascontiguousarray(cube_d, np.float32)
    assert q.shape == (16,) and c.shape == (28,)
    rec = np.ascontiguousarray(records, np.uint32).reshape(-1, 16)
    out = np.zeros((rec.shape[0], 16), np.uint32)
    bits = C.c_uint32()
    _check(L.mi355rt_debug_range_wave(int(selector), q.ctypes.data, c.ctypes.data, rec.ctypes.data, rec.shape[0], out.ctypes.data, C.byref(bits), hip_device),
           "mi355rt_debug_range_wave", L)
    return out, int(bits.value)


def debug_scatter_records(materials, records, hip_device=0):
    """debug_scatter on packed records: uint32 [n, 16] = (material, front face, direction[3], position[3], normal[3] as float bits, k0, k1, x,
    sample, ray).  Returns uint32 [n, 16]: the float bits of scattered, origin[3], direction[3], attenuation[3], emitted[3], then three zero words."""
    sc = abi.Scene()
    sc.materials, sc.n_materials = materials, len(materials)
    sc.miss_color[:] = (0.5, 0.5, 0.5)
    rec = np.ascontiguousarray(records, np.uint32).reshape(-1, 16)
    out = np.zeros((rec.shape[0], 16), np.uint32)
    ctx = Context(hip_device)
    try:
        ctx.set_scene(sc, abi.Camera(), abi.Settings(1, 1, 1, 1))
        _check(lib().mi355rt_debug_scatter(ctx._h, C.c_void_p(rec.ctypes.data), rec.shape[0], C.c_void_p(out.ctypes.data)), "mi355rt_debug_scatter")
        return out
    finally:
        ctx.close()


# mi355rt_debug_stages (csrc/refs/rt_stages.hip; the oracle's twin is oracle_debug_stages): stage numbers and the argument record
STAGES = {"lattice": 0, "half": 1, "acos": 2, "atan2": 3, "tex": 4, "sky": 5, "atan2_exact": 6, "fmod_exact": 7}


class StageArgs(C.Structure):
    _fields_ = [("stage", C.c_uint32), ("form", C.c_uint32), ("first", C.c_uint64), ("stride", C.c_uint64),
                ("ggx", C.c_uint32), ("axis", C.c_uint32), ("set", C.c_uint32), ("img_w", C.c_uint32), ("img_h", C.c_uint32), ("pad0", C.c_uint32),
                ("rough", C.c_float), ("fixed_u", C.c_float), ("h_offset", C.c_float), ("pad1", C.c_float),
                ("n", C.c_float * 4), ("rd", C.c_float * 4)]


def stage_words(stage):
    """Words per element of a stage's output (0: the exact stages, which return 3 words per call)."""
    return 1 if stage in (2, 3) else (0 if stage >= 6 else 8)


def _ptr(a):
    return None if a is None else a.ctypes.data


def debug_stages(args, n, in4=None, mat=None, tex_rgba=None, sky=None, hip_device=0):
    """Diagnostic (reference build): stage `args.stage` on n elements on the device.  in4: float32 [n, 4] explicit inputs or None; mat: an
    abi.Material (HALF); tex_rgba: uint32 [img_h, img_w] texels (TEX); sky: float32 [img_h, img_w, 3] (SKY).  Returns uint32 [n, words], or
    uint32 [3] for the exact stages (mismatches, the smallest mismatching index, results one f32 step off on atan2's diagonal)."""
    L = refs()
    W = stage_words(args.stage)
    out = np.zeros(n * W if W else 3, np.uint32)
    in4 = None if in4 is None else np.ascontiguousarray(in4, np.float32)
    tex_rgba = None if tex_rgba is None else np.ascontiguousarray(tex_rgba, np.uint32)
    sky = None if sky is None else np.ascontiguousarray(sky, np.float32)
    _check(L.mi355rt_debug_stages(C.addressof(args), n, _ptr(in4), C.addressof(mat) if mat is not None else None, _ptr(tex_rgba), _ptr(sky),
                                  out.ctypes.data, hip_device), "mi355rt_debug_stages", L)
    return out.reshape(n, W) if W else out


def lib():
    global _lib
    if _lib is None:
        _lib = _bind(os.environ.get("MI355RT_DEVICE_SO", build.DEVICE_SO))     # override: diagnostic builds only (tools/)
    return _lib


def _bind(so):
    if True:
        if not os.path.exists(so):
            raise RuntimeError(f"{so} is missing: the HIP extension must be built "
                               "(__graft_entry__.build()); there is no CPU fallback")
        L = C.CDLL(so)
        L.mi355rt_last_error.restype = C.c_char_p
        L.mi355rt_abi_version.restype = C.c_uint32
        L.mi355rt_render.restype = C.c_int
        L.mi355rt_render.argtypes = [C.POINTER(abi.Scene), C.POINTER(abi.Camera), C.POINTER(abi.Settings),
                                     C.POINTER(abi.Options), C.c_void_p, C.c_void_p, C.POINTER(abi.Stats)]
        L.mi355rt_render_multi.restype = C.c_int
        L.mi355rt_render_multi.argtypes = [C.POINTER(abi.Scene), C.POINTER(abi.Camera), C.POINTER(abi.Settings), C.POINTER(abi.Options),
                                           C.POINTER(C.c_int), C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(abi.Stats)]
        L.mi355rt_context_create.restype = C.c_int
        L.mi355rt_context_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        L.mi355rt_context_destroy.argtypes = [C.c_void_p]
        L.mi355rt_context_set_scene.restype = C.c_int
        L.mi355rt_context_set_scene.argtypes = [C.c_void_p, C.POINTER(abi.Scene), C.POINTER(abi.Camera), C.POINTER(abi.Settings)]
        L.mi355rt_rows_selected.restype = C.c_int
        L.mi355rt_rows_selected.argtypes = [C.POINTER(abi.Settings), C.POINTER(abi.Options), C.POINTER(C.c_uint32)]
        L.mi355rt_context_render.restype = C.c_int
        L.mi355rt_context_render.argtypes = [C.c_void_p, C.POINTER(abi.Options), C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.POINTER(abi.Stats)]
        L.mi355rt_context_render_progressive.restype = C.c_int
        L.mi355rt_context_render_progressive.argtypes = [C.c_void_p, C.POINTER(abi.Options), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                                         C.c_void_p, C.c_void_p, C.POINTER(abi.Stats)]
        L.mi355rt_context_set_timing.restype = C.c_int
        L.mi355rt_context_set_timing.argtypes = [C.c_void_p, C.c_int]
        L.mi355rt_context_read_timing.restype = C.c_int
        L.mi355rt_context_read_timing.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint32)]
        L.mi355rt_context_check.restype = C.c_int
        L.mi355rt_context_check.argtypes = [C.c_void_p]
        L.mi355rt_context_set_share.restype = C.c_int
        L.mi355rt_context_set_share.argtypes = [C.c_void_p, C.c_uint32]
        L.mi355rt_multi_context_create.restype = C.c_int
        L.mi355rt_multi_context_create.argtypes = [C.POINTER(C.c_int), C.c_uint32, C.POINTER(C.c_void_p)]
        L.mi355rt_multi_context_destroy.restype = None
        L.mi355rt_multi_context_destroy.argtypes = [C.c_void_p]
        L.mi355rt_multi_context_set_scene.restype = C.c_int
        L.mi355rt_multi_context_set_scene.argtypes = [C.c_void_p, C.POINTER(abi.Scene), C.POINTER(abi.Camera), C.POINTER(abi.Settings)]
        L.mi355rt_multi_context_render.restype = C.c_int
        L.mi355rt_multi_context_render.argtypes = [C.c_void_p, C.POINTER(abi.Options), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(abi.Stats)]
        L.mi355rt_multi_context_check.restype = C.c_int
        L.mi355rt_multi_context_check.argtypes = [C.c_void_p]
        L.mi355rt_multi_context_render_progressive.restype = C.c_int
        L.mi355rt_multi_context_render_progressive.argtypes = [C.c_void_p, C.POINTER(abi.Options), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                                               C.c_void_p, C.c_void_p, C.POINTER(abi.Stats)]
        L.mi355rt_render_progressive_multi.restype = C.c_int
        L.mi355rt_render_progressive_multi.argtypes = [C.POINTER(abi.Scene), C.POINTER(abi.Camera), C.POINTER(abi.Settings), C.POINTER(abi.Options),
                                                       C.POINTER(C.c_int), C.c_uint32, C.c_uint32, abi.ProgressFn, C.c_void_p,
                                                       C.c_void_p, C.c_void_p, C.POINTER(abi.Stats)]
        L.mi355rt_context_trace_rays.restype = C.c_int
        L.mi355rt_context_trace_rays.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        L.mi355rt_context_first_hits.restype = C.c_int
        L.mi355rt_context_first_hits.argtypes = [C.c_void_p, C.POINTER(abi.Options), C.c_void_p, C.c_void_p]
        L.mi355rt_trace_rays.restype = C.c_int
        L.mi355rt_trace_rays.argtypes = [C.POINTER(abi.Scene), C.c_void_p, C.c_uint32, C.c_void_p]
        L.mi355rt_denoise_scratch_bytes.restype = C.c_int
        L.mi355rt_denoise_scratch_bytes.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]
        L.mi355rt_context_denoise.restype = C.c_int
        L.mi355rt_context_denoise.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(abi.DenoiseParams), C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_void_p]
        L.mi355rt_denoise.restype = C.c_int
        L.mi355rt_denoise.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(abi.DenoiseParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mi355rt_context_occluded.restype = C.c_int
        L.mi355rt_context_occluded.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        L.mi355rt_occluded.restype = C.c_int
        L.mi355rt_occluded.argtypes = [C.POINTER(abi.Scene), C.c_void_p, C.c_uint32, C.c_void_p]
        L.mi355rt_context_ambient_occlusion.restype = C.c_int
        L.mi355rt_context_ambient_occlusion.argtypes = [C.c_void_p, C.POINTER(abi.Options), C.POINTER(abi.AoParams), C.c_void_p, C.c_void_p, C.c_void_p]
        L.mi355rt_radiance_scratch_bytes.restype = C.c_int
        L.mi355rt_radiance_scratch_bytes.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]
        L.mi355rt_context_trace_radiance.restype = C.c_int
        L.mi355rt_context_trace_radiance.argtypes = [C.c_void_p, C.POINTER(abi.RadianceParams), C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mi355rt_trace_radiance.restype = C.c_int
        L.mi355rt_trace_radiance.argtypes = [C.POINTER(abi.Scene), C.POINTER(abi.RadianceParams), C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        L.mi355rt_view_scratch_bytes.restype = C.c_int
        L.mi355rt_view_scratch_bytes.argtypes = [C.POINTER(abi.View), C.c_uint32, C.POINTER(C.c_uint64)]
        L.mi355rt_context_view_rays.restype = C.c_int
        L.mi355rt_context_view_rays.argtypes = [C.c_void_p, C.POINTER(abi.View), C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p]
        L.mi355rt_context_render_view.restype = C.c_int
        L.mi355rt_context_render_view.argtypes = [C.c_void_p, C.POINTER(abi.View), C.POINTER(abi.RadianceParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mi355rt_context_probe_rays.restype = C.c_int
        L.mi355rt_context_probe_rays.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p]
        L.mi355rt_context_probe_radiance.restype = C.c_int
        L.mi355rt_context_probe_radiance.argtypes = [C.c_void_p, C.POINTER(abi.RadianceParams), C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mi355rt_noise_device_create.restype = C.c_int
        L.mi355rt_noise_device_create.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]
        L.mi355rt_noise_device_destroy.restype = None
        L.mi355rt_noise_device_destroy.argtypes = [C.c_void_p]
        L.mi355rt_noise_device_reset.restype = C.c_int
        L.mi355rt_noise_device_reset.argtypes = [C.c_void_p, C.c_void_p]
        L.mi355rt_noise_device_update.restype = C.c_int
        L.mi355rt_noise_device_update.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        L.mi355rt_noise_device_evaluate.restype = C.c_int
        L.mi355rt_noise_device_evaluate.argtypes = [C.c_void_p, C.POINTER(abi.NoiseParams), C.c_void_p, C.c_void_p, C.c_void_p]
        L.mi355rt_debug_multi_part_ms.restype = C.c_int
        L.mi355rt_debug_multi_part_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_uint32, C.POINTER(C.c_uint32)]
        L.mi355rt_debug_set_knob.restype = C.c_int
        L.mi355rt_debug_set_knob.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
        L.mi355rt_debug_has_variant.restype = C.c_int
        L.mi355rt_debug_has_variant.argtypes = [C.c_uint32]
        L.mi355rt_debug_prepare_scene.restype = C.c_int
        L.mi355rt_debug_prepare_scene.argtypes = [C.POINTER(abi.Scene), C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                                  C.c_void_p, C.POINTER(C.c_uint32), C.c_void_p, C.POINTER(C.c_uint32), C.c_void_p, C.POINTER(C.c_uint32)]
        L.mi355rt_debug_camera_masks.restype = C.c_int
        L.mi355rt_debug_camera_masks.argtypes = [C.POINTER(abi.Scene), C.POINTER(abi.Camera), C.POINTER(abi.Settings), C.POINTER(abi.Options), C.c_int,
                                                 C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        L.mi355rt_debug_plan_render.restype = C.c_int
        L.mi355rt_debug_plan_render.argtypes = [C.POINTER(abi.Settings), C.POINTER(abi.Options), C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p,
                                                C.POINTER(C.c_uint32), C.c_void_p, C.POINTER(C.c_uint32), C.c_void_p, C.POINTER(C.c_uint32)]
        if L.mi355rt_abi_version() != abi.ABI_VERSION:
            raise RuntimeError("libmi355rt.so ABI version does not match abi.py")
    return L


class RenderError(RuntimeError):
    def __init__(self, what, rc, library=None):
        super().__init__(f"{what} failed ({rc}): {(library or lib()).mi355rt_last_error().decode()}")
        self.rc = rc


def _check(rc, what, library=None):
    if rc != 0:
        raise RenderError(what, rc, library)


def set_knob(name, value, library=None):
    """Diagnostic: process-wide default knob for every context created afterwards (also inside the one-shot calls).
    Knobs: kernel, guided_mult, spin_idle, spin_entry, wave_times, row_order, cam_cull, resolve_skip, denoise_staged, ao_form, radiance_items, inline_steps, trav_min (rt_debug.cpp)."""
    L = library or lib()
    _check(L.mi355rt_debug_set_knob(None, name.encode(), int(value)), f"mi355rt_debug_set_knob({name})", L)


def clear_knobs(library=None):
    L = library or lib()
    _check(L.mi355rt_debug_set_knob(None, None, 0), "mi355rt_debug_set_knob(clear)", L)


# The device-resident records of rt_device.h (DevPrim, DevNode, DevTri), as prepare_scene() returns them.
PRIM_DTYPE = np.dtype([("kind", "<u4"), ("material", "<u4"), ("node_begin", "<u4"), ("run_end", "<u4"), ("d", "<f4", 52), ("mat0", "<f4", 4)])
NODE_DTYPE = np.dtype([("bmin", "<f4", 3), ("a", "<u4"), ("bmax", "<f4", 3), ("b", "<u4")])
TRI_DTYPE = np.dtype([("v0", "<f4", 3), ("e1", "<f4", 3), ("e2", "<f4", 3), ("n", "<f4", 3)])
Prepared = collections.namedtuple("Prepared", "variant inline_steps prims nodes tris")


def prepare_scene(scene, forced_variant=-1, library=None):
    """Diagnostic (mi355rt_debug_prepare_scene): what set_scene would upload and choose for `scene` -- validation, the re-laid BVH, the
    primitive records, the kernel variant (forced_variant: the "kernel" knob) and inline_steps.  No GPU and no context are needed.
    Returns Prepared(variant, inline_steps, prims [PRIM_DTYPE], nodes [NODE_DTYPE], tris [TRI_DTYPE]); raises RenderError on a refusal."""
    L = library or lib()
    sc = getattr(scene, "c", scene)
    variant, inline_steps, n_prims, n_nodes, n_tris = (C.c_uint32() for _ in range(5))
    _check(L.mi355rt_debug_prepare_scene(C.byref(sc), int(forced_variant), C.byref(variant), C.byref(inline_steps), None, C.byref(n_prims),
                                         None, C.byref(n_nodes), None, C.byref(n_tris)), "mi355rt_debug_prepare_scene", L)
    prims, nodes, tris = np.zeros(n_prims.value, PRIM_DTYPE), np.zeros(n_nodes.value, NODE_DTYPE), np.zeros(n_tris.value, TRI_DTYPE)
    _check(L.mi355rt_debug_prepare_scene(C.byref(sc), int(forced_variant), C.byref(variant), C.byref(inline_steps), prims.ctypes.data, C.byref(n_prims),
                                         nodes.ctypes.data, C.byref(n_nodes), tris.ctypes.data, C.byref(n_tris)), "mi355rt_debug_prepare_scene", L)
    return Prepared(variant.value, inline_steps.value, prims, nodes, tris)


def entry_kernel(variant, has_sky, library=None):
    """Diagnostic (mi355rt_debug_entry_kernel): the name of the kernel a scene on `variant` is launched on, with or without a sky texture.  One
    kernel per variant, except 14: k_render_ctr_simple_qc is compiled without the sky lookup, scenes with a texture run k_render_sky_simple_qc.
    No GPU and no context are needed."""
    L = library or lib()
    f = L.mi355rt_debug_entry_kernel
    f.restype = C.c_char_p
    f.argtypes = [C.c_uint32, C.c_int]
    name = f(int(variant), 1 if has_sky else 0)
    return None if name is None else name.decode()


def camera_masks(scene, camera, settings, options=None, forced_variant=-1, library=None):
    """Diagnostic (mi355rt_debug_camera_masks): the per-pixel primitive masks set_scene builds for the camera pass of k_render_ctr_simple_qc -- bit i
    of a pixel's word set = a camera ray of that pixel may hit primitive i.  No GPU and no context are needed.  Without options: uint32
    [height, width], the image's table; with options: uint32 [rows, width], the table a render with those options reads (its selected rows).
    None when the scene gets no table (more than 32 primitives, or another kernel serves it)."""
    L = library or lib()
    sc = getattr(scene, "c", scene)
    n = C.c_uint64()
    opt = C.byref(options) if options is not None else None
    _check(L.mi355rt_debug_camera_masks(C.byref(sc), C.byref(camera), C.byref(settings), opt, int(forced_variant), None, 0, C.byref(n)),
           "mi355rt_debug_camera_masks", L)
    if n.value == 0:
        return None
    out = np.zeros(n.value, np.uint32)
    _check(L.mi355rt_debug_camera_masks(C.byref(sc), C.byref(camera), C.byref(settings), opt, int(forced_variant), out.ctypes.data, out.size, C.byref(n)),
           "mi355rt_debug_camera_masks", L)
    return out.reshape(-1, settings.width)


KERNEL_VARIANTS, WORK_SHARDS = 15, 8                                  # rt_device.h


class PlanProbeArgs(C.Structure):                                     # the context's side of a render's inputs (rt_debug.cpp PlanProbeArgs)
    _fields_ = [(n, C.c_uint32) for n in ("s0", "s1", "have_accum", "variant", "has_mesh", "n_prims", "row_probe", "grid_div", "guided_mult")] + \
               [("block_slots", C.c_uint32 * KERNEL_VARIANTS)]


class RenderPlan(C.Structure):                                        # rt_prepare.h RenderPlan
    _fields_ = [(n, C.c_uint64) for n in ("seed", "total_pixels", "band_pixels")] + \
               [(n, C.c_uint32) for n in ("rng_mode", "fixed_aabb", "variant", "order_groups", "spp", "n_bands", "block_threads")] + \
               [(n, C.c_float) for n in ("width_f", "height_f", "inv_width_rn", "inv_height_rn", "inv_spp")] + \
               [(n, C.c_uint32) for n in ("spp_mul", "spp_shift", "width_mul", "width_shift", "accum_load", "sample0", "seed_lo", "seed_hi",
                                          "width", "resident", "guided_mult", "row_probe")]


BAND_DTYPE = np.dtype([(n, "<u4") for n in ("band_pixel0", "band_pixels", "band_samples", "shard_samples", "grid", "guided_div")])   # rt_prepare.h RenderBand
Planned = collections.namedtuple("Planned", "plan halved bands natural processing out_row")


def plan_render(settings, options=None, s0=0, s1=None, have_accum=False, variant=0, has_mesh=False, n_prims=1, row_cost=None, row_probe=False,
                block_slots=512, grid_div=1, guided_mult=16, halvings=0, library=None):
    """Diagnostic (mi355rt_debug_plan_render): what Context.render / render_progressive with these inputs would launch -- the plan_render, halve_bands,
    render_band and row_tables of the render call itself.  No GPU and no context are needed.  s1 None: settings.samples_per_pixel; block_slots: the
    workgroups the device holds of each variant (one number for all, or KERNEL_VARIANTS of them); row_cost: a cost per image row (the processing
    order); halvings: "the band did not fit" steps taken first.  Returns Planned(plan: RenderPlan, halved: steps that existed, bands [BAND_DTYPE],
    natural, processing, out_row: the three row tables); raises RenderError on a refusal."""
    L = library or lib()
    slots = [int(block_slots)] * KERNEL_VARIANTS if np.isscalar(block_slots) else [int(v) for v in block_slots]
    a = PlanProbeArgs(int(s0), int(settings.samples_per_pixel if s1 is None else s1), int(bool(have_accum)), int(variant), int(bool(has_mesh)), int(n_prims),
                      int(bool(row_probe)), int(grid_div), int(guided_mult), (C.c_uint32 * KERNEL_VARIANTS)(*slots))
    cost = np.zeros(0, np.float32) if row_cost is None else np.ascontiguousarray(row_cost, np.float32)
    opt = C.byref(options) if options is not None else None
    plan, halved, n_bands, n_rows = RenderPlan(), C.c_uint32(), C.c_uint32(), C.c_uint32()

    def call(bands, tables):
        _check(L.mi355rt_debug_plan_render(C.byref(settings), opt, C.addressof(a), cost.ctypes.data if cost.size else None, cost.size, int(halvings),
                                           C.addressof(plan), C.byref(halved), bands, C.byref(n_bands), tables, C.byref(n_rows)), "mi355rt_debug_plan_render", L)

    call(None, None)
    bands, t = np.zeros(n_bands.value, BAND_DTYPE), np.zeros(3 * n_rows.value, np.uint32)
    call(bands.ctypes.data, t.ctypes.data)
    n = n_rows.value
    return Planned(plan, halved.value, bands, t[:n], t[n:2 * n], t[2 * n:])


def render(scene, camera, settings, options=None, want_linear=True, want_stats=True, library=None):
    """One-shot mi355rt_render with host buffers (what src/main.rs:57 would call).
    Returns (packed u32 [rows, W], linear f32 [rows, W, 3] or None, abi.Stats or None)."""
    L = library or lib()
    sc = getattr(scene, "c", scene)
    rows = len(abi.rows_selected(settings.height, options))
    W = settings.width
    packed = np.zeros((rows, W), np.uint32)
    linear = np.zeros((rows, W, 3), np.float32) if want_linear else None
    stats = abi.Stats() if want_stats else None
    _check(L.mi355rt_render(C.byref(sc), C.byref(camera), C.byref(settings),
                            C.byref(options) if options is not None else None,
                            packed.ctypes.data, linear.ctypes.data if want_linear else None,
                            C.byref(stats) if want_stats else None), "mi355rt_render", L)
    return packed, linear, stats


def render_multi(scene, camera, settings, devices, options=None, want_linear=True, library=None):
    """mi355rt_render_multi: one process, the listed HIP devices (a device may repeat).  Same returns as render()."""
    sc = getattr(scene, "c", scene)
    rows = len(abi.rows_selected(settings.height, options)) if options is not None else settings.height
    packed = np.zeros((rows, settings.width), np.uint32)
    linear = np.zeros((rows, settings.width, 3), np.float32) if want_linear else None
    stats = abi.Stats()
    devs = (C.c_int * len(devices))(*devices)
    L = library or lib()
    _check(L.mi355rt_render_multi(C.byref(sc), C.byref(camera), C.byref(settings), C.byref(options) if options is not None else None,
                                  devs, len(devices), packed.ctypes.data, linear.ctypes.data if want_linear else None, C.byref(stats)),
           "mi355rt_render_multi", L)
    return packed, linear, stats


def render_progressive_multi(scene, camera, settings, devices, chunk_spp, on_chunk=None, options=None, want_linear=True, library=None):
    """mi355rt_render_progressive_multi: mi355rt_render_multi in chunks of `chunk_spp` samples (the last one may be shorter).  After every
    chunk `on_chunk(samples_done, samples_total, packed)` sees the image so far (packed: uint32 [rows, W], a view of the result buffer that
    the next chunk overwrites -- copy it to keep it); a truthy return stops early and leaves the image of `samples_done` samples.
    Same returns as render_multi()."""
    sc = getattr(scene, "c", scene)
    rows = len(abi.rows_selected(settings.height, options)) if options is not None else settings.height
    packed = np.zeros((rows, settings.width), np.uint32)
    linear = np.zeros((rows, settings.width, 3), np.float32) if want_linear else None
    stats = abi.Stats()
    devs = (C.c_int * max(len(devices), 1))(*devices)
    raised = []

    def _cb(user, done, total, _ptr):
        try:
            return 1 if on_chunk(int(done), int(total), packed) else 0
        except BaseException as e:                                         # never unwind through the C frames: stop, re-raise below
            raised.append(e)
            return 1

    cb = abi.ProgressFn(_cb) if on_chunk is not None else abi.ProgressFn()
    L = library or lib()
    rc = L.mi355rt_render_progressive_multi(C.byref(sc), C.byref(camera), C.byref(settings), C.byref(options) if options is not None else None,
                                            devs, len(devices), int(chunk_spp), cb, None, packed.ctypes.data,
                                            linear.ctypes.data if want_linear else None, C.byref(stats))
    if raised:
        raise raised[0]
    _check(rc, "mi355rt_render_progressive_multi", L)
    return packed, linear, stats


def trace_rays(scene, rays, library=None):
    """One-shot mi355rt_trace_rays with host buffers: the closest hit of every ray in `scene`.  rays: a numpy array of abi.RAY_DTYPE (or
    float32 [n, 8]: origin, pad, direction, pad; the directions need not be unit).  Returns an array of abi.HIT_DTYPE, one record per ray."""
    L = library or lib()
    sc = getattr(scene, "c", scene)
    rays = np.ascontiguousarray(rays)
    if rays.dtype != abi.RAY_DTYPE:
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8).view(abi.RAY_DTYPE).reshape(-1)
    hits = np.zeros(rays.size, abi.HIT_DTYPE)
    _check(L.mi355rt_trace_rays(C.byref(sc), C.c_void_p(rays.ctypes.data), rays.size, C.c_void_p(hits.ctypes.data)), "mi355rt_trace_rays", L)
    return hits


def occluded(scene, segments, library=None):
    """One-shot mi355rt_occluded with host buffers: 1 where the closest hit of a segment's ray lies strictly below its t_max, else 0.  segments: a
    numpy array of abi.SEGMENT_DTYPE (or float32 [n, 8]: origin, pad, direction, t_max; the directions need not be unit).  Returns uint32 [n]."""
    L = library or lib()
    sc = getattr(scene, "c", scene)
    segments = np.ascontiguousarray(segments)
    if segments.dtype != abi.SEGMENT_DTYPE:
        segments = np.ascontiguousarray(segments, np.float32).reshape(-1, 8).view(abi.SEGMENT_DTYPE).reshape(-1)
    out = np.zeros(segments.size, np.uint32)
    _check(L.mi355rt_occluded(C.byref(sc), C.c_void_p(segments.ctypes.data), segments.size, C.c_void_p(out.ctypes.data)), "mi355rt_occluded", L)
    return out


def radiance_scratch_bytes(n_rays, samples, library=None):
    """mi355rt_radiance_scratch_bytes: the size of Context.trace_radiance's d_scratch for n_rays rays and samples = sample_end - sample_begin."""
    L = library or lib()
    n = C.c_uint64()
    _check(L.mi355rt_radiance_scratch_bytes(int(n_rays), int(samples), C.byref(n)), "mi355rt_radiance_scratch_bytes", L)
    return n.value


def view_scratch_bytes(view, samples, library=None):
    """mi355rt_view_scratch_bytes: the size of Context.render_view's d_scratch for `view` (abi.View) and samples = sample_end - sample_begin."""
    L = library or lib()
    n = C.c_uint64()
    _check(L.mi355rt_view_scratch_bytes(C.byref(view) if view is not None else None, int(samples), C.byref(n)), "mi355rt_view_scratch_bytes", L)
    return n.value


def trace_radiance(scene, rays, params, accum=None, want_linear=True, library=None):
    """One-shot mi355rt_trace_radiance with host buffers: samples [params.sample_begin, params.sample_end) of a whole path along every ray of
    `scene`, added to the running sums.  rays: a numpy array of abi.PATH_RAY_DTYPE; params: abi.RadianceParams; accum: float32 [n, 4] sums of the
    samples before sample_begin (needed when sample_begin > 0; not changed).  Returns (accum float32 [n, 4], linear float32 [n, 3] or None)."""
    L = library or lib()
    sc = getattr(scene, "c", scene)
    rays = np.ascontiguousarray(rays)
    if rays.dtype != abi.PATH_RAY_DTYPE:
        raise ValueError("trace_radiance: rays must be an array of abi.PATH_RAY_DTYPE")
    n = rays.size
    if accum is None:
        if params.sample_begin > 0:
            raise ValueError("trace_radiance: sample_begin > 0 continues running sums: pass accum")
        accum = np.zeros((n, 4), np.float32)
    else:
        accum = np.array(accum, np.float32, order="C").reshape(n, 4)
    linear = np.zeros((n, 3), np.float32) if want_linear else None
    _check(L.mi355rt_trace_radiance(C.byref(sc), C.byref(params), C.c_void_p(rays.ctypes.data), n, C.c_void_p(accum.ctypes.data),
                                    C.c_void_p(linear.ctypes.data) if want_linear else None), "mi355rt_trace_radiance", L)
    return accum, linear


def denoise_scratch_bytes(width, rows, library=None):
    """mi355rt_denoise_scratch_bytes: the size of Context.denoise's d_scratch for a window of rows x width pixels."""
    L = library or lib()
    n = C.c_uint64()
    _check(L.mi355rt_denoise_scratch_bytes(int(width), int(rows), C.byref(n)), "mi355rt_denoise_scratch_bytes", L)
    return n.value


def denoise(linear, hits, params=None, want_linear=True, want_packed=True, library=None):
    """One-shot mi355rt_denoise with host buffers on device 0.  linear: float32 [rows, W, 3]; hits: abi.HIT_DTYPE [rows * W] (what first_hits
    wrote for the same window); params: abi.DenoiseParams or None for the defaults.  Returns (linear f32 [rows, W, 3] or None, packed u32 [rows, W] or None)."""
    L = library or lib()
    linear = np.ascontiguousarray(linear, np.float32)
    rows, W = linear.shape[0], linear.shape[1]
    hits = np.ascontiguousarray(hits)
    if hits.dtype != abi.HIT_DTYPE or hits.size != rows * W or linear.shape != (rows, W, 3):
        raise ValueError("denoise: linear must be [rows, W, 3] and hits rows * W records of abi.HIT_DTYPE")
    out_linear = np.zeros((rows, W, 3), np.float32) if want_linear else None
    out_packed = np.zeros((rows, W), np.uint32) if want_packed else None
    _check(L.mi355rt_denoise(W, rows, C.byref(params) if params is not None else None, C.c_void_p(linear.ctypes.data), C.c_void_p(hits.ctypes.data),
                             C.c_void_p(out_linear.ctypes.data) if want_linear else None, C.c_void_p(out_packed.ctypes.data) if want_packed else None),
           "mi355rt_denoise", L)
    return out_linear, out_packed


def debug_scatter(materials, records, hip_device=0, textures=None):
    """Diagnostic: one Material::scatter per record on the device.  materials: ctypes array of abi.Material;
    records: (material index, front_face, rd[3], p[3], n[3], (k0, k1, x, s, ray)).  Returns float32 [n, 10] rows
    (scattered, origin[3], direction[3], attenuation[3]) -- the layout of the oracle's hook."""
    sc = abi.Scene()
    sc.materials, sc.n_materials = materials, len(materials)
    if textures is not None:
        sc.textures, sc.n_textures = textures, len(textures)
    sc.miss_color[:] = (0.5, 0.5, 0.5)
    ctx = Context(hip_device)
    try:
        ctx.set_scene(sc, abi.Camera(), abi.Settings(1, 1, 1, 1))
        n = len(records)
        rin = np.zeros((n, 16), np.uint32)
        for i, (mi, ff, rd, p, nn, ctr) in enumerate(records):
            rin[i, 0], rin[i, 1] = mi, 1 if ff else 0
            rin[i, 2:11] = np.concatenate([np.asarray(rd, np.float32), np.asarray(p, np.float32), np.asarray(nn, np.float32)]).view(np.uint32)
            rin[i, 11:16] = ctr
        out = np.zeros((n, 16), np.float32)
        _check(lib().mi355rt_debug_scatter(ctx._h, C.c_void_p(rin.ctypes.data), n, C.c_void_p(out.ctypes.data)), "mi355rt_debug_scatter")
        return out[:, :10].copy()
    finally:
        ctx.close()


def debug_hit(scene, rays, hip_device=0):
    """Diagnostic: closest hit of each (origin, unnormalised direction) against `scene` on the device.  Returns float32 [n, 10]:
    position[3], normal[3], t, material, front_face, hit."""
    ctx = Context(hip_device)
    try:
        ctx.set_scene(scene, abi.Camera(), abi.Settings(1, 1, 1, 1))
        n = len(rays)
        rin = np.zeros((n, 6), np.float32)
        for i, (o, d) in enumerate(rays):
            rin[i, :3], rin[i, 3:] = o, d
        out = np.zeros((n, 12), np.float32)
        _check(lib().mi355rt_debug_hit(ctx._h, C.c_void_p(rin.ctypes.data), n, C.c_void_p(out.ctypes.data)), "mi355rt_debug_hit")
        return out[:, :10].copy()
    finally:
        ctx.close()


class Context:
    """Resident-scene API: upload once, render many times into DEVICE buffers."""

    def __init__(self, hip_device=0, library=None):
        self._L = library or lib()
        self._h = C.c_void_p()
        _check(self._L.mi355rt_context_create(hip_device, C.byref(self._h)), "mi355rt_context_create", self._L)
        self.settings = None

    def set_knob(self, name, value):
        """Diagnostic knob of this context (before set_scene); see device.set_knob."""
        _check(self._L.mi355rt_debug_set_knob(self._h, name.encode(), int(value)), f"mi355rt_debug_set_knob({name})", self._L)

    def set_share(self, share_of):
        """mi355rt_context_set_share: this context is one of `share_of` contexts whose frames are in flight together (own stream each): its
        persistent kernels launch 1 / share_of of the grid that fills the device."""
        _check(self._L.mi355rt_context_set_share(self._h, int(share_of)), "mi355rt_context_set_share", self._L)

    def check(self):
        """mi355rt_context_check: waits for every render enqueued on this context and raises if a kernel left an image incomplete."""
        _check(self._L.mi355rt_context_check(self._h), "mi355rt_context_check", self._L)

    def set_scene(self, scene, camera, settings):
        sc = getattr(scene, "c", scene)
        _check(self._L.mi355rt_context_set_scene(self._h, C.byref(sc), C.byref(camera), C.byref(settings)),
               "mi355rt_context_set_scene", self._L)
        self.settings = abi.Settings(settings.width, settings.height, settings.samples_per_pixel, settings.max_depth)

    def rows_selected(self, options=None):
        n = C.c_uint32()
        _check(self._L.mi355rt_rows_selected(C.byref(self.settings), C.byref(options) if options is not None else None,
                                           C.byref(n)), "mi355rt_rows_selected", self._L)
        return n.value

    def render(self, d_out_packed, d_out_linear=None, options=None, stream=None, want_stats=False):
        """d_out_*: integer device addresses (e.g. torch tensor .data_ptr()); stream: hipStream_t handle or None."""
        stats = abi.Stats() if want_stats else None
        _check(self._L.mi355rt_context_render(self._h, C.byref(options) if options is not None else None,
                                            C.c_void_p(d_out_packed), C.c_void_p(d_out_linear) if d_out_linear else None,
                                            C.c_void_p(stream) if stream else None,
                                            C.byref(stats) if want_stats else None), "mi355rt_context_render", self._L)
        return stats

    def render_progressive(self, sample_begin, sample_end, d_accum, d_out_packed, d_out_linear=None, options=None, stream=None, want_stats=False):
        """Samples [sample_begin, sample_end) added to the running sums in d_accum (float4 per selected pixel, device address)."""
        stats = abi.Stats() if want_stats else None
        _check(self._L.mi355rt_context_render_progressive(self._h, C.byref(options) if options is not None else None,
                                                        int(sample_begin), int(sample_end), C.c_void_p(d_accum), C.c_void_p(d_out_packed),
                                                        C.c_void_p(d_out_linear) if d_out_linear else None,
                                                        C.c_void_p(stream) if stream else None,
                                                        C.byref(stats) if stats is not None else None), "mi355rt_context_render_progressive", self._L)
        return stats

    def trace_rays(self, d_rays, n, d_hits, stream=None):
        """mi355rt_context_trace_rays: the closest hit of n rays in the resident scene, enqueued on `stream`.  d_rays / d_hits: integer device
        addresses (16-byte aligned) of n abi.Ray and n abi.Hit records; every word of every record is written."""
        _check(self._L.mi355rt_context_trace_rays(self._h, C.c_void_p(d_rays) if d_rays else None, int(n), C.c_void_p(d_hits) if d_hits else None,
                                                  C.c_void_p(stream) if stream else None), "mi355rt_context_trace_rays", self._L)

    def first_hits(self, d_hits, options=None, stream=None):
        """mi355rt_context_first_hits: the closest hit of the ray through the centre of every selected pixel (rows as render() selects them);
        d_hits: device address of rows_selected(options) * width abi.Hit records, row-major over the selected rows."""
        _check(self._L.mi355rt_context_first_hits(self._h, C.byref(options) if options is not None else None, C.c_void_p(d_hits) if d_hits else None,
                                                  C.c_void_p(stream) if stream else None), "mi355rt_context_first_hits", self._L)

    def occluded(self, d_segments, n, d_out, stream=None):
        """mi355rt_context_occluded: for n segments of the resident scene, 1 where the closest hit lies strictly below t_max, else 0, enqueued on
        `stream`.  d_segments: integer device address (16-byte aligned) of n abi.Segment records; d_out: n uint32 words, every one written."""
        _check(self._L.mi355rt_context_occluded(self._h, C.c_void_p(d_segments) if d_segments else None, int(n), C.c_void_p(d_out) if d_out else None,
                                                C.c_void_p(stream) if stream else None), "mi355rt_context_occluded", self._L)

    def ambient_occlusion(self, d_hits, d_out, params=None, options=None, stream=None):
        """mi355rt_context_ambient_occlusion: one float per selected pixel, 1 - (occluded samples) / samples around the pixel's first hit.  d_hits:
        what first_hits wrote for the same options; d_out: rows_selected(options) * width floats; params: abi.AoParams or None for the defaults."""
        _check(self._L.mi355rt_context_ambient_occlusion(self._h, C.byref(options) if options is not None else None,
                                                         C.byref(params) if params is not None else None, C.c_void_p(d_hits) if d_hits else None,
                                                         C.c_void_p(d_out) if d_out else None, C.c_void_p(stream) if stream else None),
               "mi355rt_context_ambient_occlusion", self._L)

    def trace_radiance(self, params, d_rays, n, d_accum, d_scratch, d_out_linear=None, stream=None):
        """mi355rt_context_trace_radiance: samples [params.sample_begin, params.sample_end) of a whole path along each of n rays of the resident
        scene, enqueued on `stream`.  Integer device addresses (16-byte aligned): d_rays n abi.PathRay records, d_accum n float4 running sums (read
        when sample_begin > 0, always written), d_scratch radiance_scratch_bytes(n, sample_end - sample_begin) bytes; d_out_linear: n * 3 floats,
        sum / sample_end, or None.  params: abi.RadianceParams."""
        p = lambda a: C.c_void_p(a) if a else None
        _check(self._L.mi355rt_context_trace_radiance(self._h, C.byref(params) if params is not None else None, p(d_rays), int(n), p(d_accum),
                                                      p(d_out_linear), p(d_scratch), p(stream)), "mi355rt_context_trace_radiance", self._L)

    def view_rays(self, view, sample, d_rays, seed=0, stream=None):
        """mi355rt_context_view_rays: the rays of sample index `sample` of every pixel of `view` (abi.View), made on the device and written to d_rays
        (integer device address, 16-byte aligned, view.width * view.height abi.PathRay records), enqueued on `stream`."""
        p = lambda a: C.c_void_p(a) if a else None
        _check(self._L.mi355rt_context_view_rays(self._h, C.byref(view) if view is not None else None, int(sample), int(seed), p(d_rays), p(stream)),
               "mi355rt_context_view_rays", self._L)

    def render_view(self, view, params, d_accum, d_scratch, d_out_linear=None, d_out_packed=None, stream=None):
        """mi355rt_context_render_view: samples [params.sample_begin, params.sample_end) of every pixel of `view` (abi.View) of the resident scene,
        the rays made on the device, enqueued on `stream`.  Integer device addresses: d_accum width * height float4 running sums (16-byte aligned; read
        when sample_begin > 0, always written), d_scratch view_scratch_bytes(view, sample_end - sample_begin) bytes (16-byte aligned); d_out_linear:
        width * height * 3 floats, sum / sample_end, or None; d_out_packed: width * height words 0x00RRGGBB, or None.  params: abi.RadianceParams."""
        p = lambda a: C.c_void_p(a) if a else None
        _check(self._L.mi355rt_context_render_view(self._h, C.byref(view) if view is not None else None, C.byref(params) if params is not None else None,
                                                   p(d_accum), p(d_out_linear), p(d_out_packed), p(d_scratch), p(stream)), "mi355rt_context_render_view", self._L)

    def probe_rays(self, d_probes, n, sample, d_rays, seed=0, stream=None):
        """mi355rt_context_probe_rays: the cosine-hemisphere ray of sample index `sample` of each of n probes (abi.Probe records at the integer device
        address d_probes, 16-byte aligned), made on the device and written to d_rays (n abi.PathRay records, 16-byte aligned), enqueued on `stream`."""
        p = lambda a: C.c_void_p(a) if a else None
        _check(self._L.mi355rt_context_probe_rays(self._h, p(d_probes), int(n), int(sample), int(seed), p(d_rays), p(stream)),
               "mi355rt_context_probe_rays", self._L)

    def probe_radiance(self, params, d_probes, n, d_accum, d_scratch, d_out_linear=None, stream=None):
        """mi355rt_context_probe_radiance: samples [params.sample_begin, params.sample_end) of the cosine-weighted mean radiance at each of n probes
        of the resident scene (irradiance / pi), the rays made on the device, enqueued on `stream`.  Integer device addresses (16-byte aligned): d_probes
        n abi.Probe records, d_accum n float4 running sums (read when sample_begin > 0, always written), d_scratch radiance_scratch_bytes(n,
        sample_end - sample_begin) bytes; d_out_linear: n * 3 floats, sum / sample_end, or None.  params: abi.RadianceParams."""
        p = lambda a: C.c_void_p(a) if a else None
        _check(self._L.mi355rt_context_probe_radiance(self._h, C.byref(params) if params is not None else None, p(d_probes), int(n), p(d_accum),
                                                      p(d_out_linear), p(d_scratch), p(stream)), "mi355rt_context_probe_radiance", self._L)

    def denoise(self, width, rows, d_linear_in, d_hits, d_scratch, d_out_linear=None, d_out_packed=None, params=None, stream=None):
        """mi355rt_context_denoise: the a-trous filter of mi355rt.h over a contiguous window of rows x width pixels, enqueued on `stream`.  Integer
        device addresses: d_linear_in rows * width * 3 floats, d_hits what first_hits wrote for the window, d_scratch denoise_scratch_bytes(width, rows)
        bytes; at least one of d_out_linear (may be d_linear_in) and d_out_packed.  params: abi.DenoiseParams or None for the defaults."""
        p = lambda a: C.c_void_p(a) if a else None
        _check(self._L.mi355rt_context_denoise(self._h, int(width), int(rows), C.byref(params) if params is not None else None, p(d_linear_in), p(d_hits),
                                               p(d_scratch), p(d_out_linear), p(d_out_packed), p(stream)), "mi355rt_context_denoise", self._L)

    def kernel_variant(self):
        """Diagnostic: the counter-mode kernel chosen for the resident scene (0 lockstep, 1 lockstep+mesh, 2 state machine, 3 lockstep simple)."""
        v = C.c_uint32()
        _check(self._L.mi355rt_debug_kernel_variant(self._h, C.byref(v)), "mi355rt_debug_kernel_variant", self._L)
        return v.value

    def kernel_entry(self):
        """Diagnostic: (kernel name, workgroups per CU, VGPRs) of the entry point the resident scene is launched on (see entry_kernel)."""
        f = self._L.mi355rt_debug_kernel_entry
        f.restype = C.c_char_p
        f.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        blocks, vgprs = C.c_uint32(), C.c_uint32()
        name = f(self._h, C.byref(blocks), C.byref(vgprs))
        if name is None:
            raise RuntimeError("mi355rt_debug_kernel_entry: the context has no scene")
        return name.decode(), blocks.value, vgprs.value

    def row_tables(self):
        """Diagnostic: (natural, processing, out_row) row tables of the last render on this context and the per-image-row cost (rays per path
        of set_scene's probe; empty when the rows are processed in image order)."""
        n, nc = C.c_uint32(), C.c_uint32()
        f = self._L.mi355rt_debug_read_row_tables
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
        _check(f(self._h, None, 0, C.byref(n), None, 0, C.byref(nc)), "mi355rt_debug_read_row_tables", self._L)
        t = np.zeros(3 * n.value, np.uint32); cost = np.zeros(nc.value, np.float32)
        _check(f(self._h, t.ctypes.data, t.size, C.byref(n), cost.ctypes.data, cost.size, C.byref(nc)), "mi355rt_debug_read_row_tables", self._L)
        return t[:n.value], t[n.value:2 * n.value], t[2 * n.value:], cost

    def set_timing(self, enable=True):
        _check(self._L.mi355rt_context_set_timing(self._h, 1 if enable else 0), "mi355rt_context_set_timing", self._L)

    def read_timing(self):
        """(render_kernel_ms, resolve_kernel_ms, launches) summed since the last read; call after syncing the stream."""
        a, b, n = C.c_double(), C.c_double(), C.c_uint32()
        _check(self._L.mi355rt_context_read_timing(self._h, C.byref(a), C.byref(b), C.byref(n)), "mi355rt_context_read_timing", self._L)
        return a.value, b.value, n.value

    def close(self):
        if self._h:
            self._L.mi355rt_context_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_hip_rt = None


def _hip():
    """The HIP runtime the device library is linked against, for NoiseDevice's own buffers (torch is not needed here)."""
    global _hip_rt
    if _hip_rt is None:
        H = C.CDLL("libamdhip64.so")
        H.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        H.hipHostMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t, C.c_uint]
        H.hipFree.argtypes = [C.c_void_p]
        H.hipHostFree.argtypes = [C.c_void_p]
        H.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        H.hipStreamSynchronize.argtypes = [C.c_void_p]
        H.hipSetDevice.argtypes = [C.c_int]
        _hip_rt = H
    return _hip_rt


class NoiseDevice:
    """mi355rt_noise_device_*: the noise estimate of a progressive render on the device, beside the running sums (include/mi355rt.h has the
    definition).  update() reads d_accum where it is; evaluate() returns (error map float32 [rows, width] or None, abi.NoiseSummary).  The
    object owns a device buffer for the map and a pinned word for the summary; update, reset and evaluate_into only enqueue."""

    def __init__(self, width, rows, device=0, library=None):
        self._L = library or lib()
        self._h = C.c_void_p()
        self._d_error = C.c_void_p()
        self._h_summary = C.c_void_p()
        _check(self._L.mi355rt_noise_device_create(int(device), int(width), int(rows), C.byref(self._h)), "mi355rt_noise_device_create", self._L)
        self.width, self.rows, self.device = int(width), int(rows), int(device)

    def reset(self, stream=None):
        _check(self._L.mi355rt_noise_device_reset(self._h, C.c_void_p(stream) if stream else None), "mi355rt_noise_device_reset", self._L)

    def update(self, d_accum_ptr, samples_total, stream=None):
        """d_accum_ptr: integer device address of rows * width * 4 floats (d_accum of render_progressive); samples_total: the chunk's sample_end."""
        _check(self._L.mi355rt_noise_device_update(self._h, C.c_void_p(d_accum_ptr) if d_accum_ptr else None, int(samples_total),
                                                   C.c_void_p(stream) if stream else None), "mi355rt_noise_device_update", self._L)

    def evaluate_into(self, d_out_error, d_out_summary, params=None, stream=None):
        """Enqueue only: the map to the device address d_out_error (or None) and the 56-byte summary to d_out_summary, in stream order."""
        _check(self._L.mi355rt_noise_device_evaluate(self._h, C.byref(params) if params is not None else None,
                                                     C.c_void_p(d_out_error) if d_out_error else None, C.c_void_p(d_out_summary) if d_out_summary else None,
                                                     C.c_void_p(stream) if stream else None), "mi355rt_noise_device_evaluate", self._L)

    def _hip_check(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"NoiseDevice: {what} failed (hipError_t {rc})")

    def evaluate(self, params=None, want_map=True, stream=None):
        H = _hip()
        self._hip_check(H.hipSetDevice(self.device), "hipSetDevice")
        if not self._h_summary:
            self._hip_check(H.hipHostMalloc(C.byref(self._h_summary), C.sizeof(abi.NoiseSummary), 0), "hipHostMalloc")
        if want_map and not self._d_error:
            self._hip_check(H.hipMalloc(C.byref(self._d_error), self.rows * self.width * 4), "hipMalloc")
        self.evaluate_into(self._d_error.value if want_map else None, self._h_summary.value, params, stream)
        self._hip_check(H.hipStreamSynchronize(C.c_void_p(stream) if stream else None), "hipStreamSynchronize")
        summary = abi.NoiseSummary.from_buffer_copy(C.string_at(self._h_summary.value, C.sizeof(abi.NoiseSummary)))
        err = None
        if want_map:
            err = np.empty((self.rows, self.width), np.float32)
            self._hip_check(H.hipMemcpy(err.ctypes.data, self._d_error, err.nbytes, 2), "hipMemcpy")      # 2: device to host
        return err, summary

    def free(self):
        """The caller has synchronised the streams that carry this object's work."""
        if self._h:
            self._L.mi355rt_noise_device_destroy(self._h)
            self._h = C.c_void_p()
        if self._d_error:
            _hip().hipFree(self._d_error); self._d_error = C.c_void_p()
        if self._h_summary:
            _hip().hipHostFree(self._h_summary); self._h_summary = C.c_void_p()

    close = free

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class MultiContext:
    """mi355rt_multi_context_*: one process drives the listed HIP devices (a device may repeat; every entry is one part with its own
    context and stream) and keeps scene, staging buffers and row table across calls.  Outputs live on devices[0]."""

    def __init__(self, devices, library=None):
        self._L = library or lib()
        self._h = C.c_void_p()
        self.devices = [int(d) for d in devices]
        devs = (C.c_int * max(len(self.devices), 1))(*self.devices)
        _check(self._L.mi355rt_multi_context_create(devs, len(self.devices), C.byref(self._h)), "mi355rt_multi_context_create", self._L)
        self.settings = None

    def set_scene(self, scene, camera, settings):
        sc = getattr(scene, "c", scene)
        _check(self._L.mi355rt_multi_context_set_scene(self._h, C.byref(sc), C.byref(camera), C.byref(settings)),
               "mi355rt_multi_context_set_scene", self._L)
        self.settings = abi.Settings(settings.width, settings.height, settings.samples_per_pixel, settings.max_depth)

    def rows_selected(self, options=None):
        """Rows the outputs hold: the window of `options` (the strips are dealt over the parts, all of them land in the output)."""
        if self.settings is None:
            raise RuntimeError("MultiContext has no scene (set_scene)")
        window = None
        if options is not None:
            window = abi.Options.make(row_begin=options.row_begin, row_end=options.row_end)
        n = C.c_uint32()
        _check(self._L.mi355rt_rows_selected(C.byref(self.settings), C.byref(window) if window is not None else None, C.byref(n)),
               "mi355rt_rows_selected", self._L)
        return n.value

    def render(self, out_packed, out_linear=None, options=None, stream=None, want_stats=False):
        """out_packed: uint32/int32 device tensor on devices[0] with >= rows * width elements; out_linear: float32 tensor with
        >= rows * width * 3 elements, or None; stream: a torch stream of devices[0] (or a raw hipStream_t), None = its default stream.
        Without want_stats the call only enqueues (the stream orders the result); with it, it waits and returns abi.Stats."""
        if self.settings is not None:
            need = self.rows_selected(options) * self.settings.width
            for t, k, name in ((out_packed, 1, "out_packed"), (out_linear, 3, "out_linear")):
                if t is not None and t.numel() < need * k:
                    raise ValueError(f"{name} holds {t.numel()} elements, the selected rows need {need * k}")
        stats = abi.Stats() if want_stats else None
        s = getattr(stream, "cuda_stream", stream)
        _check(self._L.mi355rt_multi_context_render(self._h, C.byref(options) if options is not None else None,
                                                    C.c_void_p(out_packed.data_ptr()) if out_packed is not None else None,
                                                    C.c_void_p(out_linear.data_ptr()) if out_linear is not None else None,
                                                    C.c_void_p(s) if s else None, C.byref(stats) if want_stats else None),
               "mi355rt_multi_context_render", self._L)
        return stats

    def render_progressive(self, sample_begin, sample_end, out_packed, out_linear=None, accum=None, options=None, stream=None, want_stats=False):
        """mi355rt_multi_context_render_progressive: samples [sample_begin, sample_end) added to every part's running sums (kept on the
        parts); the outputs then hold the image of the first sample_end samples.  sample_begin 0 starts a sequence, anything else must
        continue the last chunk with the same rows, rng_mode, seed and flags.  Tensors as in render(); accum: float32 device tensor on
        devices[0] with >= rows * width * 4 elements that receives the gathered sums (the layout of Context.render_progressive's d_accum),
        or None."""
        if self.settings is not None:
            need = self.rows_selected(options) * self.settings.width
            for t, k, name in ((out_packed, 1, "out_packed"), (out_linear, 3, "out_linear"), (accum, 4, "accum")):
                if t is not None and t.numel() < need * k:
                    raise ValueError(f"{name} holds {t.numel()} elements, the selected rows need {need * k}")
            if accum is not None and accum.data_ptr() % 16:
                raise ValueError("accum must start on 16 bytes (float4 per pixel)")
        stats = abi.Stats() if want_stats else None
        s = getattr(stream, "cuda_stream", stream)
        _check(self._L.mi355rt_multi_context_render_progressive(self._h, C.byref(options) if options is not None else None,
                                                                int(sample_begin), int(sample_end),
                                                                C.c_void_p(accum.data_ptr()) if accum is not None else None,
                                                                C.c_void_p(out_packed.data_ptr()) if out_packed is not None else None,
                                                                C.c_void_p(out_linear.data_ptr()) if out_linear is not None else None,
                                                                C.c_void_p(s) if s else None, C.byref(stats) if want_stats else None),
               "mi355rt_multi_context_render_progressive", self._L)
        return stats

    def check(self):
        """mi355rt_multi_context_check: waits for every render enqueued so far and raises if a part left its strips incomplete."""
        _check(self._L.mi355rt_multi_context_check(self._h), "mi355rt_multi_context_check", self._L)

    def part_kernel_ms(self):
        """Diagnostic: render + resolve kernel ms of every part in the last render given want_stats."""
        n = C.c_uint32()
        out = (C.c_double * max(len(self.devices), 1))()
        _check(self._L.mi355rt_debug_multi_part_ms(self._h, out, len(out), C.byref(n)), "mi355rt_debug_multi_part_ms", self._L)
        return list(out)[:n.value]

    def close(self):
        if self._h:
            self._L.mi355rt_multi_context_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
