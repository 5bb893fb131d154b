"""ctypes mirror of include/mi355rt.h (the C ABI).  Pure declarations: no library is loaded here.

Every Structure below must stay field-for-field identical to the header; tests/test_abi.py checks
the sizes against the values the C compiler reports (`mi355rt_host` exports them).
"""
import ctypes as C

import numpy as np

ABI_VERSION = 5

OK, ERR_INVALID, ERR_NO_DEVICE, ERR_HIP, ERR_OOM, ERR_IO, ERR_UNSUPPORTED = 0, -1, -2, -3, -4, -5, -6

MAT_LAMBERT_SOLID, MAT_LAMBERT_CHECKER, MAT_METAL, MAT_DIELECTRIC, MAT_EMISSIVE, MAT_PLASTIC, \
    MAT_ROUGH_GGX, MAT_ROUGH_BECKMANN, MAT_NULL, MAT_TEXTURE = range(10)
PRIM_SPHERE, PRIM_PLANE, PRIM_QUAD, PRIM_CUBE, PRIM_MESH = range(5)
RNG_CTR, RNG_REF = 0, 1
FLAG_FIXED_AABB = 1

f32, u32, u64 = C.c_float, C.c_uint32, C.c_uint64


class Camera(C.Structure):
    _fields_ = [("position", f32 * 3), ("forward", f32 * 3), ("right", f32 * 3), ("true_up", f32 * 3),
                ("half_width", f32), ("half_height", f32)]


class Settings(C.Structure):
    _fields_ = [("width", u32), ("height", u32), ("samples_per_pixel", u32), ("max_depth", u32)]


class Material(C.Structure):
    _fields_ = [("kind", u32), ("albedo", f32 * 3), ("aux", f32 * 3), ("p0", f32), ("p1", f32),
                ("eta", f32 * 3), ("k", f32 * 3), ("texture", u32)]


class Texture(C.Structure):
    _fields_ = [("rgba8", C.POINTER(C.c_uint8)), ("width", u32), ("height", u32)]


class Primitive(C.Structure):
    _fields_ = [("kind", u32), ("material", u32), ("mesh", u32), ("_pad", u32), ("data", f32 * 32)]


class Triangle(C.Structure):
    _fields_ = [("v0", f32 * 3), ("v1", f32 * 3), ("v2", f32 * 3), ("normal", f32 * 3)]


class BvhNode(C.Structure):
    _fields_ = [("bmin", f32 * 3), ("bmax", f32 * 3), ("left", u32), ("right", u32),
                ("first_index", u32), ("index_count", u32)]


class Mesh(C.Structure):
    _fields_ = [("first_triangle", u32), ("triangle_count", u32), ("first_node", u32), ("node_count", u32),
                ("first_index", u32), ("index_count", u32), ("max_depth", u32), ("_pad", u32)]


class Scene(C.Structure):
    _fields_ = [("primitives", C.POINTER(Primitive)), ("n_primitives", u32),
                ("materials", C.POINTER(Material)), ("n_materials", u32),
                ("meshes", C.POINTER(Mesh)), ("n_meshes", u32),
                ("triangles", C.POINTER(Triangle)), ("n_triangles", u32),
                ("nodes", C.POINTER(BvhNode)), ("n_nodes", u32),
                ("tri_indices", C.POINTER(u32)), ("n_tri_indices", u32),
                ("miss_color", f32 * 3), ("sky_width", u32), ("sky_height", u32),
                ("sky_rgb", C.POINTER(f32)), ("textures", C.POINTER(Texture)), ("n_textures", u32)]


class Options(C.Structure):
    _fields_ = [("abi_version", u32), ("rng_mode", u32), ("seed", u64),
                ("row_begin", u32), ("row_end", u32), ("strip_rows", u32), ("n_parts", u32), ("part", u32),
                ("flags", u32), ("workspace_bytes", u64)]

    @classmethod
    def make(cls, rng_mode=RNG_CTR, seed=0, row_begin=0, row_end=0, strip_rows=1, n_parts=1, part=0,
             workspace_bytes=0, flags=0):
        return cls(ABI_VERSION, rng_mode, seed, row_begin, row_end, strip_rows, n_parts, part, flags, workspace_bytes)


class Stats(C.Structure):
    _fields_ = [("render_kernel_ms", C.c_double), ("resolve_kernel_ms", C.c_double), ("total_ms", C.c_double),
                ("samples", u64), ("rays", u64), ("rows_rendered", u32), ("bands", u32),
                ("grid_blocks", u32), ("block_threads", u32), ("kernel_vgprs", u32), ("kernel_sgprs", u32)]


NO_HIT = 0xFFFFFFFF


class Ray(C.Structure):                                   # mi355rt_ray, 32 bytes
    _fields_ = [("origin", f32 * 3), ("_pad0", f32), ("direction", f32 * 3), ("_pad1", f32)]


class Hit(C.Structure):                                   # mi355rt_hit, 48 bytes
    _fields_ = [("position", f32 * 3), ("t", f32), ("normal", f32 * 3), ("front_face", u32),
                ("primitive", u32), ("material", u32), ("_pad", u32 * 2)]


# numpy twins of Ray / Hit: arrays of them are what the query calls read and write
RAY_DTYPE = np.dtype([("origin", "<f4", 3), ("_pad0", "<f4"), ("direction", "<f4", 3), ("_pad1", "<f4")])
HIT_DTYPE = np.dtype([("position", "<f4", 3), ("t", "<f4"), ("normal", "<f4", 3), ("front_face", "<u4"),
                      ("primitive", "<u4"), ("material", "<u4"), ("_pad", "<u4", 2)])


class Segment(C.Structure):                               # mi355rt_segment, 32 bytes: a Ray whose last pad is read
    _fields_ = [("origin", f32 * 3), ("_pad0", f32), ("direction", f32 * 3), ("t_max", f32)]


SEGMENT_DTYPE = np.dtype([("origin", "<f4", 3), ("_pad0", "<f4"), ("direction", "<f4", 3), ("t_max", "<f4")])


class PathRay(C.Structure):                               # mi355rt_path_ray, 32 bytes: a Ray whose pads are the stream address words
    _fields_ = [("origin", f32 * 3), ("x", u32), ("direction", f32 * 3), ("row", u32)]


PATH_RAY_DTYPE = np.dtype([("origin", "<f4", 3), ("x", "<u4"), ("direction", "<f4", 3), ("row", "<u4")])


class RadianceParams(C.Structure):                        # mi355rt_radiance_params, 32 bytes
    _fields_ = [("sample_begin", u32), ("sample_end", u32), ("max_depth", u32), ("flags", u32), ("seed", u64), ("reserved", u64)]

    @classmethod
    def make(cls, sample_begin, sample_end, max_depth, seed=0):
        return cls(sample_begin, sample_end, max_depth, 0, seed, 0)


class Probe(C.Structure):                                 # mi355rt_probe, 32 bytes: a PathRay whose vectors are a surface point and its normal
    _fields_ = [("position", f32 * 3), ("x", u32), ("normal", f32 * 3), ("row", u32)]


PROBE_DTYPE = np.dtype([("position", "<f4", 3), ("x", "<u4"), ("normal", "<f4", 3), ("row", "<u4")])


def probes_from_hits(hits, width):
    """abi.PROBE_DTYPE [hits that hit]: a probe at every first-hit record of `hits` (abi.HIT_DTYPE, row-major over an image `width` pixels across, as
    Context.first_hits writes them), misses dropped: position and normal as the record holds them, x = i % width and row = i // width of record i."""
    hits = np.asarray(hits).reshape(-1)
    if hits.dtype != HIT_DTYPE:
        raise ValueError("probes_from_hits: hits must be an array of abi.HIT_DTYPE")
    if int(width) <= 0:
        raise ValueError("probes_from_hits: width must be positive")
    i = np.nonzero(hits["primitive"] != NO_HIT)[0]
    out = np.zeros(i.size, PROBE_DTYPE)
    out["position"], out["normal"] = hits["position"][i], hits["normal"][i]
    out["x"], out["row"] = i % int(width), i // int(width)
    return out


VIEW_PINHOLE, VIEW_THIN_LENS = 0, 1
VIEW_CENTRE = 1


class View(C.Structure):                                  # mi355rt_view, 96 bytes
    _fields_ = [("camera", Camera), ("model", u32), ("width", u32), ("height", u32), ("flags", u32), ("lens_radius", f32), ("focus_distance", f32),
                ("reserved", u32 * 4)]

    @classmethod
    def make(cls, camera, width, height, model=VIEW_PINHOLE, flags=0, lens_radius=0.0, focus_distance=0.0):
        v = cls()
        C.memmove(C.byref(v.camera), C.byref(camera), C.sizeof(Camera))
        v.model, v.width, v.height, v.flags, v.lens_radius, v.focus_distance = model, width, height, flags, lens_radius, focus_distance
        return v


class AoParams(C.Structure):                             # mi355rt_ao_params, 16 bytes
    _fields_ = [("samples", u32), ("seed", u32), ("radius", f32), ("_pad", u32)]

    @classmethod
    def make(cls, samples=16, seed=0, radius=float("inf")):
        """The defaults are what the call uses for a null pointer."""
        return cls(samples, seed, radius, 0)


class DenoiseParams(C.Structure):                         # mi355rt_denoise_params, 16 bytes
    _fields_ = [("levels", u32), ("normal_squarings", u32), ("sigma_color", f32), ("sigma_plane", f32)]

    @classmethod
    def make(cls, levels=5, normal_squarings=5, sigma_color=2.0, sigma_plane=0.05):
        """The defaults are what the calls use for a null pointer."""
        return cls(levels, normal_squarings, sigma_color, sigma_plane)


DENOISE_DEFAULTS = (5, 5, 2.0, 0.05)


class ReprojectParams(C.Structure):                       # mi355rt_reproject_params (include/mi355rt_post.h), 16 bytes
    _fields_ = [("max_history", u32), ("flags", u32), ("normal_min", f32), ("plane_tolerance", f32)]

    @classmethod
    def make(cls, max_history=32, normal_min=0.9, plane_tolerance=0.05, flags=0):
        """The defaults are what mi355rt_post_reproject uses for a null pointer."""
        return cls(max_history, flags, normal_min, plane_tolerance)


REPROJECT_DEFAULTS = (32, 0, 0.9, 0.05)
POST_ABI_VERSION = 1


class SvgfAccumulateParams(C.Structure):                  # mi355rt_svgf_accumulate_params (include/mi355rt_svgf.h), 32 bytes
    _fields_ = [("max_history", u32), ("flags", u32), ("normal_min", f32), ("plane_tolerance", f32),
                ("min_temporal", u32), ("normal_squarings", u32), ("sigma_plane", f32), ("reserved", u32)]

    @classmethod
    def make(cls, max_history=32, normal_min=0.9, plane_tolerance=0.05, min_temporal=4, normal_squarings=5, sigma_plane=0.05, flags=0, reserved=0):
        """The defaults are what mi355rt_svgf_accumulate uses for a null pointer."""
        return cls(max_history, flags, normal_min, plane_tolerance, min_temporal, normal_squarings, sigma_plane, reserved)


class SvgfFilterParams(C.Structure):                      # mi355rt_svgf_filter_params, 24 bytes
    _fields_ = [("levels", u32), ("normal_squarings", u32), ("sigma_luminance", f32), ("sigma_plane", f32), ("flags", u32), ("reserved", u32)]

    @classmethod
    def make(cls, levels=5, normal_squarings=5, sigma_luminance=1.0, sigma_plane=0.05, flags=0, reserved=0):
        """The defaults are what mi355rt_svgf_filter uses for a null pointer."""
        return cls(levels, normal_squarings, sigma_luminance, sigma_plane, flags, reserved)


SVGF_ACCUMULATE_DEFAULTS = (32, 0, 0.9, 0.05, 4, 5, 0.05, 0)
SVGF_FILTER_DEFAULTS = (5, 5, 1.0, 0.05, 0, 0)
SVGF_GATHERS_ONLY = 1
SVGF_ABI_VERSION = 1


class NoiseParams(C.Structure):                           # mi355rt_noise_params, 32 bytes
    _fields_ = [("threshold", C.c_double), ("floor", C.c_double), ("min_chunks", u32), ("_pad", u32), ("allowed_above", u64)]

    @classmethod
    def make(cls, threshold=0.02, floor=0.01, min_chunks=4, allowed_above=0):
        """The defaults are what mi355rt_noise_evaluate uses for a null pointer."""
        return cls(threshold, floor, min_chunks, 0, allowed_above)


NOISE_DEFAULTS = (0.02, 0.01, 4, 0, 0)


class NoiseSummary(C.Structure):                          # mi355rt_noise_summary, 56 bytes
    _fields_ = [("chunks", u32), ("samples", u32), ("pixels", u64), ("above", u64), ("nonfinite", u64),
                ("max_error", C.c_double), ("mean_error", C.c_double), ("converged", u32), ("_pad", u32)]


# mi355rt_progress_fn: int (*)(void* user, uint32_t samples_done, uint32_t samples_total, const uint32_t* packed_rgb)
ProgressFn = C.CFUNCTYPE(C.c_int, C.c_void_p, u32, u32, C.POINTER(u32))


class LoadOverrides(C.Structure):
    _fields_ = [("width", u32), ("height", u32), ("samples_per_pixel", u32), ("max_depth", u32),
                ("skip_unknown_primitives", u32), ("wo3_four_index_stride", u32)]


STRUCT_SIZES = {  # what sizeof() must report in C
    "mi355rt_camera": 56, "mi355rt_settings": 16, "mi355rt_material": 64, "mi355rt_primitive": 144,
    "mi355rt_triangle": 48, "mi355rt_bvh_node": 40, "mi355rt_mesh": 32,
}


def rows_selected(height, opt=None):
    """Rows an Options selects, in output order (mirror of the rule in mi355rt.h)."""
    if opt is None:
        return list(range(height))
    rb, re_ = opt.row_begin, (opt.row_end or height)
    strip, parts, part = max(opt.strip_rows, 1), max(opt.n_parts, 1), opt.part
    return [y for y in range(rb, re_) if (y // strip) % parts == part]
