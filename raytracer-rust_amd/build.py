"""Build recipes for the native libraries (in-tree, gfx950 only).

  libmi355rt.so       hipcc: HIP kernels + the device half of the C ABI (csrc/device; rt_query.hip: the ray-query kernels, a translation unit
                             of their own; rt_denoise.hip: the denoiser's kernels, likewise; rt_occlusion.hip: the occlusion
                             and ambient-occlusion kernels, likewise; rt_noise.hip: the noise estimate's kernels and its five entry points; rt_radiance.hip,
                             rt_view.hip, rt_probe.hip: the kernels of the radiance queries, the camera views and the surface probes; rt_api.cpp: the context,
                             set_scene and the renders; rt_queries.cpp: the calls that only read the resident scene; rt_debug.cpp: the debug hooks and
                             the knobs; rt_prepare.cpp: scene preparation and the plans, no HIP in it; rt_multi.cpp: the multi-device context;
                             rt_oneshot.cpp: the calls with host buffers, clients of the public functions)
  libmi355rt_post.so  hipcc: image-space post stages on device buffers, a library of its own (csrc/post; include/mi355rt_post.h): post_reproject.hip: the
                             temporal reprojection's kernel; post_plan.cpp: its defaults, refusals and launch geometry, no HIP in it; post_api.cpp: the exports.
                             Nothing of csrc/device is linked in (rt_math.h is included for the packing); kernel_hash() does not cover it.
  libmi355rt_svgf.so  hipcc: the variance-guided temporal filter on device buffers, a library of its own (csrc/svgf; include/mi355rt_svgf.h): svgf_kernels.hip: the
                             kernels of accumulate and filter; svgf_plan.cpp: defaults, refusals and launch geometry, no HIP in it; svgf_api.cpp: the exports.
                             Nothing of csrc/device or csrc/post is linked in (rt_math.h is included for the packing); kernel_hash() does not cover it.
                             (libmi355rt_svgf_grid3.so: the tests' variant with grids of at most 3 workgroups, build_svgf_grid3; not part of build_all.)
  libmi355rt_host.so  g++:   CPU-side producers -- scene loader, mesh readers, BVH build, PNG (csrc/host)
  rt_render           g++:   CLI that stands in for the Rust `main` (csrc/tools)

Outputs go to raytracer-rust_amd/_build/ (git-ignored, but they travel to the GPU box with gpurun).
hipcc cross-compiles gfx950 without a GPU, so this also runs in the CPU-only container.
"""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(HERE, "_build")
CSRC = os.path.join(HERE, "csrc")

DEVICE_SO = os.path.join(OUT, "libmi355rt.so")
HOST_SO = os.path.join(OUT, "libmi355rt_host.so")
POST_SO = os.path.join(OUT, "libmi355rt_post.so")
SVGF_SO = os.path.join(OUT, "libmi355rt_svgf.so")
CLI = os.path.join(OUT, "rt_render")

# -ffp-contract=off: no FMA contraction -- the reference (rustc) never fuses a*b+c, and parity with the
# CPU oracle is bit-level.  Correctly rounded f32 divide/sqrt are HIP's default; stated explicitly.
# -fno-slp-vectorize: hipcc's SLP pass packs adjacent f32 ops into v_pk_mul/add_f32, which issue slower than
# the two scalar ops they replace on gfx950 (measured: -6 % kernel time on cornell, identical results).
# -amdgpu-atomic-optimizer-strategy=None: the kernels' atomics (the work cursor, the wavefront kernels' queue tickets) are issued by ONE lane already; the
# optimizer pass wraps each of them in a second single-lane election (mbcnt, bcnt, a multiply, readfirstlane: ~10 instructions per atomic) that can never
# merge anything.  Round 5: mesh scenes and veach-mis -0.6 ... -0.8 %, cornell +-0 (profiles/r05/ab_scalar_diet.txt).
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
               "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-slp-vectorize", "-mllvm", "-amdgpu-atomic-optimizer-strategy=None", "-fPIC", "-shared", "-Wall",
               "-Wno-unused-command-line-argument"]
CXX_FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-Wall", "-pthread"]

DEVICE_SRCS = [os.path.join(CSRC, "device", "rt_kernels.hip"), os.path.join(CSRC, "device", "rt_query.hip"), os.path.join(CSRC, "device", "rt_denoise.hip"),
               os.path.join(CSRC, "device", "rt_occlusion.hip"), os.path.join(CSRC, "device", "rt_noise.hip"), os.path.join(CSRC, "device", "rt_radiance.hip"), os.path.join(CSRC, "device", "rt_view.hip"),
               os.path.join(CSRC, "device", "rt_probe.hip"),
               os.path.join(CSRC, "device", "rt_api.cpp"), os.path.join(CSRC, "device", "rt_queries.cpp"), os.path.join(CSRC, "device", "rt_debug.cpp"),
               os.path.join(CSRC, "device", "rt_prepare.cpp"), os.path.join(CSRC, "device", "rt_multi.cpp"),
               os.path.join(CSRC, "device", "rt_oneshot.cpp")]
DEVICE_HEADERS = sorted(os.path.join(CSRC, "device", f) for f in os.listdir(os.path.join(CSRC, "device")) if f.endswith(".h"))
DEVICE_DEPS = DEVICE_SRCS + DEVICE_HEADERS + [os.path.join(ROOT, "include", "mi355rt.h")]
# Compiled into the tests' reference build (-DMI355RT_REFS) only, so neither the product library nor kernel_hash() contains it:
# mi355rt_debug_stages, the transcendental stages over enumerated inputs (tests/test_gpu_transcendental_stages.py);
# mi355rt_debug_resolve / mi355rt_debug_gather, the shipped resolve and gather launchers on caller-supplied buffers (tests/test_gpu_resolve_stage.py);
# mi355rt_debug_rng_block, one generator block through each form of the draw address at a chosen ray and try (tests/test_gpu_rng_stepped.py).
REFS_SRCS = [os.path.join(CSRC, "refs", "rt_stages.hip"), os.path.join(CSRC, "refs", "rt_resolve_probe.hip"), os.path.join(CSRC, "refs", "rt_rng_probe.hip")]
# ... and mi355rt_debug_scatter_wave, the bounce's shipped pieces on caller-chosen waves (tests/test_gpu_scatter_wave.py).  The probe has to live
# in the kernels' translation unit (unit_ball_cooperative is defined there), so the reference build compiles REFS_KERNELS in the place of
# rt_kernels.hip: that file, included unchanged, and the probe's header behind it.  No file that kernel_hash() covers is touched.
REFS_KERNELS = os.path.join(CSRC, "refs", "rt_kernels_refs.hip")
REFS_HEADERS = [os.path.join(CSRC, "refs", "rt_scatter_wave_probe.h"),
                os.path.join(CSRC, "refs", "rt_range_wave_probe.h")]      # mi355rt_debug_range_wave, likewise (tests/test_gpu_range_wave.py)


def _host_srcs():
    d = os.path.join(CSRC, "host")
    return sorted(os.path.join(d, f) for f in os.listdir(d) if f.endswith(".cpp")) if os.path.isdir(d) else []


def _host_deps():
    d = os.path.join(CSRC, "host")
    hs = sorted(os.path.join(d, f) for f in os.listdir(d) if f.endswith((".hpp", ".h"))) if os.path.isdir(d) else []
    return _host_srcs() + hs + [os.path.join(ROOT, "include", "mi355rt.h")]


def _code_only(text):
    """C++ source without its comments, whitespace runs collapsed (string and character literals are kept as they are)."""
    out, i, n = [], 0, len(text)
    while i < n:
        c = text[i]
        if c in "\"'":                                      # a literal: copy to its closing quote
            j = i + 1
            while j < n and text[j] != c:
                j += 2 if text[j] == "\\" else 1
            out.append(text[i:j + 1]); i = j + 1
        elif text.startswith("//", i):
            j = text.find("\n", i); i = n if j < 0 else j
        elif text.startswith("/*", i):
            j = text.find("*/", i + 2); i = n if j < 0 else j + 2
            out.append(" ")
        else:
            out.append(c); i += 1
    return " ".join("".join(out).split())


def kernel_hash():
    """sha256 over everything that decides the device code AND how it is launched: the kernel source, every header of csrc/device, the
    host half (rt_api.cpp, rt_queries.cpp and rt_debug.cpp: the launches of the renders, of the queries and of the debug hooks; rt_prepare.cpp: the scene records, the choice of the kernel variant, the plan of a render -- grid size, shard size, guided_div; rt_multi.cpp and rt_oneshot.cpp: the multi-device context and the calls with host buffers, built on the public
    entry points) and the hipcc flags -- the CODE of those
    files: comments and whitespace are stripped first, so that correcting a comment does not orphan the committed counters.
    profiles/pmc_counters.json records it, and bench.py refuses counters taken on another library."""
    import hashlib
    h = hashlib.sha256()
    for f in DEVICE_SRCS + DEVICE_HEADERS:                  # rt_kernels.hip, rt_query.hip, rt_denoise.hip, rt_occlusion.hip, rt_noise.hip, rt_radiance.hip, rt_view.hip, rt_probe.hip, rt_api.cpp, rt_queries.cpp, rt_debug.cpp, rt_prepare.cpp, rt_multi.cpp, rt_oneshot.cpp and every header they include (rt_device.h, rt_math.h, ...)
        h.update(_code_only(open(f, encoding="utf-8").read()).encode())
    h.update(" ".join(HIPCC_FLAGS).encode())
    return h.hexdigest()[:16]


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps if os.path.exists(d))


def hipcc_path():
    p = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(p):
        raise RuntimeError("hipcc not found: the HIP path cannot be built (there is no CPU fallback)")
    return p


def build_device(force=False, extra_flags=(), verbose=False):
    os.makedirs(OUT, exist_ok=True)
    if force or _stale(DEVICE_SO, DEVICE_DEPS):
        cmd = [hipcc_path(), *HIPCC_FLAGS, *extra_flags, "-o", DEVICE_SO, *DEVICE_SRCS]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
    return DEVICE_SO


def build_device_variant(name, defines=(), force=False, verbose=False, flags=()):
    """Diagnostic / A-B builds (e.g. cycle stamps) into their own library; never loaded by the product path."""
    os.makedirs(OUT, exist_ok=True)
    so = os.path.join(OUT, f"libmi355rt_{name}.so")
    srcs = list(DEVICE_SRCS)
    if "MI355RT_REFS" in defines:
        srcs = [REFS_KERNELS if s == DEVICE_SRCS[0] else s for s in DEVICE_SRCS] + REFS_SRCS
    if force or _stale(so, DEVICE_DEPS + srcs + REFS_HEADERS):
        cmd = [hipcc_path(), *HIPCC_FLAGS, *flags, *[f"-D{d}" for d in defines], "-o", so, *srcs]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
    return so


# k_render_ctr_simple_qc with the guarded short arithmetic it had before its range arithmetic (rt_math.h, "Range arithmetic"): every step's define at 0,
# which builds every kernel of the library as it was (profiles/isa_diff_range_arithmetic_vs_parent.txt).  The tests render with both libraries and
# compare bit for bit (tests/test_gpu_range_arithmetic.py); never loaded by the product path.
RANGE_OFF_DEFINES = ["MI355RT_QC_RENORM_CLOSED=0", "MI355RT_QC_NORM_RANGED=0", "MI355RT_QC_QUAD_NOFIX=0", "MI355RT_QC_CUBE_NOFIX=0"]


def build_range_off(force=False, verbose=False):
    return build_device_variant("range_off", RANGE_OFF_DEFINES, force=force, verbose=verbose)


# k_render_ctr_simple_qc as it was before it carried its path state in place (rt_kernels.hip, MI355RT_QC_*): every step's define at 0.  The tests render
# with both libraries and compare bit for bit (tests/test_gpu_state_in_place.py); never loaded by the product path.
# (MI355RT_QC_EMPTY_PASS=0: the camera pass without its empty-pass shortcut, the fourth bit of FORM.)
# (... and without the range arithmetic that came after it, RANGE_OFF_DEFINES: the listing tests/test_state_in_place_isa.py knows as the form before.)
QC_FORM0_DEFINES = ["MI355RT_QC_HIT_IN_PLACE=0", "MI355RT_QC_STATE_IN_PLACE=0", "MI355RT_QC_TERM_SELECT=0", "MI355RT_QC_EMPTY_PASS=0"] + RANGE_OFF_DEFINES


def build_qc_form0(force=False, verbose=False):
    return build_device_variant("qc_form0", QC_FORM0_DEFINES, force=force, verbose=verbose)


# The library that spends its full price on pixels that see nothing (rt_kernels.hip): the camera pass walks a pass whose masks are 0, the resolve reads
# every sample.  Kernel for kernel the library before the two steps (tests/test_empty_pass_isa.py, profiles/isa_diff_empty_pass_vs_parent.txt); never
# loaded by the product path.
EMPTY_PASS_OFF_DEFINES = ["MI355RT_QC_EMPTY_PASS=0", "MI355RT_RESOLVE_SKIP=0"]


def build_empty_pass_off(force=False, verbose=False):
    # (with the later range arithmetic off as well, RANGE_OFF_DEFINES: "the library before the two steps" is the one the parent of that change built)
    return build_device_variant("empty_pass_off", EMPTY_PASS_OFF_DEFINES + RANGE_OFF_DEFINES, force=force, verbose=verbose)


POST_SRCS = [os.path.join(CSRC, "post", f) for f in ("post_reproject.hip", "post_plan.cpp", "post_api.cpp")]
POST_DEPS = POST_SRCS + [os.path.join(CSRC, "post", "post_plan.h"), os.path.join(CSRC, "device", "rt_math.h"), os.path.join(CSRC, "device", "rt_device.h"),
                         os.path.join(ROOT, "include", "mi355rt.h"), os.path.join(ROOT, "include", "mi355rt_post.h")]


def build_post(force=False, verbose=False):
    """libmi355rt_post.so: the device library's compiler and flags (gfx950, -ffp-contract=off, no xnack), its own sources."""
    os.makedirs(OUT, exist_ok=True)
    if force or _stale(POST_SO, POST_DEPS):
        cmd = [hipcc_path(), *HIPCC_FLAGS, "-o", POST_SO, *POST_SRCS]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
    return POST_SO


SVGF_SRCS = [os.path.join(CSRC, "svgf", f) for f in ("svgf_kernels.hip", "svgf_plan.cpp", "svgf_api.cpp")]
SVGF_DEPS = SVGF_SRCS + [os.path.join(CSRC, "svgf", "svgf_plan.h"), os.path.join(CSRC, "device", "rt_math.h"), os.path.join(CSRC, "device", "rt_device.h"),
                         os.path.join(ROOT, "include", "mi355rt.h"), os.path.join(ROOT, "include", "mi355rt_svgf.h")]


def build_svgf(force=False, verbose=False):
    """libmi355rt_svgf.so: the device library's compiler and flags (gfx950, -ffp-contract=off, no xnack), its own sources."""
    os.makedirs(OUT, exist_ok=True)
    if force or _stale(SVGF_SO, SVGF_DEPS):
        cmd = [hipcc_path(), *HIPCC_FLAGS, "-o", SVGF_SO, *SVGF_SRCS]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
    return SVGF_SO


def build_svgf_variant(name, defines=(), force=False, verbose=False):
    """libmi355rt_svgf_<name>.so: the same sources and flags with `defines`, a library of its own; never loaded by the product path and not part of
    build_all.  svgf.open_library(path) binds it."""
    os.makedirs(OUT, exist_ok=True)
    so = os.path.join(OUT, f"libmi355rt_svgf_{name}.so")
    if force or _stale(so, SVGF_DEPS):
        cmd = [hipcc_path(), *HIPCC_FLAGS, *[f"-D{d}" for d in defines], "-o", so, *SVGF_SRCS]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
    return so


# The library whose grids have at most 3 workgroups (svgf_plan.h: MAX_BLOCKS), so that a frame of 9 tiles walks every kernel's tile loop three times and
# one of 45 tiles fifteen times -- the trips a frame below 2^28 pixels never takes in the product library (tests/test_gpu_svgf_rough.py).
SVGF_GRID3_DEFINES = ["MI355RT_SVGF_MAX_BLOCKS=3"]


def build_svgf_grid3(force=False, verbose=False):
    return build_svgf_variant("grid3", SVGF_GRID3_DEFINES, force=force, verbose=verbose)


def build_host(force=False, verbose=False):
    os.makedirs(OUT, exist_ok=True)
    srcs = _host_srcs()
    if not srcs:
        raise RuntimeError("csrc/host has no sources")
    if force or _stale(HOST_SO, _host_deps()):
        cmd = ["g++", *CXX_FLAGS, "-shared", "-o", HOST_SO, *srcs, "-lz"]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
    return HOST_SO


def build_cli(force=False, verbose=False):
    src = os.path.join(CSRC, "tools", "rt_render.cpp")
    if not os.path.exists(src):
        return None
    build_device(force=False)
    build_host(force=False)
    if force or _stale(CLI, [src, DEVICE_SO, HOST_SO]):
        cmd = ["g++", *CXX_FLAGS, "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-o", CLI, src, "-L" + OUT, "-lmi355rt", "-lmi355rt_host",
               "-Wl,-rpath,$ORIGIN", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"]     # (HIP: --denoise-out's device buffers)
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
    return CLI


def build_verify(force=False, verbose=False):
    """tools/verify/short_arithmetic: the exhaustive comparison of rt_math.h's short reciprocal / square root / division (and rt_rng.h's
    range conversion) with the compiler's correctly rounded forms -- the product's headers, the product's flags, a standalone program
    that a gpu test runs (tests/test_gpu_short_arithmetic.py)."""
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "verify", "short_arithmetic.hip")
    exe = src[:-4]
    if force or _stale(exe, [src] + DEVICE_HEADERS):
        cmd = [hipcc_path(), *[f for f in HIPCC_FLAGS if f not in ("-fPIC", "-shared")], "-Wno-unused-value", "-Wno-unused-result", "-o", exe, src]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
    return exe


def build_verify_range(force=False, verbose=False):
    """tools/verify/range_arithmetic: the enumerations behind rt_math.h's range arithmetic (the closed-form second normalisation, the ranged first one,
    the reciprocal and the division without a fix-up) on the shipped functions -- the product's headers, the product's flags, a standalone program
    that a gpu test runs (tests/test_gpu_range_arithmetic.py)."""
    src = os.path.join(ROOT, "tools", "verify", "range_arithmetic.hip")
    exe = src[:-4]
    if force or _stale(exe, [src] + DEVICE_HEADERS):
        cmd = [hipcc_path(), *[f for f in HIPCC_FLAGS if f not in ("-fPIC", "-shared")], "-Wno-unused-value", "-Wno-unused-result", "-o", exe, src]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
    return exe


def build_all(force=False, verbose=False):
    return build_device(force, verbose=verbose), build_host(force, verbose=verbose), build_cli(force, verbose=verbose), build_post(force, verbose=verbose), build_svgf(force, verbose=verbose)


if __name__ == "__main__":
    import sys
    print(build_all(force="--force" in sys.argv, verbose=True))
