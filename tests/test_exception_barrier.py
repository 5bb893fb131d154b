"""mi355rt.h: "nothing aborts, nothing throws across the ABI".  Every extern "C" entry of libmi355rt.so and libmi355rt_host.so runs inside
an exception barrier; here host allocations are made to fail (RLIMIT_AS lowered after the libraries are loaded, in a subprocess) and the
calls must come back with MI355RT_ERR_OOM and a message -- not std::terminate.  No GPU and no compute: the calls fail before any HIP work.
Reference contract: the call the library replaces is infallible-or-panic inside one Rust process (src/renderer.rs:67)."""
import os
import subprocess
import sys
import textwrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = textwrap.dedent("""
    import ctypes as C, importlib, json, os, resource, sys
    sys.path.insert(0, sys.argv[1])
    abi = importlib.import_module("raytracer-rust_amd.abi")
    build = importlib.import_module("raytracer-rust_amd.build")
    dev = C.CDLL(build.DEVICE_SO); host = C.CDLL(build.HOST_SO)
    dev.mi355rt_last_error.restype = C.c_char_p; host.mi355rt_host_last_error.restype = C.c_char_p
    dev.mi355rt_rows_selected.argtypes = [C.POINTER(abi.Settings), C.POINTER(abi.Options), C.POINTER(C.c_uint32)]
    host.mi355rt_write_png.argtypes = [C.c_char_p, C.c_void_p, C.c_uint32, C.c_uint32]
    host.mi355rt_write_exr.argtypes = [C.c_char_p, C.c_void_p, C.c_uint32, C.c_uint32]
    out = {}
    st = abi.Settings(1, (1 << 24) - 1, 1, 1)                       # 16 M rows: the row list alone is 64 MB
    n = C.c_uint32()
    out["rows_ok"] = [dev.mi355rt_rows_selected(C.byref(st), None, C.byref(n)), n.value]
    W = H = 8192                                                     # write_png's raw scanlines: 192 MB
    img = (C.c_uint32 * 16)()                                        # never read: the allocation fails first
    vm = int([l for l in open("/proc/self/status") if l.startswith("VmSize")][0].split()[1]) * 1024
    resource.setrlimit(resource.RLIMIT_AS, (vm + (24 << 20), vm + (24 << 20)))
    out["rows"] = [dev.mi355rt_rows_selected(C.byref(st), None, C.byref(n)), dev.mi355rt_last_error().decode()]
    out["png"] = [host.mi355rt_write_png(os.path.join(sys.argv[2], "x.png").encode(), img, W, H), host.mi355rt_host_last_error().decode()]
    out["exr"] = [host.mi355rt_write_exr(os.path.join(sys.argv[2], "x.exr").encode(), img, 1 << 24, 1), host.mi355rt_host_last_error().decode()]
    out["png_file"] = os.path.exists(os.path.join(sys.argv[2], "x.png"))
    resource.setrlimit(resource.RLIMIT_AS, (resource.RLIM_INFINITY, resource.RLIM_INFINITY)) if False else None
    print(json.dumps(out))
""")


def test_allocation_failures_come_back_as_error_codes(tmp_path):
    import json
    script = tmp_path / "child.py"
    script.write_text(CHILD)
    out = subprocess.run([sys.executable, str(script), ROOT, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])          # -6 here would be SIGABRT: std::terminate
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r["rows_ok"] == [0, (1 << 24) - 1]                                   # the same call succeeds while memory is to be had
    assert r["rows"][0] == -4 and "allocation failed" in r["rows"][1]           # MI355RT_ERR_OOM
    assert r["png"][0] == -4 and "write_png" in r["png"][1] and not r["png_file"]
    assert r["exr"][0] == -4 and "write_exr" in r["exr"][1]


def test_every_entry_point_sits_behind_the_barrier():
    """Source check: every `mi355rt_*` function defined at file scope in ANY .cpp or .hip of csrc/device is an export of the built library and the other
    way round, each defined once; each `int` one opens with the guard; and the host writers open with theirs."""
    import importlib
    import re
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    isa_stats = importlib.import_module("isa_stats")
    build = importlib.import_module("raytracer-rust_amd.build")
    dev_dir = os.path.join(ROOT, "raytracer-rust_amd/csrc/device")
    src = {n: open(os.path.join(dev_dir, n)).read() for n in sorted(os.listdir(dev_dir)) if n.endswith((".cpp", ".hip", ".h"))}
    # a definition at file scope: return type and name at the start of a line, the parameter list, ` {`; what follows on that line and the next line
    definition = re.compile(r"^(?:extern \"C\" )?([A-Za-z_][\w ]*?[ \*]+)(mi355rt_\w+)\((?:[^()]|\([^()]*\))*\) \{([^\n]*)(?=\n([^\n]*))", re.M)
    defs = [(name, m.group(1).strip(), m.group(2), m.group(3), m.group(4)) for name, text in src.items() if not name.endswith(".h")
            for m in definition.finditer(text)]
    names = [d[2] for d in defs]
    assert len(names) == len(set(names)), sorted(n for n in names if names.count(n) > 1)
    # ... against the dynamic symbol table of the built library
    table = subprocess.check_output([os.path.join(isa_stats.LLVM, "llvm-readelf"), "--dyn-syms", "-W", build.DEVICE_SO], text=True)
    exported = {f[7] for f in (line.split() for line in table.splitlines()) if len(f) == 8 and f[3] == "FUNC" and f[6] != "UND" and f[7].startswith("mi355rt_")}
    assert set(names) == exported, (sorted(set(names) - exported), sorted(exported - set(names)))
    # every int-returning one, with what follows its opening brace.  The count is the parent tree's, where the barrier test saw 38 of them in three files
    # and four per-feature tests the other 12 in their .hip files: 38 + 3 (rt_radiance.hip) + 3 (rt_view.hip) + 2 (rt_probe.hip) + 4 (rt_noise.hip) = 50, and
    # mi355rt_debug_has_variant, whose one line calls nothing that throws.  Now: 9 in rt_api.cpp, 13 in rt_queries.cpp, 10 (and has_variant) in rt_debug.cpp,
    # 6 in rt_multi.cpp, 8 in rt_oneshot.cpp, 4 in rt_noise.hip, none elsewhere; 7 more exports return something else (two destroys, a version, four strings).
    ints = [d for d in defs if d[1] == "int"]
    per_file = {name: sum(1 for d in ints if d[0] == name) for name in src if any(d[0] == name for d in ints)}
    assert per_file == {"rt_api.cpp": 9, "rt_queries.cpp": 13, "rt_debug.cpp": 11, "rt_multi.cpp": 6, "rt_oneshot.cpp": 8, "rt_noise.hip": 4}, per_file
    assert len(ints) == 51 and len(defs) == 58
    bare = [d[2] for d in ints if d[3].strip() != "" or "return guard([&]() -> int {" not in d[4]]
    assert bare == ["mi355rt_debug_has_variant"], bare
    # the context struct is seen by the three sources that implement its calls, and by nothing else
    assert sorted(n for n, text in src.items() if '"rt_context.h"' in text) == ["rt_api.cpp", "rt_debug.cpp", "rt_queries.cpp"]
    # the handlers besides the barrier's own: rt_prepare.cpp's (fail_noexcept lives with the last error) and what rt_api.cpp held before the
    # calls with host buffers moved out of it -- the thread deal (now rt_host.h) and the part of mi355rt_render_multi (now rt_oneshot.cpp)
    assert sum(src[n].count("catch") for n in ("rt_api.cpp", "rt_queries.cpp", "rt_debug.cpp", "rt_oneshot.cpp", "rt_host.h", "rt_prepare.cpp")) >= 5
    png = open(os.path.join(ROOT, "raytracer-rust_amd/csrc/host/png_write.cpp")).read()
    assert png.count("return mi355rt_host::guard(") == 3
    # ... and EVERY `int mi355rt_*(...)` the host library defines, whichever file it lives in (bvh_build* and scene_load_json had
    # ad-hoc handlers that could throw again while building their message and had no catch (...))
    host_dir = os.path.join(ROOT, "raytracer-rust_amd/csrc/host")
    seen = []
    for name in sorted(os.listdir(host_dir)):
        if not name.endswith(".cpp"):
            continue
        src = open(os.path.join(host_dir, name)).read()
        for m in re.finditer(r"\n(?:extern \"C\" )?int (mi355rt_\w+)\((?:[^()]|\([^()]*\))*\) \{\n((?:.*\n){1,6})", src):
            seen.append(m.group(1))
            assert "mi355rt_host::guard(" in m.group(2), f"{name}: {m.group(1)} does not open with the barrier"
    assert {"mi355rt_bvh_build", "mi355rt_bvh_build_threads", "mi355rt_scene_load_json", "mi355rt_write_png", "mi355rt_write_pfm", "mi355rt_write_exr"} <= set(seen), seen
