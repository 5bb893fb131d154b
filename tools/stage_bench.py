"""What the stage benches (radiance_bench, view_bench, probe_bench, occlusion_bench, denoise_bench, reproject_bench, query_bench) share: the
package's modules, the no-GPU exit, the timed batches, the interleaved rounds, the kernel table and the report's first line and tail.  No main
of its own.  A tool imports torch before it calls anything here (tests/conftest.py: one HIP runtime in the process)."""
import importlib
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tools"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def packages(*names):
    """The modules of raytracer-rust_amd asked for, in that order."""
    return [importlib.import_module("raytracer-rust_amd." + n) for n in names]


def require_gpu(tool_name):
    import torch
    if not torch.cuda.is_available():
        sys.exit(f"{tool_name}: no GPU visible -- nothing is measured on the CPU")


def timed_batch(stream, call, batch):
    """ms per call: one pair of device events around `batch` calls enqueued back to back."""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(batch):
        call()
    b.record(stream)
    torch.cuda.synchronize()
    return a.elapsed_time(b) / batch


def timed_launches(stream, call, batch):
    """[ms] of `batch` calls enqueued back to back, each between a pair of device events of its own."""
    import torch
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(batch)]
    for a, b in evs:
        a.record(stream); call(); b.record(stream)
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in evs]


def render_kernel_batch(ctx, d_packed, stream_handle, batch):
    """(path-tracing kernel ms, resolve kernel ms) per call of `batch` mi355rt_context_render calls, from the timing pool (summed over the bands)."""
    import torch
    for _ in range(batch):
        ctx.render(d_packed.data_ptr(), None, None, stream_handle)
    torch.cuda.synchronize()
    r, v, _ = ctx.read_timing()
    return r / batch, v / batch


def interleaved_rounds(calls, seconds, batch, timed=None, after_round=None, warmed=None):
    """calls: {line: call()}.  A warm-up batch of every line, in order (warmed(line) after each: where a tool records what the line computed); then
    rounds of one batch per line, in order, and after_round() behind each, until every line has at least `seconds` of timed work.
    timed(call) -> ms per call of one batch; None: timed_batch on the current stream.  {line: [ms per call, one per round]}."""
    if timed is None:
        import torch
        stream = torch.cuda.current_stream()
        timed = lambda call: timed_batch(stream, call, batch)
    for name, call in calls.items():
        timed(call)
        if warmed:
            warmed(name)
    ms = {name: [] for name in calls}
    while min(sum(v) * batch for v in ms.values()) < seconds * 1e3:
        for name, call in calls.items():
            ms[name].append(timed(call))
        if after_round:
            after_round()
    return ms


def summary(ms):
    """({line: median}, {line: (max - min) / median}) of {line: [ms]}."""
    med = {k: statistics.median(v) for k, v in ms.items()}
    return med, {k: (max(v) - min(v)) / med[k] for k, v in ms.items()}


def kernel_table(so, match, name_width, insts=True):
    """The registers, spills and code size of the kernels of `so` whose short name match() accepts (None: all), as the comment lines of a report,
    and {short name: stats} of those kernels (tools/isa_stats.py)."""
    import isa_stats
    cols = [("code B", 7, "code_bytes")] + ([("insts", 6, "insts")] if insts else []) + \
           [("vgpr", 5, "vgpr_count"), ("sgpr", 5, "sgpr_count"), ("vspill", 6, "vgpr_spill_count"), ("sspill", 6, "sgpr_spill_count"),
            ("private B", 9, "private_segment_fixed_size"), ("LDS B", 6, "group_segment_fixed_size"), ("scratch_ insts", 14, "scratch_insts")]
    rows = sorted(((isa_stats.short(k), st) for k, st in isa_stats.kernel_stats(so).items()), key=lambda row: row[0])
    rows = [row for row in rows if match is None or match(row[0])]
    lines = [f"# {'kernel':{name_width}s} " + " ".join(f"{title:>{w}s}" for title, w, _ in cols)]
    lines += [f"# {k:{name_width}s} " + " ".join(f"{st.get(key, 0):{w}d}" for _, w, key in cols) for k, st in rows]
    return lines, dict(rows)


def header(tool, args_text, device_name=True):
    """The first line of a report: the command, build.kernel_hash() and, unless the tool's own process holds no GPU, the device's name."""
    build, = packages("build")
    line = f"# python tools/{tool}.py {args_text}   kernel_hash {build.kernel_hash()}"
    if device_name:
        import torch
        line += f"   {torch.cuda.get_device_name(0)}"
    return line


def write_report(lines, out, echo=True):
    """Prints the report (echo=False: the tool printed its lines as they came) and writes it to `out`."""
    if echo:
        print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", out)
