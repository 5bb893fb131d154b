"""Surface probes on the resident scene (mi355rt_context_probe_rays, mi355rt_context_probe_radiance): cosine-hemisphere rays made on the device
from caller-supplied points and normals, in front of the radiance queries' path loop.

The references are the numpy maker of tests/probe_cases.py (bit for bit: a ray is + - * / sqrt), mi355rt_context_trace_radiance called once per
sample along the maker's rays (probe_radiance's definition), and two scenes whose answer is known exactly: a furnace and a light behind the surface."""
import numpy as np
import pytest

import probe_cases as PC
import view_cases as VC
from conftest import load_for_both
from device_buffers import RadianceBuffers, scene_contexts

pytestmark = pytest.mark.gpu

F = np.float32


# ---- device plumbing ------------------------------------------------------------------------------------------------------------------
def buffers(device, probes, samples=1, fill_nan=True):
    """The buffers of n probes and up to `samples` samples per call, the probe records among them."""
    return RadianceBuffers("probe_radiance", len(probes), device.radiance_scratch_bytes(len(probes), samples), probes=probes, fill_nan=fill_nan)


def probe_radiance(ctx, abi, buf, begin, end, depth=PC.DEPTH, seed=0, stream=None):
    ctx.probe_radiance(abi.RadianceParams.make(begin, end, depth, seed), buf.probes.ptr, buf.n, buf.accum.ptr, buf.scratch.ptr,
                       buf.linear.ptr, stream)


def one_call(device, abi, ctx, probes, S, depth=PC.DEPTH, seed=0):
    import torch
    buf = buffers(device, probes, S)
    probe_radiance(ctx, abi, buf, 0, S, depth, seed)
    torch.cuda.synchronize()
    ctx.check()
    return buf.read()


def by_query(device, abi, oracle_mod, ctx, probes, S, depth=PC.DEPTH, seed=0):
    """The probes through mi355rt_context_trace_radiance: one call per sample along the maker's rays, the sums carried.  (sums, means)."""
    return buffers(device, probes).by_query(ctx, abi, S, lambda s: PC.probe_rays(oracle_mod, abi, probes, s, seed), depth, seed)


def device_rays(device, abi, ctx, probes, s, seed):
    import torch
    buf = buffers(device, probes)
    ctx.probe_rays(buf.probes.ptr, buf.n, s, buf.rays.ptr, seed)
    torch.cuda.synchronize()
    return buf.read_rays(abi, "probe_rays")


def sphere_scene(abi, host, centre, radius, colour, miss):
    """One emissive sphere."""
    from oracle import scene_loader as L
    m = abi.Material(); m.kind = abi.MAT_EMISSIVE
    m.albedo[:] = [float(F(v)) for v in colour]
    p = abi.Primitive(); p.kind, p.material = abi.PRIM_SPHERE, 0
    p.data[0:4] = [float(F(v)) for v in centre] + [float(F(radius))]
    sc = L.LoadedScene()
    sc.materials, sc.primitives, sc.meshes = [m], [p], []
    sc.triangles = np.zeros((0, 12), F)
    sc.finalize()
    sc.c.miss_color[:] = [float(F(v)) for v in miss]
    sc._keep = host.attach_bvh(sc)
    return sc


@pytest.fixture(scope="module")
def scenes(native, oracle_mod, abi):
    host, _ = native
    return {n: load_for_both(n, oracle_mod, host, width=PC.W, height=PC.H, spp=1, max_depth=PC.DEPTH) for n in PC.SCENES}


@pytest.fixture(scope="module")
def sets(scenes, oracle_mod, abi):
    return {n: PC.probe_set(oracle_mod, abi, n, scenes[n]) for n in PC.SCENES}


@pytest.fixture(scope="module")
def contexts(native, abi, scenes):
    """One context per scene, with a view the calls never look at."""
    yield from scene_contexts(native[1], abi, scenes)


# ---- 1: the rays ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PC.SCENES)
def test_probe_rays_are_the_numpy_makers_word_for_word(name, native, oracle_mod, abi, sets, contexts):
    _, device = native
    probes = sets[name]
    worst = 0
    for seed in PC.SEEDS:
        for s in range(max(PC.SAMPLES)):
            want, _, tried, _ = PC.probe_rays(oracle_mod, abi, probes, s, seed, want=True)
            worst = max(worst, int(tried.max()))
            got = device_rays(device, abi, contexts[name], probes, s, seed)
            assert got.tobytes() == want.tobytes(), (seed, s)
        for n in PC.counts(len(probes))[:2]:                                   # one probe, 37 probes: the launch's only wave is a partial one
            got = device_rays(device, abi, contexts[name], probes[:n], 3, seed)
            assert got.tobytes() == PC.probe_rays(oracle_mod, abi, probes[:n], 3, seed).tobytes(), (seed, n)
        # d = N + normalized(p) exactly zero: the near_zero branch on the device, the ray leaves along N
        cancel = PC.cancelling_probes(oracle_mod, abi, probes[:37], seed)
        want, _, _, nz = PC.probe_rays(oracle_mod, abi, cancel, 0, seed, want=True)
        assert nz.all()
        got = device_rays(device, abi, contexts[name], cancel, 0, seed)
        assert got.tobytes() == want.tobytes(), (seed, "near_zero")
        assert (got["direction"] == cancel["normal"]).sum() > 0 and np.abs(got["direction"] - cancel["normal"]).max() < 1e-6
    assert worst >= 4                                                           # rejected tries ran on the device
    got = device_rays(device, abi, contexts[name], probes, 0xFFFFFFFF, 2 ** 64 - 1)                       # any 32-bit sample index, any 64-bit seed
    assert got.tobytes() == PC.probe_rays(oracle_mod, abi, probes, 0xFFFFFFFF, 2 ** 64 - 1).tobytes()


# ---- 2: probe_radiance is the query along the maker's rays --------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("S", PC.SAMPLES)
@pytest.mark.parametrize("count", [0, 1, 2])
@pytest.mark.parametrize("name", PC.SCENES)
def test_probe_radiance_is_the_radiance_query_along_the_makers_rays(name, count, S, seed, native, oracle_mod, abi, sets, contexts):
    _, device = native
    seed = PC.SEEDS[seed]
    n = PC.counts(len(sets[name]))[count]
    probes = sets[name][len(sets[name]) - n:] if count == 1 else sets[name][:n]              # 37: the free-space probes and the odd normals among them
    assert (n * S) % 64 != 0
    sums, means = one_call(device, abi, contexts[name], probes, S, PC.DEPTH, seed)
    want_sums, want_means = by_query(device, abi, oracle_mod, contexts[name], probes, S, PC.DEPTH, seed)
    assert sums.tobytes() == want_sums.tobytes() and means.tobytes() == want_means.tobytes()
    assert np.isfinite(means).all() and (sums[:, 3] == 0).all()
    if n > 1:
        assert len(np.unique(means, axis=0)) > 1


@pytest.mark.parametrize("name", PC.SCENES)
def test_the_near_zero_branch_in_the_path_kernel(name, native, oracle_mod, abi, sets, contexts):
    _, device = native
    for seed in PC.SEEDS:
        cancel = PC.cancelling_probes(oracle_mod, abi, sets[name][:37], seed)
        sums, means = one_call(device, abi, contexts[name], cancel, 1, PC.DEPTH, seed)
        want_sums, want_means = by_query(device, abi, oracle_mod, contexts[name], cancel, 1, PC.DEPTH, seed)
        assert sums.tobytes() == want_sums.tobytes() and means.tobytes() == want_means.tobytes()


# ---- 3: chunking and K ----------------------------------------------------------------------------------------------------------------------
_whole = {}


def whole(device, abi, contexts, sets):
    """[0, 17) of cornell's whole set in one call with the default K: computed once, shared, read-only."""
    if "cornell" not in _whole:
        out = one_call(device, abi, contexts["cornell"], sets["cornell"], 17, PC.DEPTH, PC.SEEDS[1])
        for a in out:
            a.setflags(write=False)
        _whole["cornell"] = out
    return _whole["cornell"]


def test_any_chunking_gives_the_words_of_one_call(native, abi, sets, contexts):
    import torch
    _, device = native
    sums, means = whole(device, abi, contexts, sets)
    assert np.isfinite(sums).all() and (sums[:, :3] > 0).any()             # the NaN the sums were pre-filled with was not read
    for chunks in (((0, 5), (5, 16), (16, 17)), ((0, 16), (16, 17)), tuple((s, s + 1) for s in range(17))):
        buf = buffers(device, sets["cornell"], 16)                         # the scratch is sized for the largest chunk
        for a, b in chunks:
            probe_radiance(contexts["cornell"], abi, buf, a, b, PC.DEPTH, PC.SEEDS[1])
        torch.cuda.synchronize()
        got = buf.read()
        assert got[0].tobytes() == sums.tobytes() and got[1].tobytes() == means.tobytes(), chunks


@pytest.mark.parametrize("K", [1, 2, 64])
def test_items_per_lane_does_not_change_a_word(K, native, abi, sets, contexts):
    _, device = native
    ctx = contexts["cornell"]
    want = whole(device, abi, contexts, sets)                              # 298 * 17 = 5066 items: 80 waves at K = 1, 2 at K = 64
    try:
        ctx.set_knob("radiance_items", K)
        got = one_call(device, abi, ctx, sets["cornell"], 17, PC.DEPTH, PC.SEEDS[1])
    finally:
        ctx.set_knob("radiance_items", 0)
    assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want))


# ---- 4: scenes with a known answer ----------------------------------------------------------------------------------------------------------
def test_inside_a_furnace_the_mean_is_the_furnaces_colour(native, abi):
    """Every ray from inside an emissive sphere ends on it with throughput 1: sixteen samples of (0.5, 0.25, 1.0) sum without rounding, and
    * (1 / 16) is exact."""
    host, device = native
    colour = (0.5, 0.25, 1.0)
    sc = sphere_scene(abi, host, (0.0, 1.0, 0.0), 10.0, colour, (0.0, 0.0, 0.0))
    probes = np.concatenate([PC.free_probes(abi), PC.odd_probes(abi)])     # any normal will do: a zero normal's ray is normalized(p)
    ctx = device.Context(0)
    try:
        ctx.set_scene(sc, abi.Camera(), abi.Settings(1, 1, 1, 1))
        sums, means = one_call(device, abi, ctx, probes, 16, PC.DEPTH, 9)
        assert (means == np.array(colour, F)[None, :]).all() and (sums[:, :3] == F(16.0) * np.array(colour, F)[None, :]).all()
        _, means = one_call(device, abi, ctx, probes, 16, 0, 9)            # max_depth 0: 1 * BLACK
        assert (means.view(np.uint32) == 0).all()
    finally:
        ctx.close()


def test_a_light_behind_the_tangent_plane_is_not_seen(native, abi):
    """Probes on the shell of radius 5 about an emissive sphere of radius 2, the normals pointing away from it: the sphere lies wholly behind every
    tangent plane, every direction has dot(d, N) >= 0, so every ray misses and every mean is the miss colour -- exactly (dyadic, 16 samples).  With the
    normals turned round the light is seen."""
    host, device = native
    miss = (0.25, 0.5, 0.125)
    sc = sphere_scene(abi, host, (0.0, 0.0, 0.0), 2.0, (4.0, 4.0, 4.0), miss)
    probes = PC.free_probes(abi, 60, seed=5)
    probes["position"] = probes["normal"] * F(5.0)
    ctx = device.Context(0)
    try:
        ctx.set_scene(sc, abi.Camera(), abi.Settings(1, 1, 1, 1))
        _, means = one_call(device, abi, ctx, probes, 16, PC.DEPTH, 3)
        assert (means == np.array(miss, F)[None, :]).all()
        probes["normal"] = -probes["normal"]
        _, means = one_call(device, abi, ctx, probes, 16, PC.DEPTH, 3)
        # the sphere fills the form factor (2 / 5)^2 = 0.16 of the hemisphere: a probe's 16 samples all miss it with probability 0.84^16 = 0.06
        assert (means.max(axis=1) > 0.5).mean() > 0.5 and (means >= np.array(miss, F)[None, :]).all()
    finally:
        ctx.close()


# ---- 5: beside a render ---------------------------------------------------------------------------------------------------------------------
def test_beside_a_render_of_the_same_context(native, oracle_mod, abi, sets):
    """A probe_radiance enqueued on a second stream while a render of the same context is in flight: both results are those of their solo runs."""
    import torch
    host, device = native
    W, H = 64, 48
    sc = load_for_both("cornell", oracle_mod, host, width=W, height=H, spp=16, max_depth=8)
    ctx = device.Context(0)
    try:
        ctx.set_scene(sc, sc.camera, sc.settings)
        probes = sets["cornell"]
        want = one_call(device, abi, ctx, probes, 17, PC.DEPTH, 5)
        want_packed = torch.zeros((H, W), dtype=torch.int32, device="cuda")
        ctx.render(want_packed.data_ptr())
        torch.cuda.synchronize()
        s_render, s_probe = torch.cuda.Stream(), torch.cuda.Stream()
        packed = torch.zeros((H, W), dtype=torch.int32, device="cuda")
        buf = buffers(device, probes, 17)
        torch.cuda.synchronize()
        ctx.render(packed.data_ptr(), None, None, s_render.cuda_stream)
        probe_radiance(ctx, abi, buf, 0, 17, PC.DEPTH, 5, stream=s_probe.cuda_stream)
        ctx.render(packed.data_ptr(), None, None, s_render.cuda_stream)
        torch.cuda.synchronize()
        ctx.check()
        got = buf.read()
        assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want))
        assert torch.equal(packed, want_packed)
    finally:
        ctx.close()


# ---- 6: refusals on a live context ----------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_sums_untouched_and_one_probe_works(native, oracle_mod, abi, sets, contexts):
    import torch
    _, device = native
    ctx = contexts["cornell"]
    probes = sets["cornell"][:5]
    buf = buffers(device, probes, 4, fill_nan=False)
    prm = abi.RadianceParams.make(0, 4, PC.DEPTH)

    def refused(word, params=prm, probes_at=None, n=5, accum=None, scratch=None, linear=None):
        with pytest.raises(device.RenderError) as e:
            ctx.probe_radiance(params, buf.probes.ptr if probes_at is None else probes_at, n, buf.accum.ptr if accum is None else accum,
                               buf.scratch.ptr if scratch is None else scratch, linear)
        assert e.value.rc == abi.ERR_INVALID and word in str(e.value) and "probe_radiance: " in str(e.value), (word, str(e.value))

    refused("params.sample_begin", params=abi.RadianceParams.make(4, 4, PC.DEPTH))
    refused("params.flags", params=abi.RadianceParams(0, 4, PC.DEPTH, 1, 0, 0))
    refused("params.reserved", params=abi.RadianceParams(0, 4, PC.DEPTH, 0, 0, 1))
    refused("d_probes must be 16-byte aligned", probes_at=buf.probes.ptr + 8)
    refused("d_accum must be 16-byte aligned", accum=buf.accum.ptr + 4)
    refused("d_scratch must be 16-byte aligned", scratch=buf.scratch.ptr + 8)
    refused("d_out_linear must be 4-byte aligned", linear=buf.linear.ptr + 2)
    refused("split the call", params=abi.RadianceParams.make(0, 65536, PC.DEPTH), n=65536)
    with pytest.raises(device.RenderError) as e:
        ctx.probe_radiance(prm, None, 5, buf.accum.ptr, buf.scratch.ptr)
    assert "d_probes is null" in str(e.value)
    with pytest.raises(device.RenderError) as e:
        ctx.probe_rays(buf.probes.ptr, 5, 0, buf.rays.ptr + 8)
    assert "probe_rays: d_rays must be 16-byte aligned" in str(e.value)
    with pytest.raises(device.RenderError) as e:
        ctx.probe_rays(buf.probes.ptr + 4, 5, 0, buf.rays.ptr)
    assert "probe_rays: d_probes must be 16-byte aligned" in str(e.value)
    ctx.probe_radiance(prm, None, 0, None, None)                           # n == 0: MI355RT_OK, nothing is looked at
    ctx.probe_rays(None, 0, 0, None)
    torch.cuda.synchronize()
    ctx.check()
    assert all(t.untouched() for t in (buf.accum, buf.linear, buf.scratch, buf.rays))      # nothing was enqueued
    # one probe, one sample: the query along the maker's ray, and the same words again
    one = sets["cornell"][7:8]
    sums, means = one_call(device, abi, ctx, one, 1, PC.DEPTH, 0)
    want_sums, want_means = by_query(device, abi, oracle_mod, ctx, one, 1, PC.DEPTH, 0)
    assert sums.tobytes() == want_sums.tobytes() and means.tobytes() == want_means.tobytes()
    assert sums[0, :3].tobytes() == means[0].tobytes() and sums[0, 3] == 0
    sums2, _ = one_call(device, abi, ctx, one, 1, PC.DEPTH, 0)
    assert sums2.tobytes() == sums.tobytes()
