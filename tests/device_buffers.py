"""Device buffers for the GPU tests (not a test; imported like probe_cases): every buffer a call writes has guard bytes behind it, and every read
checks them.  torch is imported inside the functions, as in the tests."""
import numpy as np

F = np.float32
PATTERN = 0xA5
GUARD = 64                                                              # bytes behind every buffer: they keep the pattern


class Guarded:
    """A buffer of `size` bytes on `device` with `guard` bytes of PATTERN behind it; the payload starts as PATTERN too, or as `data`."""

    def __init__(self, size, data=None, guard=GUARD, device="cuda"):
        import torch
        self.size, self.guard = size, guard
        self.t = torch.full((size + guard,), PATTERN, dtype=torch.uint8, device=device)
        if data is not None:
            self.upload(data)

    @property
    def ptr(self):
        return self.t.data_ptr()

    def upload(self, records):
        import torch
        raw = np.ascontiguousarray(records).view(np.uint8).reshape(-1)
        assert raw.size == self.size
        self.t[:self.size].copy_(torch.from_numpy(raw.copy()))

    def fill_nan_f32(self):
        import torch
        self.t[:self.size].view(torch.float32).fill_(float("nan"))

    def read(self, dtype, what):
        """A copy of the payload as `dtype`, after checking that the guard is whole; `what` names the call and the buffer."""
        raw = self.t.cpu().numpy()
        assert len(raw) == self.size + self.guard and (raw[self.size:] == PATTERN).all(), f"{what}: written past its end"
        return raw[:self.size].view(dtype).copy()

    def untouched(self):
        return bool((self.t.cpu().numpy() == PATTERN).all())


def packed_of(linear):
    """src/color.rs:87-93 (color_to_u32 of renderer.rs:112-120's sqrt(mean)) in numpy float32: sqrt, clamp to [0, 1] (a NaN becomes 0 by the cast's
    rule), * 255, truncate; 0x00RRGGBB."""
    with np.errstate(invalid="ignore"):
        c = np.sqrt(np.asarray(linear, F))
        c = np.where(c < 0, F(0), np.where(c > 1, F(1), c)).astype(F) * F(255.0)
        w = np.where(np.isnan(c), 0, c).astype(np.uint32)
    return ((w[..., 0] << 16) | (w[..., 1] << 8) | w[..., 2]).astype(np.uint32)


class RadianceBuffers:
    """The device buffers of one call of the radiance family (`call` names it: trace_radiance, render_view, probe_radiance) over n rays, pixels or
    probes: rays, float4 sums, means, scratch, with `packed` the packed words and with `probes` the 32-byte probe records.  fill_nan: the sums start as
    NaN (a call with sample_begin == 0 must not read them)."""

    def __init__(self, call, n, scratch_bytes, packed=False, probes=None, fill_nan=True):
        self.call, self.n = call, n
        self.rays, self.accum, self.linear, self.scratch = Guarded(n * 32), Guarded(n * 16), Guarded(n * 12), Guarded(scratch_bytes)
        self.packed = Guarded(n * 4) if packed else None
        self.probes = Guarded(n * 32, probes) if probes is not None else None
        if fill_nan:
            self.accum.fill_nan_f32()

    def read_rays(self, abi, maker):
        return self.rays.read(abi.PATH_RAY_DTYPE, f"{maker}: rays")

    def read(self):
        """(sums float32 [n, 4], means float32 [n, 3]) and with `packed` (..., packed uint32 [n]), after checking every guard."""
        self.scratch.read(np.uint8, f"{self.call}: scratch")
        out = (self.accum.read(F, f"{self.call}: sums").reshape(-1, 4), self.linear.read(F, f"{self.call}: means").reshape(-1, 3))
        return out + ((self.packed.read(np.uint32, f"{self.call}: packed"),) if self.packed is not None else ())

    def by_query(self, ctx, abi, S, rays_of, depth, seed=0):
        """Through mi355rt_context_trace_radiance: one call [s, s + 1) per sample along rays_of(s), the sums carried.  (sums, means)."""
        import torch
        for s in range(S):
            self.rays.upload(rays_of(s))
            ctx.trace_radiance(abi.RadianceParams.make(s, s + 1, depth, seed), self.rays.ptr, self.n, self.accum.ptr, self.scratch.ptr, self.linear.ptr)
        torch.cuda.synchronize()
        ctx.check()
        return self.read()[:2]


def scene_contexts(device, abi, scenes):
    """Yields {name: a context holding scenes[name]}, with a view the calls never look at; closes all of them at the end."""
    out = {}
    try:
        for name, sc in scenes.items():
            out[name] = device.Context(0)
            out[name].set_scene(sc, abi.Camera(), abi.Settings(1, 1, 1, 1))
        yield out
    finally:
        for c in out.values():
            c.close()
