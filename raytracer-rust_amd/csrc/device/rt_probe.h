// rt_probe.h -- launch interface of the surface-probe kernels (rt_probe.hip): mi355rt_context_probe_rays, mi355rt_context_probe_radiance.
// Internal to libmi355rt.so, shared by rt_probe.hip and rt_api.cpp.
#pragma once
#include "rt_device.h"
#include "rt_radiance.h"

namespace mi355rt {

// The caller's probes as the kernels read them: n mi355rt_probe records (32 B, 16-byte aligned: two 16-byte loads per probe).
struct ProbeParams {
    const void* probes;
};
// k_probe_rays: the rays of one sample index, n mi355rt_path_ray records.
struct ProbeRaysOut {
    void* rays;
    uint32_t n, sample, seed_lo, seed_hi;
};
constexpr uint32_t PROBE_TRIES = 64;               // rejected tries of the unit-ball point after which it is (0, 0, 0)

// The path kernels are instantiated per has_mesh; p.rays is not read.  The sum is radiance_sum<false>, instantiated in rt_probe.hip.
int launch_probe_rays(const ProbeParams& b, const ProbeRaysOut& r, void* stream);
int launch_probe_paths(const RadianceParams& p, const ProbeParams& b, const RadianceSum& s, bool has_mesh, uint32_t grid_paths, uint32_t grid_sum, void* stream);

// The host halves of the entry points, which stand in rt_probe.hip behind the exception barrier (as rt_view.hip's do).  Both need the context
// struct (rt_api.cpp); neither may be called outside a guard().
int context_probe_rays(mi355rt_context* ctx, const void* d_probes, uint32_t n, uint32_t sample, uint64_t seed, void* d_rays, void* hip_stream);
int context_probe_radiance(mi355rt_context* ctx, const mi355rt_radiance_params* params, const void* d_probes, uint32_t n, void* d_accum,
                           void* d_out_linear_or_null, void* d_scratch, void* hip_stream);

}  // namespace mi355rt
