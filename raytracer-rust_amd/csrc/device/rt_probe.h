// rt_probe.h -- launch interface of the surface-probe kernels (rt_probe.hip): mi355rt_context_probe_rays, mi355rt_context_probe_radiance.
// Internal to libmi355rt.so, shared by rt_probe.hip and rt_queries.cpp (the entry points).
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

}  // namespace mi355rt
