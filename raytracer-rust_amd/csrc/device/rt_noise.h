// rt_noise.h -- the layout the noise kernels (rt_noise.hip) keep on the device: mi355rt_noise_device_*.
// Internal to libmi355rt.so.  The estimate itself and the reduction tree are defined in include/mi355rt.h.
#pragma once
#include "rt_prepare.h"

namespace mi355rt {

// A tile is NOISE_TILE consecutive pixels, one per lane of a workgroup of NOISE_TILE threads (NOISE_WAVES waves of 64).  The cut depends on the
// pixel count alone, so the tree of mean_error does not change with the launch geometry.
constexpr uint32_t NOISE_TILE = 256, NOISE_WAVES = NOISE_TILE / 64;

// The state of a pixel, two 16-byte words in two planes: prev[p] = {r, g, b, 0} (the last running sums) and tq[p] = {T, Q}.
// One record per tile, written by k_noise_evaluate and read by k_noise_finish:
struct NoisePartial {            // 32 bytes
    double sum, max;             // of err over the tile's counted pixels (the tile tree of mi355rt.h); 0 when there is none
    uint64_t above, nonfinite;
};
static_assert(sizeof(NoisePartial) == 32, "two 16-byte words per tile");

}  // namespace mi355rt
