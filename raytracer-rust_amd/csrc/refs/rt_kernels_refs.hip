// rt_kernels_refs.hip -- the kernels' translation unit as the tests' reference build compiles it (build.build_device_variant with -DMI355RT_REFS
// takes this file in the place of csrc/device/rt_kernels.hip): the product's translation unit, unchanged, and behind it what has to see its
// inlined device functions -- unit_ball_cooperative and shade_and_regenerate's other pieces are defined there and nowhere declared.
// The product library is not built from this file, and neither it nor kernel_hash() contains anything it adds.
#ifndef MI355RT_REFS
#error "the reference build's translation unit: compile with -DMI355RT_REFS"
#endif
#include "../device/rt_kernels.hip"
#include "rt_scatter_wave_probe.h"   // k_probe_scatter_wave, mi355rt_debug_scatter_wave: the bounce's pieces on caller-chosen waves (tests/test_gpu_scatter_wave.py)
#include "rt_range_wave_probe.h"     // k_probe_range_wave, mi355rt_debug_range_wave: the range arithmetic's forms on caller-chosen waves (tests/test_gpu_range_wave.py)
