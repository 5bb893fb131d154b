// svgf_api.cpp -- the exports of libmi355rt_svgf.so (include/mi355rt_svgf.h): the thread-local last error, the exception barrier of the
// library's own, and the calls -- the plan (svgf_plan.cpp, no HIP), the device, the launches (svgf_kernels.hip).
// The library links nothing of libmi355rt.so or libmi355rt_post.so: a host may load all three, and no symbol is defined twice (namespace
// mi355rt_svgf, mi355rt_svgf_*).
#include <hip/hip_runtime_api.h>

#include <new>
#include <stdexcept>
#include <string>

#include "svgf_plan.h"

namespace mi355rt_svgf {

namespace {

std::string& last_error() { thread_local std::string text; return text; }

int fail(int code, const std::string& msg) { last_error() = msg; return code; }

// (assigning a short literal to a string that exists allocates nothing, or reuses what it holds; should even that throw, the old text stays)
int fail_noexcept(int code, const char* msg) noexcept { try { last_error() = msg; } catch (...) {} return code; }

// Nothing throws across the ABI: std::bad_alloc / std::length_error -> MI355RT_ERR_OOM, anything else -> MI355RT_ERR_HIP.
template <class F> int guard(F&& f) noexcept {
    try { return f(); }
    catch (const std::bad_alloc&) { return fail_noexcept(MI355RT_ERR_OOM, "host allocation failed (std::bad_alloc)"); }
    catch (const std::length_error&) { return fail_noexcept(MI355RT_ERR_OOM, "host allocation failed (std::length_error)"); }
    catch (const std::exception& e) {
        try { return fail(MI355RT_ERR_HIP, std::string("unexpected C++ exception: ") + e.what()); } catch (...) { return fail_noexcept(MI355RT_ERR_HIP, "unexpected C++ exception"); }
    }
    catch (...) { return fail_noexcept(MI355RT_ERR_HIP, "unexpected C++ exception"); }
}

// The device of a call whose arguments passed: MI355RT_OK with hip_device current, or the code and the text.
int take_device(const char* call, int hip_device) {
    const std::string c(call);
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(MI355RT_ERR_NO_DEVICE, c + ": no HIP device visible (this library has no CPU path)");
    if (hip_device >= n) return fail(MI355RT_ERR_NO_DEVICE, c + ": hip_device out of range");
    if (hipError_t e = hipSetDevice(hip_device)) return fail(MI355RT_ERR_HIP, c + ": hipSetDevice: " + hipGetErrorString(e));
    return MI355RT_OK;
}

}  // namespace

}  // namespace mi355rt_svgf

using namespace mi355rt_svgf;

extern "C" {

const char* mi355rt_svgf_last_error(void) { return last_error().c_str(); }
uint32_t mi355rt_svgf_abi_version(void) { return MI355RT_SVGF_ABI_VERSION; }

int mi355rt_svgf_scratch_bytes(uint32_t width, uint32_t height, uint64_t* out_bytes) {
    return guard([&]() -> int {
    std::string why;
    if (int rc = plan_scratch_bytes(width, height, out_bytes, why)) return fail(rc, why);
    return MI355RT_OK;
    });
}

int mi355rt_svgf_accumulate(int hip_device, const mi355rt_view* cur, const mi355rt_view* prev_or_null, const mi355rt_svgf_accumulate_params* params_or_null,
                            const void* d_hits_cur, const void* d_color_cur, const void* d_hits_prev_or_null, const void* d_hist_prev_or_null,
                            const void* d_moments_prev_or_null, void* d_hist_out, void* d_moments_out, void* d_variance_out, void* hip_stream) {
    return guard([&]() -> int {
    static_assert(sizeof(mi355rt_svgf_accumulate_params) == 32 && sizeof(mi355rt_svgf_filter_params) == 24 && sizeof(mi355rt_view) == 96, "the records of mi355rt_svgf.h");
    AccumulatePlan plan{};
    std::string why;
    if (int rc = plan_accumulate(hip_device, cur, prev_or_null, params_or_null, d_hits_cur, d_color_cur, d_hits_prev_or_null, d_hist_prev_or_null,
                                 d_moments_prev_or_null, d_hist_out, d_moments_out, d_variance_out, plan, why)) return fail(rc, why);
    if (int rc = take_device("accumulate", hip_device)) return rc;
    const AccumulateBuffers b{d_hits_cur, d_color_cur, d_hits_prev_or_null, d_hist_prev_or_null, d_moments_prev_or_null, d_hist_out, d_moments_out, d_variance_out};
    if (int e = launch_accumulate(plan, b, hip_stream)) return fail(MI355RT_ERR_HIP, std::string("accumulate: kernel launch failed: ") + hipGetErrorString((hipError_t)e));
    return MI355RT_OK;
    });
}

int mi355rt_svgf_filter(int hip_device, uint32_t width, uint32_t height, const mi355rt_svgf_filter_params* params_or_null,
                        const void* d_hist_in, const void* d_variance_in, const void* d_hits, void* d_scratch,
                        void* d_out_linear_or_null, void* d_out_packed_or_null, void* hip_stream) {
    return guard([&]() -> int {
    FilterPlan plan{};
    std::string why;
    if (int rc = plan_filter(hip_device, width, height, params_or_null, d_hist_in, d_variance_in, d_hits, d_scratch, d_out_linear_or_null, d_out_packed_or_null, plan, why))
        return fail(rc, why);
    if (int rc = take_device("filter", hip_device)) return rc;
    const FilterBuffers b{d_hist_in, d_variance_in, d_hits, d_scratch, d_out_linear_or_null, d_out_packed_or_null};
    if (int e = launch_filter(plan, b, hip_stream)) return fail(MI355RT_ERR_HIP, std::string("filter: kernel launch failed: ") + hipGetErrorString((hipError_t)e));
    return MI355RT_OK;
    });
}

}  // extern "C"
