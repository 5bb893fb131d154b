// post_api.cpp -- the exports of libmi355rt_post.so (include/mi355rt_post.h): the thread-local last error, the exception barrier of the
// library's own, and mi355rt_post_reproject -- the plan (post_plan.cpp, no HIP), the device, the launch (post_reproject.hip).
// The library links nothing of libmi355rt.so: a host may load both, and no symbol is defined twice (namespace mi355rt_post, mi355rt_post_*).
#include <hip/hip_runtime_api.h>

#include <new>
#include <stdexcept>
#include <string>

#include "post_plan.h"

namespace mi355rt_post {

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

}  // namespace

}  // namespace mi355rt_post

using namespace mi355rt_post;

extern "C" {

const char* mi355rt_post_last_error(void) { return last_error().c_str(); }
uint32_t mi355rt_post_abi_version(void) { return MI355RT_POST_ABI_VERSION; }

int mi355rt_post_reproject(int hip_device, const mi355rt_view* cur, const mi355rt_view* prev_or_null, const mi355rt_reproject_params* params_or_null,
                           const void* d_hits_cur, const void* d_color_cur, const void* d_hits_prev_or_null, const void* d_hist_prev_or_null,
                           void* d_hist_out, void* d_out_linear_or_null, void* d_out_packed_or_null, void* hip_stream) {
    return guard([&]() -> int {
    static_assert(sizeof(mi355rt_reproject_params) == 16 && sizeof(mi355rt_view) == 96, "the records of mi355rt_post.h");
    ReprojectPlan plan{};
    std::string why;
    if (int rc = plan_reproject(hip_device, cur, prev_or_null, params_or_null, d_hits_cur, d_color_cur, d_hits_prev_or_null, d_hist_prev_or_null,
                                d_hist_out, d_out_linear_or_null, d_out_packed_or_null, plan, why)) return fail(rc, why);
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(MI355RT_ERR_NO_DEVICE, "reproject: no HIP device visible (this library has no CPU path)");
    if (hip_device >= n) return fail(MI355RT_ERR_NO_DEVICE, "reproject: hip_device out of range");
    if (hipError_t e = hipSetDevice(hip_device)) return fail(MI355RT_ERR_HIP, std::string("reproject: hipSetDevice: ") + hipGetErrorString(e));
    const ReprojectBuffers b{d_hits_cur, d_color_cur, d_hits_prev_or_null, d_hist_prev_or_null, d_hist_out, d_out_linear_or_null, d_out_packed_or_null};
    if (int e = launch_reproject(plan, b, hip_stream)) return fail(MI355RT_ERR_HIP, std::string("reproject: k_post_reproject launch failed: ") + hipGetErrorString((hipError_t)e));
    return MI355RT_OK;
    });
}

}  // extern "C"
