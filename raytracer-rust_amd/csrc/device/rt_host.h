// rt_host.h -- the HIP-side pieces shared by the C-ABI sources of libmi355rt.so (rt_api.cpp: the context and its renders; rt_queries.cpp: the calls that
// only read the resident scene; rt_debug.cpp: the debug hooks; rt_multi.cpp: the multi-device context; rt_oneshot.cpp: the calls with host buffers): HIP_TRY, device buffers, the scope that
// puts the calling thread's device back, the options of a call that deals the strips itself, and the deal of a call's parts over host
// threads.  The thread-local last error, the exception barrier of every extern "C" entry point and the row-selection rule of
// mi355rt_options come with rt_prepare.h, the HIP-free half.  Not part of the public header.
#pragma once

#include <hip/hip_runtime_api.h>

#include <string>
#include <thread>
#include <vector>

#include "rt_prepare.h"

#define HIP_TRY(expr)                                                                              \
    do { hipError_t e_ = (expr); if (e_ != hipSuccess) return mi355rt::fail(e_ == hipErrorOutOfMemory ? MI355RT_ERR_OOM : MI355RT_ERR_HIP, \
         std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)

namespace mi355rt {

// A device buffer of the CURRENT device that only grows.
template <class T> struct DevBuf {
    T* p = nullptr; size_t n = 0;
    int ensure(size_t count) {
        if (count <= n && p) return MI355RT_OK;
        if (p) { (void)hipFree(p); p = nullptr; n = 0; }
        if (count == 0) count = 1;
        HIP_TRY(hipMalloc((void**)&p, count * sizeof(T)));
        n = count;
        return MI355RT_OK;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
};

// The calling thread's current device, put back on every way out of an entry point.
struct DeviceScope {
    int dev = -1;
    DeviceScope() { if (hipGetDevice(&dev) != hipSuccess) { dev = -1; (void)hipGetLastError(); } }
    ~DeviceScope() { if (dev >= 0) (void)hipSetDevice(dev); }
};

// The options every part of a multi context passes through, made from the caller's: the strips are dealt by the call (n_parts / part must
// be left 0), strip_rows 0 -> 4.
inline int base_options(const mi355rt_options* opt, const char* who, mi355rt_options& base) {
    base = mi355rt_options{};
    if (opt) base = *opt; else { base.abi_version = MI355RT_ABI_VERSION; base.rng_mode = MI355RT_RNG_CTR; }
    if (base.n_parts > 1 || base.part != 0) return fail(MI355RT_ERR_INVALID, std::string(who) + " deals the strips itself: leave options.n_parts / part at 0");
    if (base.strip_rows == 0) base.strip_rows = 4;
    base.n_parts = 1; base.part = 0;
    return MI355RT_OK;
}

// work(0) ... work(n - 1), side by side: one host thread per further part, part 0 on the calling thread.  `work` must be noexcept -- on a
// worker thread an exception would be std::terminate.  A thread that cannot be had (std::system_error: EAGAIN under a thread / process
// limit) is not an error: that part runs on the calling thread instead, after the threads that did start have been joined -- a joinable
// std::thread must never be destroyed (std::terminate), so they are joined on the one way out by exception (no memory to note the part) too.
template <class Work> void run_parts(size_t n, Work&& work) {
    static_assert(noexcept(work(size_t{0})), "a part's work runs on a thread of its own: nothing may leave it by exception");
    std::vector<std::thread> threads;
    std::vector<size_t> inline_parts;
    try { threads.reserve(n); } catch (...) {}
    for (size_t i = 1; i < n; ++i) {
        try { threads.emplace_back([&work, i]() noexcept { work(i); }); }
        catch (...) { try { inline_parts.push_back(i); } catch (...) { for (auto& t : threads) t.join(); throw; } }
    }
    if (n) work(0);
    for (auto& t : threads) t.join();
    for (size_t i : inline_parts) work(i);
}

}  // namespace mi355rt
