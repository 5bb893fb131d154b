// rt_host.h -- host-side pieces shared by the C-ABI sources of libmi355rt.so (rt_api.cpp: contexts and one-shot calls;
// rt_multi.cpp: the multi-device context): the thread-local last error, the exception barrier of every extern "C" entry
// point, HIP_TRY, device buffers and the row-selection rule of mi355rt_options.  Not part of the public header.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../../include/mi355rt.h"

namespace mi355rt {

// Sets this thread's mi355rt_last_error() text and returns `code`.
int fail(int code, const std::string& msg);
int fail_noexcept(int code, const char* msg) noexcept;

// The exception barrier of every extern "C" entry point (mi355rt.h: "nothing aborts, nothing throws across the ABI"; the caller may
// be a Rust frame -- src/renderer.rs:67 is called from src/main.rs:57 -- into which a C++ exception must not unwind):
// std::bad_alloc / std::length_error -> MI355RT_ERR_OOM, anything else -> MI355RT_ERR_HIP with what() in mi355rt_last_error().
template <class F> int guard(F&& f) noexcept {
    try { return f(); }
    catch (const std::bad_alloc&) { return fail_noexcept(MI355RT_ERR_OOM, "host allocation failed (std::bad_alloc)"); }
    catch (const std::length_error&) { return fail_noexcept(MI355RT_ERR_OOM, "host allocation failed (std::length_error)"); }
    catch (const std::exception& e) {
        try { return fail(MI355RT_ERR_HIP, std::string("unexpected C++ exception: ") + e.what()); } catch (...) { return fail_noexcept(MI355RT_ERR_HIP, "unexpected C++ exception"); }
    }
    catch (...) { return fail_noexcept(MI355RT_ERR_HIP, "unexpected C++ exception"); }
}

}  // namespace mi355rt

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

struct RowSel { std::vector<uint32_t> rows; };

// The rows `o` selects (mi355rt.h, mi355rt_options), ascending = the order of the output buffers.
int select_rows(const mi355rt_settings& st, const mi355rt_options* o, RowSel& sel);
int check_settings(const mi355rt_settings* st);

}  // namespace mi355rt
