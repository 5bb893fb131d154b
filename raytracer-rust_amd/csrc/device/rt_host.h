// rt_host.h -- the HIP-side pieces shared by the C-ABI sources of libmi355rt.so (rt_api.cpp: contexts and one-shot calls;
// rt_multi.cpp: the multi-device context): HIP_TRY and device buffers.  The thread-local last error, the exception barrier of every
// extern "C" entry point and the row-selection rule of mi355rt_options come with rt_prepare.h, the HIP-free half.  Not part of the
// public header.
#pragma once

#include <hip/hip_runtime_api.h>

#include <string>

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

}  // namespace mi355rt
