// Host scaffolding shared by the C-ABI files (the *_capi.cpp of each library): the error string behind the library's
// *_last_error, HIP_TRY and the device guard.  Everything here has internal linkage and a library has exactly one
// *_capi.cpp, so every .so keeps an error state of its own.  The including file defines ATACOM_CAPI_E_HIP -- its
// library's code for "a HIP runtime call failed" -- before the include.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#ifndef ATACOM_CAPI_E_HIP
#error "define ATACOM_CAPI_E_HIP (the library's HIP error code) before including atacom_capi_common.h"
#endif

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(ATACOM_CAPI_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));     \
    } while (0)

// Every entry point that touches a handle runs on the handle's device and puts the caller's current device back on
// the way out (a handle on cuda:1 must not leave the calling thread -- i.e. PyTorch -- on cuda:1).
struct DeviceGuard {
    int prev = -1;
    hipError_t err;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        err = (prev == dev) ? hipSuccess : hipSetDevice(dev);
        if (prev == dev) prev = -1;               // nothing to restore
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};
#define ON_DEVICE(h)                 \
    DeviceGuard guard_((h)->device); \
    HIP_TRY(guard_.err)

}  // namespace
