// wgrt_host.h -- host-side plumbing shared by the C-ABI translation units: the error record behind
// wgrt_last_error(), the device discipline of an entry point, and the HIP error mapping.
#pragma once

#include <hip/hip_runtime.h>

#include <string>

#include "../../include/wgrt.h"

namespace wgrt {

// Record the detail of a failing entry point for wgrt_last_error() and return its status
// (wgrt_rays.hip, beside wgrt_last_error).
wgrt_status fail(wgrt_status s, const std::string &msg);

// The C ABI's device discipline: an entry point that works on a scene (or allocates, or launches on
// a stream) makes the scene's device current for its own scope and gives the caller's current
// device back when it returns, so a host that drives several GPUs from one thread keeps whatever
// device it had selected.  hipSetDevice only when the device differs (a thread-local switch).
class DeviceScope {
    int prev_ = -1;
    hipError_t err_ = hipSuccess;

public:
    explicit DeviceScope(int device) {
        err_ = hipGetDevice(&prev_);
        if (err_ != hipSuccess) prev_ = -1;
        else if (prev_ != device) err_ = hipSetDevice(device);
    }
    ~DeviceScope() {
        int cur = -1;
        if (prev_ >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev_) (void)hipSetDevice(prev_);
    }
    DeviceScope(const DeviceScope &) = delete;
    DeviceScope &operator=(const DeviceScope &) = delete;
    hipError_t error() const { return err_; }
};

// The device a stream belongs to (the current device for the null stream).
inline hipError_t stream_device(void *stream, int *device) {
    if (!stream) return hipGetDevice(device);
    return hipStreamGetDevice((hipStream_t)stream, device);
}

// The status of an allocation (hipMalloc and what initialises the buffer): out of memory is its own
// status, every other failure a HIP error; `what` names the allocation in the message.
inline wgrt_status malloc_status(hipError_t e, const char *what = "hipMalloc") {
    if (e == hipSuccess) return WGRT_OK;
    if (e == hipErrorOutOfMemory) return fail(WGRT_ERR_OUT_OF_MEMORY, std::string(what) + ": out of memory");
    return fail(WGRT_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

}  // namespace wgrt

#define DEVICE_SCOPE(name, dev)                                                                      \
    ::wgrt::DeviceScope name(dev);                                                                  \
    if (name.error() != hipSuccess)                                                                 \
        return ::wgrt::fail(WGRT_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(name.error()))

#define HIP_TRY(expr)                                                                               \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess)                                                                       \
            return ::wgrt::fail(WGRT_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));   \
    } while (0)
