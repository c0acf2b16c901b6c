// The device scope of a C ABI entry point (capi.hip, vit_forward.hip).
#pragma once
#include <hip/hip_runtime.h>

// Every launching entry point runs on the device that owns `stream` (the reference keeps the matcher on cuda:1 while
// cuda:0 is current, pope_model_api.py:181-184): the launchers' per-device state (LDS opt-in, CU count) and the
// launches themselves then belong to the right GPU whatever the caller's current device is.  NULL = the current
// device's default stream.  The previous device is restored on return.
struct StreamDevice {
    int prev = -1;
    bool switched = false;
    explicit StreamDevice(void* stream) {
        int dev = -1;
        if (!stream || hipGetDevice(&prev) != hipSuccess) return;
        if (hipStreamGetDevice(static_cast<hipStream_t>(stream), &dev) == hipSuccess && dev != prev)
            switched = hipSetDevice(dev) == hipSuccess;
    }
    ~StreamDevice() {
        if (switched) (void)hipSetDevice(prev);
    }
    StreamDevice(const StreamDevice&) = delete;
    StreamDevice& operator=(const StreamDevice&) = delete;
};
