// After a kernel launch inside an entry point of the C ABI: a launch error becomes the entry point's return value.
#pragma once
#include <hip/hip_runtime.h>

#define HIP_CHECK_LAUNCH()                       \
    do {                                         \
        hipError_t _e = hipGetLastError();       \
        if (_e != hipSuccess) return (int)_e;    \
    } while (0)
