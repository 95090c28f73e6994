// mfb_common.hpp -- what the bank (mfbank.hip) and the side handles' parts (*_api.hpp) share on the host: the status of a failed HIP
// call, the device check, the allocation seam of the handles and the exception barrier of the C ABI.  Host code only; a part of
// mfbank.hip's one translation unit.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdio.h>
#include <new>

#include "../../include/mfbank.h"

#define HIPCHK(x)                                                                            \
    do {                                                                                     \
        hipError_t e_ = (x);                                                                 \
        if (e_ != hipSuccess) {                                                              \
            fprintf(stderr, "mfbank: %s failed: %s (%s:%d)\n", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
            return (e_ == hipErrorOutOfMemory) ? MFB_ERR_ALLOC : MFB_ERR_HIP;               \
        }                                                                                    \
    } while (0)

// bytes of one IQ sample in the format MFB_SAMPLES_* (the bank's inputs and windows, the channeliser's)
static size_t sample_bytes(int fmt) { return fmt == MFB_SAMPLES_SC16 ? 4 : fmt == MFB_SAMPLES_SC8 ? 2 : 8; }

// per-device tables (the sync workspaces, the page-locked sync buffers) are indexed by the device: the handles take none above it
#define SYNC_MAX_DEVICES 64

// The one device check: `device` exists (and is below `limit`, where per-device tables are indexed by it) and is now the current one.
static int device_ok(int device, int limit = INT_MAX) {
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev || device >= limit) return MFB_ERR_ARG;
    HIPCHK(hipSetDevice(device));
    return MFB_OK;
}

// Device allocations of a handle go through dev_alloc so that a test can make the n-th one fail
// (mfb_debug_fail_alloc): the only way to exercise the free-on-error path of a create without driving
// a 288 GB device out of memory.
static thread_local int g_fail_alloc_countdown = 0;
static thread_local int g_throw_alloc_countdown = 0;      // nth < 0: the |nth|-th allocation throws std::bad_alloc instead (see guarded)
static hipError_t dev_alloc(void **p, size_t bytes) {
    if (g_fail_alloc_countdown > 0 && --g_fail_alloc_countdown == 0) {
        *p = nullptr;
        return hipErrorOutOfMemory;
    }
    if (g_throw_alloc_countdown > 0 && --g_throw_alloc_countdown == 0) {
        *p = nullptr;
        throw std::bad_alloc();
    }
    return hipMalloc(p, bytes);
}
// No C++ exception leaves the library: the entry points that do host-side preparation (filter analysis, segment spectra, tables:
// std::vector, std::thread) run inside this; a failed host allocation is MFB_ERR_ALLOC like a failed device allocation.
template <class F>
static int guarded(F &&f) noexcept {
    try {
        return f();
    } catch (const std::bad_alloc &) {
        return MFB_ERR_ALLOC;
    } catch (...) {
        return MFB_ERR_STATE;
    }
}
extern "C" int mfb_debug_fail_alloc(int nth) {
    g_fail_alloc_countdown = nth > 0 ? nth : 0;
    g_throw_alloc_countdown = nth < 0 ? -nth : 0;
    return MFB_OK;
}
