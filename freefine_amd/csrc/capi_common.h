// What every host unit of libfreefine_hip.so (the .hip files: each exports the ffn_* entries of its own kernels) shares: the error state, the launch
// check, the argument-check macros and the small launch helpers.  Host-side only; nothing here is exported.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <mutex>
#include <unordered_map>

#include "../../include/freefine_hip.h"

// the message ffn_last_error returns: one buffer per thread for the whole library (defined in capi.hip), whichever unit's entry failed.
// __thread, not thread_local: a plain TLS access from every unit, no call through an initialisation wrapper that only the defining unit could supply
extern "C" __attribute__((visibility("hidden"))) __thread char g_err[512];

static int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
static int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(FFN_EHIP, "%s: %s", what, hipGetErrorString(e));
    return FFN_OK;
}
// a stale error left behind by an unrelated earlier HIP call (e.g. a tool's probe) must not be blamed on our launch
#define LAUNCH(...)                  \
    do {                             \
        (void)hipGetLastError();     \
        hipLaunchKernelGGL(__VA_ARGS__); \
    } while (0)
#define REQUIRE(cond, ...) \
    do {                   \
        if (!(cond)) return fail(FFN_EINVAL, __VA_ARGS__); \
    } while (0)

static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
static inline int grid_for(long n, int per_block = 256, int cap = 4096) {
    long g = (n + per_block - 1) / per_block;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (int)g;
}

template <typename K>
static int set_lds(K kernel, int bytes) {
    static std::mutex mu;
    static std::unordered_map<const void*, int> done;   // one opt-in per (kernel, size)
    if (bytes > 48 * 1024) {
        std::lock_guard<std::mutex> lk(mu);
        int& have = done[reinterpret_cast<const void*>(kernel)];
        if (have >= bytes) return FFN_OK;
        have = bytes;
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        if (e != hipSuccess) return fail(FFN_EHIP, "hipFuncSetAttribute(%d): %s", bytes, hipGetErrorString(e));
    }
    return FFN_OK;
}

static inline int device_cus() {
    static const int n = [] {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = 256;
        return v;
    }();
    return n;
}
