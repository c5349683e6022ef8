// Shared device/host helpers for the MI355X (gfx950) ORB front-end kernels.
// Compiled with -ffp-contract=off on host and device: every float expression below is
// evaluated with one IEEE rounding per operation, in source order (pinned semantics P7).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/orbmi.h"
#include "extractor_plan.h"  // kEdge, kHalfPatch, kPatch, kMaxLevels, reflect101, cv_floor_f, cv_round_f
#include "wave_ops.h"

#define ORBMI_HIP(call)                                                                 \
    do {                                                                                \
        hipError_t e_ = (call);                                                         \
        if (e_ != hipSuccess) {                                                         \
            fprintf(stderr, "orbmi: %s failed: %s (%s:%d)\n", #call, hipGetErrorString(e_), \
                    __FILE__, __LINE__);                                                \
            return ORBMI_E_HIP;                                                         \
        }                                                                               \
    } while (0)

namespace orbmi {

constexpr int kWave = 64;

__device__ inline int popc256(const uint4& a0, const uint4& a1, const uint4& b0, const uint4& b1) {
    return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) +
           __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}

// Whether a kernel can read p in place: device or managed memory (host only; a null pointer and
// pageable or pinned host memory are not)
inline bool on_device(const void* p) {
    if (!p) return false;
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged;
}

// HIP events around one phase of a profiled call (host only): end() waits for the phase and adds
// its device time in milliseconds to *acc.  Off, both do nothing.
struct PhaseTimer {
    hipStream_t s;
    bool on;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    PhaseTimer(hipStream_t stream, bool on_) : s(stream), on(on_) {
        if (on && (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess)) on = false;
    }
    ~PhaseTimer() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
    void begin() { if (on) (void)hipEventRecord(e0, s); }
    template <class T>
    void end(T* acc) {
        float ms = 0;
        if (on && hipEventRecord(e1, s) == hipSuccess && hipEventSynchronize(e1) == hipSuccess &&
            hipEventElapsedTime(&ms, e0, e1) == hipSuccess)
            *acc += ms;
    }
};

// Non-blocking stream of one handle. ORBMI_PRIO_<ROLE>=high|low (ROLE = MATCHER, POSE, BA,
// VOCAB, EXTRACTOR) selects the device's greatest / least stream priority, else the default.
inline hipError_t stream_create(hipStream_t* s, const char* role) {
    char key[64];
    snprintf(key, sizeof(key), "ORBMI_PRIO_%s", role);
    const char* v = getenv(key);
    if (v && (!strcmp(v, "high") || !strcmp(v, "low"))) {
        int least = 0, greatest = 0;
        hipError_t e = hipDeviceGetStreamPriorityRange(&least, &greatest);
        if (e != hipSuccess) return e;
        return hipStreamCreateWithPriority(s, hipStreamNonBlocking, !strcmp(v, "high") ? greatest : least);
    }
    return hipStreamCreateWithFlags(s, hipStreamNonBlocking);
}

}  // namespace orbmi
