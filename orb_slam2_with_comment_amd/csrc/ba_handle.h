// The orbmi_ba handle, shared by Optimizer::LocalBundleAdjustment (lba.hip, which creates and
// destroys it) and Optimizer::BundleAdjustment (gba.hip).  Calls on one handle are serial, so the
// two share the device arena and the stream.
#pragma once
#include "orbmi_common.h"

namespace orbmi {
struct BaCtl;

// the caller's stop flag (bool* pbStopFlag, src/Optimizer.cc:483), written by other threads:
// read with an atomic load
inline bool stop_set(const volatile int* stop) { return stop && __atomic_load_n(stop, __ATOMIC_ACQUIRE) != 0; }

// The slots of a device arena, listed once and walked twice: with base null the walk sums the
// sizes (every slot 256-aligned, 8 bytes at least), with the arena's address it binds the
// pointers.  A slot is the pointer, whose type gives the element size, and the element count.
struct ArenaWalk {
    uint8_t* base = nullptr;
    size_t off = 0;
    template <class T>
    void operator()(T*& p, size_t n) {
        if (base) p = (T*)(base + off);
        const size_t bytes = n * sizeof(T);
        off += ((bytes < 8 ? 8 : bytes) + 255) & ~(size_t)255;
    }
};
}  // namespace orbmi

struct orbmi_ba {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = true;  // false after orbmi_ba_set_stream(b, s != NULL)
    hipEvent_t done = nullptr;
    uint8_t* d_buf = nullptr;
    size_t cap = 0;
    uint8_t* h_stage = nullptr;  // pinned staging of the uploaded graph (one H2D copy)
    size_t cap_stage = 0;
    hipEvent_t up_done = nullptr;  // the last upload from h_stage has been read
    // the graph upload's own stream (created at the first call): the copy depends on nothing
    // enqueued ahead of LocalBA on `stream` (a LocalMapping chain's searches), so it runs beside
    // that work and `stream` waits for up_done only
    hipStream_t up_stream = nullptr;
    uint8_t* h_out = nullptr;      // pinned staging of the results (poses, positions, erase flags)
    size_t cap_out = 0;
    orbmi::BaCtl* h_ctl = nullptr;  // pinned readback of the LM control block
    int* h_stop = nullptr;          // host-mapped mirror of the caller's stop flag
    int* d_stop = nullptr;          //   (its device address)
    int stop_at = -1;               // orbmi_ba_set_stop_at_check
    void (*enqueued)(void*) = nullptr;  // orbmi_ba_set_enqueued_hook
    void* enqueued_arg = nullptr;
    double* h_gba = nullptr;        // pinned read-back of orbmi_bundle_adjustment's trial record
};
