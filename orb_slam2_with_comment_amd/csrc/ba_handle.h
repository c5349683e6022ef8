// The orbmi_ba handle, shared by Optimizer::LocalBundleAdjustment (lba.hip, which creates and
// destroys it) and Optimizer::BundleAdjustment (gba.hip).  Calls on one handle are serial, so the
// two share the device arena and the stream.
#pragma once
#include "orbmi_common.h"

namespace orbmi {
struct BaCtl;
}

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
