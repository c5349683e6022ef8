// Device side of stereo rectification (rectify.hip): a record table in HBM and the launch of
// the bilinear remap over one image or a pair.  The tables come from rectify.h.
#pragma once
#include "orbmi_common.h"
#include "rectify.h"

namespace orbmi {

// The record table of one camera on the device: rows x cols destination pixels.
struct RectifyTable {
    rectify::Record* d_rec = nullptr;
    int rows = 0, cols = 0;
    int upload(const float* map1, const float* map2, int rows_, int cols_);  // blocking; the current device
    void release();
};

// One image of a launch: device pointers, pitches in bytes.
struct RemapImage {
    const rectify::Record* rec;
    const uint8_t* src;
    uint8_t* dst;
    int src_rows, src_cols, dst_rows, dst_cols;
    unsigned src_step, dst_step;
};

inline bool remap_source_ok(const void* src, int rows, int cols, size_t step) {
    return src && rows > 0 && cols > 0 && rows <= rectify::kMaxSource && cols <= rectify::kMaxSource &&
           step >= (size_t)cols && step <= 0xFFFFFFFFu;
}

// cv::remap(src, dst, map1, map2, INTER_LINEAR, BORDER_CONSTANT, 0) of n = 1 or 2 images in one
// launch on `stream`.
int remap_run(hipStream_t stream, const RemapImage* images, int n);

}  // namespace orbmi
