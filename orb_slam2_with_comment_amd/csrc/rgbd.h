// Launchers of the RGB-D front-end stage (rgbd.hip), for the C ABI (capi_extract.cpp) and the
// native loop (slam.cpp).
#pragma once
#include "orbmi_common.h"
#include "undistort.h"

namespace orbmi {

// Frame::UndistortKeyPoints + Frame::ComputeStereoFromRGBD on `stream` for the first
// min(n, *d_n) keypoints (d_n may be NULL); d_keys_un may be d_keys_in.  Every pointer is device
// memory; depth_type is ORBMI_DEPTH_F32 / ORBMI_DEPTH_U16, depth_step its row pitch in bytes.
int rgbd_frame_run(hipStream_t stream, const orbmi_keypoint* d_keys_in, const int* d_n, int n, const void* d_depth,
                   int depth_type, size_t depth_step, float factor, int rows, int cols, const UndistortCam& cam,
                   float bf, orbmi_keypoint* d_keys_un, float* d_u_right, float* d_depth_out);

// interleaved u8 with 3 or 4 channels -> gray (rgb: 1 = R first, 0 = B first)
int cvt_gray_run(hipStream_t stream, const uint8_t* d_src, size_t src_step, int channels, int rgb, int rows,
                 int cols, uint8_t* d_dst, size_t dst_step);

}  // namespace orbmi
