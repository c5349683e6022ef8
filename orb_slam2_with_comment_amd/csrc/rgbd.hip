// The RGB-D Frame constructor's stages after the extraction (src/Frame.cc:119-171):
// Frame::UndistortKeyPoints (:434-469) and Frame::ComputeStereoFromRGBD (:678-699) as one kernel
// over the extractor's device-resident keypoints, and Tracking::GrabImageRGBD's cvtColor
// (src/Tracking.cc:208-224).  Both are memory-trivial (a few thousand threads / one image pass).
#include "orbmi_common.h"
#include "rgbd.h"

namespace orbmi {

namespace {

// One thread per keypoint.  keys_in and keys_un may be the same array (each thread reads its own
// record before it writes it).  n_dev (optional) holds the frame's keypoint count, capped by n.
__global__ void k_rgbd_frame(const orbmi_keypoint* keys_in, const int* __restrict__ n_dev, int n,
                             const uint8_t* __restrict__ depth, int depth_type, size_t depth_step, float factor,
                             int rows, int cols, UndistortCam cam, float bf, orbmi_keypoint* keys_un,
                             float* __restrict__ u_right, float* __restrict__ depth_out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (n_dev) n = min(n, *n_dev);
    if (i >= n) return;
    orbmi_keypoint kp = keys_in[i];
    const float u = kp.x, v = kp.y;
    // imDepth.at<float>(v, u): the float arguments convert to int by truncation (src/Frame.cc:691)
    const int iu = (int)u, iv = (int)v;
    float d = -1.0f;
    // a caller's key outside the image (never an extracted one): no depth, and the key is copied
    const bool inside = iu >= 0 && iu < cols && iv >= 0 && iv < rows;
    if (inside) {
        const uint8_t* row = depth + (size_t)iv * depth_step;
        if (depth_type == ORBMI_DEPTH_U16) {
            d = (float)((const uint16_t*)row)[iu] * factor;
        } else {
            const float in = ((const float*)row)[iu];
            d = factor == 1.0f ? in : in * factor;  // (src/Tracking.cc:226-227: converted only when needed)
        }
    }
    if (inside && cam.dist[0] != 0.0f) {  // the reference tests only k1 (src/Frame.cc:437)
        float xu, yu;
        undistort_point(cam, u, v, &xu, &yu);
        kp.x = xu;
        kp.y = yu;
    }
    keys_un[i] = kp;
    if (d > 0) {  // false for NaN
        depth_out[i] = d;
        u_right[i] = kp.x - __fdiv_rn(bf, d);
    } else {
        depth_out[i] = -1.0f;
        u_right[i] = -1.0f;
    }
}

// cvtColor(RGB2GRAY / BGR2GRAY / RGBA2GRAY / BGRA2GRAY) on 8-bit pixels: OpenCV's fixed-point
// form with 14 fractional bits (R 4899, G 9617, B 1868), one thread per pixel.
__global__ void k_cvt_gray(const uint8_t* __restrict__ src, size_t src_step, int channels, int rgb, int rows,
                           int cols, uint8_t* __restrict__ dst, size_t dst_step) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= cols || y >= rows) return;
    const uint8_t* p = src + (size_t)y * src_step + (size_t)x * channels;
    const int c0 = p[0], g = p[1], c2 = p[2];
    const int r = rgb ? c0 : c2, b = rgb ? c2 : c0;
    dst[(size_t)y * dst_step + x] = (uint8_t)((r * 4899 + g * 9617 + b * 1868 + 8192) >> 14);
}

}  // namespace

int rgbd_frame_run(hipStream_t stream, const orbmi_keypoint* d_keys_in, const int* d_n, int n, const void* d_depth,
                   int depth_type, size_t depth_step, float factor, int rows, int cols, const UndistortCam& cam,
                   float bf, orbmi_keypoint* d_keys_un, float* d_u_right, float* d_depth_out) {
    if (n <= 0) return ORBMI_OK;
    const int block = 256;
    hipLaunchKernelGGL(k_rgbd_frame, dim3((n + block - 1) / block), dim3(block), 0, stream, d_keys_in, d_n, n,
                       (const uint8_t*)d_depth, depth_type, depth_step, factor, rows, cols, cam, bf, d_keys_un,
                       d_u_right, d_depth_out);
    ORBMI_HIP(hipGetLastError());
    return ORBMI_OK;
}

int cvt_gray_run(hipStream_t stream, const uint8_t* d_src, size_t src_step, int channels, int rgb, int rows,
                 int cols, uint8_t* d_dst, size_t dst_step) {
    if (rows <= 0 || cols <= 0) return ORBMI_OK;
    const int block = 256;
    hipLaunchKernelGGL(k_cvt_gray, dim3((cols + block - 1) / block, rows), dim3(block), 0, stream, d_src, src_step,
                       channels, rgb, rows, cols, d_dst, dst_step);
    ORBMI_HIP(hipGetLastError());
    return ORBMI_OK;
}

}  // namespace orbmi
