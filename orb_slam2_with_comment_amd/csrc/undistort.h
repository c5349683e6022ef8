// cv::undistortPoints(src, dst, K, distCoef, cv::Mat(), K) as Frame::UndistortKeyPoints and
// Frame::ComputeImageBounds call it (src/Frame.cc:456, 483): OpenCV 3.x cvUndistortPoints with
// R = I and P = K, five fixed iterations, k4..k6 and the tilt model absent.  Shared by the device
// stage (rgbd.hip), the host bounds (orbmi_compute_image_bounds) and the CPU check program
// (tests/cpp/undistort_check.cpp).  All arithmetic is fp64 from the float32 K and mDistCoef, one
// rounding per operation in the order written (-ffp-contract=off, pinned semantics P7).
#pragma once

#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif

namespace orbmi {

// mK and mDistCoef as Tracking keeps them (src/Tracking.cc:60-80): dist = k1 k2 p1 p2 k3, with
// k3 = 0 for a 4-entry mDistCoef
struct UndistortCam {
    float fx, fy, cx, cy;
    float dist[5];
};

__host__ __device__ inline void undistort_point(const UndistortCam& c, float u, float v, float* xu, float* yu) {
    const double fx = c.fx, fy = c.fy, cx = c.cx, cy = c.cy;
    const double k1 = c.dist[0], k2 = c.dist[1], p1 = c.dist[2], p2 = c.dist[3], k3 = c.dist[4];
    const double ifx = 1.0 / fx, ify = 1.0 / fy;
    const double x0 = ((double)u - cx) * ifx, y0 = ((double)v - cy) * ify;
    double x = x0, y = y0;
    for (int j = 0; j < 5; j++) {
        const double r2 = x * x + y * y;
        const double icdist = 1.0 / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2);
        const double dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x);
        const double dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y;
        x = (x0 - dx) * icdist;
        y = (y0 - dy) * icdist;
    }
    *xu = (float)(fx * x + cx);
    *yu = (float)(fy * y + cy);
}

// Frame::ComputeImageBounds (src/Frame.cc:471-499): out = mnMinX, mnMaxX, mnMinY, mnMaxY.  The
// reference tests only k1 (mDistCoef.at<float>(0) != 0.0).
__host__ __device__ inline void image_bounds(const UndistortCam& c, int rows, int cols, float out[4]) {
    if (c.dist[0] == 0.0f) {
        out[0] = 0.0f;
        out[1] = (float)cols;
        out[2] = 0.0f;
        out[3] = (float)rows;
        return;
    }
    const float cu[4] = {0.0f, (float)cols, 0.0f, (float)cols}, cv[4] = {0.0f, 0.0f, (float)rows, (float)rows};
    float x[4], y[4];
    for (int k = 0; k < 4; k++) undistort_point(c, cu[k], cv[k], &x[k], &y[k]);
    out[0] = x[0] < x[2] ? x[0] : x[2];  // min(mat(0,0), mat(2,0))
    out[1] = x[1] > x[3] ? x[1] : x[3];  // max(mat(1,0), mat(3,0))
    out[2] = y[0] < y[1] ? y[0] : y[1];  // min(mat(0,1), mat(1,1))
    out[3] = y[2] > y[3] ? y[2] : y[3];  // max(mat(2,1), mat(3,1))
}

}  // namespace orbmi
