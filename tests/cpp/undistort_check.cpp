// Host check of csrc/undistort.h (the header the device stage and orbmi_compute_image_bounds
// share): undistorts the points of an input file and computes the image bounds, for
// tests/test_rgbd_cpu.py to compare bit for bit with the numpy restatement.
//   undistort_check <in> <out>
// in : float32 fx fy cx cy d0 d1 d2 d3 d4, int32 rows cols n, then n x (u, v) float32
// out: n x (xu, yu) float32 (copied when d0 == 0, as Frame::UndistortKeyPoints does), then the
//      bounds mnMinX mnMaxX mnMinY mnMaxY
// Build: c++ -O2 -std=c++17 -ffp-contract=off -I orb_slam2_with_comment_amd/csrc
#include <cstdint>
#include <cstdio>
#include <vector>

#include "undistort.h"

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    float cam[9];
    int32_t dims[3];
    if (fread(cam, sizeof(float), 9, f) != 9 || fread(dims, sizeof(int32_t), 3, f) != 3 || dims[2] < 0) return 2;
    const int rows = dims[0], cols = dims[1], n = dims[2];
    std::vector<float> pts(2 * (size_t)n), out(2 * (size_t)n + 4);
    if (fread(pts.data(), sizeof(float), pts.size(), f) != pts.size()) return 2;
    fclose(f);
    orbmi::UndistortCam c{cam[0], cam[1], cam[2], cam[3], {cam[4], cam[5], cam[6], cam[7], cam[8]}};
    for (int i = 0; i < n; i++) {
        if (c.dist[0] == 0.0f) {
            out[2 * i] = pts[2 * i];
            out[2 * i + 1] = pts[2 * i + 1];
        } else {
            orbmi::undistort_point(c, pts[2 * i], pts[2 * i + 1], &out[2 * i], &out[2 * i + 1]);
        }
    }
    orbmi::image_bounds(c, rows, cols, &out[2 * (size_t)n]);
    f = fopen(argv[2], "wb");
    if (!f || fwrite(out.data(), sizeof(float), out.size(), f) != out.size()) return 2;
    fclose(f);
    printf("points %d\n", n);
    return 0;
}
