// Stereo rectification, host side (no HIP): cv::initUndistortRectifyMap(K, D, R, P[0:3,0:3], size,
// CV_32F, map1, map2) restated as OpenCV 3.x documents it, and cv::remap's conversion of float
// maps into the fixed-point records rectify.hip reads.  Everything is fp64 with
// one IEEE operation per step in source order: build with -ffp-contract=off.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/orbmi.h"

namespace orbmi {
namespace rectify {

constexpr int kInterBits = 5;                   // cv::INTER_BITS
constexpr int kInterTab = 1 << kInterBits;      // cv::INTER_TAB_SIZE: 32 phases per axis
constexpr int kMaxSource = 32767;               // rows / cols of a source image (x0, y0 are shorts)

// One destination pixel: the top-left tap (y0, x0) in the source and the phases a (x), b (y) in
// 1/32 pixel.  x0 and y0 are clamped to [-2, 32767]: below -1 or beyond 32766 every tap lies
// outside any source the kernel accepts, so the clamp changes no result.
struct Record {
    int16_t x0, y0;
    uint16_t a, b;
};
static_assert(sizeof(Record) == 8, "the kernel reads records as 8-byte words");

constexpr Record kOutside = {-2, -2, 0, 0};

// Records per row of a table: the row padded to four records, so that a thread's four
// records are one aligned 32-byte read (the padding holds kOutside).
inline size_t record_pitch(int cols) { return ((size_t)cols + 3) & ~(size_t)3; }

inline bool camera_ok(const orbmi_rectify_camera* c) {
    return c && (c->nd == 4 || c->nd == 5 || c->nd == 8) && c->rows > 0 && c->cols > 0;
}

// iR = inverse(P3 * R): the product as a dot product summed in index order, the inverse as
// cofactors times the reciprocal determinant (cv::invert's 3x3 case)
inline void inverse_projection(const double* P, const double* R, double iR[9]) {
    double S[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            double s = P[4 * i] * R[j];
            s = s + P[4 * i + 1] * R[3 + j];
            s = s + P[4 * i + 2] * R[6 + j];
            S[3 * i + j] = s;
        }
    double d = S[0] * (S[4] * S[8] - S[5] * S[7]) - S[1] * (S[3] * S[8] - S[5] * S[6]) +
               S[2] * (S[3] * S[7] - S[4] * S[6]);
    d = 1. / d;
    iR[0] = (S[4] * S[8] - S[5] * S[7]) * d;
    iR[1] = (S[2] * S[7] - S[1] * S[8]) * d;
    iR[2] = (S[1] * S[5] - S[2] * S[4]) * d;
    iR[3] = (S[5] * S[6] - S[3] * S[8]) * d;
    iR[4] = (S[0] * S[8] - S[2] * S[6]) * d;
    iR[5] = (S[2] * S[3] - S[0] * S[5]) * d;
    iR[6] = (S[3] * S[7] - S[4] * S[6]) * d;
    iR[7] = (S[1] * S[6] - S[0] * S[7]) * d;
    iR[8] = (S[0] * S[4] - S[1] * S[3]) * d;
}

// map1 / map2: rows x cols floats, contiguous.  D = k1 k2 p1 p2 [k3 [k4 k5 k6]]; the thin-prism
// and tilt terms of longer vectors are not built.
inline int init_undistort_rectify_map(const orbmi_rectify_camera* c, float* map1, float* map2) {
    if (!camera_ok(c) || !map1 || !map2) return ORBMI_E_ARG;
    const double fx = c->K[0], fy = c->K[4], cx = c->K[2], cy = c->K[5];
    double D[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int k = 0; k < c->nd; k++) D[k] = c->D[k];
    const double k1 = D[0], k2 = D[1], p1 = D[2], p2 = D[3], k3 = D[4], k4 = D[5], k5 = D[6], k6 = D[7];
    double iR[9];
    inverse_projection(c->P, c->R, iR);
    for (int i = 0; i < c->rows; i++) {
        double _x = i * iR[1] + iR[2], _y = i * iR[4] + iR[5], _w = i * iR[7] + iR[8];
        float* m1 = map1 + (size_t)i * c->cols;
        float* m2 = map2 + (size_t)i * c->cols;
        for (int j = 0; j < c->cols; j++, _x += iR[0], _y += iR[3], _w += iR[6]) {
            const double w = 1. / _w, x = _x * w, y = _y * w;
            const double x2 = x * x, y2 = y * y;
            const double r2 = x2 + y2, _2xy = 2 * x * y;
            const double kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2);
            const double xd = x * kr + p1 * _2xy + p2 * (r2 + 2 * x2);
            const double yd = y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy;
            m1[j] = (float)(fx * xd + cx);
            m2[j] = (float)(fy * yd + cy);
        }
    }
    return ORBMI_OK;
}

// round-half-even(v * 32) as cv::remap's cvRound does; false when it is a NaN or does not fit
// an int32 (the pixel is then outside)
inline bool fixed_point(float v, int32_t* out) {
    const double s = (double)v * kInterTab;
    if (!(std::fabs(s) < 2147483648.0)) return false;
    *out = (int32_t)std::nearbyint(s);
    return true;
}

inline Record make_record(float mx, float my) {
    int32_t sx, sy;
    if (!fixed_point(mx, &sx) || !fixed_point(my, &sy)) return kOutside;
    const int32_t x0 = sx >> kInterBits, y0 = sy >> kInterBits;  // arithmetic shifts: floor
    if (x0 < -1 || y0 < -1 || x0 >= kMaxSource || y0 >= kMaxSource) return kOutside;
    return Record{(int16_t)x0, (int16_t)y0, (uint16_t)(sx & (kInterTab - 1)), (uint16_t)(sy & (kInterTab - 1))};
}

// The record table of a pair of float maps: rows x record_pitch(cols).
inline int build_records(const float* map1, const float* map2, int rows, int cols, std::vector<Record>* out) {
    if (!map1 || !map2 || rows <= 0 || cols <= 0 || !out) return ORBMI_E_ARG;
    const size_t pitch = record_pitch(cols);
    out->assign((size_t)rows * pitch, kOutside);
    for (int i = 0; i < rows; i++)
        for (int j = 0; j < cols; j++)
            (*out)[(size_t)i * pitch + j] = make_record(map1[(size_t)i * cols + j], map2[(size_t)i * cols + j]);
    return ORBMI_OK;
}

// The value the kernel stores for one record: bilinear cv::remap of an 8-bit image with
// BORDER_CONSTANT 0 (host restatement, used by the stand-alone check).
inline uint8_t remap_pixel(const Record& r, const uint8_t* src, int rows, int cols, size_t step) {
    auto tap = [&](int y, int x) -> int {
        return (x >= 0 && x < cols && y >= 0 && y < rows) ? src[(size_t)y * step + x] : 0;
    };
    const int a = r.a, b = r.b;
    const int v = (kInterTab - a) * (kInterTab - b) * tap(r.y0, r.x0) + a * (kInterTab - b) * tap(r.y0, r.x0 + 1) +
                  (kInterTab - a) * b * tap(r.y0 + 1, r.x0) + a * b * tap(r.y0 + 1, r.x0 + 1);
    return (uint8_t)((v + 512) >> 10);
}

}  // namespace rectify
}  // namespace orbmi
