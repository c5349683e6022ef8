// orbmi::StereoRectifier (include/orbmi.hpp) where Examples/Stereo/stereo_euroc.cc:92-93, 122-123
// calls cv::initUndistortRectifyMap and cv::remap.
//
//   dropin_rectify cameras.bin left.raw right.raw rows cols out.bin
//
// cameras.bin: the left and the right camera, each 41 doubles K[9] D[8] nd R[9] P[12] rows cols
// (the settings file's LEFT / RIGHT values); left.raw / right.raw: rows x cols u8.  out.bin: the
// rectified left image, then the right one.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "orbmi.hpp"

static std::vector<uint8_t> read_file(const char* path, size_t n) {
    std::vector<uint8_t> v(n);
    FILE* f = fopen(path, "rb");
    if (!f || fread(v.data(), 1, n, f) != n) { fprintf(stderr, "cannot read %zu bytes of %s\n", n, path); exit(1); }
    fclose(f);
    return v;
}

static orbmi_rectify_camera camera(const double* d) {
    orbmi_rectify_camera c;
    memcpy(c.K, d, sizeof(c.K));
    memcpy(c.D, d + 9, sizeof(c.D));
    c.nd = (int)d[17];
    memcpy(c.R, d + 18, sizeof(c.R));
    memcpy(c.P, d + 27, sizeof(c.P));
    c.rows = (int)d[39];
    c.cols = (int)d[40];
    return c;
}

int main(int argc, char** argv) {
    if (argc != 7) { fprintf(stderr, "usage: dropin_rectify cameras.bin left.raw right.raw rows cols out.bin\n"); return 1; }
    const int rows = atoi(argv[4]), cols = atoi(argv[5]);
    const std::vector<uint8_t> cams = read_file(argv[1], 2 * 41 * sizeof(double));
    const double* d = reinterpret_cast<const double*>(cams.data());
    const orbmi_rectify_camera cl = camera(d), cr = camera(d + 41);
    const std::vector<uint8_t> imLeft = read_file(argv[2], (size_t)rows * cols), imRight = read_file(argv[3], (size_t)rows * cols);
    try {
        orbmi::StereoRectifier rectify(cl, cr);
        std::vector<uint8_t> imLeftRect((size_t)cl.rows * cl.cols), imRightRect((size_t)cr.rows * cr.cols);
        rectify(imLeft.data(), imRight.data(), rows, cols, cols, imLeftRect.data(), imRightRect.data(), cl.cols);
        FILE* f = fopen(argv[6], "wb");
        if (!f || fwrite(imLeftRect.data(), 1, imLeftRect.size(), f) != imLeftRect.size() ||
            fwrite(imRightRect.data(), 1, imRightRect.size(), f) != imRightRect.size() || fclose(f)) {
            fprintf(stderr, "cannot write %s\n", argv[6]);
            return 1;
        }
    } catch (const orbmi::Error& e) {
        fprintf(stderr, "%s\n", e.what());
        return 2;
    }
    return 0;
}
