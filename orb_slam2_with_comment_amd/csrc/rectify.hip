// cv::remap(src, dst, map1, map2, INTER_LINEAR, BORDER_CONSTANT, 0) for 8-bit single-channel
// images on gfx950, reading the fixed-point records of rectify.h.  One launch
// covers both images of a stereo pair.
#include "rectifier.h"

namespace orbmi {

using rectify::Record;

namespace {

constexpr int kPix = 4;        // destination pixels per thread: one 4-byte store, two 16-byte record reads
constexpr int kBlockX = 64;    // one wave along x: 256 pixels of a row
constexpr int kBlockY = 4;

struct RemapArgs {
    RemapImage im[2];
};

// (32-a)(32-b) p00 + a(32-b) p01 + (32-a) b p10 + a b p11, rounded: cv::remap's 15-bit table form
// (entries round(32768 wx wy) = 32 wx' wy' exactly for 5-bit phases; its 32767 / 1 pair at
// a = b = 0 returns p00 for every 8-bit input).  A tap outside the source reads 0.
__device__ inline unsigned remap_one(const RemapImage& I, unsigned w0, unsigned w1) {
    const int x0 = (int)(short)(w0 & 0xFFFFu), y0 = (int)w0 >> 16;
    const int a = (int)(w1 & 0xFFFFu), b = (int)(w1 >> 16);
    const bool cx0 = (unsigned)x0 < (unsigned)I.src_cols, cx1 = (unsigned)(x0 + 1) < (unsigned)I.src_cols;
    const bool ry0 = (unsigned)y0 < (unsigned)I.src_rows, ry1 = (unsigned)(y0 + 1) < (unsigned)I.src_rows;
    const uint8_t* r0 = I.src + (size_t)(ry0 ? y0 : 0) * I.src_step;
    const uint8_t* r1 = I.src + (size_t)(ry1 ? y0 + 1 : 0) * I.src_step;
    const int p00 = (ry0 && cx0) ? r0[x0] : 0;
    const int p01 = (ry0 && cx1) ? r0[x0 + 1] : 0;
    const int p10 = (ry1 && cx0) ? r1[x0] : 0;
    const int p11 = (ry1 && cx1) ? r1[x0 + 1] : 0;
    const int ia = rectify::kInterTab - a, ib = rectify::kInterTab - b;
    return (unsigned)(ia * ib * p00 + a * ib * p01 + ia * b * p10 + a * b * p11 + 512) >> 10;
}

__global__ __launch_bounds__(kBlockX* kBlockY) void k_remap_bilinear(RemapArgs A) {
    const RemapImage& I = A.im[blockIdx.z];
    const int x = (blockIdx.x * kBlockX + threadIdx.x) * kPix;
    const int y = blockIdx.y * kBlockY + threadIdx.y;
    if (y >= I.dst_rows || x >= I.dst_cols) return;
    const size_t pitch = ((size_t)I.dst_cols + 3) & ~(size_t)3;  // rectify::record_pitch
    const uint4* rp = reinterpret_cast<const uint4*>(I.rec + (size_t)y * pitch + x);
    const uint4 ra = rp[0], rb = rp[1];
    const unsigned v0 = remap_one(I, ra.x, ra.y), v1 = remap_one(I, ra.z, ra.w);
    const unsigned v2 = remap_one(I, rb.x, rb.y), v3 = remap_one(I, rb.z, rb.w);
    uint8_t* d = I.dst + (size_t)y * I.dst_step + x;
    if (x + kPix <= I.dst_cols && ((uintptr_t)d & 3) == 0) {
        *reinterpret_cast<unsigned*>(d) = v0 | (v1 << 8) | (v2 << 16) | (v3 << 24);
    } else {  // the row's tail, or a destination whose base or pitch is not 4-byte aligned
        const unsigned v[kPix] = {v0, v1, v2, v3};
#pragma unroll
        for (int k = 0; k < kPix; k++)
            if (x + k < I.dst_cols) d[k] = (uint8_t)v[k];
    }
}

}  // namespace

int remap_run(hipStream_t stream, const RemapImage* images, int n) {
    if (!images || n < 1 || n > 2) return ORBMI_E_ARG;
    RemapArgs A;
    int rows = 0, cols = 0;
    for (int k = 0; k < n; k++) {
        A.im[k] = images[k];
        rows = rows > images[k].dst_rows ? rows : images[k].dst_rows;
        cols = cols > images[k].dst_cols ? cols : images[k].dst_cols;
    }
    if (n == 1) A.im[1] = A.im[0];
    if (rows <= 0 || cols <= 0) return ORBMI_E_ARG;
    const dim3 block(kBlockX, kBlockY), grid((cols + kBlockX * kPix - 1) / (kBlockX * kPix), (rows + kBlockY - 1) / kBlockY, n);
    if (grid.y > 65535u) return ORBMI_E_UNSUPPORTED;
    hipLaunchKernelGGL(k_remap_bilinear, grid, block, 0, stream, A);
    ORBMI_HIP(hipGetLastError());
    return ORBMI_OK;
}

int RectifyTable::upload(const float* map1, const float* map2, int rows_, int cols_) {
    std::vector<Record> rec;
    const int rc = rectify::build_records(map1, map2, rows_, cols_, &rec);
    if (rc) return rc;
    release();
    ORBMI_HIP(hipMalloc((void**)&d_rec, rec.size() * sizeof(Record)));
    ORBMI_HIP(hipMemcpy(d_rec, rec.data(), rec.size() * sizeof(Record), hipMemcpyHostToDevice));
    rows = rows_;
    cols = cols_;
    return ORBMI_OK;
}

void RectifyTable::release() {
    if (d_rec) (void)hipFree(d_rec);
    d_rec = nullptr;
    rows = cols = 0;
}

}  // namespace orbmi
