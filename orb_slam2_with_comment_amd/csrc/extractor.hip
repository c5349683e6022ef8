// MI355X (gfx950) ORB extractor: ORBextractor::operator() (src/ORBextractor.cc:1043-1105)
// as kernel stages over a batch of images resident in HBM:
//   k_pyramid                     ComputePyramid            (:1107-1132)    one WG per tile, all levels
//     k_pyr_level0 + k_pyr_resize   the same level by level, for batches > kPyrTiledMaxBatch
//   k_fast2<48|80>                cell FAST + NMS + fallback (:778-829)      one wave per cell
//   k_octree                      DistributeOctTree          (:539-763)      one WG per level; up to
//                                 kFuseBlurMaxOctrees octrees the blur rides in its launch
//   k_blur                        GaussianBlur               (:1076-1090)    one WG per 128x32 tile,
//                                 on a side stream beside FAST and the octrees (larger batches)
//   k_describe4                   IC_Angle + computeOrbDescriptor (:77-147, :1091-1104)
//                                                                           four keypoints per wave
// Extractor::run enqueues them in that order.
// Results are bit-exact with the pinned CPU restatement (oracle/, DESIGN.md "Pinned semantics").
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>

#include "../../include/orbmi_pattern.h"
#include "extractor.h"
#include "fast_score.h"
#include "trig_f64.h"

namespace orbmi {

// ------------------------------------------------------------------------------ pyramid
// ComputePyramid (src/ORBextractor.cc:1107-1132) in one launch: level 0 = copyMakeBorder(image,
// 19, BORDER_REFLECT_101); level l = resize(level l-1, INTER_LINEAR) + copyMakeBorder
// (REFLECT_101|ISOLATED).  One workgroup per (image, tile of the level grid): for every level the
// tile owns a rectangle (written to HBM, with the border pixels that mirror it) and computes a
// `need` rectangle into LDS = its own rectangle plus the rows / columns the next level's need
// rectangle reads (host-built, PyrTile), so the levels chain inside the workgroup with one
// barrier per level and no HBM round trip.  Halo pixels are computed by every tile that needs
// them, with the same formula.
// pyr_store and pyr_resize_px (extractor_plan.h) are shared with the CPU run of the tile plan.

constexpr int kPyrThreads = 1024;  // 64 columns x 16 rows per step
constexpr int kPyrRows = kPyrThreads / 64;
constexpr int kPyrTiledMaxBatch = 8;  // larger batches build the pyramid level by level

// global -> LDS copy of n elements with kInFlight loads issued before the first store
template <int kInFlight, class T, class F>
__device__ inline void pyr_stage(T* dst, int n, F&& load) {
    for (int i0 = 0; i0 < n; i0 += kInFlight * kPyrThreads) {
        T v[kInFlight];
#pragma unroll
        for (int k = 0; k < kInFlight; k++) {
            const int i = i0 + k * kPyrThreads + (int)threadIdx.x;
            v[k] = i < n ? load(i) : T(0);
        }
#pragma unroll
        for (int k = 0; k < kInFlight; k++) {
            const int i = i0 + k * kPyrThreads + (int)threadIdx.x;
            if (i < n) dst[i] = v[k];
        }
    }
}

// The tile's level-0 need rectangle is its own rectangle grown by (hx, hy) (host: the largest
// halo of any tile), so it follows from blockIdx alone and the image loads go out together with
// the tile's parameter block (rectangles, level geometry, the resize taps of its need
// rectangles): one HBM round trip before all levels run out of LDS.
// It also clears the image's per-level candidate counters (k_fast2 allocates from them).
__global__ __launch_bounds__(kPyrThreads) void k_pyramid(const uint8_t* __restrict__ img, size_t step,
                                                         size_t img_stride, uint8_t* __restrict__ pyr, long long pimg,
                                                         const uint32_t* __restrict__ blobs, int blob_words,
                                                         int nlevels, int KX, int KY, int W0, int H0, int hx, int hy,
                                                         int* __restrict__ level_count, int lds0, int lds_half) {
    extern __shared__ uint32_t pw[];  // parameter block | level-0 rectangle | two need rectangles
    uint32_t* B = pw;
    uint8_t* L0 = reinterpret_cast<uint8_t*>(pw + blob_words);
    uint8_t* H2 = L0 + lds0;
    const int t = blockIdx.x, b = blockIdx.z, tid = threadIdx.x;
    const int tx = tid & 63, ty = tid >> 6;
    if (t == 0 && tid < nlevels * kFastRegions) level_count[b * nlevels * kFastRegions + tid] = 0;
    const uint8_t* im = img + b * img_stride;
    uint8_t* P = pyr + b * pimg;
    const int cx = t % KX, cy = t / KX;
    const int ox0 = W0 * cx / KX, ox1 = W0 * (cx + 1) / KX, oy0 = H0 * cy / KY, oy1 = H0 * (cy + 1) / KY;
    const int nx0 = max(ox0 - hx, 0), nx1 = min(ox1 + hx, W0), ny0 = max(oy0 - hy, 0), ny1 = min(oy1 + hy, H0);
    const int w0 = nx1 - nx0, a0 = w0 * (ny1 - ny0);
    const uint32_t* bl = blobs + (size_t)t * blob_words;
    pyr_stage<4>(B, blob_words, [&](int i) { return bl[i]; });
    pyr_stage<24>(L0, a0, [&](int i) {
        const int r = i / w0;
        return im[(size_t)(ny0 + r) * step + nx0 + (i - r * w0)];
    });
    __syncthreads();
    auto lo16 = [](uint32_t w) { return (int)(short)(w & 0xFFFF); };
    auto hi16 = [](uint32_t w) { return (int)(short)(w >> 16); };
    {   // level 0: the own rectangle with its border mirrors
        const uint32_t* G = B;
        const int W = lo16(G[kPyrWH]), H = hi16(G[kPyrWH]), stride = (int)G[kPyrStride];
        uint8_t* lvl = P + G[kPyrOff];
        for (int y = oy0 + ty; y < oy1; y += kPyrRows)
            for (int x = ox0 + tx; x < ox1; x += 64) pyr_store(lvl, W, H, stride, x, y, L0[(y - ny0) * w0 + x - nx0]);
    }
    int snx0 = nx0, sny0 = ny0, sw = w0;  // the source need rectangle of the next level
    for (int l = 1; l < nlevels; l++) {
        const uint32_t* G = B + l * kPyrLevelWords;
        const int o_x0 = lo16(G[kPyrOwnX]), o_x1 = hi16(G[kPyrOwnX]), o_y0 = lo16(G[kPyrOwnY]), o_y1 = hi16(G[kPyrOwnY]);
        const int n_x0 = lo16(G[kPyrNeedX]), n_x1 = hi16(G[kPyrNeedX]), n_y0 = lo16(G[kPyrNeedY]), n_y1 = hi16(G[kPyrNeedY]);
        const int W = lo16(G[kPyrWH]), H = hi16(G[kPyrWH]), stride = (int)G[kPyrStride], rxv = (int)G[kPyrResizeXv];
        uint8_t* lvl = P + G[kPyrOff];
        const uint32_t* XT = B + G[kPyrXTaps];  // 2 words per column of the need rectangle
        const uint32_t* YT = B + G[kPyrYTaps];  // 2 words per row
        const uint8_t* src = l == 1 ? L0 : H2 + ((l - 1) & 1) * lds_half;
        uint8_t* dst = H2 + (l & 1) * lds_half;
        const int nw = n_x1 - n_x0;
        const bool keep = l + 1 < nlevels;
        for (int y = n_y0 + ty; y < n_y1; y += kPyrRows) {
            const uint32_t y0w = YT[2 * (y - n_y0)], y1w = YT[2 * (y - n_y0) + 1];
            const YTab yy{(short)lo16(y0w), (short)hi16(y0w), (short)lo16(y1w), (short)hi16(y1w)};
            const uint8_t* r0 = src + (yy.y0 - sny0) * sw - snx0;
            const uint8_t* r1 = src + (yy.y1 - sny0) * sw - snx0;
            for (int x = n_x0 + tx; x < n_x1; x += 64) {
                const uint32_t x0w = XT[2 * (x - n_x0)], x1w = XT[2 * (x - n_x0) + 1];
                const XTab xx{(short)lo16(x0w), (short)hi16(x0w), (short)lo16(x1w), (short)hi16(x1w)};
                const uint8_t v = (uint8_t)pyr_resize_px(r0[xx.sx0], r0[xx.sx1], r1[xx.sx0], r1[xx.sx1], xx, yy, x < rxv);
                if (keep) dst[(y - n_y0) * nw + (x - n_x0)] = v;
                if (x >= o_x0 && x < o_x1 && y >= o_y0 && y < o_y1) pyr_store(lvl, W, H, stride, x, y, v);
            }
        }
        snx0 = n_x0;
        sny0 = n_y0;
        sw = nw;
        __syncthreads();
    }
}

// Large batches: one launch per level (the tiles' halo recomputation costs more than the
// launches once the batch fills the chip).  A 256-thread workgroup makes kPyrBRows padded rows of
// one level: the source rows they read are staged in LDS with aligned 16-B (level 0: 4-B) loads,
// then every thread forms 8 consecutive output bytes from LDS byte reads and stores them as one
// 8-B word (byte stores only at the row's end).  Global byte loads would bind on the texture
// addresser (one 64-lane address batch per byte).
#ifndef ORBMI_PYR_ROWS
#define ORBMI_PYR_ROWS 4
#endif
constexpr int kPyrBRows = ORBMI_PYR_ROWS;  // padded rows per workgroup (A/B builds: -DORBMI_PYR_ROWS)
constexpr int kPyrBThreads = 256;

// Level 0: copyMakeBorder(image, 19, BORDER_REFLECT_101) (src/ORBextractor.cc:1128-1129); it
// also clears the per-level candidate counters.  LDS: kPyrBRows image rows of `lrow` bytes.
__global__ __launch_bounds__(kPyrBThreads) void k_pyr_level0(const uint8_t* __restrict__ img, size_t step,
                                                             size_t img_stride, uint8_t* __restrict__ pyr, long long pimg,
                                                             LevelGeom g, int* __restrict__ level_count, int nlevels,
                                                             int lrow) {
    extern __shared__ uint32_t srow4[];
    const int b = blockIdx.z, yp0 = blockIdx.x * kPyrBRows, tid = threadIdx.x;
    if (blockIdx.x == 0 && tid < nlevels * kFastRegions) level_count[b * nlevels * kFastRegions + tid] = 0;
    const int PW = g.W + 2 * kEdge, nrow = min(kPyrBRows, g.ph - yp0);
    const int nd = (g.W + 3 + 3) / 4;  // dwords covering a row from its aligned start
    int o[kPyrBRows];
#pragma unroll
    for (int r = 0; r < kPyrBRows; r++) {
        const uint8_t* row = img + b * img_stride + (size_t)reflect101(min(yp0 + r, g.ph - 1) - kEdge, g.H) * step;
        o[r] = (int)((uintptr_t)row & 3);
    }
    for (int i = tid; i < nrow * nd; i += kPyrBThreads) {
        const int r = i / nd, d = i - r * nd;
        const uint8_t* row = img + b * img_stride + (size_t)reflect101(yp0 + r - kEdge, g.H) * step;
        srow4[r * (lrow / 4) + d] = reinterpret_cast<const uint32_t*>(row - ((uintptr_t)row & 3))[d];
    }
    __syncthreads();
    const uint8_t* sb = reinterpret_cast<const uint8_t*>(srow4);
    const int nch = (PW + 7) / 8;
    for (int t = tid; t < nrow * nch; t += kPyrBThreads) {
        const int r = t / nch, xp = 8 * (t - r * nch);
        const uint8_t* src = sb + r * lrow + o[r];
        uint8_t* dst = pyr + b * pimg + g.off + (long long)(yp0 + r) * g.stride + xp;
        uint32_t w[2] = {0u, 0u};
#pragma unroll
        for (int i = 0; i < 8; i++) w[i >> 2] |= (uint32_t)src[reflect101(min(xp + i, PW - 1) - kEdge, g.W)] << (8 * (i & 3));
        if (xp + 8 <= PW) *reinterpret_cast<uint2*>(dst) = make_uint2(w[0], w[1]);
        else
            for (int i = 0; i < PW - xp; i++) dst[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
    }
}

// Level l: resize(level l-1, INTER_LINEAR) then copyMakeBorder(REFLECT_101|ISOLATED)
// (src/ORBextractor.cc:1118-1124).  Border pixels recompute the interior pixel they mirror.
// LDS: the two source rows of each output row (whole padded rows of level l-1, `lrow` bytes),
// then the level's horizontal taps (d.W entries): read per output byte, they are 8x the bytes
// written, and from global memory every 8-B lane load of a wave touched its own cache line.
__global__ __launch_bounds__(kPyrBThreads) void k_pyr_resize(uint8_t* __restrict__ pyr, long long pimg, LevelGeom s,
                                                             LevelGeom d, const XTab* __restrict__ xtg,
                                                             const YTab* __restrict__ yt, int lrow) {
    extern __shared__ uint4 srow16[];
    const int b = blockIdx.z, yp0 = blockIdx.x * kPyrBRows, tid = threadIdx.x;
    const int PW = d.W + 2 * kEdge, nrow = min(kPyrBRows, d.ph - yp0);
    const uint8_t* S = pyr + b * pimg + s.off;
    const int n16 = s.stride / 16;
    XTab* xt = reinterpret_cast<XTab*>(srow16 + 2 * kPyrBRows * (lrow / 16));
    for (int i = tid; i < d.W; i += kPyrBThreads) xt[i] = xtg[i];
    for (int i = tid; i < 2 * nrow * n16; i += kPyrBThreads) {
        const int rr = i / n16, c = i - rr * n16;  // rr = 2 * output row + tap
        const YTab y = yt[reflect101(yp0 + (rr >> 1) - kEdge, d.H)];
        const int sy = (rr & 1) ? y.y1 : y.y0;
        srow16[rr * (lrow / 16) + c] = reinterpret_cast<const uint4*>(S + (long long)(kEdge + sy) * s.stride)[c];
    }
    __syncthreads();
    const uint8_t* sb = reinterpret_cast<const uint8_t*>(srow16) + kEdge;
    const int nch = (PW + 7) / 8;
    for (int t = tid; t < nrow * nch; t += kPyrBThreads) {
        const int r = t / nch, xp = 8 * (t - r * nch);
        const YTab y = yt[reflect101(yp0 + r - kEdge, d.H)];
        const uint8_t* r0 = sb + (2 * r) * lrow;
        const uint8_t* r1 = r0 + lrow;
        uint8_t* dst = pyr + b * pimg + d.off + (long long)(yp0 + r) * d.stride + xp;
        uint32_t w[2] = {0u, 0u};
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int ix = reflect101(min(xp + i, PW - 1) - kEdge, d.W);
            const XTab x = xt[ix];
            w[i >> 2] |= (uint32_t)pyr_resize_px(r0[x.sx0], r0[x.sx1], r1[x.sx0], r1[x.sx1], x, y, ix < d.resize_xv)
                         << (8 * (i & 3));
        }
        if (xp + 8 <= PW) *reinterpret_cast<uint2*>(dst) = make_uint2(w[0], w[1]);
        else
            for (int i = 0; i < PW - xp; i++) dst[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
    }
}

// Workgroup i of a 1-D grid runs on XCD i % 8.  With >= 8 images, xcd_image_map numbers the
// `per` workgroups of image b so that they share XCD b % 8 (unit w of image b: i = 8 (w + per
// (b / 8)) + b % 8): an XCD's L2 then serves the few images its workgroups walk together, not
// slices of every image.  Fewer images are interleaved over all XCDs (i = w nimg + b).
__host__ inline int xcd_image_grid(int per, int nimg) { return nimg >= 8 ? 8 * per * ((nimg + 7) / 8) : per * nimg; }
__device__ inline bool xcd_image_map(int nimg, int& unit, int& img) {
    const int i = blockIdx.x;
    if (nimg >= 8) {
        const int per = (int)gridDim.x / (8 * ((nimg + 7) / 8)), q = i >> 3;
        unit = q % per;
        img = 8 * (q / per) + (i & 7);
        return img < nimg;
    }
    unit = i / nimg;
    img = i - unit * nimg;
    return true;
}

// ------------------------------------------------------------------------------ FAST
constexpr int kFastCells = 2;           // waves (cells) per workgroup

// LDS writes of this wave visible to its own later reads (wave-private LDS regions)
__device__ inline void wave_sync_lds_ex() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0)
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ inline int lanes_below(unsigned long long m) {
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// k_fast2: one wave per (image, cell), kFastCells cells per workgroup, so every step syncs at
// wave level only.  The cell ROI (<= 64 x 64) is staged in the wave's LDS as aligned dwords (its
// first byte at a per-cell offset 0..3) with a compile-time pitch TS, next to a score map of the
// same pitch, so every circle / compass / NMS neighbour read is one ds_read_u8 with an immediate
// offset from the pixel's address.  FAST with nonmax at ini_th, then at min_th when that finds
// nothing (src/ORBextractor.cc:804-817), as compaction stages over a row-major list of tile
// offsets (u16 y TS + x, ballot-compacted in place, so the order is FAST_t's emission order):
//   A    every scored pixel: two cyclically adjacent compass pixels (0, 4, 8, 12) both brighter
//        or both darker at t -- necessary for a 9-arc (any 9 consecutive of 16 hold two adjacent
//        multiples of 4); the eight compares are combined as lane masks;
//   B+C  the survivors: one pass of fast_arc_strength (fast_score.h: packed 16-bit min/max, S > t
//        is the segment test at t and S - 1 the cornerScore), which both finds the corners and
//        writes their scores into the map;
//   D    strict 3x3 NMS of the corners at the threshold (score >= t; neighbours below it count 0,
//        all eight read unconditionally), compacted in place.
// A to D run first at ini_th, and at min_th only for a cell with no survivor.  The window bases
// are kept out of the reads' address folding (lds_window).
// The survivors go to one of the level's kFastRegions dense candidate regions (cell k of the
// level: region k % R) at an offset taken with one atomic per cell, as {x | y << 12 | score << 24
// (x, y relative to minBorder, :820-825), cell << 10 | rank}: the tag orders them as the
// reference's cell loop does, so their position does not matter.
// Earlier forms and measured alternatives, none of them in the tree any more: a
// per-lane kernel with a runtime pitch (~2,900 VALU instructions per cell, VALU-issue-bound);
// separate segment-test and cornerScore stages (config 5: FAST 0.289 -> 0.164 ms per 64 frames
// when they became one pass, profiles/r06/fastab.txt); the arc test bit-sliced across the wave on
// the scalar unit, which cut the VALU count by 40 % but was slower, 0.327 vs 0.307 ms per 64
// frames, since the scalar unit issues at the same per-SIMD rate as the vector unit
// (profiles/r04/fast_seg_ab.txt).
// fast_arc_strength (fast_score.h) of every lane's pixel: cm = the pixel at (X - 3, Y - 3) of the
// tile (pitch TS), so all 17 reads take non-negative immediate offsets.  The caller masks
// inactive lanes.
template <int TS>
__device__ inline int fast_strength_lane(const uint8_t* cm, int th) {
    constexpr int o[16] = {6 * TS + 3, 6 * TS + 4, 5 * TS + 5, 4 * TS + 6, 3 * TS + 6, 2 * TS + 6, TS + 5, 4,
                           3, 2, TS + 1, 2 * TS, 3 * TS, 4 * TS, 5 * TS + 1, 6 * TS + 2};
    int p[16];
#pragma unroll
    for (int k = 0; k < 16; k++) p[k] = cm[o[k]];
    return fast_arc_strength(cm[3 * TS + 3], p, th);
}

// e - back as an offset the compiler cannot fold into the reads that follow: they then take the
// window's offsets as non-negative ds_read immediates (folded, the negative ones cost a VALU add
// each)
__device__ inline int lds_window(int e, int back) {
    int b = e - back;
    asm volatile("" : "+v"(b));
    return b;
}

constexpr int fast2_tile_bytes(int TS, int maxH) { return (TS * maxH + 15) & ~15; }
__host__ __device__ inline int fast2_wave_bytes(int TS, int maxW, int maxH) {
    return 2 * fast2_tile_bytes(TS, maxH) + ((2 * (maxW - 6) * (maxH - 6) + 15) & ~15);
}

template <int TS>
__global__ __launch_bounds__(64 * kFastCells) void k_fast2(const uint8_t* __restrict__ pyr, long long pimg,
                                                           const CellGeom* __restrict__ cells, int c0, int ncells,
                                                           uint2* __restrict__ cand, int keys_cap,
                                                           int* __restrict__ level_count, int nlevels, int ini_th,
                                                           int min_th, int maxW, int maxH, int nimg) {
    extern __shared__ uint4 fast_lds[];
    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int unit, b;
    if (!xcd_image_map(nimg, unit, b)) return;
    const int c = c0 + unit * kFastCells + wid;  // cells [c0, ncells)
    if (c >= ncells) return;
    const CellGeom cg = cells[c];
    if (cg.w == 0) return;
    const long long a = b * pimg + cg.roi_off;
    const int o = (int)(a & 3);  // stride is a multiple of 64: the same offset on every row
    const unsigned* src = reinterpret_cast<const unsigned*>(pyr + (a - o));
    const int w = cg.w, h = cg.h, nd = (w + o + 3) >> 2, s4 = cg.stride >> 2;
    const int tbytes = fast2_tile_bytes(TS, maxH);
    uint8_t* wl = reinterpret_cast<uint8_t*>(fast_lds) + wid * fast2_wave_bytes(TS, maxW, maxH);
    unsigned* t4 = reinterpret_cast<unsigned*>(wl);
    uint8_t* sc = wl + tbytes;  // scores, sc[y * TS + x]
    unsigned short* L = reinterpret_cast<unsigned short*>(wl + 2 * tbytes);
    {   // lane = (row phase r0, dword d) of the tile, R rows per round: one division per lane
        const int R = 64 / nd, r0 = lane / nd, d = lane - r0 * nd;
        if (r0 < R) {
            constexpr int kLd = 8;
            for (int rb = r0; rb < h; rb += kLd * R) {
                unsigned v[kLd];
#pragma unroll
                for (int k = 0; k < kLd; k++) {
                    const int r = rb + k * R;
                    v[k] = r < h ? src[(long long)r * s4 + d] : 0u;
                }
#pragma unroll
                for (int k = 0; k < kLd; k++) {
                    const int r = rb + k * R;
                    if (r < h) t4[r * (TS / 4) + d] = v[k];
                }
            }
        }
    }
    for (int k = lane; k < tbytes / 16; k += 64) reinterpret_cast<uint4*>(sc)[k] = make_uint4(0u, 0u, 0u, 0u);
    wave_sync_lds_ex();
    const uint8_t* tb = reinterpret_cast<const uint8_t*>(t4) + o;  // tb[y * TS + x]
    const int dw = w - 6, dh = h - 6, npix = dw > 0 && dh > 0 ? dw * dh : 0;
    const int ti = min(max(ini_th, 0), 255), tm = min(max(min_th, 0), 255), tl = min(ti, tm);
    // A: compass pre-test at t over the ROI's scored pixels, row-major, into L
    auto compass = [&](int t) {
        int n = 0;
        if (npix > 0) {
            int y = lane / dw, x = lane - y * dw;
            const int q = 64 / dw, r = 64 - q * dw;
            for (int p0 = 0; p0 < npix; p0 += 64) {
                // lanes past the last pixel read the ROI's last row (masked off below)
                const int e0 = __umul24(min(y, dh - 1), TS) + x + 3;  // the pixel at (X, Y - 3)
                const uint8_t* cp = tb + e0;
                const int pc = cp[0], pd = cp[3 * TS - 3], v = cp[3 * TS], pb = cp[3 * TS + 3], pa = cp[6 * TS];
                const int hi = v + t, lo = v - t;
                const bool ba = pa > hi, bb = pb > hi, bc = pc > hi, bd = pd > hi;
                const bool da = pa < lo, db = pb < lo, dc = pc < lo, dd = pd < lo;
                const bool pass = (((ba | bc) & (bb | bd)) | ((da | dc) & (db | dd))) && p0 + lane < npix;
                const unsigned long long m = __ballot(pass);
                if (pass) L[n + lanes_below(m)] = (unsigned short)(e0 + 3 * TS);
                n += __popcll(m);
                x += r;
                y += q;
                if (x >= dw) { x -= dw; y++; }
            }
        }
        wave_sync_lds_ex();
        return n;
    };
    auto nms = [&](unsigned short* Ls, int ns, int t) {
        int kept = 0;
        for (int i0 = 0; i0 < ns; i0 += 64) {
            const int i = i0 + lane;
            bool keep = false;
            unsigned short e = 0;
            if (i < ns) {
                e = Ls[i];
                const uint8_t* q = sc + lds_window(e, TS + 1);  // the 3x3 window's top-left
                const int s = q[TS + 1];
                const int u[8] = {q[0], q[1], q[2], q[TS], q[TS + 2], q[2 * TS], q[2 * TS + 1], q[2 * TS + 2]};
                keep = s >= t && s != 0;  // a neighbour below t counts 0
#pragma unroll
                for (int k = 0; k < 8; k++) keep &= u[k] < t || s > u[k];
            }
            const unsigned long long m = __ballot(keep);
            if (keep) Ls[kept + lanes_below(m)] = e;
            kept += __popcll(m);
        }
        return kept;
    };
    // B + C at once: S = fast_arc_strength at t; a corner at t' >= t exactly when S > t', its
    // score S - 1 whatever t (fast_score.h), so the pass both finds and scores the corners and
    // NMS reads the map at either threshold (scores below it count 0 there)
    auto strength = [&](int n, int t) {
        int nc = 0;
        for (int i0 = 0; i0 < n; i0 += 64) {
            const int i = i0 + lane;
            const unsigned short e = L[min(i, n - 1)];
            const int S = fast_strength_lane<TS>(tb + lds_window(e, 3 * TS + 3), t);
            const bool pass = S > t && i < n;
            const unsigned long long m = __ballot(pass);
            if (pass) {
                L[nc + lanes_below(m)] = e;
                sc[e] = (uint8_t)(S - 1);
            }
            nc += __popcll(m);
        }
        wave_sync_lds_ex();
        return nc;
    };
    // FAST at ini_th first, from its own compass survivors (a corner at ini_th, and so every
    // neighbour NMS at ini_th counts, passes the compass at ini_th): about half the candidates
    // of the compass at min_th.  Only a cell without a survivor runs the min_th pass (the
    // scores it rewrites are the same values).  With min_th >= ini_th one pass at ini_th
    // holds the corners of both.
    const bool two = tm < ti;
    int nc = strength(compass(two ? ti : tl), two ? ti : tl);
    int total = nms(L, nc, ti);
    if (total == 0 && tm != ti) {
        if (two) nc = strength(compass(tm), tm);
        total = nms(L, nc, tm);
    }
    if (total == 0) return;
    wave_sync_lds_ex();
    int base = 0;
    if (lane == 0)
        base = atomicAdd(&level_count[(b * nlevels + cg.level) * kFastRegions + cg.lcell % kFastRegions], total);
    base = __shfl(base, 0);
    uint2* dst = cand + (long long)b * keys_cap + cg.slot_base + base;
    const unsigned tag = (unsigned)cg.lcell << 10;
    for (int i = lane; i < total; i += 64) {
        const unsigned short e = L[i];
        const int Y = e / TS, X = e - Y * TS;
        dst[i] = make_uint2((uint32_t)(X + cg.sx) | ((uint32_t)(Y + cg.sy) << 12) | ((uint32_t)sc[e] << 24),
                            tag | (unsigned)i);
    }
}

// ------------------------------------------------------------------------------ octree
// DistributeOctTree (src/ORBextractor.cc:539-763) as data-parallel passes inside one
// workgroup per (image, level).  The std::list of nodes is kept as arrays in list order:
// a pass that divides D nodes pushes their non-empty children to the list front in visit
// order, so the new list is [children in reverse push order] ++ [undivided nodes in order]
// -- two prefix scans.  Keys never move: each key carries the index of its node, remapped
// after every pass through the parent's (node, quadrant) -> child table.
constexpr int kOctThreads = 1024;
constexpr int kOctRegKeys = 12;  // candidates per thread held in registers (12,288 per level; 13 spills)
#ifdef ORBMI_OCT_TRACE  // tools/octree_trace.hip: s_memtime stamps of workgroup g_oct_trace_block
__device__ unsigned long long g_oct_trace[256];
__device__ int g_oct_trace_block;
#define OCT_STAMP(i, v)                                                                                   \
    do {                                                                                                  \
        if (threadIdx.x == 0 && (int)blockIdx.x == g_oct_trace_block && blockIdx.y == 0) g_oct_trace[i] = (v); \
    } while (0)
#define OCT_SUB(it, j) do { if ((it) < 15) OCT_STAMP(100 + 10 * (it) + (j), __builtin_amdgcn_s_memtime()); } while (0)
#else
#define OCT_STAMP(i, v) do {} while (0)
#define OCT_SUB(it, j) do {} while (0)
#endif

struct OctShared {
    int cnt[2][kOctNodeCap];
    int ccnt[kOctNodeCap][4];            // child key counts; reused as best-key words
    short remap[kOctNodeCap][4];         // (old node, quadrant) -> new index
    unsigned long long skey[kOctNodeCap];
    int tmp[kOctNodeCap];
    int newpos[kOctNodeCap];
    unsigned char dflag[kOctNodeCap];
    int scratch[kOctThreads / 64 + 2];
    int misc[8];
    int rpre[kFastRegions + 1];          // candidate regions: prefix of counts, first slots
    int rbase[kFastRegions];
    unsigned tagl[kOctThreads * kOctRegKeys];  // order tags of the register-resident keys
};

// Quadrant decisions of one axis down the quadtree's fixed geometry: bit d is the decision at
// depth d (coordinate >= the box's mid, mid = lo + ceil((hi - lo) / 2)).  A child's extent on an
// axis depends only on the parent's extent on that axis and the decision
// (ExtractorNode::DivideNode, src/ORBextractor.cc:481-537), so each axis descends alone and a
// key's quadrant in its node at depth d is ((px >> d) & 1) | ((py >> d) & 1) << 1.  Coordinates
// are < 4096, so two keys are separated within 13 divisions; 16 are kept.
__device__ inline unsigned oct_axis(int v, int lo, int hi) {
    unsigned bits = 0;
#pragma unroll
    for (int d = 0; d < 16; d++) {
        const int mid = lo + ((hi - lo + 1) >> 1);
        const bool up = v >= mid;
        bits |= (unsigned)up << d;
        lo = up ? mid : lo;
        hi = up ? hi : mid;
    }
    return bits;
}

// Root node of a key (src/ORBextractor.cc:573-579) and its path bits (x low half, y high half).
__device__ inline int oct_root(uint32_t key, const LevelGeom& g) {
    return min((int)((float)(key & 0xFFF) / g.hX), g.nIni - 1);
}
__device__ inline unsigned oct_path(uint32_t key, const LevelGeom& g) {
    const int n = oct_root(key, g);
    const int x0 = (int)(g.hX * (float)n), x1 = (int)(g.hX * (float)(n + 1));
    return oct_axis((int)(key & 0xFFF), x0, x1) | oct_axis((int)((key >> 12) & 0xFFF), 0, g.height) << 16;
}
__device__ inline int oct_quad(unsigned path, int depth) {
    return (int)(((path >> depth) & 1u) | (((path >> (16 + depth)) & 1u) << 1));
}

// Exclusive scan of n <= kOctNodeCap ints in place (2 per thread); returns the total.
__device__ inline int block_scan_array(int* a, int n, int* scratch) {
    const int i0 = 2 * threadIdx.x, i1 = i0 + 1;
    const int v0 = i0 < n ? a[i0] : 0, v1 = i1 < n ? a[i1] : 0;
    int total;
    const int e = block_excl_scan(v0 + v1, scratch, &total);
    if (i0 < n) a[i0] = e;
    if (i1 < n) a[i1] = e + v0;
    __syncthreads();
    return total;
}

__device__ inline void bitonic_sort(unsigned long long* k, int n) {  // n power of two
    for (int size = 2; size <= n; size <<= 1)
        for (int j = size >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < n; i += blockDim.x) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const bool asc = (i & size) == 0;
                    const unsigned long long a = k[i], c = k[ixj];
                    if ((a > c) == asc) { k[i] = c; k[ixj] = a; }
                }
            }
            __syncthreads();
        }
}

// Bitonic sort of n <= blockDim.x keys, one per thread (v), ascending by thread index: stages
// with a partner in the same wave exchange through lane shuffles, the others through LDS (lds,
// >= blockDim.x entries) with block barriers; every thread of the block takes part.
__device__ inline unsigned long long bitonic_sort_block(unsigned long long v, int n, unsigned long long* lds) {
    const int i = threadIdx.x;
    for (int size = 2; size <= n; size <<= 1)
        for (int j = size >> 1; j > 0; j >>= 1) {
            unsigned long long other;
            if (j >= 64) {
                lds[i] = v;
                __syncthreads();
                other = lds[i ^ j];
                __syncthreads();
            } else {
                other = __shfl_xor(v, j, 64);
            }
            const bool lower = (i & j) == 0, asc = (i & size) == 0;
            v = (lower == asc) ? (v < other ? v : other) : (v < other ? other : v);
        }
    return v;
}

__device__ __forceinline__ void octree_body(OctShared& S, int level, int b, const LevelGeom* __restrict__ levels,
                                            int nlevels, const uint2* __restrict__ cand,
                                            const int* __restrict__ level_count, const int* __restrict__ regbase,
                                            uint32_t* __restrict__ node_of, int keys_cap,
                                                         uint2* __restrict__ oct_out, int out_cap,
                                                         int* __restrict__ oct_count) {
    const int tid = threadIdx.x;
    const LevelGeom g = levels[level];
    const uint2* CK = cand + (long long)b * keys_cap;                 // {key, order tag}, regions
    uint32_t* NO = node_of + (long long)b * keys_cap + g.key_base;     // node | depth << 16

    OCT_STAMP(0, __builtin_amdgcn_s_memtime());
    // ---- the level's candidates (k_fast2's dense array, in cell-completion order): thread t
    // holds keys t R .. t R + R - 1 in registers (R = kOctRegKeys; a cell's keys are contiguous,
    // so a thread's increments mostly hit one counter); keys from kOctThreads R on stay in CK
    // with their node in NO.  Nothing below depends on the keys' order except through the tags.
    // key k lives in region j with rpre[j] <= k < rpre[j + 1], at rbase[j] + k - rpre[j]
    if (tid < 64) {
        const int cnt = tid < kFastRegions ? level_count[(b * nlevels + level) * kFastRegions + tid] : 0;
        const int incl = wave_incl_scan(cnt);
        if (tid < kFastRegions) {
            S.rpre[tid + 1] = incl;
            S.rbase[tid] = regbase[level * kFastRegions + tid];
        }
        if (tid == 0) S.rpre[0] = 0;
    }
    // per-axis path tables (x: its own root's extent, y: the level height), in the LDS of the
    // careful-mode sort keys, built while the counts above are in flight
    unsigned short* xpath = reinterpret_cast<unsigned short*>(S.skey);
    unsigned short* ypath = xpath + 4096;
    const int wx = min(g.width, 4095), hy = min(g.height, 4095);
    for (int v = tid; v <= wx + 1 + hy; v += blockDim.x) {
        if (v <= wx) {
            const int n = oct_root((uint32_t)v, g);
            xpath[v] = (unsigned short)oct_axis(v, (int)(g.hX * (float)n), (int)(g.hX * (float)(n + 1)));
        } else {
            const int y = v - wx - 1;
            ypath[y] = (unsigned short)oct_axis(y, 0, g.height);
        }
    }
    for (int i = tid; i < g.nIni; i += blockDim.x) S.cnt[0][i] = 0;  // root counts (init below)
    __syncthreads();
    const int nkeys = min(S.rpre[kFastRegions], g.key_cap);
    auto key_slot = [&](int k, int& j) {  // j: a region at or before k's (walks forward)
        while (j < kFastRegions - 1 && S.rpre[j + 1] <= k) j++;
        return S.rbase[j] + (k - S.rpre[j]);
    };
    int j0 = 0;  // region of the thread's first key: the largest j with rpre[j] <= k
    {
        const int k0 = tid * kOctRegKeys;
        int lo = 0, hi = kFastRegions - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (S.rpre[mid] <= k0) lo = mid;
            else hi = mid - 1;
        }
        j0 = lo;
    }
    uint32_t kreg[kOctRegKeys];
    int nreg[kOctRegKeys];
    {
        int j = j0;
#pragma unroll
        for (int r = 0; r < kOctRegKeys; r++) {
            const int k = tid * kOctRegKeys + r;
            uint2 kv = make_uint2(0u, 0u);
            if (k < nkeys) kv = CK[key_slot(k, j)];
            kreg[r] = kv.x;
            S.tagl[k] = kv.y;
            nreg[r] = 0;
        }
    }
    // f(k, key, node&) for every key, in increasing k per thread: the register-resident
    // ones, then the global spill
    auto for_keys = [&](auto&& f) {
#pragma unroll
        for (int r = 0; r < kOctRegKeys; r++) {
            const int k = tid * kOctRegKeys + r;
            if (k < nkeys) f(k, kreg[r], nreg[r]);
        }
        for (int k = tid + kOctThreads * kOctRegKeys; k < nkeys; k += kOctThreads) {
            int no = (int)NO[k], j = 0;
            f(k, CK[key_slot(k, j)].x, no);
            NO[k] = (uint32_t)no;
        }
    };

    // path bits of the register keys (tables built above)
    unsigned preg[kOctRegKeys];
    {
#pragma unroll
        for (int r = 0; r < kOctRegKeys; r++)
            preg[r] = xpath[min((int)(kreg[r] & 0xFFF), wx)] | (unsigned)ypath[min((int)((kreg[r] >> 12) & 0xFFF), hy)] << 16;
        __syncthreads();
    }
    OCT_STAMP(1, __builtin_amdgcn_s_memtime());
    OCT_STAMP(62, nkeys);
    // ---- initial nodes (:543-579): counts per root (zeroed before the first barrier)
    const int nIni = g.nIni;
    int cur = 0;
    {
        int run = -1, rc = 0;  // consecutive keys of a thread share a node: one atomic per run
        for_keys([&](int, uint32_t key, int& no) {
            const int n = oct_root(key, g);
            no = n;
            if (n != run) {
                if (rc) atomicAdd(&S.cnt[cur][run], rc);
                run = n;
                rc = 0;
            }
            rc++;
        });
        if (rc) atomicAdd(&S.cnt[cur][run], rc);
    }
    __syncthreads();
    // drop empty initial nodes (:581-593): a ballot scan in wave 0 (nIni <= 64), else block scans
    int L;
    if (nIni <= 64) {
        if (tid < 64) {
            const int c = tid < nIni ? S.cnt[cur][tid] : 0;
            const unsigned long long m = __ballot(c > 0);
            const int ni = c > 0 ? __popcll(m & ((1ull << tid) - 1)) : -1;
            if (tid < nIni) {
                S.remap[tid][0] = S.remap[tid][1] = S.remap[tid][2] = S.remap[tid][3] = (short)ni;
                if (ni >= 0) S.cnt[cur ^ 1][ni] = c;
            }
            if (tid == 0) S.misc[4] = __popcll(m);
        }
        __syncthreads();
        L = S.misc[4];
    } else {
        for (int i = tid; i < nIni; i += blockDim.x) S.tmp[i] = S.cnt[cur][i] > 0;
        __syncthreads();
        L = block_scan_array(S.tmp, nIni, S.scratch);
        for (int i = tid; i < nIni; i += blockDim.x) {
            const short ni = S.cnt[cur][i] > 0 ? (short)S.tmp[i] : (short)-1;
            S.remap[i][0] = S.remap[i][1] = S.remap[i][2] = S.remap[i][3] = ni;
            if (ni >= 0) S.cnt[cur ^ 1][ni] = S.cnt[cur][i];
        }
        __syncthreads();
    }
    cur ^= 1;

    const int N = g.nfeat;
    bool careful = false, finish = false;
    OCT_STAMP(2, __builtin_amdgcn_s_memtime());
    int iters = 0;
    for (int iter = 0; iter < 256 && !finish; iter++) {
        iters++;
        const int prv = cur ^ 1;
        for (int i = tid; i < L; i += blockDim.x) {
            S.ccnt[i][0] = S.ccnt[i][1] = S.ccnt[i][2] = S.ccnt[i][3] = 0;
        }
        if (tid == 0) {
            S.misc[2 + (iter & 1)] = 0;  // read at the end of pass iter - 2
            S.misc[0] = 0;               // careful mode: candidate count, size >= 64 flag
            S.misc[6] = 0;
        }
        __syncthreads();
        OCT_SUB(iter, 0);
        // keys: apply the previous pass's remap (an entry with bit 14 set means the node was
        // divided: the key moved one level down), then histogram the key's quadrant in its new
        // node.  Nodes with one key get counts too; only nodes with >= 2 keys read them.
        {
            int tgt[kOctRegKeys];
#pragma unroll
            for (int r = 0; r < kOctRegKeys; r++) tgt[r] = S.remap[nreg[r] & 0xFFFF][oct_quad(preg[r], nreg[r] >> 16)];
            OCT_SUB(iter, 6);
#pragma unroll
            for (int r = 0; r < kOctRegKeys; r++) {
                const bool v = tid * kOctRegKeys + r < nkeys;  // absent keys stay on node 0
                const int e = tgt[r], node = e & 0x3FFF, dep = (nreg[r] >> 16) + ((e >> 14) & 1);
                nreg[r] = v ? node | dep << 16 : 0;
                tgt[r] = v ? 4 * node + oct_quad(preg[r], dep) : -1;
            }
            int run = -1, rc = 0;
#pragma unroll
            for (int r = 0; r < kOctRegKeys; r++) {
                if (tgt[r] != run) {
                    if (rc && run >= 0) atomicAdd(&S.ccnt[0][0] + run, rc);
                    run = tgt[r];
                    rc = 0;
                }
                rc++;
            }
            if (rc && run >= 0) atomicAdd(&S.ccnt[0][0] + run, rc);
            OCT_SUB(iter, 7);
            // spilled keys
            for (int k = tid + kOctThreads * kOctRegKeys; k < nkeys; k += kOctThreads) {
                int j = 0;
                const unsigned path = oct_path(CK[key_slot(k, j)].x, g);
                const int no = (int)NO[k];
                const int e = S.remap[no & 0xFFFF][oct_quad(path, no >> 16)];
                const int node = e & 0x3FFF, dep = (no >> 16) + ((e >> 14) & 1);
                NO[k] = (uint32_t)(node | dep << 16);
                atomicAdd(&S.ccnt[node][oct_quad(path, dep)], 1);
            }
            OCT_SUB(iter, 8);
        }
        __syncthreads();
        OCT_SUB(iter, 1);
        // which nodes divide, and in which push order
        int ncand = 0, kdiv = 0;
        if (careful) {
            // vSizeAndPointerToNode sorted by (size, creation); divided largest first (:681-733).
            // Only the nodes with >= 2 keys can divide, and their sizes are small integers: a
            // counting sort gives every such node its rank directly -- the nodes with a larger
            // size, plus the earlier nodes of its own size (per chunk of 64 nodes from the ballots
            // of the size's six bit planes, then a prefix over the chunks).  A size of 64 or more
            // takes round 5's path: a bitonic sort of the whole list, wave 0 walking the result.
            static_assert(2 * kOctThreads >= kOctNodeCap, "two nodes per thread");
            int* Wh = S.tmp;      // [32 chunks][64 sizes]: counts, then their prefix over chunks
            int* Sgt = S.newpos;  // [64]: candidates of a larger size (newpos is written after the sort)
            // a size of 64 or more anywhere takes round 5's bitonic path (misc[0], misc[6] were
            // reset at the top of the pass)
            {
                bool big = false;
                for (int i = tid; i < 32 * 64; i += blockDim.x) {
                    Wh[i] = 0;
                    big |= i < L && S.cnt[cur][i] >= 64;
                }
                if (__ballot(big) && (tid & 63) == 0) S.misc[6] = 1;
            }
            __syncthreads();
            if (!S.misc[6]) {
                int val[2], rnk[2];
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    const int i = tid + h * kOctThreads, q = i >> 6;
                    const int c = i < L ? S.cnt[cur][i] : 0;
                    const int v = c >= 2 ? c : -1;
                    // the chunk's lanes of the same size: the six bit planes of the size, combined
                    unsigned long long same = __ballot(v >= 0);
                    if (same && (tid & 63) == 0) atomicAdd(&S.misc[0], __popcll(same));
#pragma unroll
                    for (int bit = 0; bit < 6; bit++) {
                        const unsigned long long pl = __ballot((v >> bit) & 1);
                        same &= ((v >> bit) & 1) ? pl : ~pl;
                    }
                    const int rw = lanes_below(same);
                    if (v >= 0 && rw == 0) Wh[q * 64 + v] = __popcll(same);  // the size's first lane
                    val[h] = v;
                    rnk[h] = rw;
                }
                for (int i = tid; i < L; i += blockDim.x) S.dflag[i] = 0;
                __syncthreads();
                ncand = S.misc[0];
                if (tid < 64) {  // lane = size: prefix over the chunks, then the larger sizes' total
                    int run = 0;
                    for (int q0 = 0; q0 < 32; q0 += 8) {  // 8 loads in flight (the VGPR budget)
                        int t[8];
#pragma unroll
                        for (int q = 0; q < 8; q++) t[q] = Wh[(q0 + q) * 64 + tid];
#pragma unroll
                        for (int q = 0; q < 8; q++) {
                            Wh[(q0 + q) * 64 + tid] = run;
                            run += t[q];
                        }
                    }
                    const int rv = __shfl(run, 63 - tid);  // total of size 63 - lane
                    const int incl = wave_incl_scan(rv);
                    Sgt[63 - tid] = incl - rv;
                }
                __syncthreads();
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    const int i = tid + h * kOctThreads, v = val[h];
                    if (v >= 0)
                        S.skey[Sgt[v] + Wh[(i >> 6) * 64 + v] + rnk[h]] =
                            ((unsigned long long)(0xFFFFFFFFu - (unsigned)S.cnt[cur][i]) << 32) | (unsigned)i;
                }
                __syncthreads();
                // kdiv = 1 + the first r whose division brings the list to N (L + sum_{r' <= r}
                // (m_r' - 1) >= N, m the node's non-empty children), then the divided nodes' push bases
                // (prefix of m in sorted order): one block scan of m - 1 over the sorted candidates,
                // two per thread (the prefix of m is that of m - 1 plus r); the first r to reach N is
                // the only one whose exclusive prefix is still short of it, so one thread writes kdiv
                {
                    auto m_of = [&](int n) {
                        return (S.ccnt[n][0] > 0) + (S.ccnt[n][1] > 0) + (S.ccnt[n][2] > 0) + (S.ccnt[n][3] > 0);
                    };
                    if (tid == 0) S.misc[5] = ncand;  // no r reaches N: every candidate divides
                    const int r0 = 2 * tid, r1 = r0 + 1;
                    const int n0 = r0 < ncand ? (int)(S.skey[r0] & 0xFFFFFFFFu) : 0;
                    const int n1 = r1 < ncand ? (int)(S.skey[r1] & 0xFFFFFFFFu) : 0;
                    const int d0 = r0 < ncand ? m_of(n0) - 1 : 0, d1 = r1 < ncand ? m_of(n1) - 1 : 0;
                    int tot;
                    const int e0 = block_excl_scan(d0 + d1, S.scratch, &tot);  // its barriers publish misc[5]
                    if (r0 < ncand && (r0 == 0 || L + e0 < N) && L + e0 + d0 >= N) S.misc[5] = r0 + 1;
                    if (r1 < ncand && L + e0 + d0 < N && L + e0 + d0 + d1 >= N) S.misc[5] = r1 + 1;
                    __syncthreads();
                    const int kd = S.misc[5];
                    if (r0 < kd) {
                        S.dflag[n0] = 1;
                        S.newpos[n0] = e0 + r0;
                    }
                    if (r1 < kd) {
                        S.dflag[n1] = 1;
                        S.newpos[n1] = e0 + d0 + r1;
                    }
                    kdiv = kd;
                }
            } else {
                int np2 = 2;
                while (np2 < L) np2 <<= 1;
                if (np2 <= kOctThreads) {
                    const bool c2 = tid < L && S.cnt[cur][tid] >= 2;
                    const unsigned long long key =
                        c2 ? ((unsigned long long)(0xFFFFFFFFu - (unsigned)S.cnt[cur][tid]) << 32) | (unsigned)tid : ~0ull;
                    const int nw = __popcll(__ballot(c2));
                    if ((tid & 63) == 0 && nw) atomicAdd(&S.misc[0], nw);
                    const unsigned long long sorted = bitonic_sort_block(key, np2, S.skey);
                    __syncthreads();
                    if (tid < np2) S.skey[tid] = sorted;
                    for (int i = tid; i < L; i += blockDim.x) S.dflag[i] = 0;
                    ncand = S.misc[0];
                    __syncthreads();
                } else {
                    for (int i = tid; i < np2; i += blockDim.x) {
                        unsigned long long key = ~0ull;
                        if (i < L && S.cnt[cur][i] >= 2)
                            key = ((unsigned long long)(0xFFFFFFFFu - (unsigned)S.cnt[cur][i]) << 32) | (unsigned)i;
                        S.skey[i] = key;
                    }
                    for (int i = tid; i < L; i += blockDim.x) {
                        if (S.cnt[cur][i] >= 2) atomicAdd(&S.misc[0], 1);
                        S.dflag[i] = 0;
                    }
                    bitonic_sort(S.skey, np2);
                    ncand = S.misc[0];
                }
                // wave 0 walks the sorted candidates in chunks of 64 with wave scans: kdiv = 1 + the
                // first r whose division brings the list to N (L + sum_{r' <= r} (m_r' - 1) >= N),
                // then the divided nodes' push bases (prefix of m in sorted order)
                if (tid < 64) {
                    auto m_of = [&](int n) {
                        return (S.ccnt[n][0] > 0) + (S.ccnt[n][1] > 0) + (S.ccnt[n][2] > 0) + (S.ccnt[n][3] > 0);
                    };
                    int run = 0, kd = ncand;
                    for (int r0 = 0; r0 < ncand; r0 += 64) {
                        const int r = r0 + tid;
                        const int m = r < ncand ? m_of((int)(S.skey[r] & 0xFFFFFFFFu)) : 1;
                        const int incl = wave_incl_scan(m - 1);
                        const unsigned long long hit = __ballot(r < ncand && L + run + incl >= N);
                        if (hit) {
                            kd = r0 + __ffsll((long long)hit);
                            break;
                        }
                        run += __builtin_amdgcn_readlane(incl, 63);
                    }
                    int push = 0;
                    for (int r0 = 0; r0 < kd; r0 += 64) {
                        const int r = r0 + tid;
                        const int n = r < kd ? (int)(S.skey[r] & 0xFFFFFFFFu) : 0;
                        const int m = r < kd ? m_of(n) : 0;
                        const int incl = wave_incl_scan(m);
                        if (r < kd) {
                            S.dflag[n] = 1;
                            S.newpos[n] = push + incl - m;
                        }
                        push += __builtin_amdgcn_readlane(incl, 63);
                    }
                    kdiv = kd;
                }
            }
            __syncthreads();
        }
        OCT_SUB(iter, 2);
        // one packed scan over the list, two nodes per thread: child pushes of the dividing nodes
        // (outside the careful mode their push base in list order) | survivors << 16; the
        // children with more than one key go to one atomic per wave
        const int i0 = 2 * tid, i1 = i0 + 1;
        int ne = 0;
        auto classify = [&](int i) -> int {
            if (i >= L) return 0;
            const bool d = careful ? S.dflag[i] != 0 : S.cnt[cur][i] >= 2;
            if (!careful) S.dflag[i] = d;
            if (!d) return 1 << 16;
            int m = 0;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int c = S.ccnt[i][q];
                m += c > 0;
                ne += c > 1;
            }
            return m;
        };
        const int v0 = classify(i0), v1 = classify(i1);
        ne = wave_sum_i32(ne);
        if ((tid & 63) == 0 && ne) atomicAdd(&S.misc[2 + (iter & 1)], ne);
        int total;
        const int e0 = block_excl_scan(v0 + v1, S.scratch, &total);
        const int P = total & 0xFFFF, nsurv = total >> 16;
        const int nToExpand = S.misc[2 + (iter & 1)];  // every atomic precedes the scan's barriers
        OCT_SUB(iter, 3);
        auto rewrite = [&](int i, int e) {
            if (i >= L) return;
            if (S.dflag[i]) {
                int p = careful ? S.newpos[i] : (e & 0xFFFF);
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int c = S.ccnt[i][q];
                    if (c > 0) {
                        const int ni = P - 1 - p++;
                        if (ni < kOctNodeCap) S.cnt[prv][ni] = c;  // bound proven in DESIGN.md; guard LDS anyway
                        S.remap[i][q] = (short)(min(ni, kOctNodeCap - 1) | 0x4000);
                    } else {
                        S.remap[i][q] = -1;
                    }
                }
            } else {
                const int ni = min(P + (e >> 16), kOctNodeCap - 1);
                S.cnt[prv][ni] = S.cnt[cur][i];
                S.remap[i][0] = S.remap[i][1] = S.remap[i][2] = S.remap[i][3] = (short)ni;
            }
        };
        rewrite(i0, e0);
        rewrite(i1, e0 + v0);
        __syncthreads();  // the next pass clears ccnt and reads cnt[prv] / remap
        OCT_SUB(iter, 4);
        const int newL = min(P + nsurv, kOctNodeCap);
        // the remap just written maps list `cur` to list `prv`; keys apply it next pass
        cur = prv;
        if (newL >= N || newL == L) finish = true;
        else if (!careful && newL + nToExpand * 3 > N) careful = true;
        L = newL;
        (void)ncand;
        (void)kdiv;
        if (iter < 50) OCT_STAMP(3 + iter, __builtin_amdgcn_s_memtime() | ((unsigned long long)careful << 63));
    }
    OCT_STAMP(61, iters);
    (void)iters;
    OCT_STAMP(60, L);

    // ---- keep the max-response key per node, first in original order on ties (:744-760):
    // one 64-bit max per node over score << 56 | (2^24 - 1 - tag) << 24 | (y << 12 | x)
    unsigned long long* best = reinterpret_cast<unsigned long long*>(&S.ccnt[0][0]);  // 2 per row
    for (int i = tid; i < L; i += blockDim.x) best[2 * i] = 0;
    __syncthreads();
    {
        int fn[kOctRegKeys];  // final node of each register key, all reads first
#pragma unroll
        for (int r = 0; r < kOctRegKeys; r++) {
            const bool v = tid * kOctRegKeys + r < nkeys;
            const int e = S.remap[nreg[r] & 0xFFFF][oct_quad(preg[r], nreg[r] >> 16)];
            fn[r] = v ? (e & 0x3FFF) : -1;
        }
        uint32_t treg[kOctRegKeys];  // order tags
#pragma unroll
        for (int r = 0; r < kOctRegKeys; r++) treg[r] = S.tagl[tid * kOctRegKeys + r];
#pragma unroll
        for (int r = 0; r < kOctRegKeys; r++) {
            const uint32_t key = kreg[r];
            if (fn[r] >= 0)
                atomicMax(&best[2 * fn[r]], ((unsigned long long)(key >> 24) << 56) |
                                                ((unsigned long long)(0xFFFFFFu - treg[r]) << 24) | (key & 0xFFFFFFu));
        }
        for (int k = tid + kOctThreads * kOctRegKeys; k < nkeys; k += kOctThreads) {
            int j = 0;
            const uint2 kv = CK[key_slot(k, j)];
            const uint32_t key = kv.x, tg = kv.y;
            const int no = (int)NO[k];
            const int n = S.remap[no & 0xFFFF][oct_quad(oct_path(key, g), no >> 16)] & 0x3FFF;
            atomicMax(&best[2 * n], ((unsigned long long)(key >> 24) << 56) |
                                        ((unsigned long long)(0xFFFFFFu - tg) << 24) | (key & 0xFFFFFFu));
        }
    }
    __syncthreads();
    const int minB = kEdge - 3;
    uint2* out = oct_out + (long long)b * out_cap + g.out_base;
    for (int i = tid; i < L && i < g.out_cap; i += blockDim.x) {
        const unsigned long long v = best[2 * i];
        const uint32_t key = (uint32_t)(v & 0xFFFFFFu);
        out[i] = make_uint2(((key & 0xFFF) + minB) | ((((key >> 12) & 0xFFF) + minB) << 16), (uint32_t)(v >> 56));
    }
    if (tid == 0) oct_count[b * nlevels + level] = min(L, g.out_cap);
    OCT_STAMP(59, __builtin_amdgcn_s_memtime());
}

// ------------------------------------------------------------------------------ blur
// GaussianBlur(7x7, sigma 2, REFLECT_101) of every level (src/ORBextractor.cc:1085-1086), pinned
// as P3: separable integer taps {18,34,49,55,49,34,18}, float column pass for x < blur_xv,
// integer tail.  The reflect-101 border of the padded pyramid supplies the taps outside the
// image.  One 128x32 output tile per workgroup: 16-B loads of the padded rows (interior column
// x0 - 3 sits at a 16-B boundary) staged in LDS, row sums in registers, 4x4 outputs per thread stored as dwords
// into the interior-only blurred layout.
constexpr int kBlurInH = kBlurTH + 6, kBlurChunks = (kBlurTW + 6 + 15) / 16;  // 38 rows x 9 x 16 B
constexpr int kBlurInS = 16 * kBlurChunks;                                     // 144
struct BlurShared {
    uint4 in4[kBlurInH * kBlurChunks];
};
// One tile on a 256-thread slice of the workgroup (tid = 0..255).  The slice's block-wide barrier
// is reached by every slice, also one without a tile (valid = false).  The input rows are staged
// in LDS; thread (column group cg, row group rg) then forms the integer row sums of its 4 columns
// for the 10 input rows its 4 output rows read (3 aligned dword reads per row) in registers and
// the column pass from them: no row-sum array round-trips LDS.
__device__ __forceinline__ void blur_tile(BlurShared& B, const uint8_t* __restrict__ pyr, uint8_t* __restrict__ blur,
                                          long long pimg, long long bimg, const LevelGeom* __restrict__ levels,
                                          int2 t, int b, int tid, bool valid) {
    uint4* in4 = B.in4;
    const LevelGeom g = levels[valid ? t.x : 0];
    const int x0 = t.y & 0xFFFF, y0 = t.y >> 16;
    const uint8_t* lvl = pyr + b * pimg + g.off + kEdge - 3 + x0;  // column x0 - 3 of padded row 0
    for (int i = tid; valid && i < kBlurInH * kBlurChunks; i += 256) {
        const int r = i / kBlurChunks, ch = i - r * kBlurChunks;
        const int yy = min(y0 - 3 + r, g.H + 2);  // rows past H + 2 feed only discarded outputs
        in4[i] = *reinterpret_cast<const uint4*>(lvl + (long long)(kEdge + yy) * g.stride + 16 * ch);
    }
    __syncthreads();
    if (!valid) return;
    const int cq = 4 * (tid & 31), rb = 4 * (tid >> 5);  // 4 columns x 4 output rows per thread
    if (y0 + rb >= g.H) return;
    const unsigned* in = reinterpret_cast<const unsigned*>(in4);
    // row pass: the 7 taps of column cq + c are bytes c .. c + 6 of (w0, w1, w2): two v_dot4
    // over byte-aligned dwords (v_alignbyte), weights (18, 34, 49, 55) and (49, 34, 18, 0)
    constexpr unsigned kW0 = 18u | 34u << 8 | 49u << 16 | 55u << 24, kW1 = 49u | 34u << 8 | 18u << 16;
    unsigned rs[10][4];  // row sums of input rows rb .. rb + 9 (output row rb + rr reads rb + rr .. + 6)
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const unsigned* q = in + (rb + r) * (kBlurInS / 4) + cq / 4;  // bytes = input columns cq - 3 ..
        const unsigned w0 = q[0], w1 = q[1], w2 = q[2];
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const unsigned a = c ? __builtin_amdgcn_alignbyte(w1, w0, c) : w0;
            const unsigned h = c ? __builtin_amdgcn_alignbyte(w2, w1, c) : w1;
            rs[r][c] = __builtin_amdgcn_udot4(h, kW1, __builtin_amdgcn_udot4(a, kW0, 0u, false), false);
        }
    }
    // column pass: S = 55 c3 + 49 p1 + 34 p2 + 18 p3 < 2^24 unless the result saturates, so the
    // reference's float path (SymmColumnVec_32s8u: S / 65536 in float, one rounding per operation,
    // then rint) is exact: round-half-even of S / 65536; the scalar tail rounds half up
    uint8_t* dst = blur + b * bimg + g.boff;
#pragma unroll
    for (int rr = 0; rr < 4; rr++) {
        const int y = y0 + rb + rr;
        if (y >= g.H) break;
        unsigned packedv = 0;
#pragma unroll
        for (int cc = 0; cc < 4; cc++) {
            const int x = x0 + cq + cc;
            const unsigned S = __umul24(rs[rr + 3][cc], 55u) + __umul24(rs[rr + 2][cc] + rs[rr + 4][cc], 49u) +
                               __umul24(rs[rr + 1][cc] + rs[rr + 5][cc], 34u) + __umul24(rs[rr][cc] + rs[rr + 6][cc], 18u);
            const unsigned up = x < g.blur_xv ? (S >> 16) & 1u : 1u;
            const unsigned v = min((S + 0x7FFFu + up) >> 16, 255u);
            packedv |= v << (8 * cc);
        }
        if (x0 + cq < g.bstride)
            *reinterpret_cast<unsigned*>(dst + (long long)y * g.bstride + x0 + cq) = packedv;
    }
}

// DistributeOctTree and GaussianBlur in one launch, on a 1-D grid: the first blocks run one
// (image, level) octree each and are dispatched first; the blocks after them blur four
// 128x32 tiles each on the CUs the octrees leave idle.  A level-0 octree is the launch's longest
// workgroup (its candidates are the most), so the blur hides behind it instead of following it.
// Both only read the pyramid; the blur slices reuse the octree's LDS.
static_assert(sizeof(OctShared) >= 4 * sizeof(BlurShared), "blur slices overlay the octree LDS");
constexpr int kFuseBlurMaxOctrees = 64;  // octree workgroups up to which the blur rides along
__global__ __launch_bounds__(kOctThreads) void k_octree(const LevelGeom* __restrict__ levels, int nlevels,
                                                         const uint2* __restrict__ cand,
                                                         const int* __restrict__ level_count,
                                                         const int* __restrict__ regbase,
                                                         uint32_t* __restrict__ node_of,
                                                         int keys_cap, uint2* __restrict__ oct_out, int out_cap,
                                                         int* __restrict__ oct_count, const uint8_t* __restrict__ pyr,
                                                         uint8_t* __restrict__ blur, long long pimg, long long bimg,
                                                         const int2* __restrict__ btiles, int nbtiles, int batch) {
    __shared__ OctShared S;
    // workgroup i goes to XCD i % 8, and workgroups are dispatched in index order.  A large batch
    // takes two rounds of one octree workgroup per CU, so the octrees are numbered longest first
    // (level-major from the top level down: alone, every level takes 47-52 us and the top one
    // 84 us at config 5), each level spread over all XCDs (image 8 s + i % 8 for slot s).
    const int b8 = (batch + 7) / 8, noct = nlevels * 8 * b8;
    if ((int)blockIdx.x < noct) {
        const int q = blockIdx.x >> 3, lv = nlevels - 1 - q / b8, img = 8 * (q % b8) + (blockIdx.x & 7);
#ifdef ORBMI_OCT_ONLY_LEVEL  // timing experiment (tools: A/B builds): run the octrees of one level only
        if ((ORBMI_OCT_ONLY_LEVEL >= 0) != (lv == (ORBMI_OCT_ONLY_LEVEL < 0 ? -1 - ORBMI_OCT_ONLY_LEVEL : ORBMI_OCT_ONLY_LEVEL)))
            return;
#endif
        if (img < batch)
            octree_body(S, lv, img, levels, nlevels, cand, level_count, regbase, node_of, keys_cap, oct_out, out_cap,
                        oct_count);
        return;
    }
    const int slice = threadIdx.x >> 8, ti = ((int)blockIdx.x - noct) * 4 + slice;  // over (image, tile)
    const bool valid = ti < nbtiles * batch;
    const int img = valid ? ti / nbtiles : 0, tile = valid ? ti - img * nbtiles : 0;
    BlurShared* B = reinterpret_cast<BlurShared*>(&S) + slice;
    blur_tile(*B, pyr, blur, pimg, bimg, levels, btiles[tile], img, threadIdx.x & 255, valid);
}

// GaussianBlur alone: one 128x32 tile per 256-thread workgroup.
__global__ __launch_bounds__(256) void k_blur(const uint8_t* __restrict__ pyr, uint8_t* __restrict__ blur,
                                              long long pimg, long long bimg, const LevelGeom* __restrict__ levels,
                                              const int2* __restrict__ tiles, int nimg) {
    __shared__ BlurShared B;
    int tile, b;
    if (!xcd_image_map(nimg, tile, b)) return;
    blur_tile(B, pyr, blur, pimg, bimg, levels, tiles[tile], b, threadIdx.x, true);
}

// ------------------------------------------------------------------------------ describe
constexpr int kBR = 18;                 // rotated rBRIEF samples lie within 18 px (pattern radius 18.4)
constexpr int kBW = 2 * kBR + 1;        // blurred window 37 x 37
constexpr int kUR = 15;                 // IC_Angle patch radius (HALF_PATCH_SIZE)

__device__ inline float fast_atan2_deg(float y, float x) {
    // cv::fastAtan2 (OpenCV 3.x mathfuncs): polynomial in degrees
    const float p1 = 0.9997878412794807f * (float)(180 / M_PI);
    const float p3 = -0.3258083974640975f * (float)(180 / M_PI);
    const float p5 = 0.1555786518463281f * (float)(180 / M_PI);
    const float p7 = -0.04432655554792128f * (float)(180 / M_PI);
    const float ax = fabsf(x), ay = fabsf(y);
    float a, c, c2;
    if (ax >= ay) {
        c = ay / (ax + (float)2.220446049250313e-16);
        c2 = c * c;
        a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    } else {
        c = ax / (ay + (float)2.220446049250313e-16);
        c2 = c * c;
        a = 90.f - (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    }
    if (x < 0) a = 180.f - a;
    if (y < 0) a = 360.f - a;
    return a;
}

// Four keypoints per wave, one DPP row (16 lanes) each: the per-keypoint scalar work -- the
// moment sums' reduction, fastAtan2, the fp64 sincos, the output record -- runs once for four
// keypoints, and the lane-parallel parts keep their instruction count per keypoint:
//   * IC_Angle (:77-104) straight from the unblurred level: the 749 patch pixels as <= 213
//     aligned dwords (c_ictab[ou], per 4-B phase ou of the patch's first byte), each dword
//     weighted by three v_dot4_u32_u8: (u + 16), (v + 16) and 1 on the circle's bytes, 0 off it,
//     so m_10 = S_u - 16 S_1 and m_01 = S_v - 16 S_1 (integers: exact);
//   * the blurred 37 x 37 window staged in LDS with 8-B loads (rows of kBP bytes);
//   * rBRIEF (:108-147, pinned P6): lane l takes the pairs 16 l + k, k = 15 .. 0; the rotation
//     in packed fp32 (the same products and sums, rounded as the reference's float expression),
//     cvRound by adding 1.5 * 2^23 (round-half-even to an integer in the low mantissa bits, which
//     index LDS directly), and the bits shifted into one 16-bit word per lane: lane l holds bytes
//     2l, 2l+1 of its keypoint's descriptor.
// A workgroup takes kDescKpWG consecutive slots per step and strides over the image's slots.
constexpr int kDescGroups = 4;                        // keypoints per wave
constexpr int kDescWaves = 4;                         // waves per workgroup
constexpr int kDescKpWG = kDescGroups * kDescWaves;  // slots per workgroup step
constexpr int kDescTargetWG = 1536;                   // workgroups per launch (3 per CU, 2 rounds)
#ifndef ORBMI_DESC_BP
#define ORBMI_DESC_BP 48
#endif
constexpr int kBP = ORBMI_DESC_BP;                    // LDS pitch: 37 bytes from any 8-B phase need 44
constexpr int kBQ = kBP / 8;                          // 8-B loads per window row
struct DescLevel { long long off, boff; int stride, bstride, out_base; float scale, size; };
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
__constant__ float4 c_pattern_f[256];     // (x0, x1, y0, y1) of pair t = 16 l + k at 16 k + l
__constant__ uint4 c_ictab[4][kIcItems];  // {u + 16 weights, circle mask, window row, 4 * dword}

__device__ inline unsigned row16_sum(unsigned v) {  // sum over the lane's DPP row, in every lane
    v += dpp_mov_u32<kDppXor1>(v);
    v += dpp_mov_u32<kDppXor2>(v);
    v += dpp_mov_u32<kDppHalfMirror>(v);
    return v + dpp_mov_u32<kDppRor8>(v);
}

__global__ __launch_bounds__(64 * kDescWaves) void k_describe4(const uint8_t* __restrict__ pyr,
                                                               const uint8_t* __restrict__ blur, long long pimg,
                                                               long long bimg, const LevelGeom* __restrict__ levels,
                                                               int nlevels, const uint2* __restrict__ oct_out,
                                                               int oct_cap, const int* __restrict__ oct_count,
                                                               orbmi_keypoint* __restrict__ kps,
                                                               uint8_t* __restrict__ desc, int* __restrict__ counts,
                                                               int capacity, int out_cap, int nimg) {
    __shared__ float4 spat[256];
    __shared__ uint4 sic[4][kIcItems];
    __shared__ DescLevel slv[kMaxLevels];
    __shared__ int spre[kMaxLevels], scnt[kMaxLevels];
    __shared__ __attribute__((aligned(16))) uint8_t swin[kDescKpWG][kBW * kBP];
    // the gx workgroups of an image share an XCD (xcd_image_map)
    int w, b;
    if (!xcd_image_map(nimg, w, b)) return;
    const int gx = (int)gridDim.x / (nimg >= 8 ? 8 * ((nimg + 7) / 8) : nimg);
    const int tid = threadIdx.x, wid = tid >> 6, lane = tid & 63, grp = lane >> 4, l = lane & 15;
    spat[tid] = c_pattern_f[tid];
    for (int i = tid; i < 4 * kIcItems; i += 64 * kDescWaves) (&sic[0][0])[i] = (&c_ictab[0][0])[i];
    const int* lc = oct_count + b * nlevels;
    if (tid < nlevels) {
        const LevelGeom& g = levels[tid];
        slv[tid] = DescLevel{g.off, g.boff, g.stride, g.bstride, g.out_base, g.scale, g.size};
        int pre = 0;
        for (int q = 0; q < tid; q++) pre += lc[q];
        spre[tid] = pre;
        scnt[tid] = lc[tid];
        if (w == 0 && tid == nlevels - 1) counts[b] = pre + lc[tid];
    }
    __syncthreads();
    uint8_t* W = swin[wid * kDescGroups + grp];
    const int nchunks = (out_cap + kDescKpWG - 1) / kDescKpWG;
    for (int ch = w; ch < nchunks; ch += gx) {
        const int j = ch * kDescKpWG + wid * kDescGroups + grp;
        int level = -1;
        for (int q = 0; q < nlevels; q++)
            if (j >= levels[q].out_base && j < levels[q].out_base + levels[q].out_cap) level = q;
        const int lv = level < 0 ? 0 : level;
        const DescLevel G = slv[lv];
        const int idx = j - G.out_base;
        const bool valid = level >= 0 && idx < scnt[lv];
        if (__ballot(valid) == 0) continue;  // wave-uniform
        int x = 0, y = 0;
        unsigned resp = 0;
        if (valid) {
            const uint2 o = oct_out[(long long)b * oct_cap + j];
            x = o.x & 0xFFFF;
            y = o.x >> 16;
            resp = o.y;
        }
        // the blurred window, rows of kBP bytes from its 8-B aligned start: lanes 0..11 of the
        // group load 8-B column q = l % 6 of rows 2k + l / 6 (byte offsets inside the image's planes)
        const uint8_t* bimgp = blur + (long long)b * bimg;
        const uint8_t* pimgp = pyr + (long long)b * pimg;
        const unsigned sb = (unsigned)G.boff + (unsigned)((y - kBR) * G.bstride + x - kBR);
        const int ob = (int)(sb & 7);
        if (valid && l < 2 * kBQ) {
            const int par = l >= kBQ ? 1 : 0, q = l - par * kBQ;
            const unsigned go = sb - ob + 8 * q + par * G.bstride;
            uint8_t* wd = W + 8 * q + kBP * par;
            constexpr int kPairs = (kBW + 1) / 2;
            uint2 v[kPairs];
#pragma unroll
            for (int k = 0; k < kPairs; k++)
                v[k] = (2 * k + par < kBW) ? *reinterpret_cast<const uint2*>(bimgp + go + 2 * k * G.bstride)
                                           : make_uint2(0u, 0u);
#pragma unroll
            for (int k = 0; k < kPairs; k++)
                if (2 * k + par < kBW) *reinterpret_cast<uint2*>(wd + 2 * kBP * k) = v[k];
        }
        // IC_Angle: the patch's dwords from the padded level, weighted by c_ictab[ou]
        unsigned s_u = 0, s_v = 0, s_1 = 0;
        if (valid) {
            const unsigned su = (unsigned)G.off + (unsigned)((kEdge + y - kUR) * G.stride + kEdge + x - kUR);
            const int ou = (int)(su & 3);
            const unsigned sua = su - ou;
            unsigned val[kIcItems / 16];
            uint4 it[kIcItems / 16];
#pragma unroll
            for (int k = 0; k < kIcItems / 16; k++) {
                it[k] = sic[ou][l + 16 * k];
                val[k] = *reinterpret_cast<const unsigned*>(pimgp + (sua + __umul24(it[k].z, G.stride) + it[k].w));
            }
#pragma unroll
            for (int k = 0; k < kIcItems / 16; k++) {
                s_u = __builtin_amdgcn_udot4(val[k], it[k].x, s_u, false);
                s_1 = __builtin_amdgcn_udot4(val[k], it[k].y, s_1, false);
                // (v + 16) on the circle bytes: a packed 16-bit multiply (__umul24 would drop the top byte)
                const u16x2 wv = __builtin_bit_cast(u16x2, it[k].y) * (unsigned short)(it[k].z + 1);
                s_v = __builtin_amdgcn_udot4(val[k], __builtin_bit_cast(unsigned, wv), s_v, false);
            }
        }
        s_u = row16_sum(s_u);
        s_v = row16_sum(s_v);
        s_1 = row16_sum(s_1);
        const int m10 = (int)s_u - 16 * (int)s_1, m01 = (int)s_v - 16 * (int)s_1;
        const float angle = fast_atan2_deg((float)m01, (float)m10);
        const float ang = angle * (float)(3.14159265358979323846 / 180.0);
        double sd, cd;
        orbmi_sincos_f64((double)ang, &sd, &cd);
        const float ca = valid ? (float)cd : 1.f, sa = valid ? (float)sd : 0.f;
        // the window stores of this wave visible to its reads
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_s_waitcnt(0xc07f);
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // rBRIEF: window (kBR + r, kBR + c) at W[ob + (kBR + r) kBP + kBR + c]; with r, c as the low
        // bits of (value + 1.5 * 2^23) the constant part folds into kadd (uint32 wrap-around)
        const float kMagic = 12582912.0f;
        const unsigned kadd = (unsigned)(ob + kBR * kBP + kBR) - 0x400000u * (unsigned)kBP - 0x4B400000u;
        unsigned word = 0;
#pragma unroll
        for (int k = 15; k >= 0; k--) {
            const float4 P = spat[16 * k + l];  // pair 16 l + k (k-major: one iteration reads 256 contiguous bytes)
            const f32x2 px = {P.x, P.y}, py = {P.z, P.w};
            const f32x2 cx = (px * ca - py * sa) + kMagic;
            const f32x2 ry = (px * sa + py * ca) + kMagic;
            const unsigned i0 = __umul24(__float_as_uint(ry.x), (unsigned)kBP) + __float_as_uint(cx.x) + kadd;
            const unsigned i1 = __umul24(__float_as_uint(ry.y), (unsigned)kBP) + __float_as_uint(cx.y) + kadd;
            word = 2 * word + (W[i0] < W[i1] ? 1u : 0u);
        }
        if (valid && spre[lv] + idx < capacity) {
            const long long oi = (long long)b * capacity + spre[lv] + idx;
            reinterpret_cast<unsigned short*>(desc + oi * 32)[l] = (unsigned short)word;
            if (l == 0) {
                orbmi_keypoint kp;
                kp.x = level == 0 ? (float)x : (float)x * G.scale;
                kp.y = level == 0 ? (float)y : (float)y * G.scale;
                kp.size = G.size;
                kp.angle = angle;
                kp.response = (float)resp;
                kp.octave = level;
                kp.class_id = -1;
                kps[oi] = kp;
            }
        }
    }
}

// ------------------------------------------------------------------------------ host
static_assert(sizeof(BlurTile) == sizeof(int2) && alignof(BlurTile) <= alignof(int2) && offsetof(BlurTile, xy) == offsetof(int2, y),
              "k_blur reads the plan's blur tiles as int2");
static_assert(sizeof(DescribeTables::pattern) == sizeof(float4[256]) && sizeof(DescribeTables::ic) == sizeof(uint4[4][kIcItems]),
              "k_describe4 reads the describe tables as float4 / uint4");

int Extractor::init(int dev, int nf, float sf, int nl, int ini, int mn) {
    if (nf < 0 || nl < 1 || nl > kMaxLevels || !(sf > 1.0f)) return ORBMI_E_ARG;
    device = dev; ini_th = ini; min_th = mn;
    ORBMI_HIP(hipSetDevice(device));
    ORBMI_HIP(orbmi::stream_create(&stream, "EXTRACTOR"));
    tab = orb_tables(nf, sf, nl);
    DescribeTables dt;
    const int rc = describe_tables(tab.umax, ORBMI_PATTERN, &dt);
    if (rc) return rc;
    ORBMI_HIP(hipMemcpyToSymbol(HIP_SYMBOL(c_pattern_f), dt.pattern, sizeof(dt.pattern)));
    ORBMI_HIP(hipMemcpyToSymbol(HIP_SYMBOL(c_ictab), dt.ic, sizeof(dt.ic)));
    const char* e = getenv("ORBMI_BLUR");
    blur_mode = !e ? -1 : !strcmp(e, "side") ? 0 : !strcmp(e, "fused") ? 1 : !strcmp(e, "serial") ? 2 : -1;
    std::vector<float> st(tab.scale);
    st.insert(st.end(), tab.inv_scale.begin(), tab.inv_scale.end());
    ORBMI_HIP(hipMalloc((void**)&d_scale_tab, st.size() * sizeof(float)));
    ORBMI_HIP(hipMemcpy(d_scale_tab, st.data(), st.size() * sizeof(float), hipMemcpyHostToDevice));
    return ORBMI_OK;
}

// The device mirrors of a plan's tables: set_geometry fills them from this list, release frees them.
std::array<Extractor::GeomTable, 7> Extractor::geom_tables(const ExtractorPlan& p) {
    auto tb = [](auto** d, const auto& v) { return GeomTable{(void**)d, v.data(), v.size() * sizeof(v[0])}; };
    return {tb(&d_levels, p.levels), tb(&d_cells, p.cells), tb(&d_regbase, p.regbase), tb(&d_pyr_blob, p.blob),
            tb(&d_btiles, p.btiles), tb(&d_xtab, p.xtab), tb(&d_ytab, p.ytab)};
}

// The handle either describes one geometry completely -- rows, cols, plan and the device tables
// agree -- or is marked as having none.  A refused size leaves it as it was (the plan is built
// into a local); once the tables of the next size start replacing the old ones the handle is
// marked, and it takes the next geometry only after the last upload.
int Extractor::set_geometry(int r, int c) {
    if (r == rows && c == cols && !plan.levels.empty()) return ORBMI_OK;
    ORBMI_HIP(hipSetDevice(device));
    ExtractorPlan next;
    const int rc = extractor_plan(tab, r, c, &next);
    if (rc) return rc;
    rows = cols = 0;
    plan = ExtractorPlan{};
    bcap = 0;  // the per-image buffers are sized by the plan: reserve() makes them again
    out_capacity = 0;
    last_batch = 0;  // the last outputs were the old geometry's
    for (const GeomTable& t : geom_tables(next)) {
        if (*t.dev) { (void)hipFree(*t.dev); *t.dev = nullptr; }
        ORBMI_HIP(hipMalloc(t.dev, t.bytes ? t.bytes : 1));
        if (t.bytes) ORBMI_HIP(hipMemcpy(*t.dev, t.host, t.bytes, hipMemcpyHostToDevice));
    }
    plan = std::move(next);
    rows = r; cols = c;
    return ORBMI_OK;
}

// Per-image buffers for `batch` images and internal outputs of `capacity` keypoints each.  The
// buffers of a group share one capacity (bcap, out_capacity), which is 0 while they are made again:
// a failure part-way leaves it 0, and the next call starts over.
int Extractor::reserve(int batch, int capacity) {
    int rc;
    auto regrow = [](auto** p, size_t n) { size_t cap = 0; return ensure_buf(p, &cap, n); };
    const int nlevels = tab.nlevels;
    if (batch > bcap) {
        bcap = 0;
        out_capacity = 0;  // internal outputs are sized per bcap: re-reserve below
        last_batch = 0;
        if ((rc = regrow(&d_pyr, (size_t)batch * plan.pimg))) return rc;
        if ((rc = regrow(&d_blur, (size_t)batch * plan.bimg))) return rc;
        if ((rc = regrow(&d_level_count, (size_t)batch * nlevels * kFastRegions))) return rc;
        if ((rc = regrow(&d_cand, (size_t)batch * plan.keys_cap))) return rc;
        if ((rc = regrow(&d_node_of, (size_t)batch * plan.keys_cap))) return rc;
        if ((rc = regrow(&d_oct, (size_t)batch * plan.out_cap))) return rc;
        if ((rc = regrow(&d_oct_count, (size_t)batch * nlevels))) return rc;
        if ((rc = regrow(&d_counts, (size_t)batch))) return rc;
        bcap = batch;
    }
    if (capacity > out_capacity) {  // internal outputs (host API): bcap images x capacity
        out_capacity = 0;
        last_batch = 0;
        if ((rc = regrow(&d_kps, (size_t)bcap * capacity))) return rc;
        if ((rc = regrow(&d_desc, (size_t)bcap * capacity * 32))) return rc;
        out_capacity = capacity;
    }
    return ORBMI_OK;
}

// The side stream and its events, created on first use: only the large batches that put the
// blur on a side stream need them, and an idle stream per extractor would otherwise count
// against the process's hardware queues (GPU_MAX_HW_QUEUES) for nothing.
int Extractor::ensure_side_stream() {
    if (bstream) return ORBMI_OK;
    ORBMI_HIP(orbmi::stream_create(&bstream, "EXTRACTOR"));
    ORBMI_HIP(hipEventCreateWithFlags(&ev_pyr, hipEventDisableTiming));
    ORBMI_HIP(hipEventCreateWithFlags(&ev_blur, hipEventDisableTiming));
    return ORBMI_OK;
}

int Extractor::run(const uint8_t* d_images, int batch, size_t step, size_t image_stride,
                   orbmi_keypoint* kps, uint8_t* desc, int* counts, int capacity) {
    ORBMI_HIP(hipSetDevice(device));
    const std::vector<LevelGeom>& levels = plan.levels;
    const int nlevels = tab.nlevels, ncells = (int)plan.cells.size(), nbtiles = (int)plan.btiles.size();
    const int fast_maxw = plan.fast_maxw, fast_maxh = plan.fast_maxh, keys_cap = plan.keys_cap, out_cap = plan.out_cap;
    const long long pimg = plan.pimg, bimg = plan.bimg;
    // GaussianBlur needs only the pyramid.  Small batches (<= kFuseBlurMaxOctrees octrees): it rides
    // in the octree launch as extra workgroups on the CUs the octrees leave idle (a side stream's
    // event round trip costs more there: 7.8k vs 6.9k stereo frames/s).  Large batches: it runs on
    // a side stream (bstream) beside FAST and the octrees, and the describe waits for it (88.3k
    // vs 84.9k frames/s at config 5).  ORBMI_BLUR=side|fused|serial overrides.
    const int blur_mode = this->blur_mode >= 0 ? this->blur_mode : batch * nlevels <= kFuseBlurMaxOctrees ? 1 : 0;
    if (blur_mode == 0) {
        const int rc = ensure_side_stream();
        if (rc) return rc;
    }
    // ---- pyramid
    if (batch > kPyrTiledMaxBatch) {
        for (int l = 0; l < nlevels; l++) {
            const LevelGeom& g = levels[l];
            dim3 grid((g.ph + kPyrBRows - 1) / kPyrBRows, 1, batch);
            hipEvent_t ev = prof_begin(l == 0 ? ORBMI_STAGE_PYR_LEVEL0 : ORBMI_STAGE_PYR_RESIZE);
            if (l == 0) {
                const int lrow = (g.W + 3 + 3 + 15) & ~15;  // an image row from its aligned start
                hipLaunchKernelGGL(k_pyr_level0, grid, dim3(kPyrBThreads), kPyrBRows * lrow, stream, d_images, step,
                                   image_stride, d_pyr, pimg, g, d_level_count, nlevels, lrow);
            } else {
                const int lrow = levels[l - 1].stride;  // a padded source row (64-B multiple)
                hipLaunchKernelGGL(k_pyr_resize, grid, dim3(kPyrBThreads), 2 * kPyrBRows * lrow + 8 * g.W, stream, d_pyr, pimg,
                                   levels[l - 1], g, d_xtab + g.xtab_off, d_ytab + g.ytab_off, lrow);
            }
            prof_end(l == 0 ? ORBMI_STAGE_PYR_LEVEL0 : ORBMI_STAGE_PYR_RESIZE, ev);
        }
    } else {
        hipEvent_t ev = prof_begin(ORBMI_STAGE_PYR_LEVEL0);  // the whole pyramid
        hipLaunchKernelGGL(k_pyramid, dim3(plan.kx * plan.ky, 1, batch), dim3(kPyrThreads),
                           4 * plan.blob_words + plan.lds0 + 2 * plan.lds_half, stream, d_images, step, image_stride, d_pyr,
                           pimg, d_pyr_blob, plan.blob_words, nlevels, plan.kx, plan.ky, levels[0].W, levels[0].H, plan.hx,
                           plan.hy, d_level_count, plan.lds0, plan.lds_half);
        prof_end(ORBMI_STAGE_PYR_LEVEL0, ev);
    }
    if (blur_mode == 0) {  // side: the blur on the side stream from this point of the stream
        ORBMI_HIP(hipEventRecord(ev_pyr, stream));
        ORBMI_HIP(hipStreamWaitEvent(bstream, ev_pyr, 0));
        hipEvent_t eb = prof_begin(ORBMI_STAGE_BLUR, bstream);
        hipLaunchKernelGGL(k_blur, dim3(xcd_image_grid(nbtiles, batch)), dim3(256), 0, bstream, d_pyr, d_blur, pimg, bimg,
                           d_levels, d_btiles, batch);
        prof_end(ORBMI_STAGE_BLUR, eb, bstream);
        ORBMI_HIP(hipEventRecord(ev_blur, bstream));
    }
    // ---- FAST
    hipEvent_t ev = prof_begin(ORBMI_STAGE_FAST);
    {
        const bool narrow = fast_maxw + 3 <= 48;
        const size_t lds = kFastCells * fast2_wave_bytes(narrow ? 48 : 80, fast_maxw, fast_maxh);
        auto* kf = narrow ? k_fast2<48> : k_fast2<80>;
        hipLaunchKernelGGL(kf, dim3(xcd_image_grid((ncells + kFastCells - 1) / kFastCells, batch)), dim3(64 * kFastCells), lds,
                           stream, d_pyr, pimg, d_cells, 0, ncells, d_cand, keys_cap, d_level_count, nlevels, ini_th, min_th,
                           fast_maxw, fast_maxh, batch);
    }
    prof_end(ORBMI_STAGE_FAST, ev);
    // ---- octree (+ the fused blur)
    ev = prof_begin(ORBMI_STAGE_OCTREE);
    const bool fused = blur_mode == 1;
    const int blur_blocks = fused ? (nbtiles * batch + 3) / 4 : 0;
    hipLaunchKernelGGL(k_octree, dim3(nlevels * 8 * ((batch + 7) / 8) + blur_blocks), dim3(kOctThreads), 0, stream,
                       d_levels, nlevels,
                       d_cand, d_level_count, d_regbase, d_node_of, keys_cap, d_oct, out_cap, d_oct_count, d_pyr, d_blur,
                       pimg, bimg, d_btiles, fused ? nbtiles : 0, batch);
    prof_end(ORBMI_STAGE_OCTREE, ev);
    if (blur_mode == 2) {  // serial
        ev = prof_begin(ORBMI_STAGE_BLUR);
        hipLaunchKernelGGL(k_blur, dim3(xcd_image_grid(nbtiles, batch)), dim3(256), 0, stream, d_pyr, d_blur, pimg, bimg,
                           d_levels, d_btiles, batch);
        prof_end(ORBMI_STAGE_BLUR, ev);
    }
    // ---- describe
    if (blur_mode == 0) ORBMI_HIP(hipStreamWaitEvent(stream, ev_blur, 0));
    ev = prof_begin(ORBMI_STAGE_DESCRIBE);
    {
        const int nch = (out_cap + kDescKpWG - 1) / kDescKpWG;
        const int gx = std::max(1, std::min(nch, (kDescTargetWG + batch - 1) / batch));
        hipLaunchKernelGGL(k_describe4, dim3(xcd_image_grid(gx, batch)), dim3(64 * kDescWaves),
                           0, stream, d_pyr, d_blur,
                           pimg, bimg, d_levels, nlevels, d_oct, out_cap, d_oct_count, kps, desc, counts, capacity,
                           out_cap, batch);
    }
    prof_end(ORBMI_STAGE_DESCRIBE, ev);
    ORBMI_HIP(hipGetLastError());
    last_batch = batch;
    last_kps = kps; last_desc = desc; last_counts = counts; last_capacity = capacity;
    return ORBMI_OK;
}

hipEvent_t Extractor::prof_event() {
    hipEvent_t e = nullptr;
    if (!prof_pool.empty()) { e = prof_pool.back(); prof_pool.pop_back(); return e; }
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}

hipEvent_t Extractor::prof_begin(int stage, hipStream_t s) {
    if (!(prof_mask >> stage & 1u)) return nullptr;
    hipEvent_t a = prof_event();
    if (a) (void)hipEventRecord(a, s ? s : stream);
    return a;
}

void Extractor::prof_end(int stage, hipEvent_t a, hipStream_t s) {
    if (!a) return;
    hipEvent_t b = prof_event();
    if (!b) return;
    (void)hipEventRecord(b, s ? s : stream);
    prof_pending.push_back(ProfPair{stage, a, b});
}

// ---- host images into HBM (orbmi_extract_batch_host) -------------------------------------------
// The image bytes are read straight from pinned host memory by a copy kernel on the handle's
// stream: the host never waits (hipMemcpyAsync from host memory measured as waiting for the
// stream's earlier work, which serialised the host with the extraction it had queued).  16-B
// loads, 4 in flight per lane before the stores (PCIe read latency); bytewise when unaligned.
__global__ __launch_bounds__(256) void k_copy_host(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                   size_t n) {
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (size_t)gridDim.x * blockDim.x;
    if ((((uintptr_t)src | (uintptr_t)dst) & 15) == 0) {
        const uint4* s4 = (const uint4*)src;
        uint4* d4 = (uint4*)dst;
        const size_t n16 = n >> 4;
        size_t i = tid;
        for (; i + 3 * nth < n16; i += 4 * nth) {
            const uint4 a = s4[i], b = s4[i + nth],
                        c = s4[i + 2 * nth], d = s4[i + 3 * nth];
            d4[i] = a;
            d4[i + nth] = b;
            d4[i + 2 * nth] = c;
            d4[i + 3 * nth] = d;
        }
        for (; i < n16; i += nth) d4[i] = s4[i];
        for (size_t j = (n16 << 4) + tid; j < n; j += nth) dst[j] = src[j];
    } else {
        for (size_t j = tid; j < n; j += nth) dst[j] = src[j];
    }
}

int Extractor::upload_host(const uint8_t* h_images, size_t bytes, const uint8_t** d_out) {
    const int rc = ensure_buf(&d_image, &image_bytes, bytes);
    if (rc) return rc;
    hipPointerAttribute_t at;
    bool pinned = false;
    if (hipPointerGetAttributes(&at, h_images) == hipSuccess) pinned = at.type == hipMemoryTypeHost;
    else (void)hipGetLastError();
    const uint8_t* src = h_images;
    hipEvent_t staged = nullptr;
    if (!pinned) {  // pageable: one host copy into a pinned staging buffer of the handle (two, alternating)
        const int k = stage_next;
        stage_next ^= 1;
        if (bytes > stage_bytes[k]) {
            if (stage_ev[k]) ORBMI_HIP(hipEventSynchronize(stage_ev[k]));
            if (h_stage[k]) (void)hipHostFree(h_stage[k]);
            h_stage[k] = nullptr;
            stage_bytes[k] = 0;
            ORBMI_HIP(hipHostMalloc((void**)&h_stage[k], bytes, hipHostMallocDefault));
            stage_bytes[k] = bytes;
        }
        if (!stage_ev[k]) ORBMI_HIP(hipEventCreateWithFlags(&stage_ev[k], hipEventDisableTiming));
        else ORBMI_HIP(hipEventSynchronize(stage_ev[k]));  // its last copy kernel has read it
        std::memcpy(h_stage[k], h_images, bytes);
        src = h_stage[k];
        staged = stage_ev[k];
    }
    const int blocks = (int)std::min<size_t>(1024, (bytes / 16 + 255) / 256 + 1);
    hipLaunchKernelGGL(k_copy_host, dim3(blocks), dim3(256), 0, stream, src, d_image, bytes);
    ORBMI_HIP(hipGetLastError());
    if (staged) ORBMI_HIP(hipEventRecord(staged, stream));  // the staging buffer is free again after the copy
    *d_out = d_image;
    return ORBMI_OK;
}

void Extractor::release() {
    for (int k = 0; k < 2; k++) {
        if (stage_ev[k]) { (void)hipEventSynchronize(stage_ev[k]); (void)hipEventDestroy(stage_ev[k]); }
        if (h_stage[k]) (void)hipHostFree(h_stage[k]);
        stage_ev[k] = nullptr;
        h_stage[k] = nullptr;
        stage_bytes[k] = 0;
    }
    for (auto& p : prof_pending) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
    for (auto e : prof_pool) (void)hipEventDestroy(e);
    prof_pending.clear();
    prof_pool.clear();
    if (device >= 0) (void)hipSetDevice(device);
    for (const GeomTable& t : geom_tables(plan))
        if (*t.dev) (void)hipFree(*t.dev);
    void* ptrs[] = {d_blur, d_pyr, d_level_count, d_cand, d_node_of, d_oct, d_oct_count, d_kps, d_desc, d_counts,
                    d_image, d_scale_tab, d_row_start, d_row_list, d_sad, d_stereo_u, d_stereo_d};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    if (stream) (void)hipStreamDestroy(stream);
    stream = nullptr;
    if (bstream) (void)hipStreamDestroy(bstream);
    bstream = nullptr;
    if (ev_pyr) (void)hipEventDestroy(ev_pyr);
    if (ev_blur) (void)hipEventDestroy(ev_blur);
    ev_pyr = ev_blur = nullptr;
}

}  // namespace orbmi
