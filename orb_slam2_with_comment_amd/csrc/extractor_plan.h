// The host plan of the device ORB extractor (extractor.hip): everything that follows from the
// extractor's parameters and the image size alone, as the kernels read it.  HIP-free
// (include/orbmi.h and the standard library only), so a plain C++ program builds it and runs the
// pyramid's tile plan on the CPU with the kernel's own arithmetic: tests/cpp/extractor_plan_check.cpp.
//   orb_tables       ORBextractor::ORBextractor's tables (src/ORBextractor.cc:410-470)
//   describe_tables  k_describe4's pattern and IC_Angle tables
//   extractor_plan   one image size: level geometry, the FAST cell grid of ComputeKeyPointsOctTree
//                    (:778-829) with its candidate regions, DistributeOctTree's capacities
//                    (:539-560), cv::resize's taps, k_pyramid's tiles, the blur tiles
// The structs the kernels read are laid out as the kernels read them; extractor.hip uploads them
// as they stand.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <utility>
#include <vector>

#include "../../include/orbmi.h"

#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif

namespace orbmi {

constexpr int kEdge = 19;        // EDGE_THRESHOLD  src/ORBextractor.cc:74
constexpr int kHalfPatch = 15;   // HALF_PATCH_SIZE src/ORBextractor.cc:73
constexpr int kPatch = 31;       // PATCH_SIZE      src/ORBextractor.cc:72
constexpr int kMaxLevels = 16;

__host__ __device__ inline int reflect101(int p, int len) {
    if ((unsigned)p < (unsigned)len) return p;
    if (len == 1) return 0;
    do {
        if (p < 0) p = -p;
        else p = 2 * len - 2 - p;
    } while ((unsigned)p >= (unsigned)len);
    return p;
}

__host__ __device__ inline int cv_floor_f(float v) { int i = (int)v; return i - (i > v); }

// cvRound(float): round-half-even (v_rndne_f32 on device, rint under the default mode on host)
__host__ __device__ inline int cv_round_f(float v) { return (int)__builtin_rintf(v); }

// Per pyramid level constants, resident in device memory (one copy per handle geometry).
struct LevelGeom {
    int W, H;            // interior size  (ComputePyramid :1111-1112)
    int stride, ph;      // padded row pitch (>= W+38, 64-aligned) and padded height H+38
    long long off;       // byte offset of the padded level inside one image's pyramid
    int cell_begin, cell_end;   // FAST cell range (global cell index)
    int nfeat;           // mnFeaturesPerLevel[level]
    int out_base, out_cap;      // octree output slots (per image)
    int key_base, key_cap;      // candidate scratch (per image)
    int width, height;   // octree area maxBorderX-minBorderX, maxBorderY-minBorderY
    int nIni;            // DistributeOctTree initial node count
    float hX;            // (float)width / nIni
    float scale;         // mvScaleFactor[level]
    float size;          // (float)(int)(PATCH_SIZE * scale)
    int blur_xv;         // first column of the GaussianBlur scalar tail (4*floor(W/4))
    int resize_xv;       // first column of the resize vertical scalar tail
    int xtab_off, ytab_off;     // offsets into the resize coefficient tables (level >= 1)
    long long boff;      // byte offset of the blurred level (interior only) inside one image's blur
    int bstride;         // blurred row pitch (W rounded up to 128)
};

// One FAST cell of ComputeKeyPointsOctTree (src/ORBextractor.cc:789-829).
struct CellGeom {
    short x0, y0, w, h;  // ROI in interior coordinates; w == 0 -> skipped cell
    short sx, sy;        // j*wCell, i*hCell shift added to ROI coordinates
    int slot_base;       // base of the cell's candidate region (per image; cells of one level
                         // share kFastRegions regions, cell k of the level writes region k % R)
    int level;
    long long roi_off;   // byte offset of the ROI's first pixel in one image's pyramid (level plane,
                         // border, stride folded in: k_fast2 needs no LevelGeom load)
    int stride;          // the level's row stride
    int lcell;           // index of the cell within its level
};

struct XTab { short sx0, sx1, a0, a1; };  // horizontal resize: source taps and 11-bit weights
struct YTab { short y0, y1, b0, b1; };    // vertical resize
struct PyrRect { short x0, x1, y0, y1; };  // half-open interior rectangle of one level
struct PyrTile { PyrRect own, need; };     // k_pyramid tile of one level: written to HBM / computed in LDS
struct BlurTile { int level, xy; };        // GaussianBlur tile {level, x0 | y0 << 16}: the device's int2

constexpr int kOctNodeCap = 2048;  // live quadtree nodes per level held in LDS
constexpr int kFastRegions = 16;   // candidate regions per level (spreads k_fast2's allocation atomics)
constexpr int kTile = 64;          // max cell ROI edge (wCell+6, hCell+6): it fits k_fast2<80>'s tile
constexpr int kBlurTW = 128, kBlurTH = 32;  // GaussianBlur output tile
constexpr int kIcItems = 224;      // k_describe4's IC dwords per phase (<= 213 used): 14 per lane

// A k_pyramid tile's parameter block: kPyrLevelWords words per level, then the resize taps of the
// tile's need rectangles (2 words per column, 2 per row), at the word offsets the level names.
enum PyrWord {
    kPyrOwnX = 0,     // own rectangle x0 | x1 << 16
    kPyrOwnY,         // y0 | y1 << 16
    kPyrNeedX,        // need rectangle x0 | x1 << 16
    kPyrNeedY,        // y0 | y1 << 16
    kPyrWH,           // W | H << 16
    kPyrStride,       // padded row pitch
    kPyrOff,          // byte offset of the padded level
    kPyrResizeXv,     // LevelGeom::resize_xv
    kPyrXTaps,        // word offset of the need rectangle's x taps (level >= 1)
    kPyrYTaps,        // word offset of its y taps
    kPyrLevelWords
};

// interior (x, y) of a padded level and every border pixel mirroring it (one reflection: W, H > kEdge)
__host__ __device__ inline void pyr_store(uint8_t* lvl, int W, int H, int stride, int x, int y, uint8_t v) {
    int xs[3], ys[3], nx = 0, ny = 0;
    xs[nx++] = x;
    if (x >= 1 && x <= kEdge) xs[nx++] = -x;
    if (x >= W - 1 - kEdge && x <= W - 2) xs[nx++] = 2 * W - 2 - x;
    ys[ny++] = y;
    if (y >= 1 && y <= kEdge) ys[ny++] = -y;
    if (y >= H - 1 - kEdge && y <= H - 2) ys[ny++] = 2 * H - 2 - y;
    for (int j = 0; j < ny; j++)
        for (int i = 0; i < nx; i++) lvl[(long long)(ys[j] + kEdge) * stride + xs[i] + kEdge] = v;
}

// cv::resize INTER_LINEAR 8U of one pixel from its four taps (pinned P2: the SSE2 vertical pass
// for x < resize_xv, the scalar tail after it).
__host__ __device__ inline int pyr_resize_px(int p00, int p01, int p10, int p11, const XTab& x, const YTab& y, bool vec) {
    const int h0 = p00 * x.a0 + p01 * x.a1;
    const int h1 = p10 * x.a0 + p11 * x.a1;
    int v;
    if (vec)  // VResizeLinearVec_32s8u lanes
        v = ((((h0 >> 4) * y.b0) >> 16) + (((h1 >> 4) * y.b1) >> 16) + 2) >> 2;
    else
        v = (h0 * y.b0 + h1 * y.b1 + (1 << 21)) >> 22;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// ---- ORBextractor::ORBextractor  src/ORBextractor.cc:410-470 (same float/double steps)
struct OrbTables {
    int nfeatures = 0, nlevels = 0;
    float scale_factor = 0.f;
    std::vector<float> scale, inv_scale, sigma2, inv_sigma2;
    std::vector<int> nfeat, umax;
};

inline OrbTables orb_tables(int nf, float sf, int nl) {
    OrbTables t;
    t.nfeatures = nf; t.scale_factor = sf; t.nlevels = nl;
    t.scale.assign(nl, 1.f); t.sigma2.assign(nl, 1.f); t.inv_scale.resize(nl); t.inv_sigma2.resize(nl);
    const double sfd = (double)sf;
    for (int i = 1; i < nl; i++) {
        t.scale[i] = (float)((double)t.scale[i - 1] * sfd);
        t.sigma2[i] = t.scale[i] * t.scale[i];
    }
    for (int i = 0; i < nl; i++) { t.inv_scale[i] = 1.0f / t.scale[i]; t.inv_sigma2[i] = 1.0f / t.sigma2[i]; }
    t.nfeat.resize(nl);
    const float factor = (float)(1.0f / sfd);
    float ndes = (float)nf * (1 - factor) / (1 - (float)pow((double)factor, (double)nl));
    int sum = 0;
    for (int l = 0; l < nl - 1; l++) { t.nfeat[l] = cv_round_f(ndes); sum += t.nfeat[l]; ndes *= factor; }
    t.nfeat[nl - 1] = std::max(nf - sum, 0);
    t.umax.assign(kHalfPatch + 1, 0);
    const int vmax = cv_floor_f(kHalfPatch * sqrtf(2.f) / 2 + 1);
    const int vmin = (int)ceilf(kHalfPatch * sqrtf(2.f) / 2);
    const double hp2 = kHalfPatch * kHalfPatch;
    for (int v = 0; v <= vmax; ++v) t.umax[v] = (int)lrint(sqrt(hp2 - v * v));
    for (int v = kHalfPatch, v0 = 0; v >= vmin; --v) {
        while (t.umax[v0] == t.umax[v0 + 1]) ++v0;
        t.umax[v] = v0;
        ++v0;
    }
    return t;
}

// k_describe4's tables: the pattern as (x0, x1, y0, y1) floats, pair t = 16 l + k at 16 k + l (the
// device's float4), and per 4-B phase ou of the IC patch's first byte the dwords covering each
// circle row, {u + 16 byte weights, byte mask, window row, 4 * dword} (the device's uint4).
struct DescribeTables {
    float pattern[256][4];
    uint32_t ic[4][kIcItems][4];
    int ic_items[4];  // entries used per phase
};

// pattern: the 256 rBRIEF pairs (x0, y0, x1, y1).  ORBMI_E_ARG when a phase needs more than kIcItems.
inline int describe_tables(const std::vector<int>& umax, const signed char (*pattern)[4], DescribeTables* out) {
    for (int t = 0; t < 256; t++) {
        float* f = out->pattern[16 * (t & 15) + (t >> 4)];
        f[0] = pattern[t][0]; f[1] = pattern[t][2]; f[2] = pattern[t][1]; f[3] = pattern[t][3];
    }
    memset(out->ic, 0, sizeof(out->ic));
    for (int ou = 0; ou < 4; ou++) {
        int n = 0;
        for (int v = -kHalfPatch; v <= kHalfPatch; v++) {
            const int d = umax[v < 0 ? -v : v], r = v + kHalfPatch;
            for (int dd = (ou + kHalfPatch - d) / 4; dd <= (ou + kHalfPatch + d) / 4; dd++) {
                if (n >= kIcItems) return ORBMI_E_ARG;
                unsigned wa = 0, wm = 0;
                for (int p = 0; p < 4; p++) {
                    const int u = 4 * dd + p - ou - kHalfPatch;
                    if (u >= -d && u <= d) { wa |= (unsigned)(u + 16) << (8 * p); wm |= 1u << (8 * p); }
                }
                uint32_t* e = out->ic[ou][n++];
                e[0] = wa; e[1] = wm; e[2] = (unsigned)r; e[3] = (unsigned)(4 * dd);
            }
        }
        out->ic_items[ou] = n;
    }
    return ORBMI_OK;
}

// ---- the geometry of one image size
struct ExtractorPlan {
    std::vector<LevelGeom> levels;  // empty: no geometry
    std::vector<CellGeom> cells;
    std::vector<int> regbase;       // [level][region] first slot of each candidate region (per image)
    std::vector<XTab> xtab;
    std::vector<YTab> ytab;
    std::vector<BlurTile> btiles;
    long long pimg = 0;             // bytes of one padded pyramid
    long long bimg = 0;             // bytes of one blurred pyramid
    int keys_cap = 0, out_cap = 0;  // candidate / octree output slots per image
    int fast_maxw = 0, fast_maxh = 0;  // largest cell ROI (k_fast2's LDS per wave)
    // k_pyramid: the tile grid, level 0's halo, the parameter blocks (blob_words per tile) and the
    // bytes of the level-0 rectangle and of one need rectangle in LDS
    int kx = 0, ky = 0, hx = 0, hy = 0, blob_words = 0, lds0 = 0, lds_half = 0;
    std::vector<uint32_t> blob;
};

// Level l's sizes and offsets, appended behind level l - 1's.  false: the level is too small for
// one 30-pixel cell inside its borders.
inline bool plan_level(const OrbTables& t, int rows, int cols, int l, ExtractorPlan& p) {
    LevelGeom& g = p.levels[l];
    g.W = cv_round_f((float)cols * t.inv_scale[l]);
    g.H = cv_round_f((float)rows * t.inv_scale[l]);
    const int minB = kEdge - 3, maxBX = g.W - kEdge + 3, maxBY = g.H - kEdge + 3;
    if (maxBX - minB < 30 || maxBY - minB < 30) return false;
    g.stride = (g.W + 2 * kEdge + 63) & ~63;
    g.ph = g.H + 2 * kEdge;
    g.off = p.pimg;
    p.pimg += (long long)g.stride * g.ph;
    g.bstride = (g.W + 127) & ~127;
    g.boff = p.bimg;
    p.bimg += (long long)g.bstride * g.H;
    g.scale = t.scale[l];
    g.size = (float)(int)(kPatch * t.scale[l]);
    g.blur_xv = (g.W / 4) * 4;
    int x = 0;  // where cv::resize's SIMD vertical pass ends
    while (x <= g.W - 16) x += 16;
    while (x < g.W - 4) x += 4;
    g.resize_xv = x;
    g.nfeat = t.nfeat[l];
    g.width = maxBX - minB;
    g.height = maxBY - minB;
    return true;
}

// Level l's FAST cells (src/ORBextractor.cc:778-829) and candidate regions: region j holds the
// cells k % R == j of the level, sized for their caps.  false: a cell wider than k_fast2's tile, or
// more candidates or cells than the order tags hold (cell index within the level (14 bits) << 10 |
// rank in the cell (< 1024)).
inline bool plan_cells(int l, ExtractorPlan& p) {
    LevelGeom& g = p.levels[l];
    const int minB = kEdge - 3, maxBX = minB + g.width, maxBY = minB + g.height;
    const float width = (float)g.width, height = (float)g.height;
    const int nCols = (int)(width / 30.f), nRows = (int)(height / 30.f);
    const int wCell = (int)ceilf(width / nCols), hCell = (int)ceilf(height / nRows);
    if (wCell + 6 > kTile || hCell + 6 > kTile) return false;
    const int cap = ((wCell + 1) / 2) * ((hCell + 1) / 2);
    int key = p.keys_cap;
    g.cell_begin = (int)p.cells.size();
    g.key_base = key;
    for (int i = 0; i < nRows; i++) {
        const float iniY = (float)(minB + i * hCell);
        float maxY = iniY + hCell + 6;
        const bool skipY = iniY >= maxBY - 3;
        if (maxY > maxBY) maxY = (float)maxBY;
        for (int j = 0; j < nCols; j++) {
            const float iniX = (float)(minB + j * wCell);
            float maxX = iniX + wCell + 6;
            CellGeom cg{};
            cg.level = l;
            if (!skipY && !(iniX >= maxBX - 6)) {
                if (maxX > maxBX) maxX = (float)maxBX;
                cg.x0 = (short)(int)iniX; cg.y0 = (short)(int)iniY;
                cg.w = (short)((int)maxX - (int)iniX); cg.h = (short)((int)maxY - (int)iniY);
                cg.sx = (short)(j * wCell); cg.sy = (short)(i * hCell);
                key += cap;
            }
            cg.roi_off = g.off + (long long)(kEdge + cg.y0) * g.stride + kEdge + cg.x0;
            cg.stride = g.stride;
            cg.lcell = (int)p.cells.size() - g.cell_begin;
            p.cells.push_back(cg);
        }
    }
    g.cell_end = (int)p.cells.size();
    g.key_cap = key - g.key_base;
    p.keys_cap = key;
    int rcap[kFastRegions] = {0}, base = g.key_base;
    for (int k = 0; k < g.cell_end - g.cell_begin; k++)
        if (p.cells[g.cell_begin + k].w) rcap[k % kFastRegions] += cap;
    for (int j = 0; j < kFastRegions; j++) {
        p.regbase[l * kFastRegions + j] = base;
        base += rcap[j];
    }
    for (int k = 0; k < g.cell_end - g.cell_begin; k++)
        p.cells[g.cell_begin + k].slot_base = p.regbase[l * kFastRegions + k % kFastRegions];
    return !(g.key_cap > (1 << 20) || g.cell_end - g.cell_begin >= (1 << 14) || cap >= 1024);
}

// Level l's DistributeOctTree constants (src/ORBextractor.cc:539-560) and output slots.  false:
// no initial node (the reference indexes an empty vector there), or more nodes than k_octree holds.
inline bool plan_octree(int l, ExtractorPlan& p) {
    LevelGeom& g = p.levels[l];
    g.nIni = (int)roundf((float)g.width / (float)g.height);
    if (g.nIni < 1) return false;
    g.hX = (float)g.width / g.nIni;
    g.out_cap = std::max(g.nfeat + 3, 4 * g.nIni) + 1;
    if (g.out_cap > kOctNodeCap || 4 * g.nIni > kOctNodeCap) return false;
    g.out_base = p.out_cap;
    p.out_cap += g.out_cap;
    return true;
}

// Level l >= 1 from level l - 1: cv::resize INTER_LINEAR 8U coefficients
inline void plan_resize_taps(int l, ExtractorPlan& p) {
    LevelGeom& g = p.levels[l];
    const LevelGeom& s = p.levels[l - 1];
    g.xtab_off = (int)p.xtab.size();
    g.ytab_off = (int)p.ytab.size();
    const double scale_x = 1. / ((double)g.W / s.W), scale_y = 1. / ((double)g.H / s.H);
    auto w11 = [](float f) { return (short)std::min(std::max(cv_round_f(f * 2048), -32768), 32767); };
    int xmax = g.W;
    std::vector<int> sxs(g.W);
    std::vector<float> fxs(g.W);
    for (int dx = 0; dx < g.W; dx++) {
        float fx = (float)((dx + 0.5) * scale_x - 0.5);
        int sx = cv_floor_f(fx);
        fx -= sx;
        if (sx < 0) { fx = 0; sx = 0; }
        if (sx + 1 >= s.W) { xmax = std::min(xmax, dx); if (sx >= s.W - 1) { fx = 0; sx = s.W - 1; } }
        sxs[dx] = sx; fxs[dx] = fx;
    }
    for (int dx = 0; dx < g.W; dx++) {
        XTab e;
        e.sx0 = (short)sxs[dx];
        if (dx < xmax) { e.sx1 = (short)(sxs[dx] + 1); e.a0 = w11(1.f - fxs[dx]); e.a1 = w11(fxs[dx]); }
        else { e.sx1 = (short)sxs[dx]; e.a0 = 2048; e.a1 = 0; }
        p.xtab.push_back(e);
    }
    for (int dy = 0; dy < g.H; dy++) {
        float fy = (float)((dy + 0.5) * scale_y - 0.5);
        int sy = cv_floor_f(fy);
        fy -= sy;
        YTab e;
        e.b0 = w11(1.f - fy);
        e.b1 = w11(fy);
        e.y0 = (short)std::min(std::max(sy, 0), s.H - 1);
        e.y1 = (short)std::min(std::max(sy + 1, 0), s.H - 1);
        p.ytab.push_back(e);
    }
}

// k_pyramid's tiles: own rectangles split every level kx x ky ways; need rectangles from the top
// level down (need_{l-1} = own_{l-1} U the taps of need_l); level 0's need rectangle is the own
// one grown by the largest halo (hx, hy) of any tile.  The grid grows from 16 x 8 until a tile's
// LDS (parameter block, level-0 rectangle, two need rectangles) fits in 48 KB.  false: it does not
// fit in 64 KB at 4096 tiles.
inline bool plan_pyramid_tiles(ExtractorPlan& p) {
    const int nlevels = (int)p.levels.size();
    const LevelGeom& g0 = p.levels[0];
    for (int KX = 16, KY = 8;;) {
        std::vector<PyrTile> tl((size_t)KX * KY * nlevels);
        int maxarea = 0, hx = 0, hy = 0, words = 0;
        for (int ty = 0; ty < KY; ty++)
            for (int tx = 0; tx < KX; tx++) {
                PyrTile* T = &tl[((size_t)ty * KX + tx) * nlevels];
                for (int l = 0; l < nlevels; l++) {
                    const LevelGeom& g = p.levels[l];
                    T[l].own = PyrRect{(short)(g.W * tx / KX), (short)(g.W * (tx + 1) / KX), (short)(g.H * ty / KY),
                                       (short)(g.H * (ty + 1) / KY)};
                }
                T[nlevels - 1].need = T[nlevels - 1].own;
                for (int l = nlevels - 1; l >= 1; l--) {
                    const LevelGeom& g = p.levels[l];
                    PyrRect n = T[l].need, o = T[l - 1].own, r = o;
                    if (n.x1 > n.x0 && n.y1 > n.y0) {
                        const XTab* X = p.xtab.data() + g.xtab_off;
                        const YTab* Y = p.ytab.data() + g.ytab_off;
                        r.x0 = std::min<short>(o.x0, X[n.x0].sx0);
                        r.x1 = std::max<short>(o.x1, (short)(X[n.x1 - 1].sx1 + 1));
                        r.y0 = std::min<short>(o.y0, Y[n.y0].y0);
                        r.y1 = std::max<short>(o.y1, (short)(Y[n.y1 - 1].y1 + 1));
                    }
                    T[l - 1].need = r;
                }
                int w = kPyrLevelWords * nlevels;
                for (int l = 1; l < nlevels; l++) {
                    const PyrRect& n = T[l].need;
                    maxarea = std::max(maxarea, (n.x1 - n.x0) * (n.y1 - n.y0));
                    w += 2 * (n.x1 - n.x0) + 2 * (n.y1 - n.y0);
                }
                words = std::max(words, w);
                hx = std::max(hx, std::max(T[0].own.x0 - T[0].need.x0, T[0].need.x1 - T[0].own.x1));
                hy = std::max(hy, std::max(T[0].own.y0 - T[0].need.y0, T[0].need.y1 - T[0].own.y1));
            }
        int area0 = 0;
        for (int ty = 0; ty < KY; ty++)
            for (int tx = 0; tx < KX; tx++) {
                const int x0 = std::max(g0.W * tx / KX - hx, 0), x1 = std::min(g0.W * (tx + 1) / KX + hx, g0.W);
                const int y0 = std::max(g0.H * ty / KY - hy, 0), y1 = std::min(g0.H * (ty + 1) / KY + hy, g0.H);
                area0 = std::max(area0, (x1 - x0) * (y1 - y0));
            }
        const int half = (maxarea + 15) & ~15, a0 = (area0 + 15) & ~15;
        const int lds = 4 * words + a0 + 2 * half;
        if (lds > 48 * 1024 && KX * KY < 4096) {
            if (KX <= 2 * KY) KX *= 2;
            else KY *= 2;
            continue;
        }
        if (lds > 64 * 1024) return false;
        p.blob.assign((size_t)KX * KY * words, 0u);
        auto pk = [](int lo, int hi) { return (uint32_t)(uint16_t)lo | (uint32_t)(uint16_t)hi << 16; };
        for (int t = 0; t < KX * KY; t++) {
            const PyrTile* T = &tl[(size_t)t * nlevels];
            uint32_t* B = &p.blob[(size_t)t * words];
            int at = kPyrLevelWords * nlevels;
            for (int l = 0; l < nlevels; l++) {
                const LevelGeom& g = p.levels[l];
                uint32_t* G = B + l * kPyrLevelWords;
                G[kPyrOwnX] = pk(T[l].own.x0, T[l].own.x1);
                G[kPyrOwnY] = pk(T[l].own.y0, T[l].own.y1);
                G[kPyrNeedX] = pk(T[l].need.x0, T[l].need.x1);
                G[kPyrNeedY] = pk(T[l].need.y0, T[l].need.y1);
                G[kPyrWH] = pk(g.W, g.H);
                G[kPyrStride] = (uint32_t)g.stride;
                G[kPyrOff] = (uint32_t)g.off;
                G[kPyrResizeXv] = (uint32_t)g.resize_xv;
                if (l == 0) continue;
                const XTab* X = p.xtab.data() + g.xtab_off;
                const YTab* Y = p.ytab.data() + g.ytab_off;
                G[kPyrXTaps] = (uint32_t)at;
                for (int x = T[l].need.x0; x < T[l].need.x1; x++) {
                    B[at++] = pk(X[x].sx0, X[x].sx1);
                    B[at++] = pk(X[x].a0, X[x].a1);
                }
                G[kPyrYTaps] = (uint32_t)at;
                for (int y = T[l].need.y0; y < T[l].need.y1; y++) {
                    B[at++] = pk(Y[y].y0, Y[y].y1);
                    B[at++] = pk(Y[y].b0, Y[y].b1);
                }
            }
        }
        p.kx = KX; p.ky = KY; p.hx = hx; p.hy = hy;
        p.blob_words = words;
        p.lds_half = half;
        p.lds0 = a0;
        return true;
    }
}

inline void plan_blur_tiles(ExtractorPlan& p) {
    for (int l = 0; l < (int)p.levels.size(); l++)
        for (int y0 = 0; y0 < p.levels[l].H; y0 += kBlurTH)
            for (int x0 = 0; x0 < p.levels[l].W; x0 += kBlurTW) p.btiles.push_back(BlurTile{l, x0 | (y0 << 16)});
}

// The plan of a rows x cols image, or ORBMI_E_UNSUPPORTED for a size the kernels do not take;
// *out is written on success only.
inline int extractor_plan(const OrbTables& t, int rows, int cols, ExtractorPlan* out) {
    ExtractorPlan p;
    p.levels.assign(t.nlevels, LevelGeom{});
    p.regbase.assign((size_t)t.nlevels * kFastRegions, 0);
    for (int l = 0; l < t.nlevels; l++) {
        if (!plan_level(t, rows, cols, l, p) || !plan_cells(l, p) || !plan_octree(l, p)) return ORBMI_E_UNSUPPORTED;
        if (l > 0) plan_resize_taps(l, p);
    }
    if (!plan_pyramid_tiles(p)) return ORBMI_E_UNSUPPORTED;
    plan_blur_tiles(p);
    p.fast_maxw = 7; p.fast_maxh = 7;
    for (const CellGeom& cg : p.cells)
        if (cg.w) { p.fast_maxw = std::max(p.fast_maxw, (int)cg.w); p.fast_maxh = std::max(p.fast_maxh, (int)cg.h); }
    *out = std::move(p);
    return ORBMI_OK;
}

}  // namespace orbmi
