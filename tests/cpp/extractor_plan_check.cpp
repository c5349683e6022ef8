// Host check of csrc/extractor_plan.h (no HIP): for each case of a text file it builds the extractor's
// tables and the plan of one image size, as extractor.hip does, and writes every table.  For a case
// with an image it also builds the padded pyramid on the CPU in two ways and writes both:
//   a  level by level from xtab / ytab, as k_pyr_level0 and k_pyr_resize consume them
//   b  tile by tile from the parameter blocks, with k_pyramid's loop structure: stage the tile's
//      level-0 need rectangle, chain the levels through two buffers, store own rectangles with their
//      mirrors.  It aborts when a tap falls outside the source need rectangle the tile staged, a
//      rectangle outgrows the LDS the plan reserves, or a parameter block is read past its end --
//      what a GPU run cannot show.  "unwritten" counts the padded bytes no tile wrote.
// tests/test_extractor_plan_cpu.py compares everything with the CPU oracle and with brute force.
//
//   extractor_plan_check IN OUT
//
// IN:  case NAME ROWS COLS NLEVELS NFEATURES IMAGE|-   (IMAGE: ROWS x COLS bytes; pyramids -> IMAGE.a, IMAGE.b) | end
// Floats are written as their bit patterns.  A refused case starts from the plan of the case before
// it and reports whether the refusal left that plan bytewise as it was ("untouched 1").
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>

#include "extractor_plan.h"

using namespace orbmi;

static uint32_t bits(float v) { uint32_t u; memcpy(&u, &v, 4); return u; }

template <class T, class F>
static void row(FILE* f, const char* name, const std::vector<T>& v, F&& put) {
    fprintf(f, "%s", name);
    for (const T& e : v) put(e);
    fprintf(f, "\n");
}
static void row(FILE* f, const char* name, const std::vector<int>& v) {
    row(f, name, v, [&](int e) { fprintf(f, " %d", e); });
}
static void row(FILE* f, const char* name, const std::vector<float>& v) {
    row(f, name, v, [&](float e) { fprintf(f, " %u", bits(e)); });
}

#define REQUIRE(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); abort(); } } while (0)

// every field of the plan, in one string: two plans are equal when their dumps are
static void dump_plan(FILE* f, const ExtractorPlan& p) {
    for (size_t l = 0; l < p.levels.size(); l++) {
        const LevelGeom& g = p.levels[l];
        fprintf(f, "level %d %d %d %d %lld %d %d %d %d %d %d %d %d %d %d %u %u %u %d %d %d %d %lld %d\n", g.W, g.H, g.stride,
                g.ph, g.off, g.cell_begin, g.cell_end, g.nfeat, g.out_base, g.out_cap, g.key_base, g.key_cap, g.width,
                g.height, g.nIni, bits(g.hX), bits(g.scale), bits(g.size), g.blur_xv, g.resize_xv, g.xtab_off, g.ytab_off,
                g.boff, g.bstride);
    }
    row(f, "cells", p.cells, [&](const CellGeom& c) {
        fprintf(f, " %d %d %d %d %d %d %d %d %lld %d %d", c.x0, c.y0, c.w, c.h, c.sx, c.sy, c.slot_base, c.level, c.roi_off,
                c.stride, c.lcell);
    });
    row(f, "regbase", p.regbase);
    row(f, "xtab", p.xtab, [&](const XTab& e) { fprintf(f, " %d %d %d %d", e.sx0, e.sx1, e.a0, e.a1); });
    row(f, "ytab", p.ytab, [&](const YTab& e) { fprintf(f, " %d %d %d %d", e.y0, e.y1, e.b0, e.b1); });
    row(f, "btiles", p.btiles, [&](const BlurTile& t) { fprintf(f, " %d %d %d", t.level, t.xy & 0xFFFF, t.xy >> 16); });
    uint32_t h = 2166136261u;  // the parameter blocks are run below; here their FNV-1a
    for (uint32_t w : p.blob)
        for (int k = 0; k < 4; k++) h = (h ^ ((w >> (8 * k)) & 255)) * 16777619u;
    fprintf(f, "scalars %lld %lld %d %d %d %d %d %d %d %d %d %d %d %zu %u\n", p.pimg, p.bimg, p.keys_cap, p.out_cap, p.fast_maxw,
            p.fast_maxh, p.kx, p.ky, p.hx, p.hy, p.blob_words, p.lds0, p.lds_half, p.blob.size(), h);
}

static std::string plan_text(const ExtractorPlan& p) {
    char* buf = nullptr;
    size_t n = 0;
    FILE* m = open_memstream(&buf, &n);
    dump_plan(m, p);
    fclose(m);
    std::string s(buf, n);
    free(buf);
    return s;
}

// (a) k_pyr_level0, then k_pyr_resize per level: every padded pixel from the interior pixel it mirrors
static std::vector<uint8_t> pyramid_levelwise(const ExtractorPlan& p, const uint8_t* img, int cols) {
    std::vector<uint8_t> P(p.pimg, 0);
    for (size_t l = 0; l < p.levels.size(); l++) {
        const LevelGeom& g = p.levels[l];
        uint8_t* D = P.data() + g.off;
        for (int yp = 0; yp < g.ph; yp++)
            for (int xp = 0; xp < g.W + 2 * kEdge; xp++) {
                const int ix = reflect101(xp - kEdge, g.W), iy = reflect101(yp - kEdge, g.H);
                if (l == 0) { D[(long long)yp * g.stride + xp] = img[(size_t)iy * cols + ix]; continue; }
                const LevelGeom& s = p.levels[l - 1];
                const XTab x = p.xtab[g.xtab_off + ix];
                const YTab y = p.ytab[g.ytab_off + iy];
                const uint8_t* r0 = P.data() + s.off + (long long)(kEdge + y.y0) * s.stride + kEdge;
                const uint8_t* r1 = P.data() + s.off + (long long)(kEdge + y.y1) * s.stride + kEdge;
                D[(long long)yp * g.stride + xp] =
                    (uint8_t)pyr_resize_px(r0[x.sx0], r0[x.sx1], r1[x.sx0], r1[x.sx1], x, y, ix < g.resize_xv);
            }
    }
    return P;
}

// pyr_store's writes, counted
static void store_counted(std::vector<uint8_t>& P, std::vector<uint8_t>& hit, long long off, int W, int H, int stride, int x,
                          int y, uint8_t v) {
    REQUIRE(x >= 0 && x < W && y >= 0 && y < H);
    pyr_store(P.data() + off, W, H, stride, x, y, v);
    pyr_store(hit.data() + off, W, H, stride, x, y, 1);
}

// (b) k_pyramid, one tile after the other
static std::vector<uint8_t> pyramid_tiled(const ExtractorPlan& p, const uint8_t* img, int cols, long long* unwritten) {
    const int nlevels = (int)p.levels.size(), KX = p.kx, KY = p.ky, W0 = p.levels[0].W, H0 = p.levels[0].H;
    const int hx = p.hx, hy = p.hy, words = p.blob_words;
    REQUIRE(p.blob.size() == (size_t)KX * KY * words && words >= kPyrLevelWords * nlevels);
    REQUIRE(4 * words + p.lds0 + 2 * p.lds_half <= 64 * 1024);
    std::vector<uint8_t> P(p.pimg, 0), hit(p.pimg, 0);
    std::vector<uint8_t> L0(p.lds0), H2(2 * (size_t)p.lds_half);
    auto lo16 = [](uint32_t w) { return (int)(short)(w & 0xFFFF); };
    auto hi16 = [](uint32_t w) { return (int)(short)(w >> 16); };
    for (int t = 0; t < KX * KY; t++) {
        const uint32_t* B = &p.blob[(size_t)t * words];
        const int cx = t % KX, cy = t / KX;
        const int ox0 = W0 * cx / KX, ox1 = W0 * (cx + 1) / KX, oy0 = H0 * cy / KY, oy1 = H0 * (cy + 1) / KY;
        const int nx0 = std::max(ox0 - hx, 0), nx1 = std::min(ox1 + hx, W0), ny0 = std::max(oy0 - hy, 0), ny1 = std::min(oy1 + hy, H0);
        const int w0 = nx1 - nx0, a0 = w0 * (ny1 - ny0);
        REQUIRE(a0 <= p.lds0);
        for (int i = 0; i < a0; i++) L0[i] = img[(size_t)(ny0 + i / w0) * cols + nx0 + i % w0];
        {
            const uint32_t* G = B;
            // the kernel takes level 0's own rectangle from blockIdx: it must be the block's
            REQUIRE(lo16(G[kPyrOwnX]) == ox0 && hi16(G[kPyrOwnX]) == ox1 && lo16(G[kPyrOwnY]) == oy0 && hi16(G[kPyrOwnY]) == oy1);
            const int W = lo16(G[kPyrWH]), H = hi16(G[kPyrWH]), stride = (int)G[kPyrStride];
            REQUIRE(W == W0 && H == H0 && stride == p.levels[0].stride && (long long)G[kPyrOff] == p.levels[0].off);
            for (int y = oy0; y < oy1; y++)
                for (int x = ox0; x < ox1; x++) store_counted(P, hit, G[kPyrOff], W, H, stride, x, y, L0[(y - ny0) * w0 + x - nx0]);
        }
        int snx0 = nx0, sny0 = ny0, sw = w0, sh = ny1 - ny0;  // the source need rectangle of the next level
        for (int l = 1; l < nlevels; l++) {
            const uint32_t* G = B + l * kPyrLevelWords;
            const int o_x0 = lo16(G[kPyrOwnX]), o_x1 = hi16(G[kPyrOwnX]), o_y0 = lo16(G[kPyrOwnY]), o_y1 = hi16(G[kPyrOwnY]);
            const int n_x0 = lo16(G[kPyrNeedX]), n_x1 = hi16(G[kPyrNeedX]), n_y0 = lo16(G[kPyrNeedY]), n_y1 = hi16(G[kPyrNeedY]);
            const int W = lo16(G[kPyrWH]), H = hi16(G[kPyrWH]), stride = (int)G[kPyrStride], rxv = (int)G[kPyrResizeXv];
            const LevelGeom& g = p.levels[l];
            REQUIRE(W == g.W && H == g.H && stride == g.stride && (long long)G[kPyrOff] == g.off && rxv == g.resize_xv);
            // the own rectangle lies inside the need rectangle, or nothing of it would be stored
            REQUIRE(o_x0 >= n_x0 && o_x1 <= n_x1 && o_y0 >= n_y0 && o_y1 <= n_y1);
            const int nw = n_x1 - n_x0, nh = n_y1 - n_y0;
            REQUIRE(nw >= 0 && nh >= 0 && nw * nh <= p.lds_half);
            REQUIRE((long long)G[kPyrXTaps] + 2 * nw <= words && (long long)G[kPyrYTaps] + 2 * nh <= words);
            const uint32_t* XT = B + G[kPyrXTaps];
            const uint32_t* YT = B + G[kPyrYTaps];
            const uint8_t* src = l == 1 ? L0.data() : H2.data() + ((l - 1) & 1) * p.lds_half;
            uint8_t* dst = H2.data() + (l & 1) * p.lds_half;
            const bool keep = l + 1 < nlevels;
            for (int y = n_y0; y < n_y1; y++) {
                const uint32_t y0w = YT[2 * (y - n_y0)], y1w = YT[2 * (y - n_y0) + 1];
                const YTab yy{(short)lo16(y0w), (short)hi16(y0w), (short)lo16(y1w), (short)hi16(y1w)};
                REQUIRE(yy.y0 >= sny0 && yy.y0 < sny0 + sh && yy.y1 >= sny0 && yy.y1 < sny0 + sh);
                const uint8_t* r0 = src + (yy.y0 - sny0) * sw - snx0;
                const uint8_t* r1 = src + (yy.y1 - sny0) * sw - snx0;
                for (int x = n_x0; x < n_x1; x++) {
                    const uint32_t x0w = XT[2 * (x - n_x0)], x1w = XT[2 * (x - n_x0) + 1];
                    const XTab xx{(short)lo16(x0w), (short)hi16(x0w), (short)lo16(x1w), (short)hi16(x1w)};
                    REQUIRE(xx.sx0 >= snx0 && xx.sx0 < snx0 + sw && xx.sx1 >= snx0 && xx.sx1 < snx0 + sw);
                    const uint8_t v = (uint8_t)pyr_resize_px(r0[xx.sx0], r0[xx.sx1], r1[xx.sx0], r1[xx.sx1], xx, yy, x < rxv);
                    if (keep) dst[(y - n_y0) * nw + (x - n_x0)] = v;
                    if (x >= o_x0 && x < o_x1 && y >= o_y0 && y < o_y1) store_counted(P, hit, G[kPyrOff], W, H, stride, x, y, v);
                }
            }
            snx0 = n_x0; sny0 = n_y0; sw = nw; sh = nh;
        }
    }
    *unwritten = 0;
    for (const LevelGeom& g : p.levels)
        for (int yp = 0; yp < g.ph; yp++)
            for (int xp = 0; xp < g.W + 2 * kEdge; xp++) *unwritten += !hit[g.off + (long long)yp * g.stride + xp];
    return P;
}

// the padded levels, rows of W + 38 bytes, one after the other (the oracle's layout)
static void write_levels(const std::string& path, const ExtractorPlan& p, const std::vector<uint8_t>& P) {
    FILE* f = fopen(path.c_str(), "wb");
    REQUIRE(f);
    for (const LevelGeom& g : p.levels)
        for (int yp = 0; yp < g.ph; yp++) fwrite(P.data() + g.off + (long long)yp * g.stride, 1, g.W + 2 * kEdge, f);
    fclose(f);
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    std::ifstream in(argv[1]);
    FILE* f = fopen(argv[2], "w");
    if (!in || !f) return 2;
    signed char pattern[256][4];  // a stand-in for the rBRIEF pattern: every entry tells its place
    for (int t = 0; t < 256; t++)
        for (int k = 0; k < 4; k++) pattern[t][k] = (signed char)((4 * t + k) % 251 - 125);
    ExtractorPlan plan;  // carried from case to case: a refused case must leave it alone
    std::string tok, name, image;
    int rows, cols, nlevels, nfeatures;
    while (in >> tok && tok == "case" && in >> name >> rows >> cols >> nlevels >> nfeatures >> image) {
        const OrbTables tab = orb_tables(nfeatures, 1.2f, nlevels);
        const std::string before = plan_text(plan);
        unsigned char raw[sizeof(ExtractorPlan)];
        memcpy(raw, (const void*)&plan, sizeof(plan));
        const auto t0 = std::chrono::steady_clock::now();
        const int rc = extractor_plan(tab, rows, cols, &plan);
        const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
        fprintf(f, "case %s %d\n", name.c_str(), rc);
        if (rc) {
            fprintf(f, "untouched %d\n", memcmp(raw, (const void*)&plan, sizeof(plan)) == 0 && plan_text(plan) == before);
            continue;
        }
        fprintf(f, "plan_us %.1f\n", us);
        row(f, "scale", tab.scale);
        row(f, "inv_scale", tab.inv_scale);
        row(f, "sigma2", tab.sigma2);
        row(f, "inv_sigma2", tab.inv_sigma2);
        row(f, "nfeat", tab.nfeat);
        row(f, "umax", tab.umax);
        DescribeTables dt;
        fprintf(f, "describe %d\n", describe_tables(tab.umax, pattern, &dt));
        fprintf(f, "pattern");
        for (int t = 0; t < 256; t++)
            for (int k = 0; k < 4; k++) fprintf(f, " %d", (int)dt.pattern[t][k]);
        fprintf(f, "\n");
        for (int ou = 0; ou < 4; ou++) {
            fprintf(f, "ic %d", ou);
            for (int i = 0; i < dt.ic_items[ou]; i++) fprintf(f, " %u %u %u %u", dt.ic[ou][i][0], dt.ic[ou][i][1], dt.ic[ou][i][2], dt.ic[ou][i][3]);
            fprintf(f, "\n");
        }
        dump_plan(f, plan);
        if (image != "-") {
            std::vector<uint8_t> img((size_t)rows * cols);
            FILE* fi = fopen(image.c_str(), "rb");
            REQUIRE(fi && fread(img.data(), 1, img.size(), fi) == img.size());
            fclose(fi);
            write_levels(image + ".a", plan, pyramid_levelwise(plan, img.data(), cols));
            long long unwritten = 0;
            write_levels(image + ".b", plan, pyramid_tiled(plan, img.data(), cols, &unwritten));
            fprintf(f, "unwritten %lld\n", unwritten);
        }
    }
    // an overfull IC table is refused: 31 rows of 31 pixels need 8 or 9 dwords each
    DescribeTables dt;
    fprintf(f, "describe_overflow %d\n", describe_tables(std::vector<int>(kHalfPatch + 1, kHalfPatch), pattern, &dt));
    fclose(f);
    return tok == "end" ? 0 : 2;
}
