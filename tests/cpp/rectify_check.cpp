// Stand-alone check of csrc/rectify.h (no HIP, no GPU): reads cases from a binary file, runs the
// map builder, the record conversion and the host remap, and writes what they gave
// (tests/test_rectify_cpu.py compares it with the numpy restatement bit for bit).
//
//   rectify_check in.bin out.bin
//
// in.bin is a sequence of cases, each an int32 kind followed by
//   1 (camera): 41 doubles K[9] D[8] nd R[9] P[12] rows cols
//       -> int32 rc; when 0: map1, map2 (rows x cols f32), records (rows x cols x 4 int16)
//   2 (maps):   int32 rows cols, map1, map2 (f32)
//       -> int32 rc; when 0: records
//   3 (remap):  int32 rows cols, map1, map2, int32 src_rows src_cols src_step, the source bytes
//       -> int32 rc; when 0: the destination (rows x cols u8)
//   0: end
// A table's padding records must be kOutside; the program exits with 2 when they are not.
#include <cstdio>
#include <cstdlib>

#include "rectify.h"

using namespace orbmi::rectify;

static FILE *fin, *fout;

template <class T>
static std::vector<T> get(size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, fin) != n) { fprintf(stderr, "short input\n"); exit(1); }
    return v;
}
template <class T>
static void put(const T* p, size_t n) {
    if (n && fwrite(p, sizeof(T), n, fout) != n) { fprintf(stderr, "write failed\n"); exit(1); }
}

// the table's logical records, with its padding checked
static std::vector<int16_t> unpadded(const std::vector<Record>& rec, int rows, int cols) {
    const size_t pitch = record_pitch(cols);
    if (rec.size() != (size_t)rows * pitch) exit(2);
    std::vector<int16_t> out;
    out.reserve((size_t)rows * cols * 4);
    for (int i = 0; i < rows; i++)
        for (size_t j = 0; j < pitch; j++) {
            const Record& r = rec[(size_t)i * pitch + j];
            if (j >= (size_t)cols) {
                if (r.x0 != kOutside.x0 || r.y0 != kOutside.y0 || r.a || r.b) exit(2);
                continue;
            }
            out.push_back(r.x0); out.push_back(r.y0); out.push_back((int16_t)r.a); out.push_back((int16_t)r.b);
        }
    return out;
}

int main(int argc, char** argv) {
    if (argc != 3 || !(fin = fopen(argv[1], "rb")) || !(fout = fopen(argv[2], "wb"))) {
        fprintf(stderr, "usage: rectify_check in.bin out.bin\n");
        return 1;
    }
    for (;;) {
        const int32_t kind = get<int32_t>(1)[0];
        if (kind == 0) break;
        if (kind == 1) {
            const std::vector<double> d = get<double>(41);
            orbmi_rectify_camera c;
            memcpy(c.K, &d[0], sizeof(c.K));
            memcpy(c.D, &d[9], sizeof(c.D));
            c.nd = (int)d[17];
            memcpy(c.R, &d[18], sizeof(c.R));
            memcpy(c.P, &d[27], sizeof(c.P));
            c.rows = (int)d[39];
            c.cols = (int)d[40];
            const size_t n = c.rows > 0 && c.cols > 0 ? (size_t)c.rows * c.cols : 0;
            std::vector<float> m1(n), m2(n);
            std::vector<Record> rec;
            int32_t rc = init_undistort_rectify_map(&c, m1.data(), m2.data());
            if (!rc) rc = build_records(m1.data(), m2.data(), c.rows, c.cols, &rec);
            put(&rc, 1);
            if (rc) continue;
            put(m1.data(), n);
            put(m2.data(), n);
            const std::vector<int16_t> r = unpadded(rec, c.rows, c.cols);
            put(r.data(), r.size());
            continue;
        }
        const std::vector<int32_t> sz = get<int32_t>(2);
        const int rows = sz[0], cols = sz[1];
        const size_t n = (size_t)rows * cols;
        const std::vector<float> m1 = get<float>(n), m2 = get<float>(n);
        std::vector<Record> rec;
        int32_t rc = build_records(m1.data(), m2.data(), rows, cols, &rec);
        if (kind == 2) {
            put(&rc, 1);
            if (rc) continue;
            const std::vector<int16_t> r = unpadded(rec, rows, cols);
            put(r.data(), r.size());
            continue;
        }
        const std::vector<int32_t> s = get<int32_t>(3);
        const std::vector<uint8_t> src = get<uint8_t>((size_t)s[0] * s[2]);
        put(&rc, 1);
        if (rc) continue;
        std::vector<uint8_t> dst(n);
        const size_t pitch = record_pitch(cols);
        for (int i = 0; i < rows; i++)
            for (int j = 0; j < cols; j++)
                dst[(size_t)i * cols + j] = remap_pixel(rec[(size_t)i * pitch + j], src.data(), s[0], s[1], (size_t)s[2]);
        put(dst.data(), n);
    }
    fclose(fin);
    return fclose(fout) ? 1 : 0;
}
