// Host check of csrc/sim3_horn.h (the header the device kernel, the C ABI and the C++ adapter
// share): every hypothesis of one Sim3Solver problem through sim3_horn and sim3_is_inlier, for
// tests/test_sim3_cpu.py to compare bit for bit with the numpy restatement.  A scalar port of the
// library's own arithmetic, not the reference program.
//   sim3_check <in> <out> [reps]
// in : int32 n H fix_scale, float32 k1[4] k2[4], X1 (n x 3) X2 (n x 3) float32, e1 e2 (n) int32,
//      triples (H x 3) int32
// out: T12 (H x 12) T21 (H x 12) s (H) float32, count (H) int32, mask (H x (n + 63) / 64) uint64
// reps > 0: the loop over the H hypotheses is run that many times more and its mean time printed.
// Build: c++ -O2 -std=c++17 -ffp-contract=off -I orb_slam2_with_comment_amd/csrc
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sim3_horn.h"

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hd[3];
    float k[8];
    if (fread(hd, sizeof(int32_t), 3, f) != 3 || fread(k, sizeof(float), 8, f) != 8) return 2;
    const int n = hd[0], H = hd[1], fix_scale = hd[2];
    if (n < 3 || H < 0) return 2;
    std::vector<float> X1(3 * (size_t)n), X2(3 * (size_t)n);
    std::vector<int32_t> e1(n), e2(n), tri(3 * (size_t)H);
    if (fread(X1.data(), sizeof(float), X1.size(), f) != X1.size() || fread(X2.data(), sizeof(float), X2.size(), f) != X2.size() ||
        fread(e1.data(), sizeof(int32_t), n, f) != (size_t)n || fread(e2.data(), sizeof(int32_t), n, f) != (size_t)n ||
        fread(tri.data(), sizeof(int32_t), tri.size(), f) != tri.size())
        return 2;
    fclose(f);
    for (int32_t t : tri)
        if (t < 0 || t >= n) return 2;
    const size_t words = ((size_t)n + 63) / 64;
    std::vector<float> T12(12 * (size_t)H), T21(12 * (size_t)H), s(H);
    std::vector<int32_t> count(H);
    std::vector<uint64_t> mask((size_t)H * words);
    auto run = [&]() {
        for (int h = 0; h < H; h++) {
            float P1[9], P2[9];
            for (int i = 0; i < 3; i++)
                for (int r = 0; r < 3; r++) {
                    P1[3 * i + r] = X1[3 * (size_t)tri[3 * h + i] + r];
                    P2[3 * i + r] = X2[3 * (size_t)tri[3 * h + i] + r];
                }
            orbmi::Sim3Hyp hyp;
            orbmi::sim3_horn(P1, P2, fix_scale, &hyp);
            int c = 0;
            for (size_t w = 0; w < words; w++) mask[h * words + w] = 0;
            for (int i = 0; i < n; i++)
                if (orbmi::sim3_is_inlier(hyp, &X1[3 * (size_t)i], &X2[3 * (size_t)i], k, k + 4, e1[i], e2[i])) {
                    mask[h * words + (i >> 6)] |= 1ull << (i & 63);
                    c++;
                }
            for (int j = 0; j < 12; j++) {
                T12[12 * (size_t)h + j] = hyp.T12[j];
                T21[12 * (size_t)h + j] = hyp.T21[j];
            }
            s[h] = hyp.s;
            count[h] = c;
        }
    };
    run();
    const int reps = argc > 3 ? atoi(argv[3]) : 0;
    if (reps > 0) {
        const auto t0 = std::chrono::steady_clock::now();
        for (int r = 0; r < reps; r++) run();
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        printf("host_loop_ms %.6f\n", ms / reps);
    }
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    bool ok = fwrite(T12.data(), sizeof(float), T12.size(), f) == T12.size() &&
              fwrite(T21.data(), sizeof(float), T21.size(), f) == T21.size() &&
              fwrite(s.data(), sizeof(float), s.size(), f) == s.size() &&
              fwrite(count.data(), sizeof(int32_t), count.size(), f) == count.size() &&
              fwrite(mask.data(), sizeof(uint64_t), mask.size(), f) == mask.size();
    fclose(f);
    if (!ok) return 2;
    printf("hypotheses %d\n", H);
    return 0;
}
