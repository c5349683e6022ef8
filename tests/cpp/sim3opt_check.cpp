// Host check of csrc/sim3_opt.h (the header the device kernel shares): one OptimizeSim3 problem
// through s3o_optimize_host, and one buildSystem pass at its initial estimate, for
// tests/test_sim3opt_cpu.py to compare with the numpy restatement.  A scalar port of the library's
// own arithmetic, not the reference program.
//   sim3opt_check <in> <out> [reps]
// in : int32 n fix_scale, float32 th2 k1[4] k2[4] R12[9] t12[3] s12, then float32 x3d_c1 (n x 3)
//      x3d_c2 (n x 3) obs1 (n x 2) obs2 (n x 2) inv_sigma2_1 (n) inv_sigma2_2 (n)
// out: float64 q[4] t[3] s, float32 sR[9] t_f[3], int32 n_in n_bad iterations[2], uint8 inlier (n),
//      float64 chi2 (n x 2), float64 H (49) b (7) chi2 (1) of the linearisation
// reps > 0: the optimisation is run that many times more and its mean time printed.
//   sim3opt_check lm <in> <out>
// the Levenberg decision the header takes from g2o_lm.h, over a table of steps, once per cube:
// in : text, doubles as 16 hex digits: n LAMBDA0 (a new optimize()) | b CHI (lm_begin) |
//      t OK2 TEMPCHI SCALE_SUM (lm_trial) | e (lm_end)
// out: per cube ("mul": z * z * z, "pow": std::pow(z, 3)) one line per b / t / e with lambda, ni, rho,
//      currentChi as bit patterns, qmax, nBad and the step's verdicts
// Build: c++ -O2 -std=c++17 -ffp-contract=off -I orb_slam2_with_comment_amd/csrc
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sim3_opt.h"

struct LmStep {
    char kind;
    int ok2;
    double a, b;
};

template <class Cube>
static void lm_run(const std::vector<LmStep>& steps, const char* tag, FILE* f, Cube cube) {
    orbmi::S3oLm L{};
    double lambda0 = 0;
    int it = 0;
    auto u = [](double v) { unsigned long long b; memcpy(&b, &v, 8); return b; };
    auto state = [&](const char* what, int v0, int v1) {
        fprintf(f, "%s %s %016llx %016llx %016llx %016llx %d %d %d %d\n", tag, what, u(L.lambda), u(L.ni), u(L.rho),
                u(L.currentChi), L.qmax, L.nBad, v0, v1);
    };
    for (const LmStep& s : steps) {
        if (s.kind == 'n') {
            L = orbmi::S3oLm{};
            lambda0 = s.a;
            it = 0;
        } else if (s.kind == 'b') {
            orbmi::lm_begin(L, it, s.a, [lambda0] { return lambda0; });
            state("b", 0, 0);
        } else if (s.kind == 't') {
            bool more = false;
            const bool accept = orbmi::lm_trial(L, s.ok2 != 0, s.a, s.b, &more, cube);
            state("t", accept, more);
        } else {
            state("e", orbmi::lm_end(L), 0);
            it++;
        }
    }
}

static int lm_table(const char* in, const char* out) {
    FILE* f = fopen(in, "r");
    if (!f) return 2;
    std::vector<LmStep> steps;
    char kind[4];
    auto dbl = [&](double* v) { unsigned long long b; if (fscanf(f, "%llx", &b) != 1) return false; memcpy(v, &b, 8); return true; };
    while (fscanf(f, "%3s", kind) == 1) {
        LmStep s{kind[0], 1, 0, 0};
        if ((s.kind == 'n' || s.kind == 'b') && !dbl(&s.a)) return 2;
        if (s.kind == 't' && (fscanf(f, "%d", &s.ok2) != 1 || !dbl(&s.a) || !dbl(&s.b))) return 2;
        steps.push_back(s);
    }
    fclose(f);
    f = fopen(out, "w");
    if (!f) return 2;
    lm_run(steps, "mul", f, orbmi::LmCubeMul());
    lm_run(steps, "pow", f, orbmi::LmCubePow());
    fclose(f);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 4 && !strcmp(argv[1], "lm")) return lm_table(argv[2], argv[3]);
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hd[2];
    float par[22];
    if (fread(hd, sizeof(int32_t), 2, f) != 2 || fread(par, sizeof(float), 22, f) != 22) return 2;
    const int n = hd[0], fix_scale = hd[1];
    if (n < 0) return 2;
    const float th2 = par[0], *k1 = par + 1, *k2 = par + 5, *R12 = par + 9, *t12 = par + 18, s12 = par[21];
    const size_t N = (size_t)n;
    std::vector<float> x1(3 * N), x2(3 * N), o1(2 * N), o2(2 * N), w1(N), w2(N);
    auto rd = [&](std::vector<float>& v) { return fread(v.data(), sizeof(float), v.size(), f) == v.size(); };
    if (!rd(x1) || !rd(x2) || !rd(o1) || !rd(o2) || !rd(w1) || !rd(w2)) return 2;
    fclose(f);
    std::vector<orbmi::S3oPair> pairs(N);
    for (size_t i = 0; i < N; i++) {
        orbmi::S3oPair& p = pairs[i];
        for (int r = 0; r < 3; r++) { p.X1[r] = (double)x1[3 * i + r]; p.X2[r] = (double)x2[3 * i + r]; }
        for (int r = 0; r < 2; r++) { p.o1[r] = (double)o1[2 * i + r]; p.o2[r] = (double)o2[2 * i + r]; }
        p.w1 = (double)w1[i];
        p.w2 = (double)w2[i];
    }
    std::vector<uint8_t> inlier(N + 1);
    std::vector<double> chi2(2 * N + 1);
    orbmi::S3oHostResult r = orbmi::s3o_optimize_host(n, pairs.data(), k1, k2, th2, fix_scale, R12, t12, s12, inlier.data(), chi2.data());
    const int reps = argc > 3 ? atoi(argv[3]) : 0;
    if (reps > 0) {
        std::vector<uint8_t> in2(N + 1);
        std::vector<double> c2(2 * N + 1);
        const auto t0 = std::chrono::steady_clock::now();
        int sink = 0;
        for (int k = 0; k < reps; k++)
            sink += orbmi::s3o_optimize_host(n, pairs.data(), k1, k2, th2, fix_scale, R12, t12, s12, in2.data(), c2.data()).n_in;
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        printf("host_loop_ms %.6f (%d)\n", ms / reps, sink);
    }
    // the linearisation at the initial estimate, over every pair
    double lin[57] = {};
    if (n > 0) {
        std::vector<uint8_t> all(N, 1);
        std::vector<double> c2(2 * N);
        orbmi::S3oHost h;
        h.n = n;
        h.pairs = pairs.data();
        for (int k = 0; k < 4; k++) { h.k1[k] = (double)k1[k]; h.k2[k] = (double)k2[k]; }
        h.delta = (double)sqrtf(th2);
        h.dsqr = h.delta * h.delta;
        h.fix_scale = fix_scale;
        h.alive = all.data();
        h.chi2 = c2.data();
        orbmi::Sim3d S0;
        orbmi::s3o_from_rts(R12, t12, s12, &S0);
        double acc[orbmi::kS3oAcc];
        h.build(S0, acc);
        int q = 0;
        for (int a = 0; a < 7; a++)
            for (int b = a; b < 7; b++, q++) lin[7 * a + b] = lin[7 * b + a] = acc[q];
        for (int a = 0; a < 7; a++) lin[49 + a] = acc[28 + a];
        lin[56] = acc[35];
    }
    float sR[9], tf[3];
    orbmi::s3o_to_float(r.S, sR, tf);
    const double head[8] = {r.S.q[0], r.S.q[1], r.S.q[2], r.S.q[3], r.S.t[0], r.S.t[1], r.S.t[2], r.S.s};
    const int32_t cnt[4] = {r.n_in, r.n_bad, r.iterations[0], r.iterations[1]};
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    bool ok = fwrite(head, sizeof(double), 8, f) == 8 && fwrite(sR, sizeof(float), 9, f) == 9 &&
              fwrite(tf, sizeof(float), 3, f) == 3 && fwrite(cnt, sizeof(int32_t), 4, f) == 4 &&
              fwrite(inlier.data(), 1, N, f) == N && fwrite(chi2.data(), sizeof(double), 2 * N, f) == 2 * N &&
              fwrite(lin, sizeof(double), 57, f) == 57;
    fclose(f);
    if (!ok) return 2;
    printf("n_in %d n_bad %d iterations %d %d\n", r.n_in, r.n_bad, r.iterations[0], r.iterations[1]);
    return 0;
}
