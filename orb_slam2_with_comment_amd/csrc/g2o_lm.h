// g2o's Levenberg decision (OptimizationAlgorithmLevenberg::solve,
// core/optimization_algorithm_levenberg.cpp:99-163), stated once for every optimiser whose trials
// are judged outside the two headline kernels: OptimizeSim3 (sim3_opt.h, host and device), the
// essential graph (essgraph.h, capi_loop.cpp) and global BA (gba.hip).  Plain C++ compiles it.
// The callers differ in three visible ways only:
//   lambda0()  computeLambdaInit: 1e-5 * max |diag H| (Sim3: its 7 entries; global BA: the device's
//              maximum), or setUserLambdaInit's 1e-16 (essential graph)
//   scale_sum  computeScale's sum x (lambda x + b) over the free vertices, however it arrives
//   cube       how (2 rho - 1)^3 is rounded: LmCubeMul, z * z * z (Sim3 and the essential graph; the
//              device can run it), or LmCubePow, std::pow(z, 3) as g2o writes it (global BA; host
//              only).  The two differ in the last bit for about a quarter of all z in (-1, 1), and
//              each is pinned bit for bit by its optimiser's restatement in tests/.
#pragma once
#include <cmath>

#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif

namespace orbmi {

#define G2O_LM_FN __host__ __device__ inline __attribute__((always_inline))

constexpr int kS3oMaxTrials = 10;  // _maxTrialsAfterFailure

// The Levenberg state of one optimize()
struct S3oLm {
    double lambda, ni, currentChi, iniChi, rho;
    int qmax, nBad;
};

struct LmCubeMul {
    G2O_LM_FN double operator()(double z) const { return z * z * z; }
};
struct LmCubePow {  // a host function: device code cannot name it
    double operator()(double z) const { return std::pow(z, 3); }
};

// After buildSystem of iteration `it`, whose chi2 is `chi`.  lambda0() is the caller's
// computeLambdaInit, evaluated in iteration 0 only, as g2o does (in k_sim3_opt it reads H from LDS,
// and evaluating it ahead of the call changes that kernel's instruction stream)
template <class Lambda0>
G2O_LM_FN void lm_begin(S3oLm& L, int it, double chi, Lambda0 lambda0) {
    L.currentChi = chi;
    L.iniChi = chi;
    if (it == 0) {
        L.lambda = lambda0();
        L.ni = 2;
        L.nBad = 0;
    }
    L.rho = 0;
    L.qmax = 0;
}

// One trial's verdict: true = the step is kept.  *more = the do-while goes on.
template <class Cube>
G2O_LM_FN bool lm_trial(S3oLm& L, bool ok2, double tempChi, double scale_sum, bool* more, Cube cube) {
    if (!ok2) tempChi = 1.7976931348623157e308;
    const double scale = scale_sum + 1e-3;
    L.rho = (L.currentChi - tempChi) / scale;
    const bool accept = L.rho > 0 && tempChi - tempChi == 0;  // isfinite
    if (accept) {
        double alpha = 1. - cube(2 * L.rho - 1);
        alpha = alpha < 2. / 3. ? alpha : 2. / 3.;
        L.lambda = L.lambda * (1. / 3. > alpha ? 1. / 3. : alpha);
        L.ni = 2;
        L.currentChi = tempChi;
    } else {
        L.lambda = L.lambda * L.ni;
        L.ni = L.ni * 2;
    }
    L.qmax++;
    *more = L.rho < 0 && L.qmax < kS3oMaxTrials;
    return accept;
}

// After the do-while: true = optimize() stops (Terminate)
G2O_LM_FN bool lm_end(S3oLm& L) {
    if (L.qmax == kS3oMaxTrials || L.rho == 0) return true;
    if ((L.iniChi - L.currentChi) * 1e3 < L.iniChi) L.nBad++;
    else L.nBad = 0;
    return L.nBad >= 3;
}

}  // namespace orbmi
