// Launch interface of the batched Sim3Solver kernel (sim3.hip), used by capi_loop.cpp.
#pragma once
#include "matcher.h"

namespace orbmi {

// One solver of a batch, resolved to device pointers (the table is read from device memory)
struct Sim3Dev {
    int n;                  // correspondences
    int iterations;         // hypotheses (0: nothing to do)
    int fix_scale;
    const float* x1;        // n x 3
    const float* x2;
    const int32_t* e1;      // n
    const int32_t* e2;
    float k1[4], k2[4];
    const int32_t* triples; // iterations x 3
    float* T12;             // iterations x 12
    float* T21;
    float* s;               // iterations
    int32_t* count;
    uint64_t* mask;         // iterations x (n + 63) / 64
};

// One wavefront per (hypothesis, solver): grid row = solver.  max_iterations = the largest
// iteration count of the table.
int launch_sim3_ransac(Matcher& m, int nsolvers, const Sim3Dev* table_dev, int max_iterations);

// One OptimizeSim3 problem of a batch, resolved to device pointers (sim3_opt.hip)
struct Sim3OptDev {
    int n;
    int fix_scale;
    float th2;
    const float* x1;   // n x 3: the points in camera 1 / camera 2
    const float* x2;
    const float* o1;   // n x 2: the observations in image 1 / image 2
    const float* o2;
    const float* w1;   // n: invSigma2 of either side
    const float* w2;
    float k1[4], k2[4];
    float R[9], t[3], s;  // the initial g2oS12
    uint8_t* inlier;   // n (out)
    double* chi2;      // n x 2 (out)
};

// The scalar part of one problem's result
struct Sim3OptOut {
    double q[4], t[3], s;
    float sR[9], t_f[3];
    int n_in, n_bad, iterations[2];
};

// One workgroup per problem
int launch_sim3_opt(Matcher& m, int nproblems, const Sim3OptDev* table_dev, Sim3OptOut* outs_dev);
// One buildSystem pass of table_dev[0] at its initial estimate: lin = H (49), b (7), robust chi2
int launch_sim3_opt_linearize(Matcher& m, const Sim3OptDev* table_dev, double* lin_dev);

}  // namespace orbmi
