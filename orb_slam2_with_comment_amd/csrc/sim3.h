// Launch interface of the batched Sim3Solver kernel (sim3.hip), used by capi_match.cpp.
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

}  // namespace orbmi
