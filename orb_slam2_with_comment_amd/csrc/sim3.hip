// Sim3Solver (src/Sim3Solver.cc) on the GPU: every RANSAC hypothesis of every solver of a batch
// in one launch.  The arithmetic is csrc/sim3_horn.h, shared with the host.
#include "orbmi_common.h"
#include "sim3.h"
#include "sim3_horn.h"

namespace orbmi {

constexpr int kSim3Waves = 4;  // hypotheses per workgroup

// One wavefront per (hypothesis, solver).  The Horn step (ComputeSim3, :239-351) is wave-uniform:
// every lane evaluates the same fp64 expressions on the same three pairs, so it costs one pass of
// the wave and needs no broadcast.  CheckInliers (:354-378) strides the n correspondences over the
// 64 lanes; per 64 correspondences a ballot is the mask word and its popcount the count, so the
// output does not depend on arrival order (no atomics).  Lanes past n vote 0.
__global__ __launch_bounds__(kSim3Waves * kWave) void k_sim3_ransac(const Sim3Dev* __restrict__ table) {
    const Sim3Dev& S = table[blockIdx.y];
    const int lane = threadIdx.x & (kWave - 1);
    const int h = blockIdx.x * kSim3Waves + (threadIdx.x >> 6);
    if (h >= S.iterations) return;  // the whole wave
    float P1[9], P2[9];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const int idx = S.triples[3 * h + i];
#pragma unroll
        for (int r = 0; r < 3; r++) {
            P1[3 * i + r] = S.x1[3 * (size_t)idx + r];
            P2[3 * i + r] = S.x2[3 * (size_t)idx + r];
        }
    }
    Sim3Hyp H;
    sim3_horn(P1, P2, S.fix_scale, &H);
    const int n = S.n, words = (n + kWave - 1) / kWave;
    uint64_t* mask = S.mask + (size_t)h * words;
    int count = 0;
    for (int w = 0; w < words; w++) {
        const int i = w * kWave + lane;
        bool ok = false;
        if (i < n) {
            const float X1[3] = {S.x1[3 * (size_t)i], S.x1[3 * (size_t)i + 1], S.x1[3 * (size_t)i + 2]};
            const float X2[3] = {S.x2[3 * (size_t)i], S.x2[3 * (size_t)i + 1], S.x2[3 * (size_t)i + 2]};
            ok = sim3_is_inlier(H, X1, X2, S.k1, S.k2, S.e1[i], S.e2[i]);
        }
        const unsigned long long word = __ballot(ok);
        if (lane == 0) mask[w] = word;
        count += __popcll(word);
    }
    if (lane == 0) {
        // static indices: H stays in registers (indexing it by the lane put it in scratch memory)
#pragma unroll
        for (int k = 0; k < 12; k++) {
            S.T12[12 * (size_t)h + k] = H.T12[k];
            S.T21[12 * (size_t)h + k] = H.T21[k];
        }
        S.s[h] = H.s;
        S.count[h] = count;
    }
}

int launch_sim3_ransac(Matcher& m, int nsolvers, const Sim3Dev* table_dev, int max_iterations) {
    if (nsolvers <= 0 || max_iterations <= 0) return ORBMI_OK;
    const dim3 grid((max_iterations + kSim3Waves - 1) / kSim3Waves, nsolvers);
    hipLaunchKernelGGL(k_sim3_ransac, grid, dim3(kSim3Waves * kWave), 0, m.ls(), table_dev);
    ORBMI_HIP(hipGetLastError());
    return ORBMI_OK;
}

}  // namespace orbmi

extern "C" {

int orbmi_sim3_iterations(int n, int min_inliers, double probability, int max_iterations, int* out) {
    if (!out || n < 0 || min_inliers < 0) return ORBMI_E_ARG;
    *out = orbmi::sim3_iterations(n, min_inliers, probability, max_iterations);
    return ORBMI_OK;
}

int orbmi_sim3_sample_triples(uint64_t seed, int solver, int n, int iterations, int32_t* out) {
    if (n < 3 || iterations < 0 || solver < 0 || (iterations > 0 && !out)) return ORBMI_E_ARG;
    std::vector<int32_t> avail((size_t)n);
    for (int it = 0; it < iterations; it++) orbmi::sim3_sample_triple(seed, solver, it, n, avail.data(), out + 3 * (size_t)it);
    return ORBMI_OK;
}

int orbmi_sim3_max_error(float sigma2, int32_t* out) {
    if (!out) return ORBMI_E_ARG;
    *out = orbmi::sim3_max_error(sigma2);
    return ORBMI_OK;
}

}  // extern "C"
