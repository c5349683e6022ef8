// Optimizer::OptimizeSim3 (src/Optimizer.cc:1145-1347) on the GPU: every problem of a ragged batch
// in one launch, one workgroup each.  The arithmetic is csrc/sim3_opt.h, shared with the host.
#include "orbmi_common.h"
#include "sim3.h"
#include "sim3_opt.h"
#include "wave_ops.h"

namespace orbmi {

constexpr int kS3oThreads = 256;
constexpr int kS3oWaves = kS3oThreads / kWave;

// Workgroup state.  S / Si are what the passes evaluate at (the estimate, or a trial); Scur is the
// vertex's estimate, S0 what was passed in.
struct S3oShared {
    Sim3d S, Si, Scur, S0;
    Sim3d P[14], Pi[14];  // linearizeOplus's pushed estimates: 2 d / 2 d + 1 = +-delta along d
    double red[kS3oWaves][kS3oAcc];
    double Hb[35], x[7];  // the linear system of the iteration and the trial's step (thread 0)
    S3oLm L;              // thread 0's Levenberg state, kept here to spare its registers
    double k1[4], k2[4];
    int more, stop, count, ok2;
};

__device__ __forceinline__ S3oPair s3o_load(const Sim3OptDev& D, int i) {
    S3oPair p;
#pragma unroll
    for (int r = 0; r < 3; r++) {
        p.X1[r] = (double)D.x1[3 * (size_t)i + r];
        p.X2[r] = (double)D.x2[3 * (size_t)i + r];
    }
#pragma unroll
    for (int r = 0; r < 2; r++) {
        p.o1[r] = (double)D.o1[2 * (size_t)i + r];
        p.o2[r] = (double)D.o2[2 * (size_t)i + r];
    }
    p.w1 = (double)D.w1[i];
    p.w2 = (double)D.w2[i];
    return p;
}

// computeActiveErrors + buildSystem at sh.S: every lane takes the live pairs strided by the block;
// the 36 sums go through the wave reduce-scatter, then one LDS slot per wave.  The caller adds the
// slots in wave order after a barrier.
__device__ __forceinline__ void s3o_pass_build(S3oShared& sh, const Sim3OptDev& D, double delta, double dsqr) {
    double acc[kS3oAcc];
#pragma unroll
    for (int k = 0; k < kS3oAcc; k++) acc[k] = 0;
    for (int i = threadIdx.x; i < D.n; i += kS3oThreads) {
        if (!D.inlier[i]) continue;
        const S3oPair p = s3o_load(D, i);
        // an offset the compiler cannot see through: the 28 pushed estimates are loop-invariant,
        // and hoisting their 224 doubles out of this loop spilled to scratch memory
        int off = 0;
        asm volatile("" : "+v"(off));
        s3o_edge(sh.S, sh.P + off, p.X2, p.o1, p.w1, sh.k1, delta, dsqr, D.fix_scale, acc);
        asm volatile("" : "+v"(off));
        s3o_edge(sh.Si, sh.Pi + off, p.X1, p.o2, p.w2, sh.k2, delta, dsqr, D.fix_scale, acc);
    }
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6;
    double v[32];
#pragma unroll
    for (int k = 0; k < 32; k++) v[k] = acc[k];
    const double r = wave_reduce_scatter32(v);
    if (!(lane & 1)) sh.red[w][lane >> 1] = r;
#pragma unroll
    for (int k = 32; k < kS3oAcc; k++) {
        const double t = wave_sum(acc[k]);
        if (lane == 0) sh.red[w][k] = t;
    }
}

// computeActiveErrors + activeRobustChi2 at sh.S: the chi2 of either edge goes to D.chi2, which is
// what the outlier pass reads (stale after a rejected trial, as the reference's are)
__device__ __forceinline__ void s3o_pass_chi2(S3oShared& sh, const Sim3OptDev& D, double delta, double dsqr) {
    double sum = 0;
    for (int i = threadIdx.x; i < D.n; i += kS3oThreads) {
        if (!D.inlier[i]) continue;
        const S3oPair p = s3o_load(D, i);
        double c12, c21;
        sum = sum + s3o_pair_chi2(sh.S, sh.Si, p, sh.k1, sh.k2, delta, dsqr, &c12, &c21);
        D.chi2[2 * (size_t)i] = c12;
        D.chi2[2 * (size_t)i + 1] = c21;
    }
    const double t = wave_sum(sum);
    if ((threadIdx.x & (kWave - 1)) == 0) sh.red[threadIdx.x >> 6][0] = t;
}

__device__ __forceinline__ double s3o_red(const S3oShared& sh, int k) {
    double t = sh.red[0][k];
#pragma unroll
    for (int w = 1; w < kS3oWaves; w++) t = t + sh.red[w][k];
    return t;
}

// One workgroup per problem.  Thread 0 owns the Levenberg state and the 7x7 solve; lanes 0-13
// build the perturbed estimates of a linearisation; every lane evaluates edges.  inlier[i] and
// chi2[i] are written and read by the same thread (i strided by the block), so they need no
// fence.  LIN: one buildSystem at the initial estimate, written to lin (49 + 7 + 1 doubles).
template <bool LIN>
__global__ __launch_bounds__(kS3oThreads) void k_sim3_opt(const Sim3OptDev* __restrict__ table,
                                                         Sim3OptOut* __restrict__ outs, double* __restrict__ lin) {
    __shared__ S3oShared sh;
    const Sim3OptDev& D = table[blockIdx.x];
    const int tid = threadIdx.x, n = D.n;
    const double delta = (double)sqrtf(D.th2), dsqr = delta * delta, th2 = (double)D.th2;
    if (tid == 0) {
        s3o_from_rts(D.R, D.t, D.s, &sh.S0);
        sh.Scur = sh.S0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            sh.k1[k] = (double)D.k1[k];
            sh.k2[k] = (double)D.k2[k];
        }
        sh.count = 0;
    }
    for (int i = tid; i < n; i += kS3oThreads) {
        D.inlier[i] = 1;
        D.chi2[2 * (size_t)i] = 0;
        D.chi2[2 * (size_t)i + 1] = 0;
    }
    __syncthreads();
    int its0 = 0, its1 = 0, n_bad = 0, n_in = 0;
    bool returned_early = false;
    for (int phase = 0; phase < 2; phase++) {
        const int iterations = phase == 0 ? 5 : (n_bad > 0 ? 10 : 5);
        for (int it = 0; it < iterations && n > 0; it++) {
            // linearizeOplus's 14 pushed estimates and the estimate itself, one lane each
            if (tid < 14) {
                s3o_perturbed(sh.Scur, tid >> 1, (tid & 1) ? -kS3oDelta : kS3oDelta, D.fix_scale, &sh.P[tid], &sh.Pi[tid]);
            } else if (tid == 14) {
                sh.S = sh.Scur;
                s3o_inverse(sh.Scur, &sh.Si);
            }
            __syncthreads();
            s3o_pass_build(sh, D, delta, dsqr);
            __syncthreads();
            if (tid == 0) {
                // the slots of the waves in order; H, b and chi2 stay in row 0
#pragma unroll
                for (int k = 0; k < kS3oAcc; k++) sh.red[0][k] = s3o_red(sh, k);
                s3o_lm_begin(sh.L, it, sh.red[0], sh.red[0][35]);
            }
            if (LIN) {
                if (tid == 0) {
                    int q = 0;
                    for (int r = 0; r < 7; r++)
                        for (int c = r; c < 7; c++, q++) {
                            lin[57 * (size_t)blockIdx.x + 7 * r + c] = sh.red[0][q];
                            lin[57 * (size_t)blockIdx.x + 7 * c + r] = sh.red[0][q];
                        }
                    for (int r = 0; r < 7; r++) lin[57 * (size_t)blockIdx.x + 49 + r] = sh.red[0][28 + r];
                    lin[57 * (size_t)blockIdx.x + 56] = sh.red[0][35];
                }
                return;
            }
            if (tid == 0) {  // the trials' chi2 pass reuses the slots
#pragma unroll
                for (int k = 0; k < 35; k++) sh.Hb[k] = sh.red[0][k];
            }
            bool more;
            do {
                __syncthreads();  // the build's slots are read; S may be replaced
                if (tid == 0) {
                    double x[7];
                    const bool ok2 = s3o_solve7(sh.Hb, sh.Hb + 28, sh.L.lambda, x);
#pragma unroll
                    for (int k = 0; k < 7; k++) sh.x[k] = x[k];
                    sh.ok2 = ok2;
                    Sim3d T = sh.Scur;
                    if (ok2) s3o_oplus(sh.Scur, x, D.fix_scale, &T);
                    sh.S = T;
                    s3o_inverse(T, &sh.Si);
                }
                __syncthreads();
                s3o_pass_chi2(sh, D, delta, dsqr);
                __syncthreads();
                if (tid == 0) {
                    const double tempChi = s3o_red(sh, 0);
                    bool m;
                    if (s3o_lm_trial(sh.L, sh.ok2 != 0, tempChi, sh.x, sh.Hb + 28, &m)) sh.Scur = sh.S;
                    sh.more = m;
                }
                __syncthreads();
                more = sh.more;
            } while (more);
            if (tid == 0) {
                if (phase == 0) its0++; else its1++;
                sh.stop = lm_end(sh.L);
            }
            __syncthreads();
            if (sh.stop) break;
        }
        if (LIN) return;  // n == 0: the caller zeroed lin
        // the chi2 pass over the live pairs: e12.chi2() > th2 || e21.chi2() > th2 (a NaN counts)
        int bad = 0, good = 0;
        for (int i = tid; i < n; i += kS3oThreads) {
            if (!D.inlier[i]) continue;
            const bool ok = D.chi2[2 * (size_t)i] <= th2 && D.chi2[2 * (size_t)i + 1] <= th2;
            if (!ok) D.inlier[i] = 0;
            bad += !ok;
            good += ok;
        }
        const int k = phase == 0 ? bad : good;
        if (k) atomicAdd(&sh.count, k);  // integers: the order does not matter
        __syncthreads();
        const int total = sh.count;
        __syncthreads();
        if (tid == 0) sh.count = 0;
        if (phase == 0) {
            n_bad = total;
            if (n - n_bad < 10) {
                returned_early = true;
                break;
            }
        } else {
            n_in = total;
        }
    }
    if (tid == 0) {
        const Sim3d R = returned_early ? sh.S0 : sh.Scur;  // an early return leaves g2oS12 as passed in
        Sim3OptOut& O = outs[blockIdx.x];
#pragma unroll
        for (int k = 0; k < 4; k++) O.q[k] = R.q[k];
#pragma unroll
        for (int k = 0; k < 3; k++) O.t[k] = R.t[k];
        O.s = R.s;
        s3o_to_float(R, O.sR, O.t_f);
        O.n_in = n_in;
        O.n_bad = n_bad;
        O.iterations[0] = its0;
        O.iterations[1] = its1;
    }
}

int launch_sim3_opt(Matcher& m, int nproblems, const Sim3OptDev* table_dev, Sim3OptOut* outs_dev) {
    if (nproblems <= 0) return ORBMI_OK;
    hipLaunchKernelGGL((k_sim3_opt<false>), dim3(nproblems), dim3(kS3oThreads), 0, m.ls(), table_dev, outs_dev,
                       (double*)nullptr);
    ORBMI_HIP(hipGetLastError());
    return ORBMI_OK;
}

int launch_sim3_opt_linearize(Matcher& m, const Sim3OptDev* table_dev, double* lin_dev) {
    hipLaunchKernelGGL((k_sim3_opt<true>), dim3(1), dim3(kS3oThreads), 0, m.ls(), table_dev, (Sim3OptOut*)nullptr, lin_dev);
    ORBMI_HIP(hipGetLastError());
    return ORBMI_OK;
}

}  // namespace orbmi
