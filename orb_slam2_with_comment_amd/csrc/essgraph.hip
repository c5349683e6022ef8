// Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:829-1118) on the GPU: the pose graph of
// VertexSim3Expmap / EdgeSim3 linearised numerically one evaluation per lane, assembled by a gather
// in edge order, solved by a block-sparse LDL^T in one workgroup, and the two arithmetic loops of
// LoopClosing::CorrectLoop.  The arithmetic is csrc/essgraph.h, shared with the host; the Levenberg
// decisions are taken on the host (capi_loop.cpp) from one small read-back per trial.
#include "orbmi_common.h"
#include "essgraph_launch.h"
#include "wave_ops.h"

namespace orbmi {

constexpr int kEgThreads = 256;
constexpr int kEgLinEdges = kEgThreads / 32;  // one edge per 32 lanes

// linearizeOplus + constructQuadraticForm.  Lane l of an edge's 32: l < 28 evaluates the error
// with vertex l / 14 pushed by +-delta (even / odd lane) along direction (l / 2) % 7, so a column
// of a Jacobian is one subtract across the lane pair; lanes 28-31 evaluate the error itself.  The
// columns meet in LDS, and the 32 lanes share the 169 entries of the edge's record.
__global__ __launch_bounds__(kEgThreads) void k_eg_linearize(const EgEdge* __restrict__ edges, const Sim3d* __restrict__ est,
                                                            int ne, int fix_scale, double* __restrict__ recs) {
    __shared__ double sh[kEgLinEdges][2 * 49 + 7];  // J[v][row k][column d] at 49 v + 7 k + d, e at 98
    const int l = threadIdx.x & 31, slot = threadIdx.x >> 5;
    const int e = blockIdx.x * kEgLinEdges + slot;
    const bool live = e < ne;
    const EgEdge E = edges[live ? e : ne - 1];  // a group past the end repeats the last edge and writes nothing
    Sim3d S0 = est[E.v0], S1 = est[E.v1];
    const int p = l >> 1, v = p >= 7, d = p - 7 * v;
    if (l < 28) {
        const double step = (l & 1) ? -kS3oDelta : kS3oDelta;
        double u[7];
#pragma unroll
        for (int k = 0; k < 7; k++) u[k] = k == d ? step : 0.0;
        Sim3d T;
        s3o_oplus(v ? S1 : S0, u, fix_scale, &T);
        if (v) S1 = T;
        else S0 = T;
    }
    double err[7];
    eg_edge_error(E.C, S0, S1, err);
    const double scalar = 1.0 / (2 * kS3oDelta);
    double col[7];
#pragma unroll
    for (int k = 0; k < 7; k++) {
        const double other = dpp_mov<kDppXor1>(err[k]);  // the lane pair's other sign
        col[k] = scalar * ((l & 1) ? other - err[k] : err[k] - other);
    }
    double* mine = sh[slot];
    if (l < 28 && !(l & 1)) {
#pragma unroll
        for (int k = 0; k < 7; k++) mine[49 * v + 7 * k + d] = col[k];
    }
    if (l == 28) {
#pragma unroll
        for (int k = 0; k < 7; k++) mine[98 + k] = err[k];
    }
    __syncthreads();
    if (!live) return;
    double* rec = recs + (size_t)e * kEgRec;
    for (int o = l; o < kEgRec; o += 32) {
        double s = 0;
        if (o < 7) {
            s = mine[98 + o];
        } else if (o == kEgRecChi) {
            for (int k = 0; k < 7; k++) s = s + mine[98 + k] * mine[98 + k];
        } else if (o < kEgRecB0) {
            const int idx = o - kEgRecH00, w = idx / 49, r = idx % 49, a = r / 7, b = r % 7;
            const double *Ja = mine + (w == 2 ? 49 : 0), *Jb = mine + (w != 0 ? 49 : 0);
            for (int k = 0; k < 7; k++) s = s + Ja[7 * k + a] * Jb[7 * k + b];
        } else if (o < kEgRecB0 + 14) {
            const int idx = o - kEgRecB0, a = idx % 7;
            const double* J = mine + (idx >= 7 ? 49 : 0);
            for (int k = 0; k < 7; k++) s = s + J[7 * k + a] * (-mine[98 + k]);
        }
        rec[o] = s;
    }
}

// One wave per block slot (the diagonal blocks with their part of b, then the off-diagonal blocks
// of the permuted lower triangle): lane q sums entry q over the slot's list, in edge order
__global__ __launch_bounds__(64) void k_eg_assemble(EgDev D) {
    const int s = blockIdx.x, q = threadIdx.x;
    if (s >= D.nf + D.nl || q >= (s < D.nf ? 56 : 49)) return;
    const double v = eg_assemble_entry(D.asm_ptr, D.asm_ent, D.recs, s, q);
    if (q >= 49) D.b[(size_t)s * 7 + (q - 49)] = v;
    else if (s < D.nf) D.Hd[(size_t)s * 49 + q] = v;
    else D.Ho[(size_t)(s - D.nf) * 49 + q] = v;
}

// The sum of n values `stride` apart in one workgroup, in wave_ops.h's fixed order
__global__ __launch_bounds__(kEgThreads) void k_eg_reduce(const double* __restrict__ src, int n, int stride, double* __restrict__ dst) {
    __shared__ double red[kEgThreads];
    const double t = strided_sum_fixed<kEgThreads>(src, n, stride, red);
    if (threadIdx.x == 0) *dst = t;
}

// (H + lambda I) x = b: a right-looking block LDL^T with 7 x 7 blocks, unpivoted, in the plan's
// elimination order, with the forward substitution riding on it, then the back substitution.
// ONE workgroup: a latency-bound chain of three barriers per column on the way down (the diagonal
// block factored by thread 0 in registers; the column's rows scaled and applied to y, one row per
// lane; the outer-product updates, one target entry per lane) and one per column on the way up.
__global__ __launch_bounds__(kEgThreads) void k_eg_factor_solve(EgDev D, double lambda) {
    __shared__ double Dg[49];
    __shared__ double red[kEgThreads];
    __shared__ int sh_fail;
    const int tid = threadIdx.x, nf = D.nf;
    if (tid == 0) sh_fail = 0;
    for (int i = tid; i < nf * 49; i += kEgThreads) {
        const double h = D.Hd[i];
        D.Ld[i] = (i % 49) % 8 == 0 ? h + lambda : h;
    }
    for (int i = tid; i < D.nl * 49; i += kEgThreads) D.Lo[i] = D.Ho[i];
    for (int i = tid; i < nf * 7; i += kEgThreads) D.y[i] = D.b[i];
    __syncthreads();
    bool fail = false;
    for (int c = 0; c < nf; c++) {
        if (tid == 0) {
            double* G = D.Ld + (size_t)c * 49;
            if (!eg_factor_diag(G)) sh_fail = 1;
#pragma unroll
            for (int k = 0; k < 49; k++) Dg[k] = G[k];
        }
        __syncthreads();
        if (sh_fail) {  // the same for every thread: a bad pivot ends the factorisation
            fail = true;
            break;
        }
        // L y = b for this column: every lane solves the 7 x 7 part itself (z), thread 0 keeps it
        const int a0 = D.col_ptr[c], m = D.col_ptr[c + 1] - a0;
        if (tid < 7 * m || tid == 0) {
            double z[7];
#pragma unroll
            for (int i = 0; i < 7; i++) z[i] = D.y[(size_t)c * 7 + i];
#pragma unroll
            for (int i = 0; i < 7; i++)
#pragma unroll
                for (int k = 0; k < i; k++) z[i] = z[i] - Dg[7 * i + k] * z[k];
            if (tid == 0) {
#pragma unroll
                for (int i = 0; i < 7; i++) D.x[(size_t)c * 7 + i] = z[i];
            }
            for (int r = tid; r < 7 * m; r += kEgThreads) {
                const int a = a0 + r / 7, i = r % 7;
                double* row = D.Lo + (size_t)a * 49 + 7 * i;
                eg_scale_row(row, Dg);
                double* yr = D.y + (size_t)D.row_of[a] * 7 + i;
                double t = *yr;
#pragma unroll
                for (int j = 0; j < 7; j++) t = t - row[j] * z[j];
                *yr = t;
            }
        }
        __syncthreads();
        const int u0 = D.upd_ptr[c], nu = D.upd_ptr[c + 1] - u0;
        for (int w = tid; w < nu * 49; w += kEgThreads) {
            const int* U = D.upd + 3 * (size_t)(u0 + w / 49);
            const int q = w % 49;
            double* T = (U[0] >= 0 ? D.Lo + (size_t)U[0] * 49 : D.Ld + (size_t)(~U[0]) * 49) + q;
            *T = eg_update_entry(*T, D.Lo + (size_t)U[1] * 49 + 7 * (q / 7), D.Lo + (size_t)U[2] * 49 + 7 * (q % 7), Dg);
        }
        if (nu) __syncthreads();  // nu depends on c alone: the same for every thread
    }
    if (!fail) {
        for (int i = tid; i < nf * 7; i += kEgThreads) D.x[i] = D.x[i] / D.Ld[(size_t)(i / 7) * 49 + 8 * (i % 7)];
        __syncthreads();
        for (int c = nf - 1; c >= 0; c--) {  // L^T x = y: wave 0, lane j owns entry j of the column's block
            if (tid < kWave) {
                const int a0 = D.col_ptr[c], a1 = D.col_ptr[c + 1];
                const int j = tid < 7 ? tid : 6;
                const double* G = D.Ld + (size_t)c * 49;
                double* yc = D.x + (size_t)c * 7;
                double t = yc[j];
                for (int a = a0; a < a1; a++) {
                    const double* yr = D.x + (size_t)D.row_of[a] * 7;
#pragma unroll
                    for (int i = 0; i < 7; i++) t = t - D.Lo[(size_t)a * 49 + 7 * i + j] * yr[i];
                }
#pragma unroll
                for (int k = 6; k >= 1; k--) {  // entry k is final once 6 .. k + 1 are applied
                    const double xk = __shfl(t, k);
                    if (j < k) t = t - G[7 * k + j] * xk;
                }
                if (tid < 7) yc[tid] = t;
            }
            __syncthreads();
        }
    } else {
        for (int i = tid; i < nf * 7; i += kEgThreads) D.x[i] = 0;
        __syncthreads();
    }
    double part = 0;  // computeScale: sum x (lambda x + b)
    for (int i = tid; i < nf * 7; i += kEgThreads) part = part + D.x[i] * (lambda * D.x[i] + D.b[i]);
    const double t = block_sum_fixed<kEgThreads>(part, red);
    if (tid == 0) {
        D.out[kEgOutScale] = t;
        D.out[kEgOutFail] = fail ? 1.0 : 0.0;
    }
}

// trial = oplus(est, x) per free vertex; the accepted estimates stay in est for the restore
__global__ __launch_bounds__(64) void k_eg_update(EgDev D, const Sim3d* __restrict__ est, Sim3d* __restrict__ trial) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= D.nf) return;
    const int v = D.vert_of[c];
    double x[7];
#pragma unroll
    for (int k = 0; k < 7; k++) x[k] = D.x[(size_t)c * 7 + k];
    Sim3d T;
    s3o_oplus(est[v], x, D.fix_scale, &T);
    trial[v] = T;
}

// computeActiveErrors at the trial: chi2 per edge
__global__ __launch_bounds__(64) void k_eg_chi2(EgDev D, const Sim3d* __restrict__ est) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= D.ne) return;
    const EgEdge E = D.edges[e];
    double err[7];
    eg_edge_error(E.C, est[E.v0], est[E.v1], err);
    D.chi2[e] = eg_chi2(err);
}

// The two arithmetic loops of CorrectLoop and the tail of OptimizeEssentialGraph
__global__ __launch_bounds__(kEgThreads) void k_eg_correct(int npoints, const float* __restrict__ points,
                                                          const int32_t* __restrict__ ref, const Sim3d* __restrict__ Srw,
                                                          const Sim3d* __restrict__ Swr, float* __restrict__ out_points, int nposes,
                                                          const Sim3d* __restrict__ poses, float* __restrict__ out_tcw) {
    const int i = blockIdx.x * kEgThreads + threadIdx.x;
    if (i < npoints) {
        const int r = ref[i];
        const float P[3] = {points[3 * (size_t)i], points[3 * (size_t)i + 1], points[3 * (size_t)i + 2]};
        float o[3];
        eg_correct_point(Srw[r], Swr[r], P, o);
        out_points[3 * (size_t)i] = o[0];
        out_points[3 * (size_t)i + 1] = o[1];
        out_points[3 * (size_t)i + 2] = o[2];
    }
    if (i < nposes) {
        float T[16];
        eg_sim3_to_tcw(poses[i], T);
#pragma unroll
        for (int k = 0; k < 16; k++) out_tcw[16 * (size_t)i + k] = T[k];
    }
}

int launch_eg_linearize(Matcher& m, const EgDev& D, const Sim3d* est) {
    if (D.ne <= 0) return ORBMI_OK;
    hipLaunchKernelGGL(k_eg_linearize, dim3((D.ne + kEgLinEdges - 1) / kEgLinEdges), dim3(kEgThreads), 0, m.ls(), D.edges, est,
                       D.ne, D.fix_scale, D.recs);
    ORBMI_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_eg_reduce, dim3(1), dim3(kEgThreads), 0, m.ls(), (const double*)(D.recs + kEgRecChi), D.ne, kEgRec,
                       D.out + kEgOutChi);
    ORBMI_HIP(hipGetLastError());
    return ORBMI_OK;
}

int launch_eg_assemble(Matcher& m, const EgDev& D) {
    if (D.nf + D.nl <= 0) return ORBMI_OK;
    hipLaunchKernelGGL(k_eg_assemble, dim3(D.nf + D.nl), dim3(64), 0, m.ls(), D);
    ORBMI_HIP(hipGetLastError());
    return ORBMI_OK;
}

int launch_eg_factor_solve(Matcher& m, const EgDev& D, double lambda) {
    hipLaunchKernelGGL(k_eg_factor_solve, dim3(1), dim3(kEgThreads), 0, m.ls(), D, lambda);
    ORBMI_HIP(hipGetLastError());
    return ORBMI_OK;
}

int launch_eg_update(Matcher& m, const EgDev& D, const Sim3d* est, Sim3d* trial) {
    if (D.nf <= 0 || D.ne <= 0) return ORBMI_OK;
    hipLaunchKernelGGL(k_eg_update, dim3((D.nf + 63) / 64), dim3(64), 0, m.ls(), D, est, trial);
    ORBMI_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_eg_chi2, dim3((D.ne + 63) / 64), dim3(64), 0, m.ls(), D, (const Sim3d*)trial);
    ORBMI_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_eg_reduce, dim3(1), dim3(kEgThreads), 0, m.ls(), (const double*)D.chi2, D.ne, 1, D.out + kEgOutChi);
    ORBMI_HIP(hipGetLastError());
    return ORBMI_OK;
}

int launch_eg_correct(Matcher& m, int npoints, const float* points, const int32_t* ref, const Sim3d* Srw, const Sim3d* Swr,
                      float* out_points, int nposes, const Sim3d* poses, float* out_tcw) {
    const int n = npoints > nposes ? npoints : nposes;
    if (n <= 0) return ORBMI_OK;
    hipLaunchKernelGGL(k_eg_correct, dim3((n + kEgThreads - 1) / kEgThreads), dim3(kEgThreads), 0, m.ls(), npoints, points, ref,
                       Srw, Swr, out_points, nposes, poses, out_tcw);
    ORBMI_HIP(hipGetLastError());
    return ORBMI_OK;
}

}  // namespace orbmi
