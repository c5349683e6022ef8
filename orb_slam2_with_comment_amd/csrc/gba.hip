// Optimizer::BundleAdjustment (src/Optimizer.cc:56-255) on MI355X, fp64: global bundle adjustment
// over any number of keyframes.
//
// One SparseOptimizer::optimize(n) with OptimizationAlgorithmLevenberg over BlockSolver_6_3.  The
// Levenberg decisions are taken on the host from one small read-back per trial, by
// g2o_lm.h; the graph's index tables and pair lists are ba_graph.h's, shared with LocalBA; the
// arithmetic runs in these kernels, all on the handle's stream:
//   per iteration
//     k_gba_linearize  thread / edge    error, robust chi2, Jacobians, the edge's blocks (ba_edge.h)
//     k_gba_reduce     thread / entry   H_ll, b_l per point in edge order; H_pp, b_p per keyframe
//                                       gathered over its edge list in edge order; |diag H|
//   per trial (lambda)
//     k_gba_prep       thread / point   D^-1 = (H_ll + lambda I)^-1, D^-1 b_l, Y = B D^-1 per edge
//     k_gba_schur      wave / block     S_ij = [H_pp + lambda I] - sum_p Y_ip B_jp^T over the block's
//                                       host-built pair list (point order), b_S on the diagonal blocks
//     k_gba_panel      one workgroup    LDL^T of a 48 x 48 diagonal block (unpivoted)
//     k_gba_rows       thread / row     the rows below it: W = A L11^-T, L = W D^-1 (b rides as a row)
//     k_gba_trail      wave / tile      S22 -= L W^T, 16 x 16 tiles on v_mfma_f64_16x16x4_f64
//     k_gba_back       per panel, in reverse: L11^T x = z, then z -= L^T x for the columns to its left
//     k_gba_update     thread / vertex  oplus into the trial buffers, computeScale terms
//     k_gba_chi        thread / edge    robust chi2 at the trial
//     k_gba_sum        one workgroup each: chi2 and computeScale in a fixed order
// S is dense: the lower triangle of 16 x 16 tiles, each tile contiguous in the MFMA's C layout, with
// one more tile row that carries b (then z, then nothing: x goes to its own vector).
// Compiled under the build's -ffp-contract=off; no floating-point atomics; every sum has a fixed
// order, so two calls return the same bits.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "ba_edge.h"
#include "ba_graph.h"
#include "ba_handle.h"
#include "g2o_lm.h"

namespace orbmi {

constexpr int kGbaMaxFreePoses = ORBMI_GBA_MAX_FREE_POSES;
constexpr int kGbaThreads = 256;
constexpr int kGbaTile = 16;                       // scalars: the MFMA tile
constexpr int kGbaPanel = 48;                      // scalars: lcm(6, 16) = 8 poses = 3 tiles
constexpr int kGbaPanelTiles = kGbaPanel / kGbaTile;
constexpr int kGbaRowsThreads = 64;
constexpr long long kGbaMaxPairs = 1LL << 28;

typedef double gba_d4 __attribute__((ext_vector_type(4)));

enum { kGbaOutChi = 0, kGbaOutScale = 1, kGbaOutFail = 2, kGbaOutMax = 3, kGbaOutN = 8 };

struct GbaDev {
    int nkf, npt, ne, nf, nblk;
    int N, Npad, NT;            // 6 nf; padded to panels; tiles per dimension (Npad / 16)
    int robust;
    const orbmi_ba_keyframe* kfs;
    const orbmi_ba_point* pts;
    const orbmi_ba_edge* edges;
    const int* pt_start;        // npt + 1: edges of point p
    const int* kf_start;        // nkf + 1: CSR by keyframe over edge indices, in edge order
    const int* kf_edges;        // ne
    const int* kf_pos;          // ne: position of edge e in the keyframe CSR
    const int* rank;            // nkf: index of the keyframe's pose block, -1 = not in the system
    const int* free_kf;         // nf
    const int* blk_ij;          // nblk x 2: pose blocks (i >= j) with at least one pair
    const int* blk_start;       // nblk + 1
    const int2* blk_pairs;      // (edge into i, edge into j) of one point, in point order
    double* Hpl;                // ne x 18
    double* Hle;                // ne x 9
    double* Hpe;                // ne x 27, keyframe-CSR order
    double* Hll;                // npt x 9
    double* bl;                 // npt x 3
    double* Hpp;                // nf x 27: upper triangle (21) + b_p (6)
    double* Dinv;               // npt x 9
    double* db;                 // npt x 3: D^-1 b_l
    double* Y;                  // ne x 18: B D^-1
    double* vmax;               // 6 nf + npt: |diag H|
    double* S;                  // tiles
    double* dinv;               // Npad: 1 / d of the factor
    double* Wb;                 // (Npad + 16) x 48: the panel's W rows
    double* Lb;                 // (Npad + 16) x 48: the panel's L rows
    double* x;                  // Npad
    double* sc;                 // nf + npt: computeScale terms
    double* chi_e;              // ne
    double* out;                // kGbaOutN
};

__host__ __device__ inline size_t gba_tile(int I, int J) { return (size_t)I * (I + 1) / 2 + J; }  // I >= J
__host__ __device__ inline int gba_tpos(int rr, int cc) { return (rr >> 2) * 64 + 16 * (rr & 3) + cc; }
__device__ inline double* gba_at(const GbaDev& a, int R, int C) {  // R >= C
    return a.S + gba_tile(R >> 4, C >> 4) * 256 + gba_tpos(R & 15, C & 15);
}
__device__ inline int upper6(int r, int c) { return r * 6 - r * (r - 1) / 2 + (c - r); }  // r <= c

// vertices: SE3Quat from float Tcw, points to double, into both estimate buffers
__global__ __launch_bounds__(kGbaThreads) void k_gba_setup(GbaDev a, double* __restrict__ T0, double* __restrict__ T1,
                                                           double* __restrict__ X0, double* __restrict__ X1) {
    const int i = blockIdx.x * kGbaThreads + threadIdx.x;
    if (i < a.nkf) {
        double Ti[8];
        tcw_to_se3(a.kfs[i].tcw, Ti);
        for (int q = 0; q < 8; q++) { T0[8 * (size_t)i + q] = Ti[q]; T1[8 * (size_t)i + q] = Ti[q]; }
    }
    if (i < a.npt)
        for (int r = 0; r < 4; r++) {
            const double v = r < 3 ? (double)a.pts[i].pos[r] : 0.0;
            X0[4 * (size_t)i + r] = v;
            X1[4 * (size_t)i + r] = v;
        }
}

__device__ inline unsigned char gba_flags(const GbaDev& a) { return a.robust ? 4 : 6; }

__global__ __launch_bounds__(kGbaThreads) void k_gba_linearize(GbaDev a, const double* __restrict__ T,
                                                               const double* __restrict__ X) {
    const int i = blockIdx.x * kGbaThreads + threadIdx.x;
    if (i >= a.ne) return;
    const orbmi_ba_edge e = a.edges[i];
    const BaCam cam = ba_cam(a.kfs[e.kf]);
    const BaHuber h = ba_huber_global();
    const unsigned char fl = gba_flags(a);
    double Tk[8], Xp[3], err[3], r0, r1;
    for (int q = 0; q < 8; q++) Tk[q] = T[8 * (size_t)e.kf + q];
    for (int q = 0; q < 3; q++) Xp[q] = X[4 * (size_t)e.point + q];
    edge_err_math(e, cam, Tk, Xp, err);
    edge_robust_math(fl, e, h, edge_chi2_math(e, err), &r0, &r1);
    a.chi_e[i] = r0;
    edge_blocks_math(e, cam, Tk, fl, h, err, Xp, a.rank[e.kf] >= 0, a.Hle + 9 * (size_t)i, a.Hpl + 18 * (size_t)i,
                     a.Hpe + 27 * (size_t)a.kf_pos[i]);
}

// thread t < npt: the point's H_ll / b_l; thread npt + 27 i + q: entry q of pose block i
__global__ __launch_bounds__(kGbaThreads) void k_gba_reduce(GbaDev a) {
    const long long t = (long long)blockIdx.x * kGbaThreads + threadIdx.x;
    if (t < a.npt) {
        const int p = (int)t, e0 = a.pt_start[p], e1 = a.pt_start[p + 1];
        double s[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int e = e0; e < e1; e++)
            for (int q = 0; q < 9; q++) s[q] = s[q] + a.Hle[9 * (size_t)e + q];
        double* H = a.Hll + 9 * (size_t)p;
        H[0] = s[0]; H[1] = s[1]; H[2] = s[2]; H[3] = s[1]; H[4] = s[3]; H[5] = s[4]; H[6] = s[2]; H[7] = s[4]; H[8] = s[5];
        for (int r = 0; r < 3; r++) a.bl[3 * (size_t)p + r] = s[6 + r];
        a.vmax[6 * (size_t)a.nf + p] = fmax(fabs(s[0]), fmax(fabs(s[3]), fabs(s[5])));
        return;
    }
    const long long u = t - a.npt;
    if (u >= 27LL * a.nf) return;
    const int i = (int)(u / 27), q = (int)(u % 27), kf = a.free_kf[i];
    double s = 0;
    for (int j = a.kf_start[kf]; j < a.kf_start[kf + 1]; j++) s = s + a.Hpe[27 * (size_t)j + q];
    a.Hpp[27 * (size_t)i + q] = s;
    for (int d = 0; d < 6; d++)
        if (q == upper6(d, d)) a.vmax[6 * (size_t)i + d] = fabs(s);
}

// computeLambdaInit's max |diag H| (a maximum does not depend on the order)
__global__ __launch_bounds__(kGbaThreads) void k_gba_max(GbaDev a) {
    __shared__ double red[kGbaThreads];
    double m = 0;
    const long long n = 6LL * a.nf + a.npt;
    for (long long i = threadIdx.x; i < n; i += kGbaThreads) m = fmax(m, a.vmax[i]);
    m = block_reduce_fixed<kGbaThreads>(m, red, [](double x, double y) { return fmax(x, y); });
    if (threadIdx.x == 0) a.out[kGbaOutMax] = m;
}

// block 0: the chi2 of the edges; block 1: computeScale over every free vertex
__global__ __launch_bounds__(kGbaThreads) void k_gba_sum(GbaDev a) {
    __shared__ double red[kGbaThreads];
    const double* src = blockIdx.x == 0 ? a.chi_e : a.sc;
    const long long n = blockIdx.x == 0 ? a.ne : (long long)a.nf + a.npt;
    const double t = strided_sum_fixed<kGbaThreads>(src, n, 1, red);
    if (threadIdx.x == 0) a.out[blockIdx.x == 0 ? kGbaOutChi : kGbaOutScale] = t;
}

__global__ __launch_bounds__(kGbaThreads) void k_gba_prep(GbaDev a, double lam) {
    const int p = blockIdx.x * kGbaThreads + threadIdx.x;
    if (p == 0) a.out[kGbaOutFail] = 0.0;
    // the padding of the last panel: unit pivots (S was cleared)
    if (p < a.Npad - a.N) *gba_at(a, a.N + p, a.N + p) = 1.0;
    if (p >= a.npt) return;
    const int e0 = a.pt_start[p], e1 = a.pt_start[p + 1];
    if (e0 == e1) return;
    double Di[9];
    point_dinv(a.Hll, p, lam, Di);
    for (int q = 0; q < 9; q++) a.Dinv[9 * (size_t)p + q] = Di[q];
    const double* b = a.bl + 3 * (size_t)p;
    for (int r = 0; r < 3; r++) a.db[3 * (size_t)p + r] = Di[r * 3] * b[0] + Di[r * 3 + 1] * b[1] + Di[r * 3 + 2] * b[2];
    for (int e = e0; e < e1; e++) {
        if (a.rank[a.edges[e].kf] < 0) continue;
        const double* B = a.Hpl + 18 * (size_t)e;
        double* Y = a.Y + 18 * (size_t)e;
        for (int r = 0; r < 6; r++)
            for (int c = 0; c < 3; c++) Y[r * 3 + c] = B[r * 3] * Di[c] + B[r * 3 + 1] * Di[3 + c] + B[r * 3 + 2] * Di[6 + c];
    }
}

// One wave per non-zero 6 x 6 block (i >= j): lane q < 36 sums entry (q / 6, q % 6) over the block's
// pair list in point order; on a diagonal block lanes 36..41 form b_S over the keyframe's edges
__global__ __launch_bounds__(64) void k_gba_schur(GbaDev a, double lam) {
    const int b = blockIdx.x, q = threadIdx.x;
    const int i = a.blk_ij[2 * b], j = a.blk_ij[2 * b + 1];
    if (q < 36) {
        const int r = q / 6, c = q % 6;
        double s = 0;
        if (i == j) s = a.Hpp[27 * (size_t)i + (r <= c ? upper6(r, c) : upper6(c, r))] + (r == c ? lam : 0.0);
        for (int t = a.blk_start[b]; t < a.blk_start[b + 1]; t++) {
            const int2 pr = a.blk_pairs[t];
            const double* Y = a.Y + 18 * (size_t)pr.x + 3 * r;
            const double* B = a.Hpl + 18 * (size_t)pr.y + 3 * c;
            s = s - (Y[0] * B[0] + Y[1] * B[1] + Y[2] * B[2]);
        }
        const int R = 6 * i + r, C = 6 * j + c;
        if (R >= C) *gba_at(a, R, C) = s;
    } else if (q < 42 && i == j) {
        const int r = q - 36, kf = a.free_kf[i];
        double s = a.Hpp[27 * (size_t)i + 21 + r];
        for (int t = a.kf_start[kf]; t < a.kf_start[kf + 1]; t++) {
            const int e = a.kf_edges[t];
            const double* B = a.Hpl + 18 * (size_t)e + 3 * r;
            const double* d = a.db + 3 * (size_t)a.edges[e].point;
            s = s - (B[0] * d[0] + B[1] * d[1] + B[2] * d[2]);
        }
        *gba_at(a, 16 * a.NT, 6 * i + r) = s;  // row 0 of the extra tile row
    }
}

// LDL^T of the diagonal block of panel k (48 x 48, lower triangle) in LDS, unpivoted.  A pivot that
// is not a positive finite number raises the failure flag; its column is zeroed so that the rest of
// the launch sequence runs on finite numbers (the host discards the step).
__global__ __launch_bounds__(kGbaThreads) void k_gba_panel(GbaDev a, int k) {
    __shared__ double A[kGbaPanel][kGbaPanel + 1];
    __shared__ double inv_s[kGbaPanel];
    const int tid = threadIdx.x, c0 = kGbaPanel * k;
    for (int idx = tid; idx < kGbaPanel * kGbaPanel; idx += kGbaThreads) {
        const int r = idx / kGbaPanel, c = idx % kGbaPanel;
        A[r][c] = r >= c ? *gba_at(a, c0 + r, c0 + c) : 0.0;
    }
    for (int c = 0; c < kGbaPanel; c++) {
        __syncthreads();
        const double d = A[c][c];
        const bool ok = d > 0.0 && isfinite(d);
        const double inv = ok ? 1.0 / d : 0.0;
        for (int idx = tid; idx < kGbaPanel * kGbaPanel; idx += kGbaThreads) {
            const int r = idx / kGbaPanel, c2 = idx % kGbaPanel;
            if (c2 > c && r >= c2) A[r][c2] = A[r][c2] - (A[r][c] * inv) * A[c2][c];
        }
        __syncthreads();
        if (tid > c && tid < kGbaPanel) A[tid][c] = A[tid][c] * inv;
        if (tid == 0) {
            inv_s[c] = inv;
            if (!ok) a.out[kGbaOutFail] = 1.0;
        }
    }
    __syncthreads();
    for (int idx = tid; idx < kGbaPanel * kGbaPanel; idx += kGbaThreads) {
        const int r = idx / kGbaPanel, c = idx % kGbaPanel;
        if (r >= c) *gba_at(a, c0 + r, c0 + c) = A[r][c];
    }
    if (tid < kGbaPanel) a.dinv[c0 + tid] = inv_s[tid];
}

// The rows below panel k, the extra tile row included, one per thread: W = A L11^-T by forward
// substitution in registers, L = W D^-1.  L goes back into S and, with W, into the panel's row
// buffers that k_gba_trail reads.
__global__ __launch_bounds__(kGbaRowsThreads) void k_gba_rows(GbaDev a, int k) {
    __shared__ double L[kGbaPanel][kGbaPanel + 1];
    __shared__ double inv_s[kGbaPanel];
    const int tid = threadIdx.x, c0 = kGbaPanel * k, R0 = c0 + kGbaPanel;
    for (int idx = tid; idx < kGbaPanel * kGbaPanel; idx += kGbaRowsThreads) {
        const int r = idx / kGbaPanel, c = idx % kGbaPanel;
        L[r][c] = r > c ? *gba_at(a, c0 + r, c0 + c) : 0.0;
    }
    if (tid < kGbaPanel) inv_s[tid] = a.dinv[c0 + tid];
    __syncthreads();
    const int g = blockIdx.x * kGbaRowsThreads + tid;  // row R0 + g
    if (g >= a.Npad + kGbaTile - R0) return;
    const int R = R0 + g;
    double w[kGbaPanel];
#pragma unroll
    for (int c = 0; c < kGbaPanel; c++) w[c] = *gba_at(a, R, c0 + c);
#pragma unroll
    for (int c = 1; c < kGbaPanel; c++)
#pragma unroll
        for (int j = 0; j < c; j++) w[c] = w[c] - w[j] * L[c][j];
    double* wb = a.Wb + (size_t)g * kGbaPanel;
    double* lb = a.Lb + (size_t)g * kGbaPanel;
#pragma unroll
    for (int c = 0; c < kGbaPanel; c++) {
        const double l = w[c] * inv_s[c];
        wb[c] = w[c];
        lb[c] = l;
        *gba_at(a, R, c0 + c) = l;
    }
}

// S22 -= L W^T behind panel k: one wave per 16 x 16 tile (I >= J) of the trailing matrix and of the
// extra tile row, twelve v_mfma_f64_16x16x4_f64 in ascending k
__global__ __launch_bounds__(kGbaThreads) void k_gba_trail(GbaDev a, int k) {
    const int lane = threadIdx.x & 63;
    const long long t = (long long)blockIdx.x * (kGbaThreads / 64) + (threadIdx.x >> 6);
    const int J0 = kGbaPanelTiles * (k + 1), m = a.NT - J0;  // m tile rows, then the extra one
    const long long ntri = (long long)m * (m + 1) / 2;
    if (t >= ntri + m) return;
    int I, J;
    if (t >= ntri) {
        I = m;
        J = (int)(t - ntri);
    } else {
        I = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
        while ((long long)I * (I + 1) / 2 > t) I--;
        while ((long long)(I + 1) * (I + 2) / 2 <= t) I++;
        J = (int)(t - (long long)I * (I + 1) / 2);
    }
    const int n = lane & 15, q = lane >> 4;
    const double* lp = a.Lb + ((size_t)16 * I + n) * kGbaPanel + q;
    const double* wp = a.Wb + ((size_t)16 * J + n) * kGbaPanel + q;
    double* dst = a.S + gba_tile(J0 + I, J0 + J) * 256 + lane;
    double lo[12], wo[12];
#pragma unroll
    for (int s = 0; s < 12; s++) { lo[s] = -lp[4 * s]; wo[s] = wp[4 * s]; }
    gba_d4 X;
#pragma unroll
    for (int s = 0; s < 4; s++) X[s] = dst[64 * s];
#pragma unroll
    for (int s = 0; s < 12; s++) X = __builtin_amdgcn_mfma_f64_16x16x4f64(lo[s], wo[s], X, 0, 0, 0);
#pragma unroll
    for (int s = 0; s < 4; s++) dst[64 * s] = X[s];
}

// Back substitution of panel k (launched for k = last .. 0): every workgroup solves L11^T x_k = z_k
// for itself in LDS (48 steps), workgroup 0 keeps x_k; then thread per column to the panel's left:
// z -= L_k^T x_k in ascending row order
__global__ __launch_bounds__(kGbaRowsThreads) void k_gba_back(GbaDev a, int k) {
    __shared__ double L[kGbaPanel][kGbaPanel + 1];
    __shared__ double xs[kGbaPanel];
    const int tid = threadIdx.x, c0 = kGbaPanel * k, Z = 16 * a.NT;
    for (int idx = tid; idx < kGbaPanel * kGbaPanel; idx += kGbaRowsThreads) {
        const int r = idx / kGbaPanel, c = idx % kGbaPanel;
        L[r][c] = r > c ? *gba_at(a, c0 + r, c0 + c) : 0.0;
    }
    if (tid < kGbaPanel) xs[tid] = *gba_at(a, Z, c0 + tid);
    for (int c = kGbaPanel - 1; c > 0; c--) {
        __syncthreads();
        if (tid < c) xs[tid] = xs[tid] - L[c][tid] * xs[c];
    }
    __syncthreads();
    if (blockIdx.x == 0 && tid < kGbaPanel) a.x[c0 + tid] = xs[tid];
    const int col = blockIdx.x * kGbaRowsThreads + tid;
    if (col >= c0) return;
    double z = *gba_at(a, Z, col);
    for (int r = 0; r < kGbaPanel; r++) z = z - *gba_at(a, c0 + r, col) * xs[r];
    *gba_at(a, Z, col) = z;
}

// oplus into the trial buffers and the vertices' computeScale terms; a failed solve is x = 0
__global__ __launch_bounds__(kGbaThreads) void k_gba_update(GbaDev a, double lam, const double* __restrict__ Tc,
                                                            const double* __restrict__ Xc, double* __restrict__ Tt,
                                                            double* __restrict__ Xt) {
    const int i = blockIdx.x * kGbaThreads + threadIdx.x;
    const bool ok = a.out[kGbaOutFail] == 0.0;
    if (i < a.nf) {
        const int kf = a.free_kf[i];
        double u[6], To[8], s = 0;
        for (int r = 0; r < 6; r++) u[r] = ok ? a.x[6 * (size_t)i + r] : 0.0;
        for (int r = 0; r < 6; r++) s = s + u[r] * (lam * u[r] + a.Hpp[27 * (size_t)i + 21 + r]);
        To[7] = 0;
        se3_oplus(u, Tc + 8 * (size_t)kf, To);
        for (int r = 0; r < 8; r++) Tt[8 * (size_t)kf + r] = To[r];
        a.sc[i] = s;
    }
    if (i < a.npt) {
        const int p = i, e0 = a.pt_start[p], e1 = a.pt_start[p + 1];
        double s = 0;
        if (e0 < e1) {
            double cl[3] = {a.bl[3 * (size_t)p], a.bl[3 * (size_t)p + 1], a.bl[3 * (size_t)p + 2]};
            for (int e = e0; e < e1; e++) {
                const int pi = a.rank[a.edges[e].kf];
                if (pi < 0) continue;
                const double* B = a.Hpl + 18 * (size_t)e;
                for (int c = 0; c < 3; c++)
                    for (int r = 0; r < 6; r++) cl[c] = cl[c] - B[r * 3 + c] * (ok ? a.x[6 * (size_t)pi + r] : 0.0);
            }
            const double* Di = a.Dinv + 9 * (size_t)p;
            for (int r = 0; r < 3; r++) {
                const double xl = ok ? Di[r * 3] * cl[0] + Di[r * 3 + 1] * cl[1] + Di[r * 3 + 2] * cl[2] : 0.0;
                Xt[4 * (size_t)p + r] = Xc[4 * (size_t)p + r] + xl;
                s = s + xl * (lam * xl + a.bl[3 * (size_t)p + r]);
            }
        }
        a.sc[(size_t)a.nf + p] = s;
    }
}

__global__ __launch_bounds__(kGbaThreads) void k_gba_chi(GbaDev a, const double* __restrict__ T, const double* __restrict__ X) {
    const int i = blockIdx.x * kGbaThreads + threadIdx.x;
    if (i >= a.ne) return;
    const orbmi_ba_edge e = a.edges[i];
    double err[3], r0, r1;
    edge_err_math(e, ba_cam(a.kfs[e.kf]), T + 8 * (size_t)e.kf, X + 4 * (size_t)e.point, err);
    edge_robust_math(gba_flags(a), e, ba_huber_global(), edge_chi2_math(e, err), &r0, &r1);
    a.chi_e[i] = r0;
}

// write back (Converter::toCvMat); what the optimisation did not hold comes back as given
__global__ __launch_bounds__(kGbaThreads) void k_gba_finish(GbaDev a, const double* __restrict__ T, const double* __restrict__ X,
                                                            float* __restrict__ out_tcw, float* __restrict__ out_pos,
                                                            unsigned char* __restrict__ out_inc) {
    const int i = blockIdx.x * kGbaThreads + threadIdx.x;
    if (i < a.nkf) {
        float* o = out_tcw + 16 * (size_t)i;
        if (a.rank[i] >= 0) se3_to_tcw(T + 8 * (size_t)i, o);
        else
            for (int q = 0; q < 16; q++) o[q] = a.kfs[i].tcw[q];
    }
    if (i < a.npt) {
        const bool inc = a.pt_start[i] < a.pt_start[i + 1];
        out_inc[i] = inc ? 1 : 0;
        for (int r = 0; r < 3; r++) out_pos[3 * (size_t)i + r] = inc ? (float)X[4 * (size_t)i + r] : a.pts[i].pos[r];
    }
}

}  // namespace orbmi

using namespace orbmi;

static_assert(sizeof(BaPair) == sizeof(int2) && alignof(BaPair) <= alignof(int2), "BaPair goes up as the kernels' int2");

extern "C" int orbmi_bundle_adjustment(orbmi_ba* b, const orbmi_ba_problem* P, int iterations, int robust,
                                       orbmi_gba_result* R, const volatile int* stop) {
    if (!b || !P || !R || P->nkf < 0 || P->npt < 0 || P->nedge < 0) return ORBMI_E_ARG;
    if (iterations < 0 || iterations > ORBMI_GBA_MAX_ITERATIONS) return ORBMI_E_ARG;
    if ((P->nkf && (!P->kfs || !R->tcw)) || (P->npt && (!P->pts || !R->pos || !R->included)) || (P->nedge && !P->edges))
        return ORBMI_E_ARG;
    const int nkf = P->nkf, npt = P->npt, ne = P->nedge;
    // ---- the plan (ba_graph.h): the graph's index tables, the pose blocks in vertex (id) order --
    // the free keyframes that an edge names -- and the pair lists of the non-zero blocks of S
    std::vector<int> pt_start(npt + 1), kf_start(nkf + 1), kf_edges(ne), kf_pos(ne), order(nkf), rank(nkf), free_kf(nkf);
    int rc = ba_graph_index(*P, pt_start.data(), kf_start.data(), kf_edges.data(), kf_pos.data(), nullptr);
    if (rc) return rc;  // ORBMI_E_ARG: the edges' validation
    const int nf = ba_graph_rank(*P, kf_start.data(), order.data(), rank.data(), free_kf.data());
    if (nf > kGbaMaxFreePoses) return ORBMI_E_UNSUPPORTED;
    const long long npair = gba_pair_count(*P, pt_start.data(), rank.data());
    if (npair > kGbaMaxPairs) return ORBMI_E_UNSUPPORTED;
    std::vector<int> blk_ij, blk_start;
    std::vector<BaPair> pairs;
    gba_pair_lists(*P, pt_start.data(), rank.data(), npair, &blk_ij, &blk_start, &pairs);
    const int nblk = (int)blk_ij.size() / 2;
    if (!gba_plan_ok(*P, nf, pt_start.data(), kf_start.data(), kf_edges.data(), kf_pos.data(), rank.data(), free_kf.data(),
                     blk_ij, blk_start, pairs))
        return ORBMI_E_ARG;
    const int N = 6 * nf, Npad = (N + kGbaPanel - 1) / kGbaPanel * kGbaPanel, NT = Npad / kGbaTile, npanel = Npad / kGbaPanel;

    orbmi_ba& h = *b;
    ORBMI_HIP(hipSetDevice(h.device));
    hipStream_t s = h.stream;
    if (!h.h_gba) ORBMI_HIP(hipHostMalloc((void**)&h.h_gba, sizeof(double) * kGbaOutN));
    // ---- one device arena, sized from the problem: every slot once (ArenaWalk)
    GbaDev a;
    a.nkf = nkf; a.npt = npt; a.ne = ne; a.nf = nf; a.nblk = nblk;
    a.N = N; a.Npad = Npad; a.NT = NT;
    a.robust = robust ? 1 : 0;
    double *Tb[2], *Xb[2];
    float *o_tcw, *o_pos;
    uint8_t* o_inc;
    const size_t ntiles = gba_tile(NT, NT) + 1;  // the lower triangle and the extra tile row
    const size_t nE = (size_t)ne, nP = (size_t)npt, nK = (size_t)nkf, nF = (size_t)nf, nrow = (size_t)Npad + kGbaTile;
    auto slots = [&](ArenaWalk& A) {
        A(a.kfs, nK); A(a.pts, nP); A(a.edges, nE); A(a.pt_start, nP + 1); A(a.kf_start, nK + 1); A(a.kf_edges, nE);
        A(a.kf_pos, nE); A(a.rank, nK); A(a.free_kf, nF); A(a.blk_ij, 2 * (size_t)nblk); A(a.blk_start, (size_t)nblk + 1);
        A(a.blk_pairs, pairs.size());
        A(Tb[0], 8 * nK); A(Tb[1], 8 * nK); A(Xb[0], 4 * nP); A(Xb[1], 4 * nP); A(a.Hpl, 18 * nE); A(a.Hle, 9 * nE);
        A(a.Hpe, 27 * nE); A(a.Hll, 9 * nP); A(a.bl, 3 * nP); A(a.Hpp, 27 * nF); A(a.Dinv, 9 * nP); A(a.db, 3 * nP);
        A(a.Y, 18 * nE); A(a.vmax, 6 * nF + nP); A(a.S, 256 * ntiles); A(a.dinv, (size_t)Npad); A(a.Wb, kGbaPanel * nrow);
        A(a.Lb, kGbaPanel * nrow); A(a.x, (size_t)Npad); A(a.sc, nF + nP); A(a.chi_e, nE); A(a.out, (size_t)kGbaOutN);
        A(o_tcw, 16 * nK); A(o_pos, 3 * nP); A(o_inc, nP);
    };
    ArenaWalk size;
    slots(size);
    ORBMI_HIP(hipStreamSynchronize(s));
    if (size.off > h.cap) {
        if (h.d_buf) (void)hipFree(h.d_buf);
        h.d_buf = nullptr;
        h.cap = 0;
        ORBMI_HIP(hipMalloc((void**)&h.d_buf, size.off));
        h.cap = size.off;
    }
    ArenaWalk bind{h.d_buf};
    slots(bind);
    const struct { const void *dst, *src; size_t bytes; } ups[] = {
        {a.kfs, P->kfs, sizeof(orbmi_ba_keyframe) * nK}, {a.pts, P->pts, sizeof(orbmi_ba_point) * nP},
        {a.edges, P->edges, sizeof(orbmi_ba_edge) * nE}, {a.pt_start, pt_start.data(), 4 * (nP + 1)},
        {a.kf_start, kf_start.data(), 4 * (nK + 1)}, {a.kf_edges, kf_edges.data(), 4 * nE}, {a.kf_pos, kf_pos.data(), 4 * nE},
        {a.rank, rank.data(), 4 * nK}, {a.free_kf, free_kf.data(), 4 * nF}, {a.blk_ij, blk_ij.data(), 8 * (size_t)nblk},
        {a.blk_start, blk_start.data(), 4 * ((size_t)nblk + 1)}, {a.blk_pairs, pairs.data(), 8 * pairs.size()}};
    for (const auto& u : ups)
        if (u.bytes) ORBMI_HIP(hipMemcpyAsync(const_cast<void*>(u.dst), u.src, u.bytes, hipMemcpyHostToDevice, s));
    ORBMI_HIP(hipStreamSynchronize(s));  // the pageable sources have been read
    int cur = 0;

    auto blocks = [](long long n, int per) { return dim3((unsigned)std::max(1LL, (n + per - 1) / per)); };
    const int nmax = std::max(std::max(nkf, npt), ne);
    PhaseTimer ph(s, getenv("ORBMI_GBA_PROFILE") != nullptr);  // the phases' device time (a synchronisation per phase)
    double phase_ms[4] = {0, 0, 0, 0};  // (into the result on success only)
    ORBMI_HIP(hipMemsetAsync(a.out, 0, 8 * kGbaOutN, s));
    hipLaunchKernelGGL(k_gba_setup, blocks(nmax, kGbaThreads), dim3(kGbaThreads), 0, s, a, Tb[0], Tb[1], Xb[0], Xb[1]);
    ORBMI_HIP(hipGetLastError());
    double* const ho = h.h_gba;
    auto read_out = [&]() -> int {
        ORBMI_HIP(hipMemcpyAsync(ho, a.out, 8 * kGbaOutN, hipMemcpyDeviceToHost, s));
        ORBMI_HIP(hipStreamSynchronize(s));
        return (int)ORBMI_OK;
    };
    // computeActiveErrors + buildSystem at the current estimate
    auto linearize = [&]() -> int {
        ph.begin();
        if (ne) hipLaunchKernelGGL(k_gba_linearize, blocks(ne, kGbaThreads), dim3(kGbaThreads), 0, s, a, Tb[cur], Xb[cur]);
        hipLaunchKernelGGL(k_gba_reduce, blocks((long long)npt + 27LL * nf, kGbaThreads), dim3(kGbaThreads), 0, s, a);
        hipLaunchKernelGGL(k_gba_max, dim3(1), dim3(kGbaThreads), 0, s, a);
        hipLaunchKernelGGL(k_gba_sum, dim3(1), dim3(kGbaThreads), 0, s, a);  // block 0 only: the chi2
        ORBMI_HIP(hipGetLastError());
        ph.end(&phase_ms[0]);
        return (int)ORBMI_OK;
    };
    // one trial: solve at lambda, update into the other buffers, chi2 and computeScale there
    auto trial = [&](double lam) -> int {
        ph.begin();
        ORBMI_HIP(hipMemsetAsync(a.S, 0, 2048 * ntiles, s));
        hipLaunchKernelGGL(k_gba_prep, blocks(std::max(npt, Npad - N), kGbaThreads), dim3(kGbaThreads), 0, s, a, lam);
        if (nblk) hipLaunchKernelGGL(k_gba_schur, dim3(nblk), dim3(64), 0, s, a, lam);
        ORBMI_HIP(hipGetLastError());
        ph.end(&phase_ms[1]);
        ph.begin();
        for (int k = 0; k < npanel; k++) {
            hipLaunchKernelGGL(k_gba_panel, dim3(1), dim3(kGbaThreads), 0, s, a, k);
            const int rows = Npad + kGbaTile - kGbaPanel * (k + 1);
            hipLaunchKernelGGL(k_gba_rows, blocks(rows, kGbaRowsThreads), dim3(kGbaRowsThreads), 0, s, a, k);
            const long long m = NT - kGbaPanelTiles * (k + 1), nt = m * (m + 1) / 2 + m;
            if (nt > 0) hipLaunchKernelGGL(k_gba_trail, blocks(nt, kGbaThreads / 64), dim3(kGbaThreads), 0, s, a, k);
        }
        for (int k = npanel - 1; k >= 0; k--)
            hipLaunchKernelGGL(k_gba_back, blocks(kGbaPanel * k, kGbaRowsThreads), dim3(kGbaRowsThreads), 0, s, a, k);
        ORBMI_HIP(hipGetLastError());
        ph.end(&phase_ms[2]);
        ph.begin();
        hipLaunchKernelGGL(k_gba_update, blocks(std::max(nf, npt), kGbaThreads), dim3(kGbaThreads), 0, s, a, lam,
                           (const double*)Tb[cur], (const double*)Xb[cur], Tb[cur ^ 1], Xb[cur ^ 1]);
        if (ne) hipLaunchKernelGGL(k_gba_chi, blocks(ne, kGbaThreads), dim3(kGbaThreads), 0, s, a, (const double*)Tb[cur ^ 1],
                                   (const double*)Xb[cur ^ 1]);
        hipLaunchKernelGGL(k_gba_sum, dim3(2), dim3(kGbaThreads), 0, s, a);
        ORBMI_HIP(hipGetLastError());
        ph.end(&phase_ms[3]);
        return (int)ORBMI_OK;
    };

    // ---- SparseOptimizer::optimize(iterations) with OptimizationAlgorithmLevenberg::solve
    // (g2o_lm.h, with g2o's own std::pow cube), as oracle/lba_oracle.cpp:333-391 restates them
    int checks = 0, stop_seen = -1, status = 0, it = 0;
    auto terminate = [&]() {
        const int idx = checks++;
        const bool st = stop_set(stop) || (h.stop_at >= 0 && idx >= h.stop_at);
        if (st && stop_seen < 0) stop_seen = idx;
        return st;
    };
    for (int i = 0; i < ORBMI_GBA_MAX_ITERATIONS; i++) R->trials[i] = 0;
    S3oLm L{};
    double chi_initial = 0, chi_last = 0;
    const bool empty = ne == 0;  // no active vertex: optimize() returns before its loop
    for (int i = 0; !empty && i < iterations && !terminate(); i++) {
        if ((rc = linearize()) || (rc = read_out())) return rc;
        if (i == 0) chi_initial = ho[kGbaOutChi];
        lm_begin(L, i, ho[kGbaOutChi], [ho] { return 1e-5 * ho[kGbaOutMax]; });
        bool more;
        do {
            if ((rc = trial(L.lambda)) || (rc = read_out())) return rc;
            const bool ok2 = ho[kGbaOutFail] == 0.0;
            if (!ok2) status |= ORBMI_GBA_SOLVE_FAILED;
            chi_last = ho[kGbaOutChi];
            if (lm_trial(L, ok2, chi_last, ho[kGbaOutScale], &more, LmCubePow())) cur ^= 1;
            else status |= ORBMI_GBA_REJECTED;
            R->trials[i] = L.qmax;
        } while (more && !terminate());
        it++;
        if (lm_end(L)) { status |= ORBMI_GBA_TERMINATE; break; }
    }
    if (empty) status |= ORBMI_GBA_TERMINATE;
    hipLaunchKernelGGL(k_gba_finish, blocks(std::max(nkf, npt), kGbaThreads), dim3(kGbaThreads), 0, s, a, (const double*)Tb[cur],
                       (const double*)Xb[cur], o_tcw, o_pos, o_inc);
    ORBMI_HIP(hipGetLastError());
    if (nkf) ORBMI_HIP(hipMemcpyAsync(R->tcw, o_tcw, 64 * nK, hipMemcpyDeviceToHost, s));
    if (npt) ORBMI_HIP(hipMemcpyAsync(R->pos, o_pos, 12 * nP, hipMemcpyDeviceToHost, s));
    if (npt) ORBMI_HIP(hipMemcpyAsync(R->included, o_inc, nP, hipMemcpyDeviceToHost, s));
    ORBMI_HIP(hipStreamSynchronize(s));
    R->iterations = it;
    R->chi2_initial = chi_initial;
    R->chi2 = chi_last;
    R->stop_check = stop_seen;
    R->checks = checks;
    R->status = status;
    R->n_free = nf;
    R->n_blocks = nblk;
    for (int k = 0; k < 4; k++) R->phase_ms[k] = phase_ms[k];
    return ORBMI_OK;
}
