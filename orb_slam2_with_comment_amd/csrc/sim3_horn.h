// The arithmetic of ORB_SLAM2::Sim3Solver (src/Sim3Solver.cc), shared by the device kernel
// (sim3.hip), the host entries (orbmi_sim3_iterations, orbmi_sim3_sample_triples), the C++ adapter
// and the CPU check program (tests/cpp/sim3_check.cpp); tests/sim3_reference.py restates it in
// numpy operation for operation.  Only +, -, *, /, sqrt and comparisons are used, one IEEE rounding
// per operation in the order written (-ffp-contract=off, pinned semantics P7), so host, device and
// numpy agree bit for bit.
//
// Deviations from the reference (parity-unpinned against OpenCV):
//  * ComputeSim3 keeps its intermediates (centroids, M, N, R, s, t) in fp64 and rounds T12 / T21
//    once to float32; the reference rounds every cv::Mat intermediate to float32.
//  * The eigenvector of N comes from a cyclic Jacobi of kSim3Sweeps sweeps, not cv::eigen.
//  * R is built from the unit quaternion directly: the reference's quaternion -> angle-axis ->
//    cv::Rodrigues route without its 0/0 for an identity rotation.
#pragma once
#include <math.h>
#include <stdint.h>

#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif

namespace orbmi {

constexpr int kSim3Sweeps = 8;  // fixed: terminates on any input, non-finite included

// One hypothesis: rows 0-2 of T12 = [s R | t] and T21 = [R^T / s | -R^T t / s] (row-major 3x4)
struct Sim3Hyp {
    float T12[12], T21[12];
    float s;
};

__host__ __device__ inline double sim3_abs(double x) { return x < 0 ? -x : x; }

// Sim3Solver::ComputeSim3 (src/Sim3Solver.cc:239-351).  P1, P2: the three points of the minimal
// set in camera 1 / camera 2, point-major (P[3 * i + r]).
__host__ __device__ inline void sim3_horn(const float* P1, const float* P2, int fix_scale, Sim3Hyp* out) {
    // Step 1: centroids and relative coordinates
    double O1[3], O2[3], Pr1[3][3], Pr2[3][3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        O1[r] = (((double)P1[r] + (double)P1[3 + r]) + (double)P1[6 + r]) / 3.0;
        O2[r] = (((double)P2[r] + (double)P2[3 + r]) + (double)P2[6 + r]) / 3.0;
    }
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int r = 0; r < 3; r++) {
            Pr1[i][r] = (double)P1[3 * i + r] - O1[r];
            Pr2[i][r] = (double)P2[3 * i + r] - O2[r];
        }
    // Step 2: M = Pr2 * Pr1^T (sum over the points in order)
    double M[3][3];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) M[r][c] = (Pr2[0][r] * Pr1[0][c] + Pr2[1][r] * Pr1[1][c]) + Pr2[2][r] * Pr1[2][c];
    // Step 3: N (:261-279)
    double A[4][4], V[4][4];
    A[0][0] = (M[0][0] + M[1][1]) + M[2][2];
    A[0][1] = M[1][2] - M[2][1];
    A[0][2] = M[2][0] - M[0][2];
    A[0][3] = M[0][1] - M[1][0];
    A[1][1] = (M[0][0] - M[1][1]) - M[2][2];
    A[1][2] = M[0][1] + M[1][0];
    A[1][3] = M[2][0] + M[0][2];
    A[2][2] = (-M[0][0] + M[1][1]) - M[2][2];
    A[2][3] = M[1][2] + M[2][1];
    A[3][3] = (-M[0][0] - M[1][1]) + M[2][2];
#pragma unroll
    for (int p = 0; p < 4; p++)
#pragma unroll
        for (int q = 0; q < 4; q++) {
            if (q < p) A[p][q] = A[q][p];
            V[p][q] = p == q ? 1.0 : 0.0;
        }
    // Step 4: eigenvector of the largest eigenvalue.  Cyclic Jacobi, pairs (0,1) (0,2) (0,3) (1,2)
    // (1,3) (2,3); p, q, k unrolled so every index is static and the matrices stay in registers on
    // the device (as tri_geom.h null_vector4)
    for (int sweep = 0; sweep < kSim3Sweeps; sweep++) {
#pragma unroll
        for (int p = 0; p < 4; p++)
#pragma unroll
            for (int q = p + 1; q < 4; q++) {
                if (A[p][q] == 0) continue;
                const double theta = (A[q][q] - A[p][p]) / (2 * A[p][q]);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (sim3_abs(theta) + __builtin_sqrt(theta * theta + 1));
                const double c = 1 / __builtin_sqrt(t * t + 1), s = t * c;
#pragma unroll
                for (int k = 0; k < 4; k++) {  // A <- J^T A J: columns, then rows
                    const double akp = A[k][p], akq = A[k][q];
                    A[k][p] = c * akp - s * akq;
                    A[k][q] = s * akp + c * akq;
                }
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const double apk = A[p][k], aqk = A[q][k];
                    A[p][k] = c * apk - s * aqk;
                    A[q][k] = s * apk + c * aqk;
                }
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - s * vkq;
                    V[k][q] = s * vkp + c * vkq;
                }
            }
    }
    double best = A[0][0], qw = V[0][0], qx = V[1][0], qy = V[2][0], qz = V[3][0];
#pragma unroll
    for (int i = 1; i < 4; i++)
        if (A[i][i] > best) { best = A[i][i]; qw = V[0][i]; qx = V[1][i]; qy = V[2][i]; qz = V[3][i]; }
    const double qn = __builtin_sqrt(((qw * qw + qx * qx) + qy * qy) + qz * qz);
    qw = qw / qn; qx = qx / qn; qy = qy / qn; qz = qz / qn;
    // R of the unit quaternion (w, x, y, z); the sign of q does not matter
    double R[3][3];
    R[0][0] = 1.0 - 2.0 * (qy * qy + qz * qz);
    R[0][1] = 2.0 * (qx * qy - qw * qz);
    R[0][2] = 2.0 * (qx * qz + qw * qy);
    R[1][0] = 2.0 * (qx * qy + qw * qz);
    R[1][1] = 1.0 - 2.0 * (qx * qx + qz * qz);
    R[1][2] = 2.0 * (qy * qz - qw * qx);
    R[2][0] = 2.0 * (qx * qz - qw * qy);
    R[2][1] = 2.0 * (qy * qz + qw * qx);
    R[2][2] = 1.0 - 2.0 * (qx * qx + qy * qy);
    // Step 5-6: rotate set 2; s = <Pr1, P3> / <P3, P3> (:306-325), summed point by point
    double nom = 0.0, den = 0.0;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int r = 0; r < 3; r++) {
            const double p3 = (R[r][0] * Pr2[i][0] + R[r][1] * Pr2[i][1]) + R[r][2] * Pr2[i][2];
            nom = nom + Pr1[i][r] * p3;
            den = den + p3 * p3;
        }
    // den == 0: three coincident points fix no rotation.  den / den is then NaN, which marks the
    // hypothesis in both modes (the reference's R is NaN there, from norm(vec) == 0 at :294)
    const double s = fix_scale ? den / den : nom / den;
    // Step 7-8: t12 = O1 - sR12 O2, sR21 = (1/s) R^T, t21 = -sR21 t12
    double sR12[3][3], sR21[3][3], t12[3], t21[3];
    const double inv = 1.0 / s;
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            sR12[r][c] = s * R[r][c];
            sR21[r][c] = inv * R[c][r];
        }
#pragma unroll
    for (int r = 0; r < 3; r++) t12[r] = O1[r] - ((sR12[r][0] * O2[0] + sR12[r][1] * O2[1]) + sR12[r][2] * O2[2]);
#pragma unroll
    for (int r = 0; r < 3; r++) t21[r] = -((sR21[r][0] * t12[0] + sR21[r][1] * t12[1]) + sR21[r][2] * t12[2]);
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            out->T12[4 * r + c] = (float)sR12[r][c];
            out->T21[4 * r + c] = (float)sR21[r][c];
        }
        out->T12[4 * r + 3] = (float)t12[r];
        out->T21[4 * r + 3] = (float)t21[r];
    }
    out->s = (float)s;
}

// Sim3Solver::Project (:396-417) of one point, float32: Rcw X + tcw, invz = 1 / z, fx x + cx.
// k = fx fy cx cy.  No depth-sign test: the reference has none.
__host__ __device__ inline void sim3_project(const float* T, const float* X, const float* k, float* u, float* v) {
    const float px = ((T[0] * X[0] + T[1] * X[1]) + T[2] * X[2]) + T[3];
    const float py = ((T[4] * X[0] + T[5] * X[1]) + T[6] * X[2]) + T[7];
    const float pz = ((T[8] * X[0] + T[9] * X[1]) + T[10] * X[2]) + T[11];
    const float invz = 1.0f / pz;
    *u = k[0] * (px * invz) + k[2];
    *v = k[1] * (py * invz) + k[3];
}

// Sim3Solver::FromCameraToImage (:419-437) of one point
__host__ __device__ inline void sim3_to_image(const float* X, const float* k, float* u, float* v) {
    const float invz = 1.0f / X[2];
    *u = k[0] * (X[0] * invz) + k[2];
    *v = k[1] * (X[1] * invz) + k[3];
}

// Sim3Solver::CheckInliers (:354-378) of one correspondence.  A NaN fails both comparisons.
__host__ __device__ inline bool sim3_is_inlier(const Sim3Hyp& h, const float* X1, const float* X2, const float* k1,
                                               const float* k2, int32_t max_err1, int32_t max_err2) {
    float u11, v11, u21, v21, u12, v12, u22, v22;
    sim3_to_image(X1, k1, &u11, &v11);         // mvP1im1
    sim3_project(h.T12, X2, k1, &u21, &v21);   // vP2im1
    sim3_project(h.T21, X1, k2, &u12, &v12);   // vP1im2
    sim3_to_image(X2, k2, &u22, &v22);         // mvP2im2
    const float dx1 = u11 - u21, dy1 = v11 - v21, dx2 = u12 - u22, dy2 = v12 - v22;
    const float err1 = dx1 * dx1 + dy1 * dy1, err2 = dx2 * dx2 + dy2 * dy2;
    return err1 < (float)max_err1 && err2 < (float)max_err2;
}

// mvnMaxError (:87-88): 9.210 * sigmaSquare stored into a vector<size_t>
// (include/Sim3Solver.h:79-80), so the product truncates to an integer
__host__ __device__ inline int32_t sim3_max_error(float sigma_square) { return (int32_t)(9.210 * (double)sigma_square); }

// The minimal-set sampler.  The reference draws from DUtils::Random (srand-seeded, not
// reproducible); the library defines its own counter-based generator instead: draw d (0-2) of
// iteration `it` of solver `solver` is
//     mix(seed ^ mix(solver << 40 ^ it << 2 ^ d))
// with mix the 64-bit finaliser of splitmix64 applied to x + 0x9E3779B97F4A7C15.  The draw is
// reduced modulo the number of available indices (a bias below 2^-50 at n <= 2^14).
inline uint64_t sim3_mix(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

inline uint64_t sim3_draw(uint64_t seed, int solver, int it, int d) {
    return sim3_mix(seed ^ sim3_mix((uint64_t)(uint32_t)solver << 40 ^ (uint64_t)(uint32_t)it << 2 ^ (uint64_t)d));
}

// :167-185: draw from the available indices, swap with the back and pop, three times.  `avail` is
// scratch of n ints; n >= 3.
inline void sim3_sample_triple(uint64_t seed, int solver, int it, int n, int32_t* avail, int32_t out[3]) {
    for (int i = 0; i < n; i++) avail[i] = i;
    int m = n;
    for (int d = 0; d < 3; d++) {
        const int randi = (int)(sim3_draw(seed, solver, it, d) % (uint64_t)m);
        out[d] = avail[randi];
        avail[randi] = avail[m - 1];
        m--;
    }
}

// Sim3Solver::SetRansacParameters (:114-138): the iteration count, clamped to [1, max_its].
// n < min_inliers -> 0 (iterate returns bNoMore at once, :147-151).  Host only (libm's log, pow).
// The reference converts ceil(...) to int unchecked; here a value that is not >= 1 (NaN, -inf
// from epsilon = 0) gives 1, which is what the clamp makes of x86's INT_MIN.
inline int sim3_iterations(int n, int min_inliers, double probability, int max_its) {
    if (n < min_inliers) return 0;
    double v = 1.0;
    if (min_inliers != n) {
        const float epsilon = (float)min_inliers / n;
        v = ceil(log(1 - probability) / log(1 - pow((double)epsilon, 3.0)));
    }
    if (v >= (double)max_its) return max_its > 1 ? max_its : 1;
    return v >= 1.0 ? (int)v : 1;
}

}  // namespace orbmi
