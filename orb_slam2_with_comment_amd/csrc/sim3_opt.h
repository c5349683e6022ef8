// The arithmetic of Optimizer::OptimizeSim3 (src/Optimizer.cc:1145-1347) with the bundled g2o's
// semantics, shared by the device kernel (sim3_opt.hip), the CPU check program
// (tests/cpp/sim3opt_check.cpp) and, operation for operation, tests/sim3opt_reference.py:
//   Sim3(Vector7d), operator*, inverse, map        types/sim3.h:70-146, 233-272
//   VertexSim3Expmap::oplusImpl, cam_map1 / 2      types/types_seven_dof_expmap.h:60-88
//   EdgeSim3ProjectXYZ / EdgeInverseSim3ProjectXYZ ::computeError                 :138-167
//   BaseBinaryEdge::linearizeOplus (numeric)       core/base_binary_edge.hpp:130-205
//   BaseBinaryEdge::constructQuadraticForm         core/base_binary_edge.hpp:91-113
//   RobustKernelHuber::robustify                   core/robust_kernel_impl.cpp:78-91
//   OptimizationAlgorithmLevenberg::solve          core/optimization_algorithm_levenberg.cpp:61-189
//                                                  (the decision itself: g2o_lm.h, shared with the
//                                                  essential graph and global BA)
// All fp64, one rounding per operation in the order written (-ffp-contract=off).  sin, cos and exp
// come from the platform (csrc/trig_f64.h on the device), so host and device agree to rounding,
// not bit for bit; the perturbations of the numeric Jacobians take the small-angle branch, which
// uses neither.
//
// Deviations from g2o, both for inputs it does not meet in a release build:
//  * a chi2 that is not <= th2 (NaN included) marks the pair an outlier; g2o's `chi2 > th2` keeps a
//    NaN edge.  A non-finite estimate therefore ends with n_in = 0 and the estimate as passed in.
//  * a failed damped solve leaves the estimate where it is (x = 0), as k_pose_opt does; g2o applies
//    whatever the solver left in x.
// The dense solve is an unpivoted LDL^T where Eigen's LDLT pivots: rounding only.  Under
// _fix_scale row and column 6 of H are exactly 0, so the pivot of row 6 is lambda, its L entries
// are 0 and x[6] = 0 / lambda = 0, which is what Eigen's pivoted factorisation returns too.
#pragma once
#include <math.h>
#include <stdint.h>

#include "g2o_lm.h"

#if defined(__HIP_DEVICE_COMPILE__)
#include "trig_f64.h"
#endif

namespace orbmi {

#define S3O_FN __host__ __device__ inline __attribute__((always_inline))

constexpr double kS3oDelta = 1e-9;  // BaseBinaryEdge::linearizeOplus
constexpr int kS3oAcc = 36;         // 28 upper entries of H, 7 of b, the robust chi2

struct Sim3d {
    double q[4];  // x y z w (Eigen's coefficient order)
    double t[3];
    double s;
};

S3O_FN void s3o_sincos(double x, double* s, double* c) {
#if defined(__HIP_DEVICE_COMPILE__)
    if (x >= 0 && x <= 6.28) {  // a norm: >= 0, and small for any sane step
        orbmi_sincos_f64(x, s, c);
        return;
    }
#endif
    *s = sin(x);
    *c = cos(x);
}

// Eigen::Quaternion(const Matrix3&), R row-major; not normalised
S3O_FN void s3o_quat_from_R(const double* m, double* q) {
    const double tr = (m[0] + m[4]) + m[8];
    if (tr > 0) {
        double t = __builtin_sqrt(tr + 1.0);
        q[3] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (m[7] - m[5]) * t;
        q[1] = (m[2] - m[6]) * t;
        q[2] = (m[3] - m[1]) * t;
        return;
    }
    int i = 0;
    if (m[4] > m[0]) i = 1;
    if (m[8] > (i == 1 ? m[4] : m[0])) i = 2;
    if (i == 0) {
        double t = __builtin_sqrt(((m[0] - m[4]) - m[8]) + 1.0);
        q[0] = 0.5 * t;
        t = 0.5 / t;
        q[3] = (m[7] - m[5]) * t;
        q[1] = (m[3] + m[1]) * t;
        q[2] = (m[6] + m[2]) * t;
    } else if (i == 1) {
        double t = __builtin_sqrt(((m[4] - m[8]) - m[0]) + 1.0);
        q[1] = 0.5 * t;
        t = 0.5 / t;
        q[3] = (m[2] - m[6]) * t;
        q[2] = (m[7] + m[5]) * t;
        q[0] = (m[1] + m[3]) * t;
    } else {
        double t = __builtin_sqrt(((m[8] - m[0]) - m[4]) + 1.0);
        q[2] = 0.5 * t;
        t = 0.5 / t;
        q[3] = (m[3] - m[1]) * t;
        q[0] = (m[2] + m[6]) * t;
        q[1] = (m[5] + m[7]) * t;
    }
}

// Eigen toRotationMatrix, row-major
S3O_FN void s3o_quat_to_R(const double* q, double* R) {
    const double tx = 2 * q[0], ty = 2 * q[1], tz = 2 * q[2];
    const double twx = tx * q[3], twy = ty * q[3], twz = tz * q[3];
    const double txx = tx * q[0], txy = ty * q[0], txz = tz * q[0];
    const double tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
    R[0] = 1 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
    R[3] = txy + twz; R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1 - (txx + tyy);
}

S3O_FN void s3o_quat_mul(const double* a, const double* b, double* o) {
    const double x = ((a[3] * b[0] + a[0] * b[3]) + a[1] * b[2]) - a[2] * b[1];
    const double y = ((a[3] * b[1] + a[1] * b[3]) + a[2] * b[0]) - a[0] * b[2];
    const double z = ((a[3] * b[2] + a[2] * b[3]) + a[0] * b[1]) - a[1] * b[0];
    const double w = ((a[3] * b[3] - a[0] * b[0]) - a[1] * b[1]) - a[2] * b[2];
    o[0] = x; o[1] = y; o[2] = z; o[3] = w;
}

// Eigen's quaternion * vector: v + w * uv + q.vec x uv, uv = 2 * (q.vec x v)
S3O_FN void s3o_rotate(const double* q, const double* v, double* o) {
    double ux = q[1] * v[2] - q[2] * v[1], uy = q[2] * v[0] - q[0] * v[2], uz = q[0] * v[1] - q[1] * v[0];
    ux = ux + ux; uy = uy + uy; uz = uz + uz;
    const double cx = q[1] * uz - q[2] * uy, cy = q[2] * ux - q[0] * uz, cz = q[0] * uy - q[1] * ux;
    o[0] = (v[0] + q[3] * ux) + cx;
    o[1] = (v[1] + q[3] * uy) + cy;
    o[2] = (v[2] + q[3] * uz) + cz;
}

// g2o::Sim3(Matrix3d, Vector3d, double) from the float arguments of OptimizeSim3's caller
S3O_FN void s3o_from_rts(const float* R, const float* t, float s, Sim3d* o) {
    double m[9];
#pragma unroll
    for (int k = 0; k < 9; k++) m[k] = (double)R[k];
    s3o_quat_from_R(m, o->q);
#pragma unroll
    for (int k = 0; k < 3; k++) o->t[k] = (double)t[k];
    o->s = (double)s;
}

// Sim3::map: s * (r * xyz) + t
S3O_FN void s3o_map(const Sim3d& S, const double* x, double* y) {
    double r[3];
    s3o_rotate(S.q, x, r);
#pragma unroll
    for (int k = 0; k < 3; k++) y[k] = S.s * r[k] + S.t[k];
}

// Sim3::operator*
S3O_FN void s3o_mul(const Sim3d& a, const Sim3d& b, Sim3d* o) {
    Sim3d r;
    double rt[3];
    s3o_quat_mul(a.q, b.q, r.q);
    s3o_rotate(a.q, b.t, rt);
#pragma unroll
    for (int k = 0; k < 3; k++) r.t[k] = a.s * rt[k] + a.t[k];
    r.s = a.s * b.s;
    *o = r;
}

// Sim3::inverse: (r.conjugate(), r.conjugate() * ((-1. / s) * t), 1. / s)
S3O_FN void s3o_inverse(const Sim3d& a, Sim3d* o) {
    Sim3d r;
    r.q[0] = -a.q[0]; r.q[1] = -a.q[1]; r.q[2] = -a.q[2]; r.q[3] = a.q[3];
    const double m = -1. / a.s;
    const double v[3] = {m * a.t[0], m * a.t[1], m * a.t[2]};
    s3o_rotate(r.q, v, r.t);
    r.s = 1. / a.s;
    *o = r;
}

// Sim3(const Vector7d&) (types/sim3.h:70-142): omega, upsilon, sigma
S3O_FN void s3o_exp(const double* u, Sim3d* o) {
    const double w0 = u[0], w1 = u[1], w2 = u[2], sigma = u[6];
    const double theta = __builtin_sqrt((w0 * w0 + w1 * w1) + w2 * w2);
    const double Om[9] = {0, -w2, w1, w2, 0, -w0, -w1, w0, 0};
    double Om2[9], R[9], W[9];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) Om2[3 * r + c] = (Om[3 * r] * Om[c] + Om[3 * r + 1] * Om[3 + c]) + Om[3 * r + 2] * Om[6 + c];
    const double s = exp(sigma);
    const double eps = 0.00001;
    double A, B, C, ra = 1.0, rb = 1.0;  // R = I + ra * Omega + rb * Omega2
    const bool small_theta = theta < eps;
    double sn = 0, cs = 1;
    if (!small_theta) {
        s3o_sincos(theta, &sn, &cs);
        ra = sn / theta;
        rb = (1 - cs) / (theta * theta);
    }
    if (fabs(sigma) < eps) {
        C = 1;
        if (small_theta) {
            A = 1. / 2.;
            B = 1. / 6.;
        } else {
            const double theta2 = theta * theta;
            A = (1 - cs) / theta2;
            B = (theta - sn) / (theta2 * theta);
        }
    } else {
        C = (s - 1) / sigma;
        if (small_theta) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1) * s + 1) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma);
        } else {
            const double a = s * sn, b = s * cs, theta2 = theta * theta, sigma2 = sigma * sigma;
            const double c = theta2 + sigma2;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2;
        }
    }
#pragma unroll
    for (int k = 0; k < 9; k++) {
        const double I = (k == 0 || k == 4 || k == 8) ? 1.0 : 0.0;
        // the small-angle branches add Omega and Omega2 as they are (ra = rb = 1 exactly)
        R[k] = small_theta ? (I + Om[k]) + Om2[k] : (I + ra * Om[k]) + rb * Om2[k];
        W[k] = (A * Om[k] + B * Om2[k]) + C * I;
    }
    s3o_quat_from_R(R, o->q);
#pragma unroll
    for (int r = 0; r < 3; r++) o->t[r] = (W[3 * r] * u[3] + W[3 * r + 1] * u[4]) + W[3 * r + 2] * u[5];
    o->s = s;
}

// VertexSim3Expmap::oplusImpl: estimate <- Sim3(update) * estimate, update[6] = 0 under _fix_scale
S3O_FN void s3o_oplus(const Sim3d& S, const double* x, int fix_scale, Sim3d* o) {
    double u[7];
#pragma unroll
    for (int k = 0; k < 7; k++) u[k] = x[k];
    if (fix_scale) u[6] = 0;
    Sim3d E;
    s3o_exp(u, &E);
    s3o_mul(E, S, o);
}

// The estimate perturbed by +-delta along direction d, and its inverse (what linearizeOplus pushes)
S3O_FN void s3o_perturbed(const Sim3d& S, int d, double step, int fix_scale, Sim3d* P, Sim3d* Pinv) {
    double u[7];
#pragma unroll
    for (int k = 0; k < 7; k++) u[k] = k == d ? step : 0.0;
    s3o_oplus(S, u, fix_scale, P);
    s3o_inverse(*P, Pinv);
}

// obs - cam_map(project(T.map(X))): T = the estimate and K1 for e12 (X = the point in camera 2),
// its inverse and K2 for e21.  k = fx fy cx cy.
S3O_FN void s3o_error(const Sim3d& T, const double* X, const double* obs, const double* k, double* e) {
    double y[3];
    s3o_map(T, X, y);
    const double px = y[0] / y[2], py = y[1] / y[2];
    e[0] = obs[0] - (px * k[0] + k[2]);
    e[1] = obs[1] - (py * k[1] + k[3]);
}

// OptimizableGraph::Edge::chi2 with information w * I
S3O_FN double s3o_chi2(const double* e, double w) { return e[0] * (w * e[0]) + e[1] * (w * e[1]); }

// RobustKernelHuber::robustify: rho[0], rho[1]
S3O_FN void s3o_huber(double c, double delta, double dsqr, double* rho0, double* rho1) {
    if (c <= dsqr) {
        *rho0 = c;
        *rho1 = 1.;
    } else {
        const double sq = __builtin_sqrt(c);
        *rho0 = 2 * sq * delta - dsqr;
        *rho1 = delta / sq;
    }
}

// One correspondence's inputs as the edges hold them (doubles of the caller's floats)
struct S3oPair {
    double X1[3], X2[3];  // the points in their own camera frames
    double o1[2], o2[2];  // observations in image 1 / 2
    double w1, w2;        // invSigma2 of either side
};

// linearizeOplus + constructQuadraticForm of one edge: T0 the (inverse) estimate, P[2 * d] /
// P[2 * d + 1] the (inverse) estimate perturbed by +-delta along d.  Adds to acc: the 28 upper
// entries of H row by row, b, and the robust chi2.  Column 6 is skipped under fix_scale: both
// perturbed estimates equal each other there, so it is exactly 0.
S3O_FN void s3o_edge(const Sim3d& T0, const Sim3d* P, const double* X, const double* obs, double w, const double* k,
                     double delta, double dsqr, int fix_scale, double* acc) {
    double e[2], J[2][7];
    s3o_error(T0, X, obs, k, e);
    const double scalar = 1.0 / (2 * kS3oDelta);
#pragma unroll
    for (int d = 0; d < 7; d++) {
        if (d == 6 && fix_scale) {
            J[0][d] = 0;
            J[1][d] = 0;
            continue;
        }
        double ep[2], em[2];
        s3o_error(P[2 * d], X, obs, k, ep);
        s3o_error(P[2 * d + 1], X, obs, k, em);
        J[0][d] = scalar * (ep[0] - em[0]);
        J[1][d] = scalar * (ep[1] - em[1]);
    }
    const double c = s3o_chi2(e, w);
    double rho0, rho1;
    s3o_huber(c, delta, dsqr, &rho0, &rho1);
    const double ww = rho1 * w;  // robustInformation
    const double r0 = -(w * e[0]) * rho1, r1 = -(w * e[1]) * rho1;  // omega_r *= rho[1]
    const int nd = fix_scale ? 6 : 7;
    int q = 0;
#pragma unroll
    for (int r = 0; r < 7; r++) {
#pragma unroll
        for (int cc = r; cc < 7; cc++, q++)
            if (cc < nd) acc[q] = acc[q] + ((J[0][r] * ww) * J[0][cc] + (J[1][r] * ww) * J[1][cc]);
        if (r < nd) acc[28 + r] = acc[28 + r] + (J[0][r] * r0 + J[1][r] * r1);
    }
    acc[35] = acc[35] + rho0;
}

// computeError of both edges of one pair at the estimate S (Si its inverse): the unrobustified
// chi2 of either edge, and their robust sum
S3O_FN double s3o_pair_chi2(const Sim3d& S, const Sim3d& Si, const S3oPair& p, const double* k1, const double* k2,
                            double delta, double dsqr, double* c12, double* c21) {
    double e[2], r0, r1, a, b;
    s3o_error(S, p.X2, p.o1, k1, e);
    *c12 = s3o_chi2(e, p.w1);
    s3o_huber(*c12, delta, dsqr, &a, &r0);
    s3o_error(Si, p.X1, p.o2, k2, e);
    *c21 = s3o_chi2(e, p.w2);
    s3o_huber(*c21, delta, dsqr, &b, &r1);
    return a + b;
}

// Damped 7x7 solve (LinearSolverDense): H as 28 upper entries row by row.  False on a pivot that
// is not a positive finite number (Eigen's isPositive); x is then 0.
S3O_FN bool s3o_solve7(const double* H, const double* b, double lam, double* x) {
    double A[7][7];
    {
        int q = 0;
#pragma unroll
        for (int r = 0; r < 7; r++)
#pragma unroll
            for (int c = r; c < 7; c++, q++) A[c][r] = H[q];
    }
#pragma unroll
    for (int j = 0; j < 7; j++) A[j][j] = A[j][j] + lam;
    bool ok = true;
    double D[7], y[7];
#pragma unroll
    for (int j = 0; j < 7; j++) {
        double d = A[j][j];
#pragma unroll
        for (int k = 0; k < j; k++) d = d - (A[j][k] * A[j][k]) * D[k];
        ok = ok && d > 0 && d < INFINITY;
        D[j] = d;
#pragma unroll
        for (int i = j + 1; i < 7; i++) {
            double s = A[i][j];
#pragma unroll
            for (int k = 0; k < j; k++) s = s - (A[i][k] * A[j][k]) * D[k];
            A[i][j] = s / d;
        }
    }
#pragma unroll
    for (int i = 0; i < 7; i++) {
        double s = b[i];
#pragma unroll
        for (int k = 0; k < i; k++) s = s - A[i][k] * y[k];
        y[i] = s;
    }
#pragma unroll
    for (int i = 0; i < 7; i++) y[i] = y[i] / D[i];
#pragma unroll
    for (int i = 6; i >= 0; i--) {
        double s = y[i];
#pragma unroll
        for (int k = i + 1; k < 7; k++) s = s - A[k][i] * x[k];
        x[i] = s;
    }
    if (!ok)
#pragma unroll
        for (int i = 0; i < 7; i++) x[i] = 0;
    return ok;
}

// The Levenberg decision is g2o_lm.h's; OptimizeSim3 brings computeLambdaInit over its 7 diagonal
// entries and computeScale's seven terms.
// After buildSystem of iteration `it`: H = the 28 upper entries
S3O_FN void s3o_lm_begin(S3oLm& L, int it, const double* H, double chi) {
    lm_begin(L, it, chi, [H] {
        double m = 0;
        int q = 0;
#pragma unroll
        for (int r = 0; r < 7; r++) {
            const double a = fabs(H[q]);
            m = a > m ? a : m;  // std::max(fabs(h), m): a NaN diagonal is passed over
            q += 7 - r;
        }
        return 1e-5 * m;
    });
}

// One trial's verdict: true = the step is kept.  *more = the do-while goes on.
S3O_FN bool s3o_lm_trial(S3oLm& L, bool ok2, double tempChi, const double* x, const double* b, bool* more) {
    double scale = 0;
#pragma unroll
    for (int j = 0; j < 7; j++) scale = scale + x[j] * (L.lambda * x[j] + b[j]);
    return lm_trial(L, ok2, tempChi, scale, more, LmCubeMul());
}

// Converter::toCvMat(g2o::Sim3): (float)(s * R) and (float)t
S3O_FN void s3o_to_float(const Sim3d& S, float* sR, float* t) {
    double R[9];
    s3o_quat_to_R(S.q, R);
#pragma unroll
    for (int k = 0; k < 9; k++) sR[k] = (float)(S.s * R[k]);
#pragma unroll
    for (int k = 0; k < 3; k++) t[k] = (float)S.t[k];
}

#ifndef __HIP_DEVICE_COMPILE__
// ---- the whole of OptimizeSim3 on the host, sequentially (the CPU check and the timing
// comparison; the device kernel restates this control flow over a workgroup) --------------------

struct S3oHostResult {
    Sim3d S;
    int n_in, n_bad, iterations[2];
};

struct S3oHost {
    int n;
    const S3oPair* pairs;
    double k1[4], k2[4], delta, dsqr;
    int fix_scale;
    uint8_t* alive;  // n
    double* chi2;    // n x 2

    double errors(const Sim3d& S) const {  // computeActiveErrors + activeRobustChi2
        Sim3d Si;
        s3o_inverse(S, &Si);
        double sum = 0;
        for (int i = 0; i < n; i++)
            if (alive[i]) sum = sum + s3o_pair_chi2(S, Si, pairs[i], k1, k2, delta, dsqr, &chi2[2 * i], &chi2[2 * i + 1]);
        return sum;
    }
    void build(const Sim3d& S, double* acc) const {  // at the estimate the errors were computed at
        Sim3d Si, P[14], Pi[14];
        s3o_inverse(S, &Si);
        for (int d = 0; d < 7; d++) {
            s3o_perturbed(S, d, kS3oDelta, fix_scale, &P[2 * d], &Pi[2 * d]);
            s3o_perturbed(S, d, -kS3oDelta, fix_scale, &P[2 * d + 1], &Pi[2 * d + 1]);
        }
        for (int k = 0; k < kS3oAcc; k++) acc[k] = 0;
        for (int i = 0; i < n; i++) {
            if (!alive[i]) continue;
            s3o_edge(S, P, pairs[i].X2, pairs[i].o1, pairs[i].w1, k1, delta, dsqr, fix_scale, acc);
            s3o_edge(Si, Pi, pairs[i].X1, pairs[i].o2, pairs[i].w2, k2, delta, dsqr, fix_scale, acc);
        }
    }
    int optimize(Sim3d& S, int iterations) const {
        S3oLm L{};
        int done = 0;
        bool any = false;
        for (int i = 0; i < n; i++) any = any || alive[i];
        if (!any) return 0;
        for (int it = 0; it < iterations; it++) {
            double acc[kS3oAcc], x[7];
            build(S, acc);
            s3o_lm_begin(L, it, acc, acc[35]);
            bool more;
            do {
                const bool ok2 = s3o_solve7(acc, acc + 28, L.lambda, x);
                Sim3d T = S;
                if (ok2) s3o_oplus(S, x, fix_scale, &T);
                const double tempChi = errors(T);
                if (s3o_lm_trial(L, ok2, tempChi, x, acc + 28, &more)) S = T;
            } while (more);
            done++;
            if (lm_end(L)) break;
        }
        return done;
    }
    int outliers(float th2, bool count_in) const {  // the chi2 pass: nBad (first) or nIn (second)
        int k = 0;
        for (int i = 0; i < n; i++) {
            if (!alive[i]) continue;
            const bool good = chi2[2 * i] <= (double)th2 && chi2[2 * i + 1] <= (double)th2;
            if (!good) alive[i] = 0;
            k += count_in ? good : !good;
        }
        return k;
    }
};

inline S3oHostResult s3o_optimize_host(int n, const S3oPair* pairs, const float* k1, const float* k2, float th2,
                                       int fix_scale, const float* R12, const float* t12, float s12, uint8_t* alive,
                                       double* chi2) {
    S3oHost h;
    h.n = n;
    h.pairs = pairs;
    for (int k = 0; k < 4; k++) { h.k1[k] = (double)k1[k]; h.k2[k] = (double)k2[k]; }
    h.delta = (double)sqrtf(th2);
    h.dsqr = h.delta * h.delta;
    h.fix_scale = fix_scale;
    h.alive = alive;
    h.chi2 = chi2;
    for (int i = 0; i < n; i++) { alive[i] = 1; chi2[2 * i] = 0; chi2[2 * i + 1] = 0; }
    S3oHostResult r{};
    s3o_from_rts(R12, t12, s12, &r.S);
    Sim3d S = r.S;
    r.iterations[0] = h.optimize(S, 5);
    r.n_bad = h.outliers(th2, false);
    if (n - r.n_bad < 10) return r;  // g2oS12 as passed in
    r.iterations[1] = h.optimize(S, r.n_bad > 0 ? 10 : 5);
    r.n_in = h.outliers(th2, true);
    r.S = S;
    return r;
}
#endif  // !__HIP_DEVICE_COMPILE__

}  // namespace orbmi
