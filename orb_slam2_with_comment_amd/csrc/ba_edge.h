// The edge arithmetic of the bundle adjustments (EdgeSE3ProjectXYZ / EdgeStereoSE3ProjectXYZ,
// types_six_dof_expmap.cpp; BaseBinaryEdge::constructQuadraticForm): one body for
// Optimizer::LocalBundleAdjustment (lba.hip) and Optimizer::BundleAdjustment (gba.hip).  The two
// differ in the Huber deltas only (BaHuber).  The including file decides the contraction mode:
// lba.hip includes this under `#pragma clang fp contract(fast)`, gba.hip under the build's
// -ffp-contract=off.
#pragma once
#include "orbmi_common.h"
#include "se3_device.h"

namespace orbmi {

__device__ inline bool edge_stereo(const orbmi_ba_edge& e) { return !(e.ur < 0); }

// The edge math works on values (the edge record, its keyframe's camera, the pose Tk) so that a
// kernel can load them once, early, and keep them in registers.
struct BaCam { float fx, fy, cx, cy, bf; };
__device__ inline BaCam ba_cam(const orbmi_ba_keyframe& k) { return BaCam{k.fx, k.fy, k.cx, k.cy, k.bf}; }

// RobustKernelHuber deltas of the mono / stereo edges: float thresholds widened to double, as the
// reference's `const float thHuberMono = sqrt(...)` passed to setDelta(double)
struct BaHuber { double mono, stereo; };
// src/Optimizer.cc:599-600 (LocalBundleAdjustment): sqrt(5.991), sqrt(7.815)
__device__ inline BaHuber ba_huber_local() { return BaHuber{(double)(float)sqrt(5.991), (double)(float)sqrt(7.815)}; }
// src/Optimizer.cc:106-107 (BundleAdjustment): sqrt(5.99), sqrt(7.815)
__device__ inline BaHuber ba_huber_global() { return BaHuber{(double)(float)sqrt(5.99), (double)(float)sqrt(7.815)}; }

// error of edge e with the point's position at Xp (3 doubles)
__device__ inline void edge_err_math(const orbmi_ba_edge& e, const BaCam& kf, const double* Tk, const double* Xp,
                                     double* err) {
    double p[3];
    se3_map(Tk, Xp, p);
    if (!edge_stereo(e)) {
        const double px = p[0] / p[2], py = p[1] / p[2];
        err[0] = (double)e.u - (px * (double)kf.fx + (double)kf.cx);
        err[1] = (double)e.v - (py * (double)kf.fy + (double)kf.cy);
        err[2] = 0;
    } else {
        const float invz = (float)(1.0f / p[2]);  // float invz (types_six_dof_expmap.cpp:151)
        const double r0 = p[0] * invz * (double)kf.fx + (double)kf.cx;
        const double r1 = p[1] * invz * (double)kf.fy + (double)kf.cy;
        const double r2 = r0 - (double)(kf.bf * invz);
        err[0] = (double)e.u - r0;
        err[1] = (double)e.v - r1;
        err[2] = (double)e.ur - r2;
    }
}

__device__ inline double edge_chi2_math(const orbmi_ba_edge& e, const double* r) {
    const double info = (double)e.inv_sigma2;
    return r[0] * (info * r[0]) + r[1] * (info * r[1]) + (edge_stereo(e) ? r[2] * (info * r[2]) : 0.0);
}

// robustified chi2 and weight rho' (RobustKernelHuber::robustify); fl = the edge's flags (bit 1:
// no robust kernel)
__device__ inline void edge_robust_math(unsigned char fl, const orbmi_ba_edge& e, const BaHuber& h, double c,
                                        double* rho0, double* rho1) {
    if (fl & 2) { *rho0 = c; *rho1 = 1.0; return; }
    const double d = edge_stereo(e) ? h.stereo : h.mono, dsqr = d * d;
    if (c <= dsqr) { *rho0 = c; *rho1 = 1.0; }
    else { const double s = sqrt(c); *rho0 = 2 * s * d - dsqr; *rho1 = d / s; }
}

// Jacobians (types_six_dof_expmap.cpp:103-134, :188-234)
__device__ inline void edge_jac_math(const orbmi_ba_edge& e, const BaCam& kf, const double* Tk, const double* Xp,
                                     double Jl[3][3], double Jp[3][6]) {
    double p[3], R[3][3];
    se3_map(Tk, Xp, p);
    q_to_matrix(load_q(Tk), R);
    // one reciprocal per edge (fast_rcp: within an ulp of 1 / z) instead of the reference's
    // divisions; the Jacobians only steer the Levenberg steps (parity 1e-4), the errors and
    // chi2 keep the exact divisions
    const double x = p[0], y = p[1], z = p[2], iz = fast_rcp(z), iz2 = iz * iz;
    const double fx = kf.fx, fy = kf.fy, bf = kf.bf;
    if (!edge_stereo(e)) {
        const double t02 = -x * iz * fx, t12 = -y * iz * fy;
        for (int c = 0; c < 3; c++) {
            Jl[0][c] = -iz * (fx * R[0][c] + t02 * R[2][c]);
            Jl[1][c] = -iz * (fy * R[1][c] + t12 * R[2][c]);
            Jl[2][c] = 0;
        }
    } else {
        for (int c = 0; c < 3; c++) {
            Jl[0][c] = -fx * R[0][c] * iz + fx * x * R[2][c] * iz2;
            Jl[1][c] = -fy * R[1][c] * iz + fy * y * R[2][c] * iz2;
            Jl[2][c] = Jl[0][c] - bf * R[2][c] * iz2;
        }
    }
    Jp[0][0] = x * y * iz2 * fx; Jp[0][1] = -(1 + (x * x * iz2)) * fx; Jp[0][2] = y * iz * fx;
    Jp[0][3] = -iz * fx; Jp[0][4] = 0; Jp[0][5] = x * iz2 * fx;
    Jp[1][0] = (1 + y * y * iz2) * fy; Jp[1][1] = -x * y * iz2 * fy; Jp[1][2] = -x * iz * fy;
    Jp[1][3] = 0; Jp[1][4] = -iz * fy; Jp[1][5] = y * iz2 * fy;
    if (edge_stereo(e)) {
        Jp[2][0] = Jp[0][0] - bf * y * iz2; Jp[2][1] = Jp[0][1] + bf * x * iz2; Jp[2][2] = Jp[0][2];
        Jp[2][3] = Jp[0][3]; Jp[2][4] = 0; Jp[2][5] = Jp[0][5] - bf * iz2;
    } else {
        for (int c = 0; c < 6; c++) Jp[2][c] = 0;
    }
}

// weight W = rho' * info and omega_r = -info * e * rho' (constructQuadraticForm), err = the
// edge's current error
__device__ inline void edge_weights_math(unsigned char fl, const orbmi_ba_edge& ed, const BaHuber& h, const double* err,
                                         double* w, double om[3]) {
    const double info = (double)ed.inv_sigma2;
    double r0, r1;
    edge_robust_math(fl, ed, h, edge_chi2_math(ed, err), &r0, &r1);
    *w = (fl & 2) ? info : r1 * info;
    const double s = (fl & 2) ? 1.0 : r1;
    for (int k = 0; k < 3; k++) om[k] = -(info * err[k]) * s;
}

// The edge's blocks of the quadratic form: B = Jp^T W Jl (6 x 3, row-major, 18), He = the upper
// triangle of Jl^T W Jl (6) then Jl^T omega_r (3), Hp = the upper triangle of Jp^T W Jp (21) then
// Jp^T omega_r (6).  B and Hp are written only for an edge into a free pose.
__device__ inline void edge_blocks_math(const orbmi_ba_edge& ed, const BaCam& kf, const double* Tk, unsigned char fl,
                                        const BaHuber& h, const double* err, const double* Xp, bool free_pose,
                                        double* He, double* B, double* Hp) {
    double Jl[3][3], Jp[3][6], w, om[3];
    edge_jac_math(ed, kf, Tk, Xp, Jl, Jp);
    edge_weights_math(fl, ed, h, err, &w, om);
    int q = 0;
    for (int r = 0; r < 3; r++)
        for (int c = r; c < 3; c++, q++)
            He[q] = Jl[0][r] * w * Jl[0][c] + Jl[1][r] * w * Jl[1][c] + Jl[2][r] * w * Jl[2][c];
    for (int r = 0; r < 3; r++) He[6 + r] = Jl[0][r] * om[0] + Jl[1][r] * om[1] + Jl[2][r] * om[2];
    if (free_pose) {
        for (int r = 0; r < 6; r++)
            for (int c = 0; c < 3; c++)
                B[r * 3 + c] = Jp[0][r] * w * Jl[0][c] + Jp[1][r] * w * Jl[1][c] + Jp[2][r] * w * Jl[2][c];
        q = 0;
        for (int r = 0; r < 6; r++)
            for (int c = r; c < 6; c++, q++)
                Hp[q] = Jp[0][r] * w * Jp[0][c] + Jp[1][r] * w * Jp[1][c] + Jp[2][r] * w * Jp[2][c];
        for (int r = 0; r < 6; r++) Hp[21 + r] = Jp[0][r] * om[0] + Jp[1][r] * om[1] + Jp[2][r] * om[2];
    }
}

// D^-1 of the point's damped 3x3 block, Hll + lambda I (cofactors, as Eigen's 3x3 inverse)
__device__ inline void point_dinv(const double* Hll, int p, double lam, double Di[9]) {
    double D[3][3];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) D[r][c] = Hll[9 * p + 3 * r + c] + (r == c ? lam : 0.0);
    const double c00 = D[1][1] * D[2][2] - D[1][2] * D[2][1];
    const double c10 = D[1][2] * D[2][0] - D[1][0] * D[2][2];
    const double c20 = D[1][0] * D[2][1] - D[1][1] * D[2][0];
    const double det = D[0][0] * c00 + D[0][1] * c10 + D[0][2] * c20;
    const double id = 1.0 / det;
    Di[0] = c00 * id; Di[3] = c10 * id; Di[6] = c20 * id;
    Di[1] = (D[0][2] * D[2][1] - D[0][1] * D[2][2]) * id;
    Di[4] = (D[0][0] * D[2][2] - D[0][2] * D[2][0]) * id;
    Di[7] = (D[0][1] * D[2][0] - D[0][0] * D[2][1]) * id;
    Di[2] = (D[0][1] * D[1][2] - D[0][2] * D[1][1]) * id;
    Di[5] = (D[0][2] * D[1][0] - D[0][0] * D[1][2]) * id;
    Di[8] = (D[0][0] * D[1][1] - D[0][1] * D[1][0]) * id;
}

// SE3Quat (x, y, z, w, tx, ty, tz, -) from a float Tcw (Converter::toSE3Quat) and back
// (Converter::toCvMat)
__device__ inline void tcw_to_se3(const float* t, double* Ti) {
    double R[3][3];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) R[r][c] = t[4 * r + c];
    Q q = q_from_matrix(R);
    q_normalize(q);
    Ti[0] = q.x; Ti[1] = q.y; Ti[2] = q.z; Ti[3] = q.w; Ti[4] = t[3]; Ti[5] = t[7]; Ti[6] = t[11]; Ti[7] = 0;
}
__device__ inline void se3_to_tcw(const double* Ti, float* o) {
    double R[3][3];
    q_to_matrix(load_q(Ti), R);
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) o[4 * r + c] = (float)R[r][c];
        o[4 * r + 3] = (float)Ti[4 + r];
    }
    o[12] = 0; o[13] = 0; o[14] = 0; o[15] = 1;
}

}  // namespace orbmi
