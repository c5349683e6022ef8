// The arithmetic of Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:829-1118) with the bundled
// g2o's semantics, shared by the device kernels (essgraph.hip), the CPU check program
// (tests/cpp/essgraph_check.cpp) and, operation for operation, tests/essgraph_reference.py:
//   Sim3::log                                      types/sim3.h:148-230
//   EdgeSim3::computeError                         types/types_seven_dof_expmap.h:106-114
//   BaseBinaryEdge::linearizeOplus (numeric)       core/base_binary_edge.hpp:130-205
//   BaseBinaryEdge::constructQuadraticForm         core/base_binary_edge.hpp:91-113
//   OptimizationAlgorithmLevenberg::solve          core/optimization_algorithm_levenberg.cpp:61-164
//                                                  (the decision itself: g2o_lm.h)
// on top of sim3_opt.h's Sim3(Vector7d), operator*, inverse, map and oplusImpl.  All fp64, one
// rounding per operation in the order written (-ffp-contract=off).  sin, cos, acos, log and exp
// come from the platform, so host and device agree to rounding, not bit for bit.
//
// Deviations from g2o:
//  * the 3x3 solve of log is a partial-pivot LU in the order written here; Eigen's order inside its
//    3x3 lu() is not pinned: rounding only.
//  * the damped solve is an unpivoted block LDL^T in a minimum-degree order where g2o calls Eigen's
//    sparse LLT: rounding only.  Under _fix_scale row and column 6 of every vertex block are
//    exactly 0, so that pivot is lambda, its L entries are 0 and x[6] = 0 / lambda = 0.
//  * a failed damped solve leaves the estimates where they are (x = 0), as sim3_opt.h does.
//  * a vertex no edge names is not optimised (g2o leaves it out of the active set as well).
#pragma once
#include "sim3_opt.h"

#include <algorithm>
#include <set>
#include <vector>

namespace orbmi {

// One edge's record, written by the linearisation and read by the assembly
constexpr int kEgRecE = 0;      // e (7)
constexpr int kEgRecChi = 7;    // chi2
constexpr int kEgRecH00 = 8;    // J0^T J0 (49, row-major)
constexpr int kEgRecH01 = 57;   // J0^T J1
constexpr int kEgRecH11 = 106;  // J1^T J1
constexpr int kEgRecB0 = 155;   // -J0^T e (7)
constexpr int kEgRecB1 = 162;   // -J1^T e
constexpr int kEgRec = 170;

// status word of an optimisation
constexpr int kEgTerminate = 1;    // Levenberg's own stop (else: ran to the iteration count)
constexpr int kEgSolveFailed = 2;  // a damped solve met a pivot that is not a positive finite number
constexpr int kEgRejected = 4;     // a trial was rejected and the estimates restored

// One EdgeSim3: vertex indices and the measurement
struct EgEdge {
    int v0, v1;
    Sim3d C;  // the measurement
};

S3O_FN double eg_acos(double x) { return acos(x); }
S3O_FN double eg_log(double x) { return log(x); }

// Sim3::log
S3O_FN void eg_sim3_log(const Sim3d& S, double* res) {
    const double sigma = eg_log(S.s);
    double R[9];
    s3o_quat_to_R(S.q, R);
    const double d = 0.5 * (((R[0] + R[4]) + R[8]) - 1);
    const double dR[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};  // deltaR
    const double eps = 0.00001;
    const bool small_theta = d > 1 - eps;
    double A, B, C, f = 0.5, theta = 0, sn = 0, cs = 1;
    if (!small_theta) {
        theta = eg_acos(d);
        f = theta / (2 * __builtin_sqrt(1 - d * d));
        s3o_sincos(theta, &sn, &cs);
    }
    const double w0 = f * dR[0], w1 = f * dR[1], w2 = f * dR[2];
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
        C = (S.s - 1) / sigma;
        if (small_theta) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1) * S.s + 1) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1) * S.s) / (sigma2 * sigma);
        } else {
            const double theta2 = theta * theta;
            const double a = S.s * sn, b = S.s * cs, c = theta2 + sigma * sigma;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2;
        }
    }
    const double Om[9] = {0, -w2, w1, w2, 0, -w0, -w1, w0, 0};
    double W[3][3];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const double om2 = (Om[3 * r] * Om[c] + Om[3 * r + 1] * Om[3 + c]) + Om[3 * r + 2] * Om[6 + c];
            W[r][c] = (A * Om[3 * r + c] + B * om2) + C * (r == c ? 1.0 : 0.0);
        }
    // upsilon = W.lu().solve(t): partial pivoting, the rows swapped through selects (no dynamic
    // indexing of the private arrays)
    double t[3] = {S.t[0], S.t[1], S.t[2]};
#pragma unroll
    for (int k = 0; k < 2; k++) {
#pragma unroll
        for (int r = k + 1; r < 3; r++) {  // row k takes the larger pivot, ties stay
            const bool sw = fabs(W[r][k]) > fabs(W[k][k]);
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const double a = W[k][c], b = W[r][c];
                W[k][c] = sw ? b : a;
                W[r][c] = sw ? a : b;
            }
            const double a = t[k], b = t[r];
            t[k] = sw ? b : a;
            t[r] = sw ? a : b;
        }
#pragma unroll
        for (int r = k + 1; r < 3; r++) {
            const double m = W[r][k] / W[k][k];
#pragma unroll
            for (int c = k + 1; c < 3; c++) W[r][c] = W[r][c] - m * W[k][c];
            t[r] = t[r] - m * t[k];
        }
    }
    const double u2 = t[2] / W[2][2];
    const double u1 = (t[1] - W[1][2] * u2) / W[1][1];
    const double u0 = ((t[0] - W[0][1] * u1) - W[0][2] * u2) / W[0][0];
    res[0] = w0; res[1] = w1; res[2] = w2;
    res[3] = u0; res[4] = u1; res[5] = u2;
    res[6] = sigma;
}

// EdgeSim3::computeError: log(C * S_v0 * S_v1^-1)
S3O_FN void eg_edge_error(const Sim3d& C, const Sim3d& S0, const Sim3d& S1, double* e) {
    Sim3d A, I, E;
    s3o_mul(C, S0, &A);
    s3o_inverse(S1, &I);
    s3o_mul(A, I, &E);
    eg_sim3_log(E, e);
}

// chi2 with the identity information: e^T e
S3O_FN double eg_chi2(const double* e) {
    double c = 0;
#pragma unroll
    for (int k = 0; k < 7; k++) c = c + e[k] * e[k];
    return c;
}

// The Levenberg decision is g2o_lm.h's, with setUserLambdaInit(1e-16), computeScale's sum over every
// free vertex handed in, and the cube of sim3_opt.h (z * z * z)
constexpr double kEgLambdaInit = 1e-16;

// CorrectLoop's pose recovery (src/LoopClosing.cc:620-628, src/Optimizer.cc:1069-1079):
// [R | t * (1. / s)] as a float 4x4 Tcw
S3O_FN void eg_sim3_to_tcw(const Sim3d& S, float* T) {
    double R[9];
    s3o_quat_to_R(S.q, R);
    const double inv = 1. / S.s;
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) T[4 * r + c] = (float)R[3 * r + c];
        T[4 * r + 3] = (float)(S.t[r] * inv);
    }
    T[12] = 0; T[13] = 0; T[14] = 0; T[15] = 1;
}

// correctedSwr.map(Srw.map((double)P)) rounded to float (src/LoopClosing.cc:607-612)
S3O_FN void eg_correct_point(const Sim3d& Srw, const Sim3d& Swr_corrected, const float* P, float* out) {
    const double x[3] = {(double)P[0], (double)P[1], (double)P[2]};
    double y[3], z[3];
    s3o_map(Srw, x, y);
    s3o_map(Swr_corrected, y, z);
    out[0] = (float)z[0]; out[1] = (float)z[1]; out[2] = (float)z[2];
}

// The 7x7 pieces of the block LDL^T, in the order both the host loop and the device kernel use.
// Blocks are row-major 49; a diagonal block holds L below its diagonal and D on it.

// factor the diagonal block in place; false on a pivot that is not a positive finite number.
// The block is worked on in registers: every loop unrolls, so the dependent chain is arithmetic
// and not a store followed by a load of the same memory.
S3O_FN bool eg_factor_diag(double* Ag) {
    double A[49];
#pragma unroll
    for (int k = 0; k < 49; k++) A[k] = Ag[k];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 7; j++) {
        double d = A[7 * j + j];
#pragma unroll
        for (int k = 0; k < j; k++) d = d - (A[7 * j + k] * A[7 * j + k]) * A[7 * k + k];
        ok = ok && d > 0 && d < INFINITY;
        A[7 * j + j] = d;
#pragma unroll
        for (int i = j + 1; i < 7; i++) {
            double s = A[7 * i + j];
#pragma unroll
            for (int k = 0; k < j; k++) s = s - (A[7 * i + k] * A[7 * j + k]) * A[7 * k + k];
            A[7 * i + j] = s / d;
        }
    }
#pragma unroll
    for (int k = 0; k < 49; k++) Ag[k] = A[k];
    return ok;
}

// row i of an off-diagonal block B (row vertex r, column vertex c) -> L_rc, against c's factor Dg
S3O_FN void eg_scale_row(double* Brow, const double* Dg) {
    double r[7];
#pragma unroll
    for (int j = 0; j < 7; j++) r[j] = Brow[j];
#pragma unroll
    for (int j = 0; j < 7; j++) {
        double s = r[j];
#pragma unroll
        for (int k = 0; k < j; k++) s = s - (r[k] * Dg[7 * j + k]) * Dg[7 * k + k];
        r[j] = s / Dg[7 * j + j];
    }
#pragma unroll
    for (int j = 0; j < 7; j++) Brow[j] = r[j];
}

// entry (i, j) of the target block: T -= La D Lb^T
S3O_FN double eg_update_entry(double t, const double* La_row, const double* Lb_row, const double* Dg) {
#pragma unroll
    for (int k = 0; k < 7; k++) t = t - (La_row[k] * Lb_row[k]) * Dg[7 * k + k];
    return t;
}

// entry q of slot s (q < 49: the block; 49 <= q < 56: b of a diagonal slot), summed in list order.
// asm_ent = edge * 8 + which * 2 + transposed (EgPlan below)
S3O_FN double eg_assemble_entry(const int* asm_ptr, const int* asm_ent, const double* recs, int s, int q) {
    double acc = 0;
    for (int k = asm_ptr[s]; k < asm_ptr[s + 1]; k++) {
        const int ent = asm_ent[k], w = (ent >> 1) & 3;
        const double* rec = recs + (size_t)(ent >> 3) * kEgRec;
        if (q < 49) {
            const int i = q / 7, j = q % 7;
            acc = acc + rec[(w == 0 ? kEgRecH00 : w == 1 ? kEgRecH01 : kEgRecH11) + ((ent & 1) ? 7 * j + i : 7 * i + j)];
        } else {
            acc = acc + rec[(w == 0 ? kEgRecB0 : kEgRecB1) + (q - 49)];
        }
    }
    return acc;
}

// ---- host only: the symbolic plan (shared with the device path) and the reference optimiser ----

// Elimination order, block structure of L, update targets and the assembly lists of one graph.
// rank = position in the elimination order; blocks of column c are rows of ascending rank.
struct EgPlan {
    int nv = 0, ne = 0, nf = 0, nl = 0;
    std::vector<int> rank_of;  // vertex -> rank, -1: fixed or without an edge
    std::vector<int> vert_of;  // rank -> vertex
    std::vector<int> col_ptr;  // nf + 1 into row_of
    std::vector<int> row_of;   // nl: the row rank of every off-diagonal block
    std::vector<int> upd_ptr;  // nf + 1 into upd (triples)
    std::vector<int> upd;      // target (>= 0: off-diagonal block, < 0: diagonal block ~target), block a, block b
    std::vector<int> asm_ptr;  // nf + nl + 1: slots = the diagonal blocks, then the off-diagonal ones
    std::vector<int> asm_ent;  // edge * 8 + which * 2 + transposed; which 0 / 1 / 2 = J0^T J0, J0^T J1, J1^T J1

    int block(int row, int col) const {  // ranks, row > col; -1 when L has no such block
        const int *b = row_of.data() + col_ptr[col], *e = row_of.data() + col_ptr[col + 1];
        const int* p = std::lower_bound(b, e, row);
        return p != e && *p == row ? (int)(p - row_of.data()) : -1;
    }
};

// false: an edge names a vertex out of range or twice, or the fixed vertex is missing
inline bool eg_args_ok(int nv, int fixed, int ne, const EgEdge* edges) {
    if (nv < 1 || fixed < 0 || fixed >= nv || ne < 0 || (ne > 0 && !edges)) return false;
    for (int e = 0; e < ne; e++) {
        const EgEdge& E = edges[e];
        if (E.v0 < 0 || E.v0 >= nv || E.v1 < 0 || E.v1 >= nv || E.v0 == E.v1) return false;
    }
    return true;
}

inline EgPlan eg_plan(int nv, int fixed, int ne, const EgEdge* edges) {
    EgPlan P;
    P.nv = nv;
    P.ne = ne;
    P.rank_of.assign((size_t)nv, -1);
    std::vector<std::set<int>> adj((size_t)nv);
    std::vector<char> isfree((size_t)nv, 0);
    for (int e = 0; e < ne; e++) {
        isfree[edges[e].v0] = 1;
        isfree[edges[e].v1] = 1;
    }
    isfree[fixed] = 0;
    for (int e = 0; e < ne; e++) {
        const int a = edges[e].v0, b = edges[e].v1;
        if (isfree[a] && isfree[b]) {
            adj[a].insert(b);
            adj[b].insert(a);
        }
    }
    for (int v = 0; v < nv; v++) P.nf += isfree[v];
    // minimum degree on the block graph, ties to the lower id; degree buckets keep it near-linear
    std::set<std::pair<int, int>> queue;  // (degree, vertex)
    for (int v = 0; v < nv; v++)
        if (isfree[v]) queue.insert({(int)adj[v].size(), v});
    std::vector<std::vector<int>> cols;  // per rank: the neighbours left at elimination (vertices)
    cols.reserve((size_t)P.nf);
    while (!queue.empty()) {
        const int p = queue.begin()->second;
        queue.erase(queue.begin());
        P.rank_of[p] = (int)P.vert_of.size();
        P.vert_of.push_back(p);
        std::vector<int> nb(adj[p].begin(), adj[p].end());
        for (int a : nb) {
            queue.erase({(int)adj[a].size(), a});
            adj[a].erase(p);
        }
        for (size_t i = 0; i < nb.size(); i++)
            for (size_t j = i + 1; j < nb.size(); j++) {
                adj[nb[i]].insert(nb[j]);
                adj[nb[j]].insert(nb[i]);
            }
        for (int a : nb) queue.insert({(int)adj[a].size(), a});
        adj[p].clear();
        cols.push_back(std::move(nb));
    }
    P.col_ptr.assign((size_t)P.nf + 1, 0);
    for (int c = 0; c < P.nf; c++) {
        std::vector<int>& rows = cols[c];
        for (int& r : rows) r = P.rank_of[r];
        std::sort(rows.begin(), rows.end());
        P.col_ptr[c + 1] = P.col_ptr[c] + (int)rows.size();
        P.row_of.insert(P.row_of.end(), rows.begin(), rows.end());
    }
    P.nl = (int)P.row_of.size();
    P.upd_ptr.assign((size_t)P.nf + 1, 0);
    for (int c = 0; c < P.nf; c++) {
        for (int a = P.col_ptr[c]; a < P.col_ptr[c + 1]; a++)
            for (int b = P.col_ptr[c]; b <= a; b++) {
                const int target = a == b ? ~P.row_of[a] : P.block(P.row_of[a], P.row_of[b]);
                P.upd.push_back(target);
                P.upd.push_back(a);
                P.upd.push_back(b);
            }
        P.upd_ptr[c + 1] = (int)P.upd.size() / 3;
    }
    // the assembly lists, in edge order per slot
    const int nslots = P.nf + P.nl;
    std::vector<int> slot_of((size_t)ne * 3, -1), tr((size_t)ne, 0);
    P.asm_ptr.assign((size_t)nslots + 1, 0);
    for (int e = 0; e < ne; e++) {
        const int r0 = P.rank_of[edges[e].v0], r1 = P.rank_of[edges[e].v1];
        if (r0 >= 0) slot_of[3 * (size_t)e] = r0;
        if (r1 >= 0) slot_of[3 * (size_t)e + 2] = r1;
        if (r0 >= 0 && r1 >= 0) {
            tr[e] = r0 < r1;  // the block's row is the later rank: J1^T J0 = (J0^T J1)^T
            slot_of[3 * (size_t)e + 1] = P.nf + (r0 > r1 ? P.block(r0, r1) : P.block(r1, r0));
        }
        for (int w = 0; w < 3; w++)
            if (slot_of[3 * (size_t)e + w] >= 0) P.asm_ptr[slot_of[3 * (size_t)e + w] + 1]++;
    }
    for (int s = 0; s < nslots; s++) P.asm_ptr[s + 1] += P.asm_ptr[s];
    P.asm_ent.assign((size_t)P.asm_ptr[nslots], 0);
    std::vector<int> fill(P.asm_ptr.begin(), P.asm_ptr.end() - 1);
    for (int e = 0; e < ne; e++)
        for (int w = 0; w < 3; w++) {
            const int s = slot_of[3 * (size_t)e + w];
            if (s >= 0) P.asm_ent[fill[s]++] = e * 8 + w * 2 + (w == 1 ? tr[e] : 0);
        }
    return P;
}

// Every index of a plan against the length of the array it reads or writes; the device path
// launches nothing on a plan that fails this
inline bool eg_plan_ok(const EgPlan& P) {
    const int nslots = P.nf + P.nl;
    if (P.nf < 0 || P.nl < 0 || (int)P.vert_of.size() != P.nf || (int)P.col_ptr.size() != P.nf + 1) return false;
    if ((int)P.row_of.size() != P.nl || (int)P.upd_ptr.size() != P.nf + 1 || (int)P.asm_ptr.size() != nslots + 1) return false;
    for (int c = 0; c < P.nf; c++) {
        if (P.vert_of[c] < 0 || P.vert_of[c] >= P.nv) return false;
        if (P.col_ptr[c] > P.col_ptr[c + 1] || P.upd_ptr[c] > P.upd_ptr[c + 1]) return false;
        for (int a = P.col_ptr[c]; a < P.col_ptr[c + 1]; a++)
            if (P.row_of[a] <= c || P.row_of[a] >= P.nf) return false;
        for (int u = P.upd_ptr[c]; u < P.upd_ptr[c + 1]; u++) {
            const int t = P.upd[3 * (size_t)u], a = P.upd[3 * (size_t)u + 1], b = P.upd[3 * (size_t)u + 2];
            if (t >= 0 ? t >= P.nl : ~t >= P.nf) return false;
            if (a < P.col_ptr[c] || a >= P.col_ptr[c + 1] || b < P.col_ptr[c] || b >= P.col_ptr[c + 1]) return false;
        }
    }
    if (P.nf && (P.col_ptr[0] != 0 || P.col_ptr[P.nf] != P.nl || P.upd_ptr[P.nf] != (int)P.upd.size() / 3)) return false;
    if (P.asm_ptr[0] != 0 || P.asm_ptr[nslots] != (int)P.asm_ent.size()) return false;
    for (int s = 0; s < nslots; s++)
        if (P.asm_ptr[s] > P.asm_ptr[s + 1]) return false;
    for (int v : P.asm_ent)
        if (v < 0 || v / 8 >= P.ne || (v & 7) > 5) return false;
    return true;
}

// linearizeOplus + constructQuadraticForm of one edge at (S0, S1) into its record
inline void eg_linearize_edge(const Sim3d& C, const Sim3d& S0, const Sim3d& S1, int fix_scale, double* rec,
                              double* Jout = nullptr) {
    double e[7], J[2][7][7];  // J[v][row][col]
    eg_edge_error(C, S0, S1, e);
    const double scalar = 1.0 / (2 * kS3oDelta);
    for (int v = 0; v < 2; v++)
        for (int d = 0; d < 7; d++) {
            double u[7] = {0, 0, 0, 0, 0, 0, 0}, ep[7], em[7];
            Sim3d T;
            u[d] = kS3oDelta;
            s3o_oplus(v ? S1 : S0, u, fix_scale, &T);
            eg_edge_error(C, v ? S0 : T, v ? T : S1, ep);
            u[d] = -kS3oDelta;
            s3o_oplus(v ? S1 : S0, u, fix_scale, &T);
            eg_edge_error(C, v ? S0 : T, v ? T : S1, em);
            for (int k = 0; k < 7; k++) J[v][k][d] = scalar * (ep[k] - em[k]);
        }
    if (Jout)  // J0 then J1, row-major 7 x 7
        for (int k = 0; k < 98; k++) Jout[k] = J[k / 49][(k % 49) / 7][k % 7];
    for (int k = 0; k < 7; k++) rec[kEgRecE + k] = e[k];
    rec[kEgRecChi] = eg_chi2(e);
    const int base[3] = {kEgRecH00, kEgRecH01, kEgRecH11};
    for (int w = 0; w < 3; w++) {
        const int va = w == 2, vb = w != 0;
        for (int a = 0; a < 7; a++)
            for (int b = 0; b < 7; b++) {
                double s = 0;
                for (int k = 0; k < 7; k++) s = s + J[va][k][a] * J[vb][k][b];
                rec[base[w] + 7 * a + b] = s;
            }
    }
    for (int v = 0; v < 2; v++)
        for (int a = 0; a < 7; a++) {
            double s = 0;
            for (int k = 0; k < 7; k++) s = s + J[v][k][a] * (-e[k]);
            rec[(v ? kEgRecB1 : kEgRecB0) + a] = s;
        }
    rec[169] = 0;  // padding
}

struct EgSystem {  // H in the factor's layout (fill blocks 0) and b, per rank
    std::vector<double> Hd, Ho, b, recs;
    double chi2 = 0;
};

// buildSystem at the estimates: chi2 summed in edge order
inline void eg_build_host(const EgPlan& P, const EgEdge* edges, const Sim3d* est, int fix_scale, EgSystem* Y) {
    Y->recs.resize((size_t)P.ne * kEgRec);
    Y->chi2 = 0;
    for (int e = 0; e < P.ne; e++) {
        eg_linearize_edge(edges[e].C, est[edges[e].v0], est[edges[e].v1], fix_scale, &Y->recs[(size_t)e * kEgRec]);
        Y->chi2 = Y->chi2 + Y->recs[(size_t)e * kEgRec + kEgRecChi];
    }
    Y->Hd.assign((size_t)P.nf * 49, 0.0);
    Y->Ho.assign((size_t)P.nl * 49, 0.0);
    Y->b.assign((size_t)P.nf * 7, 0.0);
    for (int s = 0; s < P.nf + P.nl; s++)
        for (int q = 0; q < (s < P.nf ? 56 : 49); q++) {
            const double v = eg_assemble_entry(P.asm_ptr.data(), P.asm_ent.data(), Y->recs.data(), s, q);
            if (q >= 49) Y->b[(size_t)s * 7 + (q - 49)] = v;
            else if (s < P.nf) Y->Hd[(size_t)s * 49 + q] = v;
            else Y->Ho[(size_t)(s - P.nf) * 49 + q] = v;
        }
}

// (H + lambda I) x = b by the block LDL^T in plan order; false (x = 0) on a bad pivot
inline bool eg_solve_host(const EgPlan& P, const EgSystem& Y, double lambda, std::vector<double>* x) {
    std::vector<double> Ld = Y.Hd, Lo = Y.Ho;
    for (int c = 0; c < P.nf; c++)
        for (int k = 0; k < 7; k++) Ld[(size_t)c * 49 + 8 * k] = Ld[(size_t)c * 49 + 8 * k] + lambda;
    bool ok = true;
    for (int c = 0; c < P.nf; c++) {
        double* Dg = &Ld[(size_t)c * 49];
        ok = eg_factor_diag(Dg) && ok;
        for (int a = P.col_ptr[c]; a < P.col_ptr[c + 1]; a++)
            for (int i = 0; i < 7; i++) eg_scale_row(&Lo[(size_t)a * 49 + 7 * i], Dg);
        for (int u = P.upd_ptr[c]; u < P.upd_ptr[c + 1]; u++) {
            const int t = P.upd[3 * (size_t)u];
            const double *La = &Lo[(size_t)P.upd[3 * (size_t)u + 1] * 49], *Lb = &Lo[(size_t)P.upd[3 * (size_t)u + 2] * 49];
            double* T = t >= 0 ? &Lo[(size_t)t * 49] : &Ld[(size_t)(~t) * 49];
            for (int i = 0; i < 7; i++)
                for (int j = 0; j < 7; j++) T[7 * i + j] = eg_update_entry(T[7 * i + j], La + 7 * i, Lb + 7 * j, Dg);
        }
    }
    std::vector<double>& y = *x;
    y = Y.b;
    for (int c = 0; c < P.nf; c++) {  // L y = b
        const double* Dg = &Ld[(size_t)c * 49];
        double* yc = &y[(size_t)c * 7];
        for (int i = 0; i < 7; i++)
            for (int k = 0; k < i; k++) yc[i] = yc[i] - Dg[7 * i + k] * yc[k];
        for (int a = P.col_ptr[c]; a < P.col_ptr[c + 1]; a++) {
            double* yr = &y[(size_t)P.row_of[a] * 7];
            for (int i = 0; i < 7; i++)
                for (int j = 0; j < 7; j++) yr[i] = yr[i] - Lo[(size_t)a * 49 + 7 * i + j] * yc[j];
        }
    }
    for (int c = 0; c < P.nf; c++)
        for (int k = 0; k < 7; k++) y[(size_t)c * 7 + k] = y[(size_t)c * 7 + k] / Ld[(size_t)c * 49 + 8 * k];
    for (int c = P.nf - 1; c >= 0; c--) {  // L^T x = y
        const double* Dg = &Ld[(size_t)c * 49];
        double* yc = &y[(size_t)c * 7];
        for (int a = P.col_ptr[c]; a < P.col_ptr[c + 1]; a++) {
            const double* yr = &y[(size_t)P.row_of[a] * 7];
            for (int j = 0; j < 7; j++)
                for (int i = 0; i < 7; i++) yc[j] = yc[j] - Lo[(size_t)a * 49 + 7 * i + j] * yr[i];
        }
        for (int i = 6; i >= 0; i--)
            for (int k = 6; k > i; k--) yc[i] = yc[i] - Dg[7 * k + i] * yc[k];
    }
    if (!ok) std::fill(y.begin(), y.end(), 0.0);
    return ok;
}

struct EgHostResult {
    double chi2_before = 0, chi2_after = 0;
    int iterations = 0, status = 0;
    int trials[32] = {};
};

// The whole optimisation on the host, sequentially: est (nv) in and out
inline EgHostResult eg_optimize_host(int nv, int fixed, int ne, const EgEdge* edges, int fix_scale, int iterations,
                                     Sim3d* est) {
    EgHostResult R;
    const EgPlan P = eg_plan(nv, fixed, ne, edges);
    if (iterations > 32) iterations = 32;
    if (P.nf == 0 || ne == 0 || iterations <= 0) {
        R.status = kEgTerminate;
        return R;
    }
    EgSystem Y;
    S3oLm L{};
    std::vector<double> x;
    std::vector<Sim3d> trial(est, est + nv);
    bool stopped = false;
    for (int it = 0; it < iterations; it++) {
        eg_build_host(P, edges, est, fix_scale, &Y);
        if (it == 0) R.chi2_before = Y.chi2;
        lm_begin(L, it, Y.chi2, [] { return kEgLambdaInit; });
        bool more;
        do {
            const bool ok2 = eg_solve_host(P, Y, L.lambda, &x);
            double tempChi = 0, scale = 0;
            if (ok2) {
                for (int c = 0; c < P.nf; c++) s3o_oplus(est[P.vert_of[c]], &x[(size_t)c * 7], fix_scale, &trial[P.vert_of[c]]);
                for (int e = 0; e < ne; e++) {
                    double err[7];
                    eg_edge_error(edges[e].C, trial[edges[e].v0], trial[edges[e].v1], err);
                    tempChi = tempChi + eg_chi2(err);
                }
                for (size_t k = 0; k < x.size(); k++) scale = scale + x[k] * (L.lambda * x[k] + Y.b[k]);
            } else {
                R.status |= kEgSolveFailed;
            }
            if (lm_trial(L, ok2, tempChi, scale, &more, LmCubeMul())) {
                for (int c = 0; c < P.nf; c++) est[P.vert_of[c]] = trial[P.vert_of[c]];
            } else {
                R.status |= kEgRejected;
            }
        } while (more);
        R.trials[it] = L.qmax;
        R.iterations++;
        if (lm_end(L)) {
            stopped = true;
            break;
        }
    }
    if (stopped) R.status |= kEgTerminate;
    R.chi2_after = L.currentChi;
    return R;
}
}  // namespace orbmi
