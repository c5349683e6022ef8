// C ABI of loop closing (include/orbmi.h): SearchByBoW(KF, KF), the Sim3 solver, searches and
// optimiser of ComputeSim3, and CorrectLoop's Fuse(KF, Scw), essential graph and point correction.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "capi_stage.h"
#include "essgraph_edges.h"
#include "essgraph_launch.h"
#include "sim3.h"
#include "sim3_horn.h"

using orbmi::DevFrame;
using orbmi::DevFV;
using orbmi::Matcher;
using orbmi::on_device;
using orbmi::Stage;

namespace {

// Scw = [sRcw | t] into T = [Rcw | tcw] and the camera centre Ow (src/ORBmatcher.cc:368-374,
// :1148-1153), float: scw = sqrt(row 0 . row 0) (the dot product in double, rounded to float),
// Rcw = sRcw / scw, tcw = t / scw, Ow = -Rcw^T tcw.  Returns scw; what a degenerate one means is
// the caller's business.
float decompose_scw(const float* Scw, float T[12], float Ow[3]) {
    const float scw = (float)sqrt(((double)Scw[0] * Scw[0] + (double)Scw[1] * Scw[1]) + (double)Scw[2] * Scw[2]);
    for (int k = 0; k < 12; k++) T[k] = Scw[k] / scw;
    for (int c = 0; c < 3; c++) Ow[c] = -((T[c] * T[3] + T[4 + c] * T[7]) + T[8 + c] * T[11]);
    return scw;
}

}  // namespace

extern "C" {

int orbmi_search_by_bow_kf(orbmi_matcher* h, const orbmi_frame_view* kf1, const uint8_t* ok1,
                           const orbmi_feature_vector* fv1, const orbmi_frame_view* kf2, const uint8_t* ok2,
                           const orbmi_feature_vector* fv2, float nnratio, int check_ori, int32_t* match12,
                           int* nmatches) {
    if (!h || !kf1 || !kf2 || !match12 || (kf1->n > 0 && !ok1) || (kf2->n > 0 && !ok2)) return ORBMI_E_ARG;
    if (kf1->n_device || kf2->n_device) return ORBMI_E_ARG;  // keyframes: host-known counts
    Stage s(h);
    const DevFrame K1 = s.frame(kf1, false);
    const DevFrame K2 = s.frame(kf2, false);
    const DevFV f1 = s.fv(fv1);
    const DevFV f2 = s.fv(fv2);
    const uint8_t* d_ok1 = s.in(ok1, (size_t)K1.n);
    const uint8_t* d_ok2 = s.in(ok2, (size_t)K2.n);
    int* d_n = s.scalars();
    int* d_matched2 = s.scratch<int>((size_t)K2.n);  // vbMatched2
    int* d_out = s.out(match12, (size_t)K1.n);
    if (s.rc || s.fail(orbmi::launch_bow_kf(s.m, K1, d_ok1, f1, K2, d_ok2, f2, nnratio, check_ori, d_out, d_matched2, d_n)))
        return s.rc;
    ORBMI_HIP(hipGetLastError());
    return s.finish({{nmatches, d_n}});
}

int orbmi_sim3_ransac_batch(orbmi_matcher* h, int nsolvers, const orbmi_sim3_problem* problems,
                            orbmi_sim3_hypotheses* results) {
    if (!h || nsolvers < 0 || (nsolvers > 0 && (!problems || !results))) return ORBMI_E_ARG;
    // everything is validated before anything is staged or launched
    std::vector<int> its((size_t)nsolvers);
    int max_its = 0;
    for (int k = 0; k < nsolvers; k++) {
        const orbmi_sim3_problem& P = problems[k];
        if (P.n < 0 || P.min_inliers < 0 || P.max_iterations < 0) return ORBMI_E_ARG;
        its[k] = orbmi::sim3_iterations(P.n, P.min_inliers, P.probability, P.max_iterations);
        if (its[k] == 0) continue;
        const orbmi_sim3_hypotheses& R = results[k];
        if (P.n < 3 || !P.x3d_c1 || !P.x3d_c2 || !P.max_err1 || !P.max_err2 || !R.T12 || !R.T21 || !R.s || !R.count ||
            !R.mask)
            return ORBMI_E_ARG;
        if (P.triples) {
            if (on_device(P.triples)) return ORBMI_E_ARG;
            for (int j = 0; j < 3 * its[k]; j++)
                if (P.triples[j] < 0 || P.triples[j] >= P.n) return ORBMI_E_ARG;
        }
        max_its = std::max(max_its, its[k]);
    }
    for (int k = 0; k < nsolvers; k++) results[k].iterations = its[k];
    if (max_its == 0) return ORBMI_OK;
    Stage s(h);
    std::vector<orbmi::Sim3Dev> T((size_t)nsolvers);
    std::vector<int32_t> tri, avail;
    for (int k = 0; k < nsolvers; k++) {
        const orbmi_sim3_problem& P = problems[k];
        orbmi::Sim3Dev& D = T[k];
        memset(&D, 0, sizeof(D));
        D.n = P.n;
        D.iterations = its[k];
        if (its[k] == 0) continue;
        const size_t n = (size_t)P.n, H = (size_t)its[k], words = (n + 63) / 64;
        D.fix_scale = P.fix_scale;
        D.x1 = s.in(P.x3d_c1, 3 * n);
        D.x2 = s.in(P.x3d_c2, 3 * n);
        D.e1 = s.in(P.max_err1, n);
        D.e2 = s.in(P.max_err2, n);
        memcpy(D.k1, P.k1, sizeof(D.k1));
        memcpy(D.k2, P.k2, sizeof(D.k2));
        if (P.triples) {
            D.triples = s.in(P.triples, 3 * H);
        } else {
            tri.resize(3 * H);
            avail.resize(n);
            for (int it = 0; it < its[k]; it++)
                orbmi::sim3_sample_triple(P.seed, k, it, P.n, avail.data(), tri.data() + 3 * (size_t)it);
            D.triples = s.put(tri);  // copied into the arena's mirror at once
        }
        const orbmi_sim3_hypotheses& R = results[k];
        D.T12 = s.out(R.T12, 12 * H);
        D.T21 = s.out(R.T21, 12 * H);
        D.s = s.out(R.s, H);
        D.count = s.out(R.count, H);
        D.mask = s.out(R.mask, H * words);
        if (s.rc) return s.rc;
    }
    const orbmi::Sim3Dev* d_T = s.put(T);
    if (s.rc || s.fail(orbmi::launch_sim3_ransac(s.m, nsolvers, d_T, max_its))) return s.rc;
    return s.finish();
}

int orbmi_search_by_sim3(orbmi_matcher* h, const orbmi_frame_view* kf1, const orbmi_mappoint* mps1, const uint8_t* has_mp1,
                         const orbmi_frame_view* kf2, const orbmi_mappoint* mps2, const uint8_t* has_mp2, float s12,
                         const float* R12, const float* t12, float th, int32_t* match12, int* nfound, int32_t* vn_match1,
                         int32_t* vn_match2) {
    if (!h || !kf1 || !kf2 || !R12 || !t12 || kf1->n < 0 || kf2->n < 0 || (kf1->n > 0 && (!mps1 || !has_mp1 || !match12)) ||
        (kf2->n > 0 && (!mps2 || !has_mp2)) || on_device(R12) || on_device(t12))
        return ORBMI_E_ARG;
    if (nfound) *nfound = 0;
    Stage s(h);
    orbmi::Sim3Side S[2];
    memset(S, 0, sizeof(S));
    const DevFrame K1 = s.frame(kf1, true);
    const DevFrame K2 = s.frame(kf2, true);
    if (s.rc) return s.rc;
    if (K1.tcw_dev || K2.tcw_dev) return ORBMI_E_ARG;  // the poses travel by value
    const size_t n1 = (size_t)kf1->n, n2 = (size_t)kf2->n;
    S[0].F = K2; S[0].n_src = kf1->n;
    S[1].F = K1; S[1].n_src = kf2->n;
    S[0].mps = s.in(mps1, n1); S[0].has = s.in(has_mp1, n1);
    S[1].mps = s.in(mps2, n2); S[1].has = s.in(has_mp2, n2);
    memcpy(S[0].Tcw, K1.tcw, sizeof(S[0].Tcw));
    memcpy(S[1].Tcw, K2.tcw, sizeof(S[1].Tcw));
    // sR12 = s12 * R12, sR21 = (1.0 / s12) * R12^T, t21 = -sR21 * t12 (:1304-1308): the scalar a
    // double, the matrix float, one rounding to float per entry; the products float, left to right
    const double inv = 1.0 / (double)s12;
    float sR21[9];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            S[1].S[4 * r + c] = (float)((double)s12 * (double)R12[3 * r + c]);
            sR21[3 * r + c] = (float)(inv * (double)R12[3 * c + r]);
            S[0].S[4 * r + c] = sR21[3 * r + c];
        }
    for (int r = 0; r < 3; r++) {
        S[1].S[4 * r + 3] = t12[r];
        S[0].S[4 * r + 3] = -((sR21[3 * r] * t12[0] + sR21[3 * r + 1] * t12[1]) + sR21[3 * r + 2] * t12[2]);
    }
    for (int k = 0; k < 2; k++) { S[k].fx = kf1->fx; S[k].fy = kf1->fy; S[k].cx = kf1->cx; S[k].cy = kf1->cy; }
    int* d_m12 = s.inout(match12, n1);
    S[0].vn = vn_match1 ? s.out(vn_match1, n1) : s.scratch<int>(n1);
    S[1].vn = vn_match2 ? s.out(vn_match2, n2) : s.scratch<int>(n2);
    uint8_t* d_already2 = s.scratch<uint8_t>(n2);
    orbmi::Sim3Side* d_S = s.scratch<orbmi::Sim3Side>(2);
    int* d_n = s.scalars();
    if (s.rc || s.fail(orbmi::launch_search_by_sim3(s.m, S, d_S, d_m12, d_already2, th, d_n))) return s.rc;
    return s.finish({{nfound, d_n}});
}

int orbmi_search_by_projection_sim3(orbmi_matcher* h, const orbmi_frame_view* kf, const float* Scw, const orbmi_mappoint* mps,
                                    int n, int32_t* matched, float th, int* nmatches) {
    if (!h || !kf || !Scw || n < 0 || kf->n < 0 || (n > 0 && !mps) || (kf->n > 0 && !matched) || on_device(Scw) ||
        on_device(matched))
        return ORBMI_E_ARG;
    const int nk = kf->n, cap = Matcher::kCandCap;
    for (int k = 0; k < nk; k++)
        if (matched[k] < -2 || matched[k] >= n) return ORBMI_E_ARG;
    if (nmatches) *nmatches = 0;
    if (n == 0 || nk == 0) return ORBMI_OK;
    Stage s(h);
    Matcher& m = s.m;
    int rc = 0;
    const DevFrame F = s.frame(kf, false);
    orbmi::ProjSim3Args a;
    memset(&a, 0, sizeof(a));
    (void)decompose_scw(Scw, a.T, a.Ow);  // (no test of scw here: a degenerate Scw finds nothing)
    // spAlreadyFound and the occupied keypoints
    std::vector<uint8_t> skip((size_t)n, 0), occ((size_t)nk, 0);
    for (int k = 0; k < nk; k++) {
        if (matched[k] >= 0) skip[matched[k]] = 1;
        occ[k] = matched[k] != -1;
    }
    a.mps = s.in(mps, (size_t)n);
    a.skip = s.put(skip);
    uint8_t* d_occ = s.scratch<uint8_t>((size_t)nk);
    a.list = s.scratch<unsigned long long>((size_t)n * cap);
    a.count = s.scratch<int>((size_t)n);
    a.best = s.scratch<unsigned long long>((size_t)n);
    if (s.rc) return s.rc;
    ORBMI_HIP(m.h2d(d_occ, occ.data(), (size_t)nk));
    a.occ = d_occ;
    a.first = 0;
    a.n = n;
    a.th = th;
    ORBMI_HIP(hipMemsetAsync(a.count, 0, (size_t)n * sizeof(int), m.ls()));
    if ((rc = orbmi::launch_proj_sim3(m, F, a))) return rc;
    std::vector<unsigned long long> list((size_t)n * cap);
    std::vector<int> count((size_t)n);
    ORBMI_HIP(hipMemcpyAsync(count.data(), a.count, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, m.ls()));
    ORBMI_HIP(hipMemcpyAsync(list.data(), a.list, list.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, m.ls()));
    ORBMI_HIP(hipStreamSynchronize(m.ls()));
    // the reference's loop in list order: the best unclaimed keypoint, accepted at <= TH_LOW, which
    // is the best unclaimed among the candidates <= TH_LOW
    int found = 0;
    for (int i = 0; i < n; i++) {
        if (count[i] == 0) continue;
        int idx = -1;
        if (count[i] <= cap) {
            unsigned long long* L = &list[(size_t)i * cap];
            std::sort(L, L + count[i]);
            for (int k = 0; k < count[i] && idx < 0; k++)
                if (!occ[L[k] & 0xFFFFF]) idx = (int)(L[k] & 0xFFFFF);
        } else {  // the list overflowed: enumerate this point again against the claims so far
            orbmi::ProjSim3Args b = a;
            b.first = i;
            b.n = 1;
            ORBMI_HIP(m.h2d(d_occ, occ.data(), (size_t)nk));
            ORBMI_HIP(hipMemsetAsync(a.count + i, 0, sizeof(int), m.ls()));
            if ((rc = orbmi::launch_proj_sim3(m, F, b))) return rc;
            unsigned long long best = ~0ull;
            ORBMI_HIP(hipMemcpyAsync(&best, a.best + i, sizeof(best), hipMemcpyDeviceToHost, m.ls()));
            ORBMI_HIP(hipStreamSynchronize(m.ls()));
            if (best != ~0ull && (int)(best >> 40) <= orbmi::TH_LOW) idx = (int)(best & 0xFFFFF);
        }
        if (idx < 0) continue;
        matched[idx] = i;
        occ[idx] = 1;
        found++;
    }
    if (nmatches) *nmatches = found;
    return s.finish();  // (everything was read back above)
}

int orbmi_fuse_sim3_search_batch(orbmi_matcher* h, int nkf, const orbmi_frame_view* kfs, const float* Scw,
                                 const orbmi_mappoint* mps, const uint8_t* in_kf, int n_mp, float th, int32_t* best_idx,
                                 int32_t* best_dist, int* nfused) {
    if (!h || nkf < 0 || n_mp < 0 || (nkf > 0 && (!kfs || !Scw || on_device(Scw))) ||
        (nkf > 0 && n_mp > 0 && (!mps || !best_idx || !best_dist)))
        return ORBMI_E_ARG;
    // one decomposed Scw per keyframe
    std::vector<orbmi::FuseSim3Pose> poses((size_t)nkf);
    for (int k = 0; k < nkf; k++) {
        const float scw = decompose_scw(Scw + 12 * (size_t)k, poses[k].T, poses[k].Ow);
        if (!(scw > 0.0f) || !std::isfinite(scw)) return ORBMI_E_ARG;
    }
    if (nkf == 0 || n_mp == 0) return ORBMI_OK;
    Stage s(h);
    const orbmi_mappoint* d_mps = s.in(mps, (size_t)n_mp);
    const uint8_t* d_in = s.in(in_kf, (size_t)n_mp * nkf);
    // (the poses ahead of the frames and the table, so that everything still goes up in one copy)
    const orbmi::FuseSim3Pose* d_p = s.put(poses);
    orbmi::FuseTable T;
    if (s.rc || orbmi::fuse_table(s, nkf, kfs, nullptr, false, d_in, n_mp, best_idx, best_dist, &T)) return s.rc;
    if (s.fail(orbmi::launch_fuse_sim3(s.m, nkf, T.d_k, d_p, d_mps, n_mp, th, T.ncap))) return s.rc;
    return s.finish({{nfused, T.d_cnt, nkf}});
}

namespace {

bool sim3_opt_args_ok(const orbmi_sim3_opt_problem& P) {
    if (P.n < 0) return false;
    return P.n == 0 || (P.x3d_c1 && P.x3d_c2 && P.obs1 && P.obs2 && P.inv_sigma2_1 && P.inv_sigma2_2);
}

// Stage one problem; inlier / chi2 are device arrays of n and 2 n entries
void sim3_opt_stage(Stage& s, const orbmi_sim3_opt_problem& P, uint8_t* inlier, double* chi2, orbmi::Sim3OptDev* D) {
    memset(D, 0, sizeof(*D));
    const size_t n = (size_t)P.n;
    D->n = P.n;
    D->fix_scale = P.fix_scale != 0;
    D->th2 = P.th2;
    D->x1 = s.in(P.x3d_c1, 3 * n);
    D->x2 = s.in(P.x3d_c2, 3 * n);
    D->o1 = s.in(P.obs1, 2 * n);
    D->o2 = s.in(P.obs2, 2 * n);
    D->w1 = s.in(P.inv_sigma2_1, n);
    D->w2 = s.in(P.inv_sigma2_2, n);
    memcpy(D->k1, P.k1, sizeof(D->k1));
    memcpy(D->k2, P.k2, sizeof(D->k2));
    memcpy(D->R, P.R12, sizeof(D->R));
    memcpy(D->t, P.t12, sizeof(D->t));
    D->s = P.s12;
    D->inlier = inlier;
    D->chi2 = chi2;
}

}  // namespace

int orbmi_optimize_sim3_batch(orbmi_matcher* h, int nproblems, const orbmi_sim3_opt_problem* problems,
                              orbmi_sim3_opt_result* results) {
    if (!h || nproblems < 0 || (nproblems > 0 && (!problems || !results))) return ORBMI_E_ARG;
    for (int k = 0; k < nproblems; k++)
        if (!sim3_opt_args_ok(problems[k]) || (problems[k].n > 0 && !results[k].inlier)) return ORBMI_E_ARG;
    if (nproblems == 0) return ORBMI_OK;
    Stage s(h);
    std::vector<orbmi::Sim3OptDev> T((size_t)nproblems);
    std::vector<orbmi::Sim3OptOut> O((size_t)nproblems);
    for (int k = 0; k < nproblems; k++) {
        const size_t n = (size_t)problems[k].n;
        uint8_t* d_in = n ? s.out(results[k].inlier, n) : s.scratch<uint8_t>(1);
        double* d_chi = n && results[k].chi2 ? s.out(results[k].chi2, 2 * n) : s.scratch<double>(2 * n);
        sim3_opt_stage(s, problems[k], d_in, d_chi, &T[k]);
    }
    const orbmi::Sim3OptDev* d_T = s.put(T);
    orbmi::Sim3OptOut* d_O = s.out(O.data(), (size_t)nproblems);
    if (s.rc || s.fail(orbmi::launch_sim3_opt(s.m, nproblems, d_T, d_O))) return s.rc;
    if (s.finish()) return s.rc;  // O is host memory: the call has waited
    for (int k = 0; k < nproblems; k++) {
        orbmi_sim3_opt_result& R = results[k];
        memcpy(R.q, O[k].q, sizeof(R.q));
        memcpy(R.t, O[k].t, sizeof(R.t));
        R.s = O[k].s;
        memcpy(R.sR, O[k].sR, sizeof(R.sR));
        memcpy(R.t_f, O[k].t_f, sizeof(R.t_f));
        R.n_in = O[k].n_in;
        R.n_bad = O[k].n_bad;
        R.iterations[0] = O[k].iterations[0];
        R.iterations[1] = O[k].iterations[1];
    }
    return ORBMI_OK;
}

int orbmi_debug_sim3_opt_linearize(orbmi_matcher* h, const orbmi_sim3_opt_problem* problem, double* H, double* b,
                                   double* chi2) {
    if (!h || !problem || !H || !b || !chi2 || !sim3_opt_args_ok(*problem)) return ORBMI_E_ARG;
    double lin[57] = {};
    if (problem->n > 0) {
        Stage s(h);
        const size_t n = (size_t)problem->n;
        uint8_t* d_in = s.scratch<uint8_t>(n);
        double* d_chi = s.scratch<double>(2 * n);
        orbmi::Sim3OptDev T;
        sim3_opt_stage(s, *problem, d_in, d_chi, &T);
        const orbmi::Sim3OptDev* d_T = s.upload(&T, 1);
        double* d_lin = s.out((double*)lin, 57);
        if (s.rc || s.fail(orbmi::launch_sim3_opt_linearize(s.m, d_T, d_lin))) return s.rc;
        if (s.finish()) return s.rc;
    }
    memcpy(H, lin, 49 * sizeof(double));
    memcpy(b, lin + 49, 7 * sizeof(double));
    *chi2 = lin[56];
    return ORBMI_OK;
}

}  // extern "C"

namespace {

static_assert(sizeof(orbmi::Sim3d) == 8 * sizeof(double), "a Sim3 is 8 doubles in the C interface");

bool essgraph_args_ok(const orbmi_essgraph_problem& P) {
    if (P.n_vertices < 1 || !P.vertices || P.n_edges < 0 || P.iterations < 0 || P.iterations > 32) return false;
    if (P.fixed < 0 || P.fixed >= P.n_vertices) return false;
    return P.n_edges == 0 || (P.v0 && P.v1 && P.measurements);
}

std::vector<orbmi::EgEdge> essgraph_edges_of(const orbmi_essgraph_problem& P) {
    std::vector<orbmi::EgEdge> E((size_t)P.n_edges);
    for (int e = 0; e < P.n_edges; e++) {
        E[e].v0 = P.v0[e];
        E[e].v1 = P.v1[e];
        memcpy(&E[e].C, P.measurements + 8 * (size_t)e, sizeof(orbmi::Sim3d));
    }
    return E;
}

// One call's device state: the plan's tables, the edges and two copies of the estimates
struct EssgraphCall {
    orbmi::EgPlan plan;
    orbmi::EgDev D;
    orbmi::Sim3d *est = nullptr, *trial = nullptr;
};

int essgraph_stage(Stage& s, const orbmi_essgraph_problem& P, const std::vector<orbmi::EgEdge>& E, EssgraphCall* C) {
    Matcher& m = s.m;
    C->plan = orbmi::eg_plan(P.n_vertices, P.fixed, P.n_edges, E.data());
    const orbmi::EgPlan& Q = C->plan;
    if (!orbmi::eg_plan_ok(Q)) return s.fail(ORBMI_E_ARG);  // every table index against its array, before any launch
    orbmi::EgDev& D = C->D;
    memset(&D, 0, sizeof(D));
    D.nv = Q.nv; D.ne = Q.ne; D.nf = Q.nf; D.nl = Q.nl;
    D.fix_scale = P.fix_scale != 0;
    D.edges = s.put(E);
    D.vert_of = s.put(Q.vert_of);
    D.col_ptr = s.put(Q.col_ptr);
    D.row_of = s.put(Q.row_of);
    D.upd_ptr = s.put(Q.upd_ptr);
    D.upd = s.put(Q.upd);
    D.asm_ptr = s.put(Q.asm_ptr);
    D.asm_ent = s.put(Q.asm_ent);
    auto doubles = [&](size_t n) { return s.scratch<double>(n); };
    D.recs = doubles((size_t)Q.ne * orbmi::kEgRec);
    D.Hd = doubles((size_t)Q.nf * 49); D.Ho = doubles((size_t)Q.nl * 49); D.b = doubles((size_t)Q.nf * 7);
    D.Ld = doubles((size_t)Q.nf * 49); D.Lo = doubles((size_t)Q.nl * 49); D.x = doubles((size_t)Q.nf * 7);
    D.y = doubles((size_t)Q.nf * 7);
    D.chi2 = doubles((size_t)Q.ne);
    D.out = doubles(orbmi::kEgOut);
    const size_t vb = (size_t)P.n_vertices * sizeof(orbmi::Sim3d);
    C->est = s.scratch<orbmi::Sim3d>((size_t)P.n_vertices);
    C->trial = s.scratch<orbmi::Sim3d>((size_t)P.n_vertices);
    if (s.rc) return s.rc;
    if (m.h2d(C->est, P.vertices, vb) != hipSuccess || m.h2d(C->trial, P.vertices, vb) != hipSuccess) return ORBMI_E_HIP;
    ORBMI_HIP(m.flush_up());
    if (m.up_err != hipSuccess) return ORBMI_E_HIP;
    // fill blocks are never written by the assembly
    if (Q.nl) ORBMI_HIP(hipMemsetAsync(D.Ho, 0, (size_t)Q.nl * 49 * sizeof(double), m.ls()));
    return ORBMI_OK;
}

}  // namespace

extern "C" {

int orbmi_essential_graph_edges(const orbmi_essgraph_input* g, int max_edges, int32_t* v0, int32_t* v1,
                                double* measurements, double* vScw, int* n_edges) {
    if (!g || !n_edges || !vScw || max_edges < 0 || (max_edges > 0 && (!v0 || !v1 || !measurements))) return ORBMI_E_ARG;
    orbmi::EgGraphIn G;
    G.n_ids = g->n_ids;
    G.live = g->live; G.Tcw = g->Tcw; G.parent = g->parent;
    G.loop_off = g->loop_off; G.loop_ids = g->loop_ids;
    G.cov_off = g->cov_off; G.cov_ids = g->cov_ids;
    G.n_corrected = g->n_corrected; G.corrected_ids = g->corrected_ids; G.corrected = (const orbmi::Sim3d*)g->corrected;
    G.n_noncorrected = g->n_noncorrected; G.noncorrected_ids = g->noncorrected_ids;
    G.noncorrected = (const orbmi::Sim3d*)g->noncorrected;
    G.lc_off = g->lc_off; G.lc_ids = g->lc_ids; G.lc_weight = g->lc_weight;
    G.loop_id = g->loop_id; G.cur_id = g->cur_id;
    if (!orbmi::eg_graph_args_ok(G)) return ORBMI_E_ARG;
    std::vector<orbmi::EgGraphEdge> E;
    std::vector<orbmi::Sim3d> S;
    orbmi::eg_graph_edges(G, &E, &S);
    memcpy(vScw, S.data(), S.size() * sizeof(orbmi::Sim3d));
    *n_edges = (int)E.size();
    if ((int)E.size() > max_edges) return ORBMI_E_CAP;
    for (size_t e = 0; e < E.size(); e++) {
        v0[e] = E[e].v0;
        v1[e] = E[e].v1;
        memcpy(measurements + 8 * e, &E[e].S, sizeof(orbmi::Sim3d));
    }
    return ORBMI_OK;
}

int orbmi_optimize_essential_graph(orbmi_matcher* h, const orbmi_essgraph_problem* problem, orbmi_essgraph_result* result) {
    if (!h || !problem || !result || !result->vertices || !essgraph_args_ok(*problem)) return ORBMI_E_ARG;
    const orbmi_essgraph_problem& P = *problem;
    const std::vector<orbmi::EgEdge> E = essgraph_edges_of(P);
    if (!orbmi::eg_args_ok(P.n_vertices, P.fixed, P.n_edges, E.data())) return ORBMI_E_ARG;
    orbmi_essgraph_result& R = *result;
    R.chi2_before = R.chi2_after = 0;
    R.iterations = 0;
    R.status = 0;
    memset(R.trials, 0, sizeof(R.trials));
    memset(R.phase_ms, 0, sizeof(R.phase_ms));
    const size_t vb = (size_t)P.n_vertices * sizeof(orbmi::Sim3d);
    Stage s(h);
    Matcher& m = s.m;
    EssgraphCall C;
    int rc = essgraph_stage(s, P, E, &C);
    if (rc) return rc;
    if (C.plan.nf == 0 || P.n_edges == 0 || P.iterations == 0) {  // nothing to optimise
        memmove(R.vertices, P.vertices, vb);
        R.status = ORBMI_EG_TERMINATE;
        ORBMI_HIP(hipStreamSynchronize(m.ls()));
        return ORBMI_OK;
    }
    const orbmi::EgDev& D = C.D;
    orbmi::PhaseTimer T(m.ls(), P.profile != 0);
    orbmi::S3oLm L{};
    double out[orbmi::kEgOut];
    auto read_out = [&]() -> int {
        ORBMI_HIP(hipMemcpyAsync(out, D.out, sizeof(out), hipMemcpyDeviceToHost, m.ls()));
        ORBMI_HIP(hipStreamSynchronize(m.ls()));
        return ORBMI_OK;
    };
    bool stopped = false;
    for (int it = 0; it < P.iterations; it++) {
        T.begin();
        if ((rc = orbmi::launch_eg_linearize(m, D, C.est))) return rc;
        T.end(&R.phase_ms[0]);
        T.begin();
        if ((rc = orbmi::launch_eg_assemble(m, D))) return rc;
        T.end(&R.phase_ms[1]);
        if ((rc = read_out())) return rc;
        if (it == 0) R.chi2_before = out[orbmi::kEgOutChi];
        orbmi::lm_begin(L, it, out[orbmi::kEgOutChi], [] { return orbmi::kEgLambdaInit; });
        bool more;
        do {
            T.begin();
            if ((rc = orbmi::launch_eg_factor_solve(m, D, L.lambda))) return rc;
            T.end(&R.phase_ms[2]);
            if ((rc = read_out())) return rc;
            const bool ok2 = out[orbmi::kEgOutFail] == 0;
            const double scale = ok2 ? out[orbmi::kEgOutScale] : 0.0;
            double tempChi = 0;
            if (ok2) {
                T.begin();
                if ((rc = orbmi::launch_eg_update(m, D, C.est, C.trial))) return rc;
                T.end(&R.phase_ms[3]);
                if ((rc = read_out())) return rc;
                tempChi = out[orbmi::kEgOutChi];
            } else {
                R.status |= ORBMI_EG_SOLVE_FAILED;
            }
            if (orbmi::lm_trial(L, ok2, tempChi, scale, &more, orbmi::LmCubeMul())) std::swap(C.est, C.trial);  // the step is kept
            else R.status |= ORBMI_EG_REJECTED;  // est still holds the accepted estimates
        } while (more);
        R.trials[it] = L.qmax;
        R.iterations++;
        if (orbmi::lm_end(L)) {
            stopped = true;
            break;
        }
    }
    if (stopped) R.status |= ORBMI_EG_TERMINATE;
    R.chi2_after = L.currentChi;
    ORBMI_HIP(hipMemcpyAsync(R.vertices, C.est, vb, hipMemcpyDeviceToHost, m.ls()));
    ORBMI_HIP(hipStreamSynchronize(m.ls()));
    return ORBMI_OK;
}

int orbmi_debug_essgraph_linearize(orbmi_matcher* h, const orbmi_essgraph_problem* problem, int32_t* dims,
                                   int32_t* vert_of, int32_t* col_ptr, int32_t* row_of, double* Hd, double* Ho,
                                   double* b, double* chi2) {
    if (!h || !problem || !dims || !essgraph_args_ok(*problem)) return ORBMI_E_ARG;
    const orbmi_essgraph_problem& P = *problem;
    const std::vector<orbmi::EgEdge> E = essgraph_edges_of(P);
    if (!orbmi::eg_args_ok(P.n_vertices, P.fixed, P.n_edges, E.data())) return ORBMI_E_ARG;
    if (!vert_of) {
        const orbmi::EgPlan Q = orbmi::eg_plan(P.n_vertices, P.fixed, P.n_edges, E.data());
        dims[0] = Q.nf;
        dims[1] = Q.nl;
        return ORBMI_OK;
    }
    if (!col_ptr || !row_of || !Hd || !Ho || !b || !chi2) return ORBMI_E_ARG;
    Stage s(h);
    Matcher& m = s.m;
    EssgraphCall C;
    int rc = essgraph_stage(s, P, E, &C);
    if (rc) return rc;
    const orbmi::EgPlan& Q = C.plan;
    dims[0] = Q.nf;
    dims[1] = Q.nl;
    memcpy(vert_of, Q.vert_of.data(), Q.vert_of.size() * sizeof(int32_t));
    memcpy(col_ptr, Q.col_ptr.data(), Q.col_ptr.size() * sizeof(int32_t));
    memcpy(row_of, Q.row_of.data(), Q.row_of.size() * sizeof(int32_t));
    *chi2 = 0;
    if (Q.ne > 0) {
        if ((rc = orbmi::launch_eg_linearize(m, C.D, C.est))) return rc;
        if ((rc = orbmi::launch_eg_assemble(m, C.D))) return rc;
        ORBMI_HIP(hipMemcpyAsync(chi2, C.D.out + orbmi::kEgOutChi, sizeof(double), hipMemcpyDeviceToHost, m.ls()));
        if (Q.nf) {
            ORBMI_HIP(hipMemcpyAsync(Hd, C.D.Hd, (size_t)Q.nf * 49 * sizeof(double), hipMemcpyDeviceToHost, m.ls()));
            ORBMI_HIP(hipMemcpyAsync(b, C.D.b, (size_t)Q.nf * 7 * sizeof(double), hipMemcpyDeviceToHost, m.ls()));
        }
        if (Q.nl) ORBMI_HIP(hipMemcpyAsync(Ho, C.D.Ho, (size_t)Q.nl * 49 * sizeof(double), hipMemcpyDeviceToHost, m.ls()));
    }
    ORBMI_HIP(hipStreamSynchronize(m.ls()));
    return ORBMI_OK;
}

int orbmi_correct_points_sim3(orbmi_matcher* h, int n_points, const float* points, const int32_t* ref, int n_ref,
                              const double* Srw, const double* Swr_corrected, float* out_points, int n_poses,
                              const double* poses, float* out_tcw) {
    if (!h || n_points < 0 || n_ref < 0 || n_poses < 0) return ORBMI_E_ARG;
    if (n_points > 0 && (!points || !ref || !Srw || !Swr_corrected || !out_points || n_ref < 1)) return ORBMI_E_ARG;
    if (n_poses > 0 && (!poses || !out_tcw)) return ORBMI_E_ARG;
    for (int i = 0; i < n_points; i++)
        if (ref[i] < 0 || ref[i] >= n_ref) return ORBMI_E_ARG;
    if (n_points == 0 && n_poses == 0) return ORBMI_OK;
    Stage s(h);
    const float* d_p = s.in(points, 3 * (size_t)n_points);
    const int32_t* d_r = s.in(ref, (size_t)n_points);
    const orbmi::Sim3d* d_a = s.in((const orbmi::Sim3d*)Srw, n_points ? (size_t)n_ref : 0);
    const orbmi::Sim3d* d_b = s.in((const orbmi::Sim3d*)Swr_corrected, n_points ? (size_t)n_ref : 0);
    const orbmi::Sim3d* d_s = s.in((const orbmi::Sim3d*)poses, (size_t)n_poses);
    float* d_op = n_points ? s.out(out_points, 3 * (size_t)n_points) : nullptr;
    float* d_ot = n_poses ? s.out(out_tcw, 16 * (size_t)n_poses) : nullptr;
    if (s.rc || s.fail(orbmi::launch_eg_correct(s.m, n_points, d_p, d_r, d_a, d_b, d_op, n_poses, d_s, d_ot))) return s.rc;
    return s.finish();
}

}  // extern "C"
