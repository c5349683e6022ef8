// C ABI of LocalMapping's searches (include/orbmi.h): ComputeDistinctiveDescriptors,
// SearchForTriangulation, CreateNewMapPoints, Fuse, and one LocalMapping::Run iteration as one
// call.  The order of the staging calls below is the order of the uploads: Matcher::h2d merges
// uploads into adjacent allocations into one copy, and a job's "one upload" depends on it.
#include <cstring>

#include "capi_stage.h"
#include "tri_geom.h"

using orbmi::DevFrame;
using orbmi::DevFV;
using orbmi::FuseKF;
using orbmi::FuseTable;
using orbmi::Matcher;
using orbmi::on_device;
using orbmi::Stage;
using orbmi::TriPair;

namespace orbmi {

int fuse_table(Stage& s, int nkf, const orbmi_frame_view* kfs, const DevFrame* frames, bool view_pose, const uint8_t* d_in,
               int n_mp, int32_t* best_idx, int32_t* best_dist, FuseTable* T) {
    std::vector<FuseKF> K(nkf);
    for (int k = 0; k < nkf; k++) {
        memset(&K[k], 0, sizeof(FuseKF));
        K[k].F = frames ? frames[k] : s.frame(&kfs[k], view_pose);
        if (s.rc) return s.rc;
        K[k].in_kf = d_in ? d_in + (size_t)k * n_mp : nullptr;
    }
    T->nkf = nkf;
    T->n = n_mp;
    T->d_k = s.scratch<FuseKF>((size_t)nkf);
    T->d_cnt = s.scratch<int>((size_t)nkf);
    T->d_bi = s.out(best_idx, (size_t)n_mp * nkf);
    T->d_bd = s.out(best_dist, (size_t)n_mp * nkf);
    if (s.rc || s.fail(fuse_multi_prepare(s.m, nkf, K.data(), n_mp, T->d_bi, T->d_bd, T->d_cnt, &T->ncap))) return s.rc;
    if (s.m.h2d(T->d_k, K.data(), sizeof(FuseKF) * nkf) != hipSuccess) return s.fail(ORBMI_E_HIP);
    return ORBMI_OK;
}

}  // namespace orbmi

namespace {

// ComputeDistinctiveDescriptors' arrays on the device.  in_place: obs_desc is used as it is; else
// it is host memory, staged by its row count off[np].  desc_out is updated in place (a point
// without observations keeps its descriptor).
struct Distinctive {
    const uint8_t* desc = nullptr;
    const int* off = nullptr;
    int* best = nullptr;
    uint8_t* out = nullptr;
};

int stage_distinctive(Stage& s, const uint8_t* obs_desc, const int32_t* obs_off, int np, bool in_place, int32_t* best,
                      uint8_t* desc_out, Distinctive* D) {
    D->desc = obs_desc;
    if (!in_place) {
        int total = 0;
        if (s.fail(orbmi::csr_total(obs_off, np, &total))) return s.rc;
        if (total < 0 || (total > 0 && !obs_desc)) return s.fail(ORBMI_E_ARG);
        if (total > 0) D->desc = s.upload(obs_desc, (size_t)total * 32);
    }
    D->off = s.in(obs_off, (size_t)np + 1);
    D->best = s.out(best, (size_t)np);
    D->out = s.inout(desc_out, (size_t)np * 32);
    return s.rc;
}

// The pair table of SearchForTriangulation: per pair KF2's frame, FeatureVector and flags, staged
// in that order, and F12; each(j, pair) then stages what its caller keeps beside pair j.
template <class Each>
int tri_table(Stage& s, int npairs, const orbmi_frame_view* kf2, const uint8_t* const* has_mp2,
              const orbmi_feature_vector* fv2, const float* F12, std::vector<TriPair>* pairs, Each each) {
    std::vector<float> Fh((size_t)9 * npairs);
    if (s.fail(orbmi::to_host(F12, Fh.size(), Fh.data()))) return s.rc;
    pairs->resize(npairs);
    for (int j = 0; j < npairs; j++) {
        TriPair& T = (*pairs)[j];
        memset(&T, 0, sizeof(T));
        if (!kf2[j].u_right || !has_mp2[j]) return s.fail(ORBMI_E_ARG);
        T.KF2 = s.frame(&kf2[j], true);
        T.fv2 = s.fv(&fv2[j]);
        T.has_mp2 = s.in(has_mp2[j], (size_t)std::max(T.KF2.n, 1));
        memcpy(T.F12.m, &Fh[(size_t)9 * j], sizeof(T.F12.m));
        if (s.rc || s.fail(each(j, T))) return s.rc;
    }
    return ORBMI_OK;
}

// CreateNewMapPoints in two halves, shared by orbmi_create_new_map_points and
// orbmi_local_mapping_job: cnmp_stage validates the pairs and stages everything that does not
// depend on KF1's FeatureVector (frames, triangulation sides, the pair table and the KF2 sides
// in one upload), cnmp_launch enqueues the searches and the geometry.
struct CnmpPlan {
    DevFrame K1;
    const uint8_t* has1 = nullptr;
    orbmi::tri::Side S1;
    int npairs = 0;
    std::vector<DevFrame> KF2;  // the neighbours' frames (the batched Fuse of a job reuses them)
    TriPair* d_pairs = nullptr;
    const orbmi::tri::Side* d_S2 = nullptr;
    int* d_match = nullptr;
    uint8_t* d_ok = nullptr;
    float* d_x3d = nullptr;
};

int cnmp_stage(Stage& s, const orbmi_frame_view* kf1, const orbmi_tri_keyframe* tri1, const float* cos1,
               const uint8_t* has_mp1, int npairs, const orbmi_frame_view* kf2, const orbmi_tri_keyframe* tri2,
               const float* const* cos2, const uint8_t* const* has_mp2, const orbmi_feature_vector* fv2,
               const float* F12, int32_t* match12, uint8_t* ok, float* x3d, CnmpPlan* P) {
    if (!kf1 || !tri1 || !has_mp1 || !kf1->u_right || npairs <= 0 || !kf2 || !tri2 || !has_mp2 || !fv2 || !F12 ||
        !match12 || !ok || !x3d)
        return s.fail(ORBMI_E_ARG);
    DevFrame& K1 = P->K1;
    K1 = s.frame(kf1, true);
    P->has1 = s.in(has_mp1, (size_t)std::max(K1.n, 1));
    if (s.rc) return s.rc;
    std::vector<std::vector<float>> cos_tmp;  // tables computed here (copied into the arena's mirror at once)
    cos_tmp.reserve((size_t)npairs + 1);
    // the triangulation side of a keyframe: keys / u_right from its frame view (device), the rest
    // from its tri view
    auto side = [&](const orbmi_tri_keyframe* T, const orbmi_frame_view* v, const DevFrame& D, const float* cs,
                    orbmi::tri::Side* S) -> int {
        if (!T->tcw || !T->depth || !T->level_sigma2 || !T->scale_factors || on_device(T->level_sigma2) ||
            on_device(T->scale_factors) || v->nlevels > orbmi::tri::kLevels)
            return ORBMI_E_ARG;
        orbmi::tri::make_side(*T, v->nlevels, S);
        S->keys = D.keys;
        S->ur = D.u_right;
        S->depth = s.in(T->depth, (size_t)D.n);
        if (s.rc) return s.rc;
        if (!cs) {
            if (on_device(T->depth)) return ORBMI_E_ARG;
            cos_tmp.emplace_back((size_t)std::max(D.n, 1));
            int r = orbmi_stereo_parallax_cos(T->mb, T->depth, D.n, cos_tmp.back().data());
            if (r) return r;
            cs = cos_tmp.back().data();
        }
        S->cos_stereo = s.in(cs, (size_t)D.n);
        return s.rc;
    };
    if (s.fail(side(tri1, kf1, K1, cos1, &P->S1))) return s.rc;
    std::vector<orbmi::tri::Side> S2(npairs);
    std::vector<TriPair> pairs;
    P->KF2.resize(npairs);
    if (tri_table(s, npairs, kf2, has_mp2, fv2, F12, &pairs, [&](int j, TriPair& T) {
            P->KF2[j] = T.KF2;
            return side(&tri2[j], &kf2[j], T.KF2, cos2 ? cos2[j] : nullptr, &S2[j]);
        }))
        return s.rc;
    P->npairs = npairs;
    P->d_match = s.out(match12, (size_t)K1.n * npairs);
    P->d_ok = s.out(ok, (size_t)K1.n * npairs);
    P->d_x3d = s.out(x3d, (size_t)3 * K1.n * npairs);
    if (s.rc || s.fail(orbmi::tri_pairs_prepare(s.m, K1, npairs, pairs.data(), P->d_match))) return s.rc;
    // the pair table and the KF2 sides go up in one copy
    const size_t o_s2 = (sizeof(TriPair) * npairs + 255) & ~(size_t)255;
    std::vector<uint8_t> tab(o_s2 + sizeof(orbmi::tri::Side) * npairs);
    memcpy(tab.data(), pairs.data(), sizeof(TriPair) * npairs);
    memcpy(tab.data() + o_s2, S2.data(), sizeof(orbmi::tri::Side) * npairs);
    uint8_t* d_tab = s.put(tab);
    P->d_pairs = (TriPair*)d_tab;
    P->d_S2 = (const orbmi::tri::Side*)(d_tab + o_s2);
    return s.rc;
}

int cnmp_launch(Matcher& m, const CnmpPlan& P, const DevFV& f1) {
    return orbmi::launch_create_points(m, P.K1, P.has1, f1, P.npairs, nullptr, P.d_pairs, P.S1, P.d_S2, P.d_match, P.d_ok,
                                       P.d_x3d);
}

// The batched Fuse search in the same two halves: fuse_batch_stage stages the points and the
// keyframe table (frames: the keyframes' views already resolved, or nullptr), fuse_batch_launch
// enqueues the grids and the search.
struct FusePlan {
    FuseTable T;
    const orbmi_mappoint* d_mps = nullptr;
};

int fuse_batch_stage(Stage& s, int nkf, const orbmi_frame_view* kfs, const DevFrame* frames, const orbmi_mappoint* mps,
                     const uint8_t* in_kf, int n_mp, int32_t* best_idx, int32_t* best_dist, FusePlan* P) {
    P->d_mps = s.in(mps, (size_t)n_mp);
    const uint8_t* d_in = s.in(in_kf, (size_t)std::max(n_mp, 1) * nkf);
    if (s.rc) return s.rc;
    return orbmi::fuse_table(s, nkf, kfs, frames, true, d_in, n_mp, best_idx, best_dist, &P->T);
}

int fuse_batch_launch(Matcher& m, const FusePlan& P, float th) {
    const FuseTable& T = P.T;
    return orbmi::launch_fuse_multi(m, T.nkf, nullptr, T.d_k, P.d_mps, T.n, th, T.d_bi, T.d_bd, T.d_cnt, T.ncap);
}

}  // namespace

extern "C" {

int orbmi_compute_distinctive_descriptors(orbmi_matcher* h, const uint8_t* obs_desc, const int32_t* obs_off, int np,
                                          int32_t* best, uint8_t* desc_out) {
    if (!h || np < 0 || (np > 0 && (!obs_off || !best || !desc_out))) return ORBMI_E_ARG;
    if (np == 0) return ORBMI_OK;
    Stage s(h);
    Distinctive D;
    if (stage_distinctive(s, obs_desc, obs_off, np, on_device(obs_desc), best, desc_out, &D)) return s.rc;
    if (s.fail(orbmi::launch_distinctive(s.m, D.desc, D.off, np, D.best, D.out))) return s.rc;
    return s.finish();
}

int orbmi_search_for_triangulation(orbmi_matcher* h, const orbmi_frame_view* kf1, const uint8_t* has_mp1,
                                   const orbmi_feature_vector* fv1, const orbmi_frame_view* kf2, const uint8_t* has_mp2,
                                   const orbmi_feature_vector* fv2, const float* F12, int only_stereo, int check_ori,
                                   int32_t* match12, int* nmatches) {
    if (!kf2 || !has_mp2 || !fv2 || !F12) return ORBMI_E_ARG;
    const uint8_t* mp2[1] = {has_mp2};
    return orbmi_search_for_triangulation_batch(h, kf1, has_mp1, fv1, 1, kf2, mp2, fv2, F12, only_stereo, check_ori,
                                                match12, nmatches);
}

int orbmi_search_for_triangulation_batch(orbmi_matcher* h, const orbmi_frame_view* kf1, const uint8_t* has_mp1,
                                         const orbmi_feature_vector* fv1, int npairs, const orbmi_frame_view* kf2,
                                         const uint8_t* const* has_mp2, const orbmi_feature_vector* fv2,
                                         const float* F12, int only_stereo, int check_ori, int32_t* match12,
                                         int* nmatches) {
    if (!h || !has_mp1 || !fv1 || !kf1 || !kf1->u_right || npairs < 0 || (npairs > 0 && (!kf2 || !has_mp2 || !fv2 ||
                                                                                      !F12 || !match12)))
        return ORBMI_E_ARG;
    if (npairs == 0) return ORBMI_OK;
    Stage s(h);
    const DevFrame K1 = s.frame(kf1, true);
    const DevFV f1 = s.fv(fv1);
    const uint8_t* d_mp1 = s.in(has_mp1, (size_t)std::max(K1.n, 1));
    int* d_counts = nmatches ? s.scratch<int>((size_t)npairs) : nullptr;
    if (s.rc) return s.rc;
    std::vector<TriPair> pairs;
    if (tri_table(s, npairs, kf2, has_mp2, fv2, F12, &pairs, [&](int j, TriPair& T) {
            T.nmatches = d_counts ? d_counts + j : nullptr;
            return ORBMI_OK;
        }))
        return s.rc;
    TriPair* d_pairs = s.scratch<TriPair>((size_t)npairs);
    int* d_out = s.out(match12, (size_t)K1.n * npairs);
    // (the launch fills the table's scratch pointers in and uploads it)
    if (s.rc || s.fail(orbmi::launch_triangulation(s.m, K1, d_mp1, f1, npairs, pairs.data(), d_pairs, only_stereo, check_ori,
                                                   d_out)))
        return s.rc;
    return s.finish({{nmatches, d_counts, npairs}});
}

int orbmi_create_new_map_points(orbmi_matcher* h, const orbmi_frame_view* kf1, const orbmi_tri_keyframe* tri1,
                                const float* cos1, const uint8_t* has_mp1, const orbmi_feature_vector* fv1,
                                int npairs, const orbmi_frame_view* kf2, const orbmi_tri_keyframe* tri2,
                                const float* const* cos2, const uint8_t* const* has_mp2,
                                const orbmi_feature_vector* fv2, const float* F12, int32_t* match12, uint8_t* ok,
                                float* x3d) {
    if (!h || !kf1 || !tri1 || !has_mp1 || !fv1 || !kf1->u_right || npairs < 0 ||
        (npairs > 0 && (!kf2 || !tri2 || !has_mp2 || !fv2 || !F12 || !match12 || !ok || !x3d)))
        return ORBMI_E_ARG;
    if (npairs == 0) return ORBMI_OK;
    Stage s(h);
    const DevFV f1 = s.fv(fv1);
    CnmpPlan P;
    if (s.rc || cnmp_stage(s, kf1, tri1, cos1, has_mp1, npairs, kf2, tri2, cos2, has_mp2, fv2, F12, match12, ok, x3d, &P))
        return s.rc;
    if (s.fail(cnmp_launch(s.m, P, f1))) return s.rc;
    return s.finish();
}

int orbmi_fuse_search(orbmi_matcher* h, const orbmi_frame_view* kf, const orbmi_mappoint* mps, const uint8_t* in_kf,
                      int n_mp, float th, int32_t* best_idx, int32_t* best_dist, int* ncandidates) {
    if (!h || !kf || n_mp < 0 || (n_mp > 0 && (!mps || !best_idx || !best_dist))) return ORBMI_E_ARG;
    Stage s(h);
    const DevFrame F = s.frame(kf, true);
    const orbmi_mappoint* d_mps = s.in(mps, (size_t)n_mp);
    const uint8_t* d_in = s.in(in_kf, (size_t)std::max(n_mp, 1));
    int* d_cnt = ncandidates ? s.scalars() : nullptr;  // the count only when asked for
    int* d_bi = s.out(best_idx, (size_t)n_mp);
    int* d_bd = s.out(best_dist, (size_t)n_mp);
    if (s.rc || s.fail(orbmi::launch_fuse(s.m, F, d_mps, d_in, n_mp, th, d_bi, d_bd, d_cnt))) return s.rc;
    return s.finish({{ncandidates, d_cnt}});
}

int orbmi_fuse_search_batch(orbmi_matcher* h, int nkf, const orbmi_frame_view* kfs, const orbmi_mappoint* mps,
                            const uint8_t* in_kf, int n_mp, float th, int32_t* best_idx, int32_t* best_dist,
                            int* ncandidates) {
    if (!h || nkf < 0 || n_mp < 0 || (nkf > 0 && !kfs) || (nkf > 0 && n_mp > 0 && (!mps || !best_idx || !best_dist)))
        return ORBMI_E_ARG;
    if (nkf == 0) return ORBMI_OK;
    Stage s(h);
    FusePlan P;
    if (fuse_batch_stage(s, nkf, kfs, nullptr, mps, in_kf, n_mp, best_idx, best_dist, &P)) return s.rc;
    if (s.fail(fuse_batch_launch(s.m, P, th))) return s.rc;
    return s.finish({{ncandidates, P.T.d_cnt, nkf}});
}

int orbmi_fuse_search_refresh(orbmi_matcher* h, const uint8_t* obs_desc, const int32_t* obs_off, int nd, int32_t* best,
                              uint8_t* desc_out, int nkf, const orbmi_frame_view* kfs, const orbmi_mappoint* mps,
                              const int32_t* desc_from, const uint8_t* in_kf, int n_mp, float th, int32_t* best_idx,
                              int32_t* best_dist) {
    if (!h || nd < 0 || nkf < 0 || n_mp < 0 || (nd > 0 && (!obs_off || !best || !desc_out)) ||
        (nkf > 0 && !kfs) || (nkf > 0 && n_mp > 0 && (!mps || !best_idx || !best_dist)))
        return ORBMI_E_ARG;
    Stage s(h);
    Matcher& m = s.m;
    // ComputeDistinctiveDescriptors of the nd due points
    Distinctive D;
    if (nd > 0) {
        if (stage_distinctive(s, obs_desc, obs_off, nd, on_device(obs_desc), best, desc_out, &D)) return s.rc;
        if (s.fail(orbmi::launch_distinctive(m, D.desc, D.off, nd, D.best, D.out))) return s.rc;
    }
    // the Fuse searches on records patched with the new descriptors
    if (nkf > 0 && n_mp > 0) {
        orbmi_mappoint* d_mps = s.scratch<orbmi_mappoint>((size_t)n_mp);
        if (s.rc) return s.rc;
        if (on_device(mps))
            ORBMI_HIP(hipMemcpyAsync(d_mps, mps, sizeof(orbmi_mappoint) * n_mp, hipMemcpyDeviceToDevice, m.ls()));
        else
            ORBMI_HIP(m.h2d(d_mps, mps, sizeof(orbmi_mappoint) * n_mp));
        if (desc_from && nd > 0) {
            const int* d_from = s.in(desc_from, (size_t)n_mp);
            if (s.rc || s.fail(orbmi::launch_patch_desc(m, d_mps, d_from, D.out, n_mp))) return s.rc;
        }
        const uint8_t* d_in = s.in(in_kf, (size_t)n_mp * nkf);
        FuseTable T;
        if (s.rc || orbmi::fuse_table(s, nkf, kfs, nullptr, true, d_in, n_mp, best_idx, best_dist, &T)) return s.rc;
        if (s.fail(orbmi::launch_fuse_multi(m, nkf, nullptr, T.d_k, d_mps, n_mp, th, T.d_bi, T.d_bd, T.d_cnt, T.ncap)))
            return s.rc;
    }
    return s.finish();
}

int orbmi_local_mapping_job(orbmi_matcher* h, orbmi_ba* ba, const orbmi_lm_job* J, orbmi_lm_job_result* R) {
    if (!h || !ba || !J || !R) return ORBMI_E_ARG;
    R->bow_words = R->fv_nodes = 0;
    R->failed_stage = -1;
    auto fail = [R](int stage, int rc) { R->failed_stage = stage; return rc; };
    const int np = J->n_points, nnb = J->nnb, n_kp = J->n_kf_points, n_tp = J->n_target_points;
    if (!J->kf || !J->problem || !J->result || !J->counts_host || !J->counts_event || !J->fv_node || !J->fv_off ||
        !J->fv_feat || np < 0 || nnb < 0 || n_kp < 0 || n_tp < 0 || (np > 0 && (!J->obs_off || !J->best || !J->desc_out)) ||
        (nnb > 0 && n_kp > 0 && (!J->kf_points || !J->best_idx || !J->best_dist)) ||
        (n_tp > 0 && (!J->target_points || !J->best_idx || !J->best_dist)))
        return ORBMI_E_ARG;
    if (J->voc && (J->bow_n < 0 || !J->bow_counts || !J->bow_word || !J->bow_value)) return fail(0, ORBMI_E_ARG);
    Stage s(h);  // the job's one arena generation
    if (s.rc) return s.rc;
    Matcher& m = s.m;
    auto mark = [&](int k) {  // a stage boundary for the caller's timeline (diagnostics)
        if (J->stage_events && J->stage_events[k]) (void)hipEventRecord((hipEvent_t)J->stage_events[k], m.ls());
    };
    int rc;
    // ---- ProcessNewKeyFrame: ComputeBoW (unless issued ahead) + ComputeDistinctiveDescriptors
    hipEvent_t counts_ev = (hipEvent_t)J->counts_event;
    if (J->voc) {
        if ((rc = orbmi_transform(J->voc, J->bow_desc, J->bow_n, nullptr, 4, J->bow_word, J->bow_value, J->fv_node,
                                  J->fv_off, J->fv_feat, J->bow_counts)))
            return fail(0, rc);
        void* vs = nullptr;
        if ((rc = orbmi_vocabulary_get_stream(J->voc, &vs))) return fail(0, rc);
        if ((hipStream_t)vs != m.stream && (rc = orbmi_vocabulary_synchronize(J->voc))) return fail(0, rc);
        if (hipMemcpyAsync(const_cast<int32_t*>(J->counts_host), J->bow_counts, 2 * sizeof(int), hipMemcpyDeviceToHost,
                           m.stream) != hipSuccess ||
            hipEventRecord(counts_ev, m.stream) != hipSuccess)
            return fail(0, ORBMI_E_HIP);
    }
    // enqueued first, so the stream is busy while the host builds the searches' tables
    Distinctive D;
    if (np > 0) {
        if (!on_device(J->obs_desc) && J->obs_desc) return fail(1, ORBMI_E_ARG);  // (its row count is not read back here)
        if (stage_distinctive(s, J->obs_desc, J->obs_off, np, true, J->best, J->desc_out, &D)) return fail(1, s.rc);
        if ((rc = orbmi::launch_distinctive(m, D.desc, D.off, np, D.best, D.out))) return fail(1, rc);
    }
    mark(0);
    // ---- every search's host tables: validated, built and staged now, one upload
    CnmpPlan cn;
    FusePlan fb;
    DevFrame KF;
    if (nnb > 0) {
        if (cnmp_stage(s, J->kf, J->tri, J->cos, J->has_mp, nnb, J->kf2, J->tri2, J->cos2, J->has_mp2, J->fv2, J->F12,
                       J->match12, J->ok, J->x3d, &cn))
            return fail(2, s.rc);
        if (fuse_batch_stage(s, nnb, J->kf2, cn.KF2.data(), J->kf_points, nullptr, n_kp, J->best_idx, J->best_dist, &fb))
            return fail(3, s.rc);
        KF = cn.K1;
    } else {
        KF = s.frame(J->kf, true);
    }
    const size_t o = (size_t)nnb * n_kp;  // Fuse(keyframe, targets' points) behind the targets' rows
    const orbmi_mappoint* d_tp = s.in(J->target_points, (size_t)n_tp);
    int* d_bi = s.out(J->best_idx ? J->best_idx + o : nullptr, (size_t)n_tp);
    int* d_bd = s.out(J->best_dist ? J->best_dist + o : nullptr, (size_t)n_tp);
    if (s.rc) return fail(3, s.rc);
    // ---- the FeatureVector's node count sizes SearchForTriangulation: the one host wait ahead of LocalBA
    if (hipEventSynchronize(counts_ev) != hipSuccess) return fail(0, ORBMI_E_HIP);
    const int nw = J->counts_host[0], nn = J->counts_host[1];
    if (nw < 0 || nn < 0) return fail(0, ORBMI_E_STATE);
    R->bow_words = nw;
    R->fv_nodes = nn;
    // ---- CreateNewMapPoints
    if (nnb > 0) {
        const DevFV f1{nn, nn ? J->fv_node : nullptr, nn ? J->fv_off : nullptr, nn ? J->fv_feat : nullptr};
        if ((rc = cnmp_launch(m, cn, f1))) return fail(2, rc);
    }
    mark(1);
    // ---- SearchInNeighbors: Fuse(target, keyframe's points) per target, Fuse(keyframe, targets' points)
    if (nnb > 0 && (rc = fuse_batch_launch(m, fb, J->fuse_th))) return fail(3, rc);
    if ((rc = orbmi::launch_fuse(m, KF, d_tp, nullptr, n_tp, J->fuse_th, d_bi, d_bd, nullptr))) return fail(3, rc);
    mark(2);
    // ---- ComputeDistinctiveDescriptors of the keyframe's points after fusion
    if (np > 0 && (rc = orbmi::launch_distinctive(m, D.desc, D.off, np, D.best, D.out))) return fail(4, rc);
    mark(3);
    if ((rc = s.finish())) return fail(4, rc);
    // ---- LocalBundleAdjustment (in stream order behind the searches when ba runs on this stream)
    if ((rc = orbmi_local_bundle_adjustment(ba, J->problem, J->result, J->stop))) return fail(5, rc);
    return ORBMI_OK;
}

}  // extern "C"
