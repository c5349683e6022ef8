// C ABI of the matchers (include/orbmi.h, "ORBmatcher" section): the handle, its streams and
// grids, and the tracking searches.  LocalMapping's entries are in capi_mapping.cpp, loop
// closing's in capi_loop.cpp; all stage their host arrays through capi_stage.h's call scope.
#include <new>

#include "capi_stage.h"

using orbmi::DevFrame;
using orbmi::DevFV;
using orbmi::Matcher;
using orbmi::on_device;
using orbmi::Stage;

hipStream_t orbmi_extractor_stream_(orbmi_extractor* ex);  // capi_extract.cpp

extern "C" {

int orbmi_matcher_create(int device, orbmi_matcher** out) {
    if (!out) return ORBMI_E_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return ORBMI_E_HIP;
    orbmi_matcher* h = new (std::nothrow) orbmi_matcher();
    if (!h) return ORBMI_E_ARG;
    h->m.device = device;
    if (hipSetDevice(device) != hipSuccess || orbmi::stream_create(&h->m.stream, "MATCHER") != hipSuccess) {
        delete h;
        return ORBMI_E_HIP;
    }
    *out = h;
    return ORBMI_OK;
}

int orbmi_matcher_share_stream(orbmi_matcher* h, orbmi_extractor* ex) {
    if (!h || !ex) return ORBMI_E_ARG;
    Matcher& m = h->m;
    hipStream_t s = orbmi_extractor_stream_(ex);
    if (!s) return ORBMI_E_STATE;
    ORBMI_HIP(hipSetDevice(m.device));
    ORBMI_HIP(hipStreamSynchronize(m.stream));
    if (m.own_stream) ORBMI_HIP(hipStreamDestroy(m.stream));
    m.stream = s;
    m.own_stream = false;
    return ORBMI_OK;
}

int orbmi_matcher_reserve_cus(orbmi_matcher* h, int n) {
    if (!h || n < 0) return ORBMI_E_ARG;
    Matcher& m = h->m;
    if (!m.own_stream) return ORBMI_E_STATE;
    ORBMI_HIP(hipSetDevice(m.device));
    int ncu = 0;
    ORBMI_HIP(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, m.device));
    if (n >= ncu) return ORBMI_E_ARG;
    hipStream_t s = nullptr;
    if (n == 0) {
        ORBMI_HIP(orbmi::stream_create(&s, "MATCHER"));
    } else {
        std::vector<uint32_t> mask((size_t)(ncu + 31) / 32, 0u);
        for (int c = 0; c < ncu - n; c++) mask[c >> 5] |= 1u << (c & 31);
        ORBMI_HIP(hipExtStreamCreateWithCUMask(&s, (uint32_t)mask.size(), mask.data()));
    }
    (void)hipStreamSynchronize(m.stream);
    (void)hipStreamDestroy(m.stream);
    m.stream = s;
    return ORBMI_OK;
}

int orbmi_matcher_assign_features_to_grid(orbmi_matcher* h, const orbmi_frame_view* v) {
    if (!h || !v || (v->n > 0 && !on_device(v->keys_un))) return ORBMI_E_ARG;
    Stage s(h);
    const DevFrame F = s.frame(v, false);
    if (s.rc || s.fail(orbmi::pin_grid(s.m, F))) return s.rc;
    ORBMI_HIP(hipGetLastError());
    return s.finish();
}

int orbmi_matcher_build_grid_slot(orbmi_matcher* h, const orbmi_frame_view* v, int slot, void* stream) {
    if (!h || !v || slot < 0 || slot >= orbmi::Matcher::kGridSlots || (v->n > 0 && !on_device(v->keys_un)) ||
        (v->n > 0 && !on_device(v->desc)) || (v->u_right && !on_device(v->u_right)))
        return ORBMI_E_ARG;
    Stage s(h, false);  // device arrays: nothing staged
    const DevFrame F = s.frame(v, false);
    hipStream_t st = stream ? (hipStream_t)stream : s.m.ls();
    if (s.rc || s.fail(orbmi::build_grid_slot(s.m, F, slot, st))) return s.rc;
    ORBMI_HIP(hipGetLastError());
    return ORBMI_OK;
}

int orbmi_matcher_pin_grid_slot(orbmi_matcher* h, const orbmi_frame_view* v, int slot) {
    if (!h || !v || slot < 0 || slot >= orbmi::Matcher::kGridSlots || (v->n > 0 && !on_device(v->keys_un)))
        return ORBMI_E_ARG;
    Stage s(h, false);
    const DevFrame F = s.frame(v, false);
    if (s.rc) return s.rc;
    return orbmi::pin_grid_slot(s.m, F, slot);
}

int orbmi_matcher_release_grid(orbmi_matcher* h) {
    if (!h) return ORBMI_E_ARG;
    h->m.grid_pinned = false;
    return ORBMI_OK;
}

int orbmi_matcher_get_stream(orbmi_matcher* h, void** stream) {
    if (!h || !stream) return ORBMI_E_ARG;
    *stream = (void*)h->m.stream;
    return ORBMI_OK;
}

void orbmi_matcher_destroy(orbmi_matcher* h) {
    if (!h) return;
    h->m.release();
    delete h;
}

int orbmi_is_in_frustum(orbmi_matcher* h, const orbmi_frame_view* v, const orbmi_mappoint* mps, int n_mp,
                        float viewing_cos_limit, orbmi_mappoint_track* track) {
    if (!h || n_mp < 0 || (n_mp > 0 && (!mps || !track))) return ORBMI_E_ARG;
    Stage s(h);
    const DevFrame F = s.frame(v, true);
    const orbmi_mappoint* d_mps = s.in(mps, (size_t)n_mp);
    orbmi_mappoint_track* d_tr = s.out(track, (size_t)n_mp);
    if (s.rc || s.fail(orbmi::launch_frustum(s.m, F, d_mps, n_mp, viewing_cos_limit, d_tr, nullptr))) return s.rc;
    ORBMI_HIP(hipGetLastError());
    return s.finish();
}

int orbmi_search_by_projection_local(orbmi_matcher* h, const orbmi_frame_view* v, const uint8_t* occupied,
                                     const orbmi_mappoint* mps, const orbmi_mappoint_track* track, int n_mp,
                                     float th, float nnratio, int32_t* match_mp, int* nmatches) {
    if (!h || !occupied || !match_mp || n_mp < 0 || (n_mp > 0 && (!mps || !track))) return ORBMI_E_ARG;
    Stage s(h);
    const DevFrame F = s.frame(v, false);
    const uint8_t* d_occ = s.in(occupied, (size_t)std::max(F.n, 1));
    const orbmi_mappoint* d_mps = s.in(mps, (size_t)n_mp);
    const orbmi_mappoint_track* d_tr = s.in(track, (size_t)n_mp);
    int* d_n = s.scalars();
    int* d_out = s.out(match_mp, (size_t)F.n);
    if (s.rc || s.fail(orbmi::launch_local_search(s.m, F, d_occ, d_mps, d_tr, n_mp, th, nnratio, d_out, d_n))) return s.rc;
    ORBMI_HIP(hipGetLastError());
    return s.finish({{nmatches, d_n}});
}

int orbmi_search_local_points(orbmi_matcher* h, const orbmi_frame_view* v, const uint8_t* occupied,
                              const orbmi_mappoint* mps, int n_mp, float th, int32_t* match_mp, int* nmatches,
                              int* n_to_match) {
    return orbmi_search_local_points_track(h, v, occupied, mps, n_mp, th, match_mp, nmatches, n_to_match, nullptr);
}

int orbmi_search_local_points_track(orbmi_matcher* h, const orbmi_frame_view* v, const uint8_t* occupied,
                                    const orbmi_mappoint* mps, int n_mp, float th, int32_t* match_mp, int* nmatches,
                                    int* n_to_match, orbmi_mappoint_track* track_out) {
    if (!h || !occupied || !match_mp || n_mp < 0 || (n_mp > 0 && !mps)) return ORBMI_E_ARG;
    Stage s(h);
    Matcher& m = s.m;
    const DevFrame F = s.frame(v, true);
    const uint8_t* d_occ = s.in(occupied, (size_t)std::max(F.n, 1));
    const orbmi_mappoint* d_mps = s.in(mps, (size_t)n_mp);
    if (s.rc) return s.rc;
    // k_greedy stores the match count (slot 0) unconditionally; only the nToMatch counter (slot 1,
    // atomics in k_frustum) needs zeroing, and only when the caller asks for it
    if (n_to_match) s.scalars();
    else s.fail(orbmi::ensure_buf(&m.d_scalars, &m.cap_scalars, 4));
    // the isInFrustum outputs go to the caller (host: copied back with the matches), or nowhere
    orbmi_mappoint_track* d_tr = nullptr;
    if (track_out) d_tr = s.out(track_out, (size_t)std::max(n_mp, 1));
    else if (!s.rc && !s.fail(orbmi::ensure_buf(&m.d_track, &m.cap_track, (size_t)std::max(n_mp, 1)))) d_tr = m.d_track;
    int* d_out = s.out(match_mp, (size_t)F.n);
    // Tracking::SearchLocalPoints: isInFrustum(pMP, 0.5); ORBmatcher matcher(0.8).  isInFrustum
    // runs inside the search's candidate kernel, which writes d_tr.
    if (s.rc || s.fail(orbmi::launch_local_search(m, F, d_occ, d_mps, d_tr, n_mp, th, 0.8f, d_out, m.d_scalars, d_tr, 0.5f,
                                                  n_to_match ? m.d_scalars + 1 : nullptr)))
        return s.rc;
    ORBMI_HIP(hipGetLastError());
    // nToMatch is read back (and waited for) only when the caller asks for it
    return s.finish({{nmatches, m.d_scalars}, {n_to_match, m.d_scalars + 1}});
}

namespace {

// Both SearchByProjection(CurrentFrame, LastFrame) entries: the count goes to the host (nmatches),
// or stays on the device (gate) where it also gates the search at gate_min matches
int lastframe_search(orbmi_matcher* h, const orbmi_frame_view* cf, const uint8_t* occupied, const orbmi_frame_view* lf,
                     const orbmi_lastframe_point* lf_points, float th, int mono, int check_ori, int32_t* match_lf,
                     int* nmatches, int* gate, int gate_min) {
    Stage s(h);
    const DevFrame CF = s.frame(cf, true);
    const DevFrame LF = s.frame(lf, true);
    const uint8_t* d_occ = s.in(occupied, (size_t)std::max(CF.n, 1));
    const orbmi_lastframe_point* d_lfp = s.in(lf_points, (size_t)LF.n);
    int* d_n = gate ? gate : s.scalars();
    int* d_out = s.out(match_lf, (size_t)CF.n);
    if (s.rc || s.fail(orbmi::launch_lastframe_search(s.m, CF, d_occ, LF, d_lfp, th, mono, check_ori, d_out, d_n, gate,
                                                      gate_min)))
        return s.rc;
    ORBMI_HIP(hipGetLastError());
    return s.finish({{gate ? nullptr : nmatches, d_n}});
}

}  // namespace

int orbmi_search_by_projection_last_frame(orbmi_matcher* h, const orbmi_frame_view* cf, const uint8_t* occupied,
                                          const orbmi_frame_view* lf, const orbmi_lastframe_point* lf_points,
                                          float th, int mono, int check_ori, int32_t* match_lf, int* nmatches) {
    if (!h || !occupied || !match_lf || !lf || (lf->n > 0 && !lf_points)) return ORBMI_E_ARG;
    return lastframe_search(h, cf, occupied, lf, lf_points, th, mono, check_ori, match_lf, nmatches, nullptr, 0);
}

int orbmi_search_by_projection_last_frame_if(orbmi_matcher* h, const orbmi_frame_view* cf, const uint8_t* occupied,
                                             const orbmi_frame_view* lf, const orbmi_lastframe_point* lf_points,
                                             float th, int mono, int check_ori, int32_t* match_lf, int* nmatches_dev,
                                             int min_matches) {
    if (!h || !occupied || !match_lf || !lf || (lf->n > 0 && !lf_points) || !on_device(nmatches_dev)) return ORBMI_E_ARG;
    return lastframe_search(h, cf, occupied, lf, lf_points, th, mono, check_ori, match_lf, nullptr, nmatches_dev,
                            min_matches);
}

int orbmi_track_update_matches(orbmi_matcher* h, const orbmi_frame_view* f, int stage, const uint8_t* outlier,
                               const orbmi_frame_mappoints* mp, uint8_t* occupied_out, int* counts) {
    if (!h || !f || !outlier || !mp || !counts || (stage != 0 && stage != 1)) return ORBMI_E_ARG;
    if ((mp->match_lf && (!mp->lf_points || mp->n_lf_points < 0)) || (mp->match_mp && (!mp->mps || mp->n_mps < 0)))
        return ORBMI_E_ARG;
    Stage s(h);
    const DevFrame F = s.frame(f, false);
    const size_t n = (size_t)std::max(F.n, 1);
    // the match arrays are updated in place: host arrays go through the arena and back
    int* d_lf = mp->match_lf ? s.inout(mp->match_lf, n) : nullptr;
    int* d_mp = mp->match_mp ? s.inout(mp->match_mp, n) : nullptr;
    const uint8_t* d_outl = s.in(outlier, n);
    const orbmi_lastframe_point* d_lfp = mp->match_lf ? s.in(mp->lf_points, (size_t)mp->n_lf_points) : nullptr;
    const orbmi_mappoint* d_mps = mp->match_mp ? s.in(mp->mps, (size_t)mp->n_mps) : nullptr;
    uint8_t* d_occ = occupied_out ? s.out(occupied_out, n) : nullptr;
    int* d_cnt = s.out(counts, 2);
    if (s.rc || s.fail(orbmi::launch_track_update(s.m, F, stage, d_outl, d_lf, d_lfp, mp->n_lf_points, d_mp, d_mps,
                                                  mp->n_mps, d_occ, d_cnt)))
        return s.rc;
    ORBMI_HIP(hipGetLastError());
    return s.finish();
}

int orbmi_search_by_bow(orbmi_matcher* h, const orbmi_frame_view* kf, const uint8_t* kf_mp_ok,
                        const orbmi_feature_vector* kf_fv, const orbmi_frame_view* f,
                        const orbmi_feature_vector* f_fv, float nnratio, int check_ori, int32_t* match_kf,
                        int* nmatches) {
    if (!h || !kf_mp_ok || !match_kf) return ORBMI_E_ARG;
    Stage s(h);
    const DevFrame KF = s.frame(kf, false);
    const DevFrame F = s.frame(f, false);
    const DevFV kfv = s.fv(kf_fv);
    const DevFV fv = s.fv(f_fv);
    const uint8_t* d_ok = s.in(kf_mp_ok, (size_t)std::max(KF.n, 1));
    int* d_n = s.scalars();
    int* d_out = s.out(match_kf, (size_t)F.n);
    if (s.rc || s.fail(orbmi::launch_bow(s.m, KF, d_ok, kfv, F, fv, nnratio, check_ori, d_out, d_n))) return s.rc;
    ORBMI_HIP(hipGetLastError());
    return s.finish({{nmatches, d_n}});
}

int orbmi_match_descriptors_segments(orbmi_matcher* h, const uint8_t* q_desc, int nq, const int* nq_device,
                                     const uint8_t* train_desc, int nseg, int seg_capacity, const int* seg_counts,
                                     int skip_seg, int th, float ratio, int32_t* match, int* nmatches) {
    if (!h || nq < 0 || nseg < 0 || seg_capacity < 0 || (nq > 0 && (!q_desc || !match))) return ORBMI_E_ARG;
    if ((long long)nseg * seg_capacity > 0xFFFFFFFLL) return ORBMI_E_UNSUPPORTED;
    if (nseg * seg_capacity > 0 && (!train_desc || !seg_counts)) return ORBMI_E_ARG;
    if (nq_device && !on_device(nq_device)) return ORBMI_E_ARG;
    Stage s(h);
    const uint8_t* d_q = s.in(q_desc, (size_t)nq * 32);
    const uint8_t* d_t = s.in(train_desc, (size_t)nseg * seg_capacity * 32);
    const int* d_cnt = s.in(seg_counts, (size_t)nseg);
    int* d_n = s.scalars();
    int* d_out = s.out(match, (size_t)nq);
    if (s.rc) return s.rc;
    if (nseg * seg_capacity == 0 && nq > 0) ORBMI_HIP(hipMemsetAsync(d_out, 0xFF, (size_t)nq * sizeof(int), s.m.ls()));
    else if (s.fail(orbmi::launch_xmatch(s.m, d_q, nq, nq_device, d_t, nseg, seg_capacity, d_cnt, skip_seg, th, ratio, d_out,
                                         d_n)))
        return s.rc;
    ORBMI_HIP(hipGetLastError());
    return s.finish({{nmatches, d_n}});
}

int orbmi_debug_greedy_stats(unsigned long long* out, int reset) {
    if (!out) return ORBMI_E_ARG;
    return orbmi::greedy_stats(out, reset);
}

int orbmi_debug_greedy_cycles(unsigned long long* out, int reset) {
    if (!out) return ORBMI_E_ARG;
    return orbmi::greedy_cycles(out, reset);
}

}  // extern "C"
