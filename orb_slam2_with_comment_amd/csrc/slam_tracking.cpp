// Tracking of the native SLAM loop (slam.h): the tracking arena, PoseOptimization, stereo
// initialisation, the keyframe decision, the three tracking stages and Tracking::Track.
#include "slam.h"

int orbmi_slam::track_buffers(size_t nkp, size_t nlf, size_t nrec) {
    nkp = std::max<size_t>(nkp, 1);
    nlf = std::max<size_t>(nlf, 1);
    nrec = std::max<size_t>(nrec, 1);
    TrackBuf& t = tb;
    if (nkp <= t.cap_kp && nlf <= t.cap_lf && nrec <= t.cap_rec && t.d_arena) return ORBMI_OK;
    if (nkp > t.cap_kp) t.cap_kp = nkp + nkp / 4;
    if (nlf > t.cap_lf) t.cap_lf = nlf + nlf / 4;
    if (nrec > t.cap_rec) t.cap_rec = nrec + nrec / 4;
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += al(bytes); return o; };
    const size_t o_rec = take(t.cap_rec * sizeof(orbmi_mappoint)), o_mlf = take(t.cap_kp * 4), o_occ = take(t.cap_kp);
    const size_t o_lfp = off;  // (no padding between lfp and n: TWMM's upload ends right after n)
    off += t.cap_lf * sizeof(orbmi_lastframe_point);
    off = (off + 15) & ~(size_t)15;
    const size_t o_n = take(2 * sizeof(int)), o_pose = take(sizeof(orbmi_pose_frame)), o_out = take(t.cap_kp),
                 o_m = take(t.cap_kp * 4), o_tr = take(t.cap_rec * sizeof(orbmi_mappoint_track));
    if (off > t.arena_bytes) {
        if (t.d_arena) (void)hipFree(t.d_arena);
        if (t.h_arena) (void)hipHostFree(t.h_arena);
        t.d_arena = t.h_arena = nullptr;
        t.arena_bytes = 0;
        if (hipMalloc((void**)&t.d_arena, off) != hipSuccess) return ORBMI_E_HIP;
        if (hipHostMalloc((void**)&t.h_arena, off, hipHostMallocDefault) != hipSuccess) return ORBMI_E_HIP;
        t.arena_bytes = off;
    }
    auto at = [&](uint8_t* base, size_t o) { return (void*)(base + o); };
    for (int side = 0; side < 2; side++) {
        uint8_t* B = side ? t.h_arena : t.d_arena;
        auto& rec = side ? t.h_rec : t.d_rec;
        auto& mlf = side ? t.h_mlf : t.d_mlf;
        auto& occ = side ? t.h_occ : t.d_occ;
        auto& lfp = side ? t.h_lfp : t.d_lfp;
        auto& n = side ? t.h_n : t.d_n;
        auto& pose = side ? t.h_pose : t.d_pose;
        auto& out = side ? t.h_out : t.d_out;
        auto& m = side ? t.h_m : t.d_m;
        auto& tr = side ? t.h_tr : t.d_tr;
        rec = (orbmi_mappoint*)at(B, o_rec);
        mlf = (int32_t*)at(B, o_mlf);
        occ = (uint8_t*)at(B, o_occ);
        lfp = (orbmi_lastframe_point*)at(B, o_lfp);
        n = (int*)at(B, o_n);
        pose = (orbmi_pose_frame*)at(B, o_pose);
        out = (uint8_t*)at(B, o_out);
        m = (int32_t*)at(B, o_m);
        tr = (orbmi_mappoint_track*)at(B, o_tr);
    }
    return ORBMI_OK;
}

void orbmi_slam::free_track_buffers() {
    TrackBuf& t = tb;
    if (t.d_arena) (void)hipFree(t.d_arena);
    if (t.h_arena) (void)hipHostFree(t.h_arena);
    tb = TrackBuf{};
}

// one contiguous copy of the arena's host bytes [from, to) up, or device bytes down
int orbmi_slam::up_range(const void* from, const void* to) {
    const size_t o = (const uint8_t*)from - tb.h_arena, n = (const uint8_t*)to - (const uint8_t*)from;
    return hipMemcpyAsync(tb.d_arena + o, from, n, hipMemcpyHostToDevice, tstream) == hipSuccess ? ORBMI_OK : ORBMI_E_HIP;
}

int orbmi_slam::down_range(void* from, const void* to) {
    const size_t o = (uint8_t*)from - tb.h_arena, n = (const uint8_t*)to - (uint8_t*)from;
    return hipMemcpyAsync(from, tb.d_arena + o, n, hipMemcpyDeviceToHost, tstream) == hipSuccess ? ORBMI_OK : ORBMI_E_HIP;
}

// Optimizer::PoseOptimization over keypoint i -> lfp[match[i]] (match[i] >= 0)
int orbmi_slam::pose_optimization(const TrackedFrame& cf, const std::vector<int32_t>& match,
                      const std::vector<orbmi_lastframe_point>& lfp, M4& tcw_out, std::vector<uint8_t>& out) {
    orbmi_frame_view v = view(cf, cf.tcw.data());
    orbmi_frame_mappoints fm{};
    fm.match_lf = const_cast<int32_t*>(match.data());
    fm.lf_points = lfp.data();
    fm.n_lf_points = (int)lfp.size();
    orbmi_pose_frame rec{};
    out.assign(std::max(cf.n(), 1), 0);
    SLAM_CHECK(unlocked(ORBMI_SCHED_T_POSE, cf.id, [&] {
        return orbmi_pose_optimization_frame(pose, &v, inv_level_sigma2.data(), &fm, &rec, out.data());
    }));
    std::memcpy(tcw_out.data(), rec.tcw, sizeof(rec.tcw));
    out.resize(cf.n());
    return ORBMI_OK;
}

// Frame::UnprojectStereo (src/Frame.cc:701-715) + new MapPoint + AddObservation + AddMapPoint
// + UpdateNormalAndDepth (src/Tracking.cc:602-616, :1308-1320)
void orbmi_slam::create_points(int k, TrackedFrame& cf, const std::vector<int>& idx) {
    if (idx.empty()) return;
    const float invfx = 1.f / s.fx, invfy = 1.f / s.fy;
    const M4 twc = pose_inverse(cf.tcw);
    std::vector<int> made;
    for (int i : idx) {
        const float z = cf.depth[i];
        const float x = (cf.keys[i].x - s.cx) * z * invfx;
        const float y = (cf.keys[i].y - s.cy) * z * invfy;
        MapPoint mp;
        mp.id = (int)mps.size();
        for (int r = 0; r < 3; r++) {
            const double a = (double)twc[4 * r] * (double)x + (double)twc[4 * r + 1] * (double)y +
                             (double)twc[4 * r + 2] * (double)z;
            mp.pos[r] = (float)(a + (double)twc[4 * r + 3]);  // one gemm(Rwc, x3Dc, 1, Ow, 1)
        }
        mp.ref_kf = k;
        mp.first_kf_id = k;
        std::memcpy(mp.desc, &cf.desc[32 * i], 32);  // ComputeDistinctiveDescriptors of one observation
        mps.push_back(mp);
        add_observation(mp.id, k, i);
        kfs[k].mps[i] = mp.id;
        cf.mps[i] = mp.id;
        made.push_back(mp.id);
    }
    for (int m : made) update_normal_and_depth(m);
}

int orbmi_slam::stereo_initialization(TrackedFrame& cf) {  // src/Tracking.cc:584-636
    if (cf.n() <= 500) return ORBMI_OK;
    cf.tcw = eye4();
    cf.has_tcw = true;
    const int k = new_keyframe(cf);
    std::vector<int> idx;
    for (int i = 0; i < cf.n(); i++)
        if (cf.depth[i] > 0) idx.push_back(i);
    create_points(k, cf, idx);
    SLAM_CHECK(insert_keyframe(k));
    last_kf_frame_id = cf.id;
    local_kfs = {k};
    local_mps.clear();
    for (auto& m : mps)
        if (!m.bad) local_mps.push_back(m.id);
    ref_kf = k;
    cf.ref_kf = k;
    state = OK;
    return ORBMI_OK;
}

bool orbmi_slam::need_new_keyframe(const TrackedFrame& cf, orbmi_slam_frame_stats& st) {  // src/Tracking.cc:1140-1249
    const int nkfs = keyframes_in_map();
    if (cf.id < last_reloc_frame_id + s.max_frames && nkfs > s.max_frames) return false;
    const int min_obs = nkfs <= 2 ? 2 : 3;
    const int n_ref = tracked_map_points(kfs[ref_kf], min_obs);
    int n_tracked_close = 0, n_non_tracked_close = 0;
    for (int i = 0; i < cf.n(); i++) {
        if (!(cf.depth[i] > 0 && cf.depth[i] < s.th_depth)) continue;
        if (cf.mps[i] >= 0 && !cf.outlier[i]) n_tracked_close++;
        else n_non_tracked_close++;
    }
    const bool need_close = n_tracked_close < 100 && n_non_tracked_close > 70;
    const float th_ref = nkfs < 2 ? 0.4f : 0.75f;
    bool idle = true;  // LocalMapping::AcceptKeyFrames (always, when it runs synchronously)
    size_t queued = 0;
    if (async_lm()) {
        std::lock_guard<std::mutex> g(q_mtx);
        idle = !lm_busy;
        queued = lm_queue.size();
    }
    const bool c1a = cf.id >= last_kf_frame_id + s.max_frames;
    const bool c1b = cf.id >= last_kf_frame_id + s.min_frames && idle;
    const bool c1c = matches_inliers < n_ref * 0.25 || need_close;
    const bool c2 = ((float)matches_inliers < (float)n_ref * th_ref || need_close) && matches_inliers > 15;
    st.need_kf = (c1a || c1b || c1c) && c2;
    if (!st.need_kf) return false;
    if (idle) return true;
    set_abort_ba(1);    // mpLocalMapper->InterruptBA()
    return queued < 3;  // stereo: KeyframesInQueue() < 3
}

int orbmi_slam::create_new_keyframe(TrackedFrame& cf) {  // src/Tracking.cc:1251-1330
    const int k = new_keyframe(cf);
    ref_kf = k;
    cf.ref_kf = k;
    std::vector<std::pair<float, int>> order;
    for (int i = 0; i < cf.n(); i++)
        if (cf.depth[i] > 0) order.push_back({cf.depth[i], i});
    std::sort(order.begin(), order.end());
    std::vector<int> fresh;
    int npts = 0;
    for (auto& zi : order) {
        const int i = zi.second;
        const int m = cf.mps[i];
        const bool create = m < 0 || mps[m].nobs < 1;
        if (create && m >= 0) {
            cf.mps[i] = -1;
            kfs[k].mps[i] = -1;
        }
        if (create) fresh.push_back(i);
        npts++;
        if (zi.first > s.th_depth && npts > 100) break;
    }
    create_points(k, cf, fresh);
    SLAM_CHECK(insert_keyframe(k));
    last_kf_frame_id = cf.id;
    return ORBMI_OK;
}

// ---- tracking stages ----------------------------------------------------------------------

void orbmi_slam::mp_records_into(const std::vector<int>& pts, orbmi_mappoint* rec) const {
    for (size_t j = 0; j < pts.size(); j++) {
        const MapPoint& mp = mps[pts[j]];
        orbmi_mappoint& r = rec[j];
        std::memcpy(r.pos, mp.pos, sizeof(r.pos));
        std::memcpy(r.normal, mp.normal, sizeof(r.normal));
        r.max_distance = mp.max_distance;
        r.min_distance = mp.min_distance;
        r.flags = (mp.bad ? ORBMI_MP_BAD : 0u) | (seen.count(mp.id) ? ORBMI_MP_SEEN : 0u) |
                  (mp.nobs > 0 ? ORBMI_MP_HAS_OBS : 0u);
        std::memcpy(r.desc, mp.desc, 32);
    }
}

std::vector<orbmi_lastframe_point> orbmi_slam::lf_records(const std::vector<int>& lf_mps, const std::vector<uint8_t>* outlier) const {
    std::vector<orbmi_lastframe_point> rec(std::max<size_t>(lf_mps.size(), 1));
    lf_records_into(lf_mps, outlier, rec.data());
    rec.resize(lf_mps.size());
    return rec;
}

void orbmi_slam::lf_records_into(const std::vector<int>& lf_mps, const std::vector<uint8_t>* outlier,
                     orbmi_lastframe_point* rec) const {
    std::memset(rec, 0, std::max<size_t>(lf_mps.size(), 1) * sizeof(orbmi_lastframe_point));
    for (size_t i = 0; i < lf_mps.size(); i++) {
        const int m = lf_mps[i];
        if (m < 0) continue;
        std::memcpy(rec[i].pos, mps[m].pos, sizeof(rec[i].pos));
        std::memcpy(rec[i].desc, mps[m].desc, 32);
        rec[i].flags = ORBMI_LF_HAS_MP | (mps[m].nobs > 0 ? ORBMI_MP_HAS_OBS : 0u) |
                       (outlier && (*outlier)[i] ? ORBMI_LF_OUTLIER : 0u);
    }
}

int orbmi_slam::discard_outliers(TrackedFrame& cf, const std::vector<uint8_t>& outlier) {  // -> nmatchesMap
    int nmap = 0;
    for (int i = 0; i < cf.n(); i++) {
        const int m = cf.mps[i];
        if (m < 0) continue;
        if (outlier[i]) {
            cf.mps[i] = -1;
            cf.outlier[i] = 0;
            seen.insert(m);  // pMP->mnLastFrameSeen = mCurrentFrame.mnId
        } else if (mps[m].nobs > 0) {
            nmap++;
        }
    }
    return nmap;
}

int orbmi_slam::track_reference_kf(TrackedFrame& cf, orbmi_slam_frame_stats& st, bool& ok) {  // src/Tracking.cc:871-917
    ok = false;
    SLAM_CHECK(compute_bow(cf.desc, cf.fv));
    KeyFrame& kf = kfs[ref_kf];
    if (!kf.fv.valid) SLAM_CHECK(compute_bow(kf.desc, kf.fv));
    std::vector<uint8_t> ok_mp(std::max<size_t>(kf.mps.size(), 1), 0);
    for (size_t j = 0; j < kf.mps.size(); j++) ok_mp[j] = kf.mps[j] >= 0 && !mps[kf.mps[j]].bad;
    const M4 kf_tcw = kf.tcw;
    const orbmi_frame_view vk = kf_view(kf, kf_tcw.data());
    const M4 I = eye4();
    const orbmi_frame_view vf = view(cf, I.data());
    const orbmi_feature_vector fk = kf.fv.view(), ff = cf.fv.view();
    const std::vector<int> kf_mps = kf.mps;  // the keyframe's matches when the search ran
    std::vector<int32_t> m(std::max(cf.n(), 1));
    int n = 0;
    SLAM_CHECK(unlocked(ORBMI_SCHED_T_BOW, cf.id, [&] {
        return orbmi_search_by_bow(matcher, &vk, ok_mp.data(), &fk, &vf, &ff, 0.7f, 1, m.data(), &n);
    }));
    st.bow_matches = n;
    st.track = 2;
    if (n < 15) return ORBMI_OK;
    for (int i = 0; i < cf.n(); i++) cf.mps[i] = m[i] >= 0 ? kf_mps[m[i]] : -1;
    cf.tcw = last_frame.tcw;
    cf.has_tcw = true;
    const std::vector<orbmi_lastframe_point> lfp = lf_records(kf_mps, nullptr);
    m.resize(cf.n());
    M4 tcw;
    std::vector<uint8_t> out;
    SLAM_CHECK(pose_optimization(cf, m, lfp, tcw, out));
    cf.tcw = tcw;
    cf.outlier = out;
    seen.clear();
    const int nmap = discard_outliers(cf, out);
    st.nmatches_map = nmap;
    ok = nmap >= 10;
    return ORBMI_OK;
}

// TrackWithMotionModel's result (src/Tracking.cc:1021-1062), given the search's count and, when
// it reached 20, the matches (to last-frame keypoints) and PoseOptimization's pose and outliers
void orbmi_slam::motion_model_result(TrackedFrame& cf, int n, const int32_t* m, const float* tcw, const uint8_t* out,
                                     orbmi_slam_frame_stats& st, bool& ok) {
    st.track = 1;
    st.lf_matches = n;
    if (n < 20) return;
    const int nc = cf.n();
    for (int i = 0; i < nc; i++) cf.mps[i] = m[i] >= 0 ? last_frame.mps[m[i]] : -1;
    std::memcpy(cf.tcw.data(), tcw, 16 * sizeof(float));
    cf.outlier.assign(out, out + nc);
    seen.clear();
    const int nmap = discard_outliers(cf, cf.outlier);
    st.nmatches_map = nmap;
    ok = nmap >= 10;
}

// the per-call form: each operator stages its host inputs and synchronises
int orbmi_slam::track_motion_model_staged(TrackedFrame& cf, orbmi_slam_frame_stats& st, bool& ok) {
    TrackedFrame& lf = last_frame;
    const std::vector<orbmi_lastframe_point> lfp = lf_records(lf.mps, &lf.outlier);
    std::vector<uint8_t> occ(std::max(cf.n(), 1), 0);
    const orbmi_frame_view vc = view(cf, cf.tcw.data()), vl = view(lf, lf.tcw.data());
    std::vector<int32_t> m(std::max(cf.n(), 1));
    int n = 0;
    const float th = 7.f;  // stereo (src/Tracking.cc:1011-1014)
    {
        PhaseTimer pt(&phase_ms[PH_LF_SEARCH]);
        SLAM_CHECK(unlocked(ORBMI_SCHED_T_LF, cf.id, [&] {
            int rc = orbmi_search_by_projection_last_frame(matcher, &vc, occ.data(), &vl, lfp.data(), th, 0, 1,
                                                           m.data(), &n);
            if (!rc && n < 20)
                rc = orbmi_search_by_projection_last_frame(matcher, &vc, occ.data(), &vl, lfp.data(), 2 * th, 0, 1,
                                                           m.data(), &n);
            return rc;
        }));
    }
    M4 tcw;
    std::vector<uint8_t> out;
    if (n >= 20) {
        m.resize(cf.n());
        PhaseTimer pt(&phase_ms[PH_LF_POSE]);
        SLAM_CHECK(pose_optimization(cf, m, lfp, tcw, out));
    }
    motion_model_result(cf, n, m.data(), tcw.data(), out.data(), st, ok);
    return ORBMI_OK;
}

void orbmi_slam::update_local_keyframes(TrackedFrame& cf) {  // src/Tracking.cc:1452-1580
    // keyframe counter in keyframe-id order (the std::map<KeyFrame*, int> of the reference,
    // id-ordered here): counts per id, touched ids sorted
    if (kf_counter.size() < kfs.size()) kf_counter.resize(kfs.size(), 0);
    std::vector<int> touched;
    for (int i = 0; i < cf.n(); i++) {
        const int m = cf.mps[i];
        if (m < 0) continue;
        if (mps[m].bad) { cf.mps[i] = -1; continue; }
        for (auto& o : mps[m].obs)
            if (kf_counter[o.first]++ == 0) touched.push_back(o.first);
    }
    if (touched.empty()) return;
    std::sort(touched.begin(), touched.end());
    int best = 0, kfmax = -1;
    std::vector<int> local;
    local_kf_mark.clear();  // mnTrackReferenceForFrame of the keyframes (generation stamps)
    SeenSet& mark = local_kf_mark;
    for (int id : touched) {
        const int cnt = kf_counter[id];
        kf_counter[id] = 0;
        if (kfs[id].bad) continue;
        if (cnt > best) { best = cnt; kfmax = id; }
        local.push_back(id);
        mark.insert(id);
    }
    size_t i = 0;
    std::vector<int> ch;
    while (i < local.size()) {
        if (local.size() > 80) break;
        const int k = local[i++];
        const std::vector<int>& cov = kfs[k].covisible;
        const size_t ncov = std::min<size_t>(10, cov.size());
        for (size_t c = 0; c < ncov; c++) {  // the first 10 (the list may grow below: by index)
            const int nb = kfs[k].covisible[c];
            if (!kfs[nb].bad && !mark.count(nb)) { local.push_back(nb); mark.insert(nb); break; }
        }
        ch.assign(kfs[k].children.begin(), kfs[k].children.end());
        std::sort(ch.begin(), ch.end());
        for (int c : ch)
            if (!kfs[c].bad && !mark.count(c)) { local.push_back(c); mark.insert(c); break; }
        const int p = kfs[k].parent;
        if (p >= 0 && !mark.count(p)) {
            local.push_back(p);
            mark.insert(p);
            break;
        }
    }
    local_kfs = local;
    if (kfmax >= 0) {
        ref_kf = kfmax;
        cf.ref_kf = kfmax;
    }
}

void orbmi_slam::update_local_points() {  // src/Tracking.cc:1421-1450
    std::vector<int> out;
    local_mark.clear();
    for (int k : local_kfs)
        for (int m : kfs[k].mps)
            if (m >= 0 && !local_mark.count(m) && !mps[m].bad) {
                out.push_back(m);
                local_mark.insert(m);
            }
    local_mps.swap(out);
}

// SearchLocalPoints' first loop (src/Tracking.cc:1345-1362) over the frame's own points; occ[i]:
// keypoint i keeps a point with observations
void orbmi_slam::mark_own_points(TrackedFrame& cf, uint8_t* occ) {
    for (int i = 0; i < cf.n(); i++) {
        const int m = cf.mps[i];
        occ[i] = 0;
        if (m < 0) continue;
        if (mps[m].bad) cf.mps[i] = -1;
        else {
            mps[m].visible++;  // IncreaseVisible
            seen.insert(m);
            occ[i] = mps[m].nobs > 0 ? 1 : 0;
        }
    }
}

// TrackLocalMap's count of the optimised matches (src/Tracking.cc:1087-1101)
void orbmi_slam::local_map_result(TrackedFrame& cf, orbmi_slam_frame_stats& st, bool& ok) {
    int inliers = 0;
    for (int i = 0; i < cf.n(); i++) {  // (:1087-1101)
        const int m = cf.mps[i];
        if (m < 0) continue;
        if (!cf.outlier[i]) {
            mps[m].found++;  // IncreaseFound
            if (mps[m].nobs > 0) inliers++;
        } else if (cf.ur[i] >= 0) {
            cf.mps[i] = -1;  // stereo outliers are dropped
        }
    }
    matches_inliers = inliers;
    st.inliers = inliers;
    ok = inliers >= 30;
}

// the per-call form: each operator stages its host inputs and synchronises
int orbmi_slam::track_local_map_staged(TrackedFrame& cf, orbmi_slam_frame_stats& st, bool& ok) {
    std::vector<uint8_t> occ(std::max(cf.n(), 1), 0);
    mark_own_points(cf, occ.data());
    PhaseTimer ptr(&phase_ms[PH_LOCAL_RECORDS]);
    std::vector<orbmi_mappoint> rec(local_mps.size());
    mp_records_into(local_mps, rec.data());
    ptr.stop();
    const orbmi_frame_view vc = view(cf, cf.tcw.data());
    std::vector<int32_t> m_mp(std::max(cf.n(), 1), -1);
    int nl = 0;
    // isInFrustum(0.5) -> IncreaseVisible, then SearchByProjection(F, points, th = 1), 0.8: one
    // fused call (with no point in view the search finds nothing, as the reference's skipped one)
    std::vector<orbmi_mappoint_track> tr(std::max<size_t>(rec.size(), 1));
    {
        PhaseTimer pt(&phase_ms[PH_LOCAL_SEARCH]);
        SLAM_CHECK(unlocked(ORBMI_SCHED_T_LOCAL, cf.id, [&] {
            return orbmi_search_local_points_track(matcher, &vc, occ.data(), rec.data(), (int)rec.size(), 1.f,
                                                   m_mp.data(), &nl, nullptr, tr.data());
        }));
    }
    for (size_t j = 0; j < rec.size(); j++)
        if (tr[j].in_view) mps[local_mps[j]].visible++;
    st.local_map_points = (int)local_mps.size();
    st.local_matches = nl;
    std::vector<int> cur = cf.mps;
    for (int i = 0; i < cf.n(); i++)
        if (m_mp[i] >= 0) cur[i] = local_mps[m_mp[i]];
    const std::vector<orbmi_lastframe_point> lfp = lf_records(cur, nullptr);
    std::vector<int32_t> m_lf(cf.n(), -1);
    for (int i = 0; i < cf.n(); i++)
        if (cur[i] >= 0) m_lf[i] = i;
    M4 tcw;
    std::vector<uint8_t> out;
    {
        PhaseTimer pt(&phase_ms[PH_LOCAL_POSE]);
        SLAM_CHECK(pose_optimization(cf, m_lf, lfp, tcw, out));
    }
    cf.tcw = tcw;
    cf.mps = cur;
    cf.outlier = out;
    local_map_result(cf, st, ok);
    return ORBMI_OK;
}

int orbmi_slam::track_motion_model(TrackedFrame& cf, orbmi_slam_frame_stats& st, bool& ok) {  // src/Tracking.cc:997-1063
    ok = false;
    TrackedFrame& lf = last_frame;
    lf.tcw = mul(rel_poses.back(), kfs[lf.ref_kf].tcw);  // UpdateLastFrame (pose only, SLAM mode)
    cf.tcw = mul(velocity, lf.tcw);
    cf.has_tcw = true;
    return staged_track ? track_motion_model_staged(cf, st, ok) : track_motion_model_dev(cf, st, ok);
}

int orbmi_slam::track_local_map(TrackedFrame& cf, orbmi_slam_frame_stats& st, bool& ok) {  // src/Tracking.cc:1075-1104
    ok = false;
    {
        PhaseTimer pt(&phase_ms[PH_LOCAL_UPDATE]);
        update_local_keyframes(cf);
        update_local_points();
    }
    return staged_track ? track_local_map_staged(cf, st, ok) : track_local_map_dev(cf, st, ok);
}

// Tracking::TrackWithMotionModel (src/Tracking.cc:997-1063), device-resident: the last frame's
// point records go up once; SearchByProjection(CF, LF, 7) and the retry at 14 when fewer than
// 20 matched (the count stays on the device), PoseOptimization on those matches, then one
// read-back.  The pose optimisation is enqueued even when the search will have found fewer
// than 20 matches; the host then ignores it, as the reference never runs it.
int orbmi_slam::track_motion_model_dev(TrackedFrame& cf, orbmi_slam_frame_stats& st, bool& ok) {
    TrackedFrame& lf = last_frame;
    const int nc = cf.n(), nl = lf.n();
    SLAM_CHECK(track_buffers(nc, nl, 0));
    TrackBuf& t = tb;
    lf_records_into(lf.mps, &lf.outlier, t.h_lfp);
    std::memset(t.h_occ, 0, (size_t)std::max(nc, 1));
    *t.h_n = 0;
    SLAM_CHECK(up_range(t.h_occ, t.h_n + 1));  // occ, the last frame's points, n = 0
    const orbmi_frame_view vc = view(cf, cf.tcw.data()), vl = view(lf, lf.tcw.data());
    const float th = 7.f;  // stereo (src/Tracking.cc:1011-1014)
    orbmi_frame_mappoints fm{};
    fm.match_lf = t.d_m;
    fm.lf_points = t.d_lfp;
    fm.n_lf_points = nl;
    {
        PhaseTimer pt(&phase_ms[PH_LF_SEARCH]);
        SLAM_CHECK(unlocked(ORBMI_SCHED_T_LF, cf.id, [&] {
            int rc = orbmi_search_by_projection_last_frame_if(matcher, &vc, t.d_occ, &vl, t.d_lfp, th, 0, 1, t.d_m,
                                                              t.d_n, 1);
            if (!rc) rc = orbmi_search_by_projection_last_frame_if(matcher, &vc, t.d_occ, &vl, t.d_lfp, 2 * th, 0, 1,
                                                                   t.d_m, t.d_n, 20);
            if (!rc) rc = orbmi_pose_optimization_frame(pose, &vc, inv_level_sigma2.data(), &fm, t.d_pose, t.d_out);
            if (!rc) rc = down_range(t.h_n, t.h_m + nc);  // n, pose, outliers, matches
            if (!rc && hipStreamSynchronize(tstream) != hipSuccess) rc = ORBMI_E_HIP;
            return rc;
        }));
    }
    motion_model_result(cf, *t.h_n, t.h_m, t.h_pose->tcw, t.h_out, st, ok);
    return ORBMI_OK;
}

// Tracking::TrackLocalMap (src/Tracking.cc:1075-1104), device-resident: UpdateLocalMap on the
// host, then the local map points' records, the occupancy and the frame's own point records
// go up once; SearchLocalPoints (isInFrustum + SearchByProjection(F, MPs, 1)) and
// PoseOptimization over the frame's points and the new matches (keypoint i's edge uses the
// local map point when it matched one, else its own point), then one read-back.
int orbmi_slam::track_local_map_dev(TrackedFrame& cf, orbmi_slam_frame_stats& st, bool& ok) {
    const int nc = cf.n(), nr = (int)local_mps.size();
    SLAM_CHECK(track_buffers(nc, nc, nr));
    TrackBuf& t = tb;
    mark_own_points(cf, t.h_occ);
    {
        PhaseTimer pr(&phase_ms[PH_LOCAL_RECORDS]);
        mp_records_into(local_mps, t.h_rec);
        lf_records_into(cf.mps, nullptr, t.h_lfp);
        for (int i = 0; i < nc; i++) t.h_mlf[i] = cf.mps[i] >= 0 ? i : -1;
    }
    SLAM_CHECK(up_range(t.h_rec, t.h_lfp + nc));  // local map records, own-point index, occ, own records
    const orbmi_frame_view vc = view(cf, cf.tcw.data());
    orbmi_frame_mappoints fm{};
    fm.match_lf = t.d_mlf;
    fm.lf_points = t.d_lfp;
    fm.n_lf_points = nc;
    fm.match_mp = t.d_m;
    fm.mps = t.d_rec;
    fm.n_mps = nr;
    {
        PhaseTimer pt(&phase_ms[PH_LOCAL_SEARCH]);
        SLAM_CHECK(unlocked(ORBMI_SCHED_T_LOCAL, cf.id, [&] {
            int rc = orbmi_search_local_points_track(matcher, &vc, t.d_occ, t.d_rec, nr, 1.f, t.d_m, nullptr, nullptr,
                                                     t.d_tr);
            if (!rc) rc = orbmi_pose_optimization_frame(pose, &vc, inv_level_sigma2.data(), &fm, t.d_pose, t.d_out);
            if (!rc) rc = down_range(t.h_n, t.h_tr + nr);  // pose, outliers, matches, frustum records
            if (!rc && hipStreamSynchronize(tstream) != hipSuccess) rc = ORBMI_E_HIP;
            return rc;
        }));
    }
    int nl = 0;
    for (int j = 0; j < nr; j++)
        if (t.h_tr[j].in_view) mps[local_mps[j]].visible++;
    std::vector<int> cur = cf.mps;
    for (int i = 0; i < nc; i++)
        if (t.h_m[i] >= 0) { cur[i] = local_mps[t.h_m[i]]; nl++; }
    st.local_map_points = nr;
    st.local_matches = nl;
    std::memcpy(cf.tcw.data(), t.h_pose->tcw, sizeof(t.h_pose->tcw));
    cf.mps = cur;
    cf.outlier.assign(t.h_out, t.h_out + nc);
    local_map_result(cf, st, ok);
    return ORBMI_OK;
}

// ---- Tracking::Track (stereo, SLAM mode) ------------------------------------------------------
int orbmi_slam::track(TrackedFrame& cf) {
    if (state == NO_IMAGES_YET) state = NOT_INITIALIZED;
    orbmi_slam_frame_stats st;
    std::memset(&st, 0xff, sizeof(st));  // -1 = not run
    st.frame = cf.id;
    st.n = cf.n();
    if (state == NOT_INITIALIZED) {
        SLAM_CHECK(stereo_initialization(cf));
        st.init = state == OK;
        if (state != OK) {
            st.state = state;
            st.keyframes = (int)kfs.size();
            st.mappoints = count_mappoints();
            stats.push_back(st);
            return ORBMI_OK;
        }
    } else {
        bool ok = false;
        if (state == OK) {
            for (int& m : last_frame.mps)  // Tracking::CheckReplacedInLastFrame
                if (m >= 0 && mps[m].replaced >= 0) m = mps[m].replaced;
            if (!has_velocity || cf.id < last_reloc_frame_id + 2) SLAM_CHECK(track_reference_kf(cf, st, ok));
            else {
                SLAM_CHECK(track_motion_model(cf, st, ok));
                if (!ok) SLAM_CHECK(track_reference_kf(cf, st, ok));
            }
        }  // else: Relocalization is out of scope
        cf.ref_kf = ref_kf;
        if (ok) SLAM_CHECK(track_local_map(cf, st, ok));
        state = ok ? OK : LOST;
        if (ok) {
            if (last_frame.has_tcw) {
                velocity = mul(cf.tcw, pose_inverse(last_frame.tcw));
                has_velocity = true;
            } else {
                has_velocity = false;
            }
            for (int i = 0; i < cf.n(); i++) {  // clean VO matches (:504-513)
                const int m = cf.mps[i];
                if (m >= 0 && mps[m].nobs < 1) {
                    cf.outlier[i] = 0;
                    cf.mps[i] = -1;
                }
            }
            if (need_new_keyframe(cf, st)) {
                PhaseTimer pt(&phase_ms[PH_KEYFRAME]);
                SLAM_CHECK(create_new_keyframe(cf));
            }
            for (int i = 0; i < cf.n(); i++)  // (:535-539)
                if (cf.mps[i] >= 0 && cf.outlier[i]) cf.mps[i] = -1;
        }
        // Reset if the camera gets lost soon after initialisation (src/Tracking.cc:540-551):
        // the map is cleared and the next frame initialises again; this frame is not recorded.
        // With the mapping thread running, System::Reset only raises mbReset and
        // Tracking::Reset runs at the start of the next TrackStereo (src/System.cc:139-146),
        // outside mMutexMapUpdate: a LocalBA that finishes meanwhile needs that lock for its
        // write-back, so waiting for the mapping thread here, inside Track(), would deadlock.
        if (state == LOST && keyframes_in_map() <= 5) {
            if (async_lm()) {
                request_reset();
            } else {
                SLAM_CHECK(reset());
            }
            resets++;
            st.reset = 1;
            st.state = state;
            st.keyframes = 0;
            st.mappoints = 0;
            stats.push_back(st);
            return ORBMI_OK;
        }
        if (cf.ref_kf < 0) cf.ref_kf = ref_kf;
    }
    last_frame = cf;
    have_last = true;
    if (cf.has_tcw) {
        rel_poses.push_back(mul(cf.tcw, pose_inverse(kfs[cf.ref_kf].tcw)));
        references.push_back(ref_kf);
        frame_times.push_back(cf.ts);
        lost.push_back(state == LOST);
    } else if (!rel_poses.empty()) {
        rel_poses.push_back(rel_poses.back());
        references.push_back(references.back());
        frame_times.push_back(frame_times.back());
        lost.push_back(state == LOST);
    }
    st.state = state;
    st.keyframes = (int)kfs.size();
    st.mappoints = count_mappoints();
    stats.push_back(st);
    return ORBMI_OK;
}
