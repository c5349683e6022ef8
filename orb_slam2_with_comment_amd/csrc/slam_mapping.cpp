// LocalMapping of the native SLAM loop (slam.h): the keyframe queue and the mapping thread,
// LocalMapping::Run, CreateNewMapPoints, SearchInNeighbors' Fuse searches and replays, and
// LocalBundleAdjustment's graph assembly and write-back.
#include "slam.h"

void orbmi_slam::normals(const std::vector<int>& pts) {  // UpdateNormalAndDepth of each (timed)
    PhaseTimer pt(&phase_ms[PH_LM_NORMALS]);
    for (int m : pts) update_normal_and_depth(m);
}

void orbmi_slam::connections(int k) {
    PhaseTimer pt(&phase_ms[PH_LM_CONNECTIONS]);
    update_connections(k);
}

int orbmi_slam::distinctive(const std::vector<int>& pts) {
    std::vector<uint8_t> rows;
    std::vector<int32_t> off;
    {
        PhaseTimer pt(&phase_ms[PH_LM_OBSROWS]);
        obs_rows(pts, rows, off);
    }
    if (rows.empty()) return ORBMI_OK;
    const int np = (int)pts.size();
    std::vector<int32_t> best(std::max(np, 1));
    std::vector<uint8_t> out((size_t)std::max(np, 1) * 32);
    orbmi_matcher* mt = lmm();
    SLAM_CHECK(unlocked(ORBMI_SCHED_L_DISTINCTIVE, -1, [&] {
        PhaseTimer pt(&phase_ms[PH_LM_DISTINCTIVE_CALL]);
        return orbmi_compute_distinctive_descriptors(mt, rows.data(), off.data(), np, best.data(), out.data());
    }));
    for (int j = 0; j < np; j++)
        if (off[j + 1] > off[j]) std::memcpy(mps[pts[j]].desc, &out[32 * j], 32);
    return ORBMI_OK;
}

// LocalMapping::InsertKeyFrame: run it now (synchronous mode) or queue it for the thread
int orbmi_slam::insert_keyframe(int k) {
    if (!async_lm()) return local_mapping(k);
    {
        std::lock_guard<std::mutex> g(q_mtx);
        if (lm_rc) return lm_rc;
        lm_queue.push_back(k);
        set_abort_ba(1);  // a new keyframe interrupts the running BA (src/LocalMapping.cc:134)
    }
    q_cv.notify_one();
    return ORBMI_OK;
}

bool orbmi_slam::new_keyframes_queued() {  // LocalMapping::CheckNewKeyFrames
    if (!async_lm()) return false;
    std::lock_guard<std::mutex> g(q_mtx);
    return !lm_queue.empty();
}

// the mapping thread: one keyframe at a time, holding map_mtx except inside its GPU calls.
// The keyframe is taken from the queue and AcceptKeyFrames changes only under map_mtx (as
// Tracking reads them), so the order of the map_mtx acquisitions (the schedule) decides every
// interaction of the two threads.
void orbmi_slam::lm_run() {
    on_mapping_thread = true;
    for (;;) {
        {
            std::unique_lock<std::mutex> g(q_mtx);
            q_cv.wait(g, [&] { return lm_quit || !lm_queue.empty(); });
            if (lm_queue.empty()) return;  // quit with nothing left
        }
        int rc = ORBMI_OK;
        {
            std::unique_lock<std::mutex> m(map_mtx);
            log_section(ORBMI_SCHED_L_JOB, -1);
            int k = -1;
            {
                std::lock_guard<std::mutex> g(q_mtx);
                if (!lm_queue.empty()) {  // (a reset may have dropped it meanwhile)
                    k = lm_queue.front();
                    lm_queue.pop_front();
                    lm_busy = true;  // SetAcceptKeyFrames(false)
                }
            }
            if (recording) sched.back().arg = k;
            if (k >= 0) {
                held_lock = &m;
                rc = local_mapping(k);
                held_lock = nullptr;
            }
            hold_end();
            std::lock_guard<std::mutex> g(q_mtx);
            lm_busy = false;  // SetAcceptKeyFrames(true), still under map_mtx
            if (rc && !lm_rc) lm_rc = rc;
        }
        idle_cv.notify_all();
    }
}

int orbmi_slam::wait_local_mapping() {  // until the queue is empty and the thread idle
    if (!async_lm()) return ORBMI_OK;
    std::unique_lock<std::mutex> g(q_mtx);
    idle_cv.wait(g, [&] { return lm_queue.empty() && !lm_busy; });
    return lm_rc;
}

// ---- LocalMapping (synchronous) -------------------------------------------------------------
// LocalMapping::Run for one keyframe (src/LocalMapping.cc:47-128), no other keyframe queued and
// no stop request: ProcessNewKeyFrame, MapPointCulling, CreateNewMapPoints,
// SearchInNeighbors, LocalBundleAdjustment (more than 2 keyframes), KeyFrameCulling
int orbmi_slam::local_mapping(int k) {
    PhaseTimer all(&phase_ms[PH_LM_TOTAL]);
    PhaseTimer step(&phase_ms[PH_LM_PROCESS]);
    auto next = [&](Phase p) { step.move_to(&phase_ms[p]); };
    // ProcessNewKeyFrame (src/LocalMapping.cc:152-211): ComputeBoW, the observations of the
    // keyframe's points, UpdateNormalAndDepth, ComputeDistinctiveDescriptors, UpdateConnections.
    // The transform reads only the keyframe's descriptors, so it runs in the same window with
    // the map lock released as the descriptors of the updated points: one release, and the
    // two device calls overlap (the keyframe's descriptors are copied first when it has no
    // HBM copy: Tracking may grow kfs meanwhile).
    const bool need_bow = voc && !kfs[k].fv.valid;
    std::vector<int> updated;
    for (int i = 0; i < (int)kfs[k].mps.size(); i++) {
        const int m = kfs[k].mps[i];
        if (m < 0 || mps[m].bad) continue;
        if (!mps[m].obs.count(k)) {
            add_observation(m, k, i);
            updated.push_back(m);
        } else {
            recent_mps.push_back(m);  // the new stereo points the Tracking inserted
        }
    }
    normals(updated);
    std::vector<uint8_t> rows;
    std::vector<int32_t> off;
    {
        PhaseTimer pt(&phase_ms[PH_LM_OBSROWS]);
        obs_rows(updated, rows, off);
    }
    if (need_bow || !rows.empty()) {
        const int np = (int)updated.size();
        std::vector<int32_t> best(std::max(np, 1));
        std::vector<uint8_t> out((size_t)std::max(np, 1) * 32);
        const uint8_t* d_desc = kfs[k].d_desc;
        const int nk = (int)kfs[k].keys.size();
        const std::vector<uint8_t> desc = need_bow && !d_desc ? kfs[k].desc : std::vector<uint8_t>();
        FeatVec fv;
        orbmi_matcher* mt = lmm();
        SLAM_CHECK(unlocked(need_bow ? ORBMI_SCHED_L_BOW : ORBMI_SCHED_L_DISTINCTIVE, need_bow ? k : -1, [&] {
            int rc = ORBMI_OK;
            const bool async_bow = need_bow && d_desc && nk > 0;
            if (async_bow) rc = bow_begin(d_desc, nk);
            else if (need_bow) rc = compute_bow(desc, fv);
            if (!rc && !rows.empty()) {
                PhaseTimer pt(&phase_ms[PH_LM_DISTINCTIVE_CALL]);
                rc = orbmi_compute_distinctive_descriptors(mt, rows.data(), off.data(), np, best.data(), out.data());
            }
            if (async_bow) {
                const int rc2 = bow_end(fv);
                if (!rc) rc = rc2;
            }
            return rc;
        }));
        if (need_bow && !kfs[k].fv.valid) kfs[k].fv = std::move(fv);  // (Tracking may have computed it: the same)
        if (!rows.empty())
            for (int j = 0; j < np; j++)
                if (off[j + 1] > off[j]) std::memcpy(mps[updated[j]].desc, &out[32 * j], 32);
    }
    connections(k);
    if (recording) {  // ProcessNewKeyFrame's outcome: BowVector words, FeatureVector, slots
        const FeatVec& fv = kfs[k].fv;
        uint32_t h = kFnv0;
        for (uint32_t v : fv.node) h = fnv_mix(h, v);
        for (int32_t v : fv.off) h = fnv_mix(h, (uint32_t)v);
        for (int32_t v : fv.feat) h = fnv_mix(h, (uint32_t)v);
        log_state(k, ORBMI_KF_STATE_PROCESS, fv.valid ? fv.words : -1, h, slot_hash(k));
    }
    next(PH_LM_CULL);
    map_point_culling(k);
    // SearchInNeighbors' last ComputeDistinctiveDescriptors (all the keyframe's points) rides in
    // LocalBA's device window when LocalBA runs (one map-lock release fewer per keyframe)
    std::vector<int> owed2;
    if (s.local_mapping) {
        next(PH_LM_CREATE);
        const size_t nmp0 = mps.size();
        std::vector<int> owed;
        SLAM_CHECK(create_new_map_points(k, owed));
        log_state(k, ORBMI_KF_STATE_CREATE, (int)(mps.size() - nmp0), (uint32_t)mps.size(), slot_hash(k));
        next(PH_LM_FUSE);
        if (new_keyframes_queued()) {
            sin_skipped++;
            SLAM_CHECK(distinctive(owed));
        } else {
            fuse_ops = 0;
            SLAM_CHECK(search_in_neighbors(k, owed, owed2));
            int filled = 0;
            for (int m : kfs[k].mps) filled += m >= 0;
            log_state(k, ORBMI_KF_STATE_FUSE, fuse_ops, (uint32_t)filled, slot_hash(k));
        }
    }
    set_abort_ba(0);
    lm_jobs++;
    if (new_keyframes_queued()) {
        ba_skipped++;
        SLAM_CHECK(distinctive(owed2));
    } else {
        next(PH_LM_BA);
        if (s.local_ba && keyframes_in_map() > 2) SLAM_CHECK(local_bundle_adjustment(k, owed2));
        else SLAM_CHECK(distinctive(owed2));
        next(PH_LM_KFCULL);
        if (s.local_mapping) keyframe_culling(k, s.th_depth);
    }
    return ORBMI_OK;
}

orbmi_tri_keyframe orbmi_slam::tri_view(const KeyFrame& kf) const {
    return orbmi_tri_keyframe{kf.tcw.data(), kf.keys.data(), kf.ur.data(), kf.depth.data(), s.fx, s.fy, s.cx,
                              s.cy, s.bf, s.bf / s.fx, level_sigma2.data(), scale_factors.data()};
}

// CreateNewMapPoints' decision on one neighbour (src/LocalMapping.cc:336-363): the baseline
// between the camera centres against the stereo baseline, both FeatureVectors present, then F12.
// `use`: the pair is searched (F12 is computed only then)
int orbmi_slam::create_pair(int k, int k2, const float ow1[3], float F12[9], bool& use) {
    use = false;
    float ow2[3];
    kf_ow(k2, ow2);
    const float d[3] = {ow2[0] - ow1[0], ow2[1] - ow1[1], ow2[2] - ow1[2]};
    const float baseline = (float)std::sqrt(((double)d[0] * d[0] + (double)d[1] * d[1]) + (double)d[2] * d[2]);
    if (baseline < s.bf / s.fx) return ORBMI_OK;
    if (!kfs[k].fv.valid || !kfs[k2].fv.valid) return ORBMI_OK;
    const orbmi_tri_keyframe v1 = tri_view(kfs[k]), v2 = tri_view(kfs[k2]);
    SLAM_CHECK(orbmi_compute_f12(&v1, &v2, F12));
    use = true;
    return ORBMI_OK;
}

// the triangulated point of keypoint i1 of k and i2 of k2 (src/LocalMapping.cc:547-565): the
// MapPoint, both observations, both keyframe slots, mlpRecentAddedMapPoints.  Returns its id.
int orbmi_slam::add_triangulated(int k, int i1, int k2, int i2, const float x3d[3]) {
    MapPoint mp;
    mp.id = (int)mps.size();
    std::memcpy(mp.pos, x3d, 3 * sizeof(float));
    mp.ref_kf = k;
    mp.first_kf_id = k;
    mps.push_back(mp);
    add_observation(mp.id, k, i1);
    add_observation(mp.id, k2, i2);
    kfs[k].mps[i1] = mp.id;
    kfs[k2].mps[i2] = mp.id;
    recent_mps.push_back(mp.id);
    return mp.id;
}

// src/LocalMapping.cc:290-577, stereo: the 10 best covisible keyframes.  The neighbours that
// pass the baseline test go to the device in one orbmi_create_new_map_points call (searches and
// triangulation pair by pair, the keypoints earlier pairs claimed excluded on the device), run
// on the keyframes' HBM copies with the map lock released; the new points are then made here in
// the reference's order.
// `owed`: the new points, whose ComputeDistinctiveDescriptors the caller does (with
// SearchInNeighbors' first device call when that runs: one round trip fewer)
int orbmi_slam::create_new_map_points(int k, std::vector<int>& owed) {
    owed.clear();
    float ow1[3];
    kf_ow(k, ow1);
    const std::vector<int> neigh(kfs[k].covisible.begin(),
                                 kfs[k].covisible.begin() + std::min<size_t>(10, kfs[k].covisible.size()));
    if (!kfs[k].fv.valid || !kfs[k].d_keys) return create_new_map_points_host(k);
    std::vector<int> pk, pos;  // the neighbours searched, and their index in `neigh`
    std::vector<M4> tcw2;
    std::vector<float> F12;
    std::vector<std::vector<uint8_t>> has2;
    const M4 tcw1 = kfs[k].tcw;
    for (size_t i = 0; i < neigh.size(); i++) {
        const int k2 = neigh[i];
        float F[9];
        bool use;
        SLAM_CHECK(create_pair(k, k2, ow1, F, use));
        if (!use) continue;
        if (!kfs[k2].d_keys) return create_new_map_points_host(k);
        pk.push_back(k2);
        pos.push_back((int)i);
        tcw2.push_back(kfs[k2].tcw);
        F12.insert(F12.end(), F, F + 9);
        has2.emplace_back(std::max<size_t>(kfs[k2].mps.size(), 1), 0);
        for (size_t q = 0; q < kfs[k2].mps.size(); q++) has2.back()[q] = kfs[k2].mps[q] >= 0;
    }
    const int np = (int)pk.size();
    if (np == 0) return ORBMI_OK;
    const size_t n1 = kfs[k].keys.size();
    std::vector<uint8_t> has1(std::max<size_t>(n1, 1), 0);
    for (size_t i = 0; i < n1; i++) has1[i] = kfs[k].mps[i] >= 0;
    // views on copies of the poses and on HBM arrays: valid while the lock is released
    auto tri_dev = [&](const KeyFrame& kf, const M4& tcw) {
        orbmi_tri_keyframe t = tri_view(kf);
        t.tcw = tcw.data();
        t.keys_un = kf.d_keys;
        t.u_right = kf.d_ur;
        t.depth = kf.d_depth;
        return t;
    };
    const orbmi_frame_view f1 = kf_view(kfs[k], tcw1.data());
    const orbmi_tri_keyframe t1 = tri_dev(kfs[k], tcw1);
    const orbmi_feature_vector fv1 = kfs[k].fv.view();
    const float* cos1 = kfs[k].d_cos;
    std::vector<orbmi_frame_view> f2(np);
    std::vector<orbmi_tri_keyframe> t2(np);
    std::vector<orbmi_feature_vector> fv2(np);
    std::vector<const float*> cos2(np);
    std::vector<const uint8_t*> mp2(np);
    for (int j = 0; j < np; j++) {
        const KeyFrame& K2 = kfs[pk[j]];
        f2[j] = kf_view(K2, tcw2[j].data());
        t2[j] = tri_dev(K2, tcw2[j]);
        fv2[j] = K2.fv.view();
        cos2[j] = K2.d_cos;
        mp2[j] = has2[j].data();
    }
    std::vector<int32_t> m12(std::max<size_t>(n1 * np, 1));
    std::vector<uint8_t> ok(std::max<size_t>(n1 * np, 1));
    std::vector<float> x3d(std::max<size_t>(3 * n1 * np, 1));
    orbmi_matcher* mt = lmm();
    SLAM_CHECK(unlocked(ORBMI_SCHED_L_CREATE, k, [&] {
        PhaseTimer pt(&phase_ms[PH_LM_CREATE_CALL]);
        return orbmi_create_new_map_points(mt, &f1, &t1, cos1, has1.data(), &fv1, np, f2.data(), t2.data(),
                                           cos2.data(), mp2.data(), fv2.data(), F12.data(), m12.data(), ok.data(),
                                           x3d.data());
    }));
    std::vector<int> fresh;
    for (int j = 0; j < np; j++) {
        if (pos[j] > 0 && new_keyframes_queued()) break;  // src/LocalMapping.cc:331
        const int k2 = pk[j];
        for (size_t i = 0; i < n1; i++) {
            const size_t r = (size_t)j * n1 + i;
            if (!ok[r]) continue;
            fresh.push_back(add_triangulated(k, (int)i, k2, m12[r], &x3d[3 * r]));
        }
    }
    // ComputeDistinctiveDescriptors per point, so one batch for all pairs gives the
    // reference's per-pair results; UpdateNormalAndDepth does not read the descriptor
    normals(fresh);
    owed = std::move(fresh);
    return ORBMI_OK;
}

// the same loop with a search call per pair and the host geometry (keyframes without HBM copies)
int orbmi_slam::create_new_map_points_host(int k) {
    float ow1[3];
    kf_ow(k, ow1);
    std::vector<uint8_t> has1(std::max<size_t>(kfs[k].mps.size(), 1), 0);
    for (size_t i = 0; i < kfs[k].mps.size(); i++) has1[i] = kfs[k].mps[i] >= 0;
    const std::vector<int> neigh(kfs[k].covisible.begin(),
                                 kfs[k].covisible.begin() + std::min<size_t>(10, kfs[k].covisible.size()));
    const size_t n1 = kfs[k].keys.size();
    for (size_t i = 0; i < neigh.size(); i++) {
        if (i > 0 && new_keyframes_queued()) return ORBMI_OK;  // src/LocalMapping.cc:331
        const int k2 = neigh[i];
        float F12[9];
        bool use;
        SLAM_CHECK(create_pair(k, k2, ow1, F12, use));
        if (!use) continue;
        std::vector<uint8_t> has2(std::max<size_t>(kfs[k2].mps.size(), 1), 0);
        for (size_t i = 0; i < kfs[k2].mps.size(); i++) has2[i] = kfs[k2].mps[i] >= 0;
        const M4 tcw1 = kfs[k].tcw, tcw2 = kfs[k2].tcw;
        const orbmi_frame_view f1 = kf_view(kfs[k], tcw1.data()), f2 = kf_view(kfs[k2], tcw2.data());
        const orbmi_feature_vector fv1 = kfs[k].fv.view(), fv2 = kfs[k2].fv.view();
        std::vector<int32_t> m12(std::max<size_t>(n1, 1));
        int nm = 0;
        orbmi_matcher* mt = lmm();
        SLAM_CHECK(unlocked(ORBMI_SCHED_L_CREATE_PAIR, (int)i, [&] {
            return orbmi_search_for_triangulation(mt, &f1, has1.data(), &fv1, &f2, has2.data(), &fv2, F12, 0, 0,
                                                  m12.data(), &nm);
        }));
        std::vector<int32_t> idx1, idx2;
        for (size_t i = 0; i < n1; i++)
            if (m12[i] >= 0) { idx1.push_back((int32_t)i); idx2.push_back(m12[i]); }
        if (idx1.empty()) continue;
        std::vector<float> x3d(3 * idx1.size());
        std::vector<uint8_t> ok(idx1.size());
        {
            const orbmi_tri_keyframe v1 = tri_view(kfs[k]), v2 = tri_view(kfs[k2]);
            SLAM_CHECK(orbmi_triangulate_matches(&v1, &v2, idx1.data(), idx2.data(), (int)idx1.size(), x3d.data(),
                                                 ok.data()));
        }
        std::vector<int> fresh;
        for (size_t q = 0; q < idx1.size(); q++) {
            if (!ok[q]) continue;
            fresh.push_back(add_triangulated(k, idx1[q], k2, idx2[q], &x3d[3 * q]));
            has1[idx1[q]] = 1;
        }
        SLAM_CHECK(distinctive(fresh));
        for (int m : fresh) update_normal_and_depth(m);
    }
    return ORBMI_OK;
}

// the search record of a map point (orbmi_mappoint)
orbmi_mappoint orbmi_slam::fuse_record(int m) const {
    const MapPoint& mp = mps[m];
    orbmi_mappoint r;
    std::memset(&r, 0, sizeof(r));
    std::memcpy(r.pos, mp.pos, sizeof(r.pos));
    std::memcpy(r.normal, mp.normal, sizeof(r.normal));
    r.max_distance = mp.max_distance;
    r.min_distance = mp.min_distance;
    r.flags = (mp.bad ? ORBMI_MP_BAD : 0u) | (mp.nobs > 0 ? ORBMI_MP_HAS_OBS : 0u);
    std::memcpy(r.desc, mp.desc, 32);
    return r;
}

// the search of Fuse(k, pts) on the GPU (map lock released on the mapping thread)
int orbmi_slam::fuse_search(int k, const std::vector<int>& pts, std::vector<int32_t>& best) {
    std::vector<orbmi_mappoint> rec(pts.size());
    std::vector<uint8_t> in_kf(pts.size());
    for (size_t j = 0; j < pts.size(); j++) {
        rec[j] = fuse_record(pts[j]);
        in_kf[j] = mps[pts[j]].obs.count(k) ? 1 : 0;
    }
    const M4 tcw = kfs[k].tcw;
    const orbmi_frame_view v = kf_view(kfs[k], tcw.data());
    best.assign(pts.size(), -1);
    std::vector<int32_t> dist(pts.size());
    int nc = 0;
    orbmi_matcher* mt = lmm();
    return unlocked(ORBMI_SCHED_L_FUSE, k, [&] {
        PhaseTimer pt(&phase_ms[PH_LM_FUSE_CALL]);
        return orbmi_fuse_search(mt, &v, rec.data(), in_kf.data(), (int)pts.size(), 3.f, best.data(), dist.data(), &nc);
    });
}

// the map updates of Fuse(k, pts) (src/ORBmatcher.cc:1096-1124) in list order
void orbmi_slam::fuse_replay(int k, const std::vector<int>& pts, const int32_t* best, std::set<int>& dirty) {
    for (size_t j = 0; j < pts.size(); j++) {
        const int m = pts[j], b = best[j];
        if (mps[m].bad || mps[m].obs.count(k) || b < 0) continue;
        const int in = kfs[k].mps[b];
        if (in >= 0) {
            if (!mps[in].bad) {
                fuse_touched.insert(m);
                fuse_touched.insert(in);
                if (mps[in].nobs > mps[m].nobs) {
                    if (replace(m, in)) { dirty.insert(in); fuse_ops++; }
                } else if (replace(in, m)) {
                    dirty.insert(m);
                    fuse_ops++;
                }
            }
        } else {
            fuse_touched.insert(m);
            add_observation(m, k, b);
            kfs[k].mps[b] = m;
            fuse_ops++;
        }
    }
}

// ORBmatcher::Fuse(pKF, vpMapPoints, 3.0) (src/ORBmatcher.cc:977-1127): the search for every
// point on the GPU, then the map updates in list order.  `dirty`: the survivors of Replace
// whose ComputeDistinctiveDescriptors (MapPoint::Replace, src/MapPoint.cc:212) is still due.
// The owed descriptors and the search go to the device as one orbmi_fuse_search_refresh call
// (one round trip): the search reads each due point's record with its new descriptor.
int orbmi_slam::fuse(int k, const std::vector<int>& list, std::set<int>& dirty) {
    std::vector<int> due;
    for (int m : dirty)
        if (!mps[m].bad) due.push_back(m);
    dirty.clear();
    std::vector<int> pts;
    for (int m : list)
        if (m >= 0) pts.push_back(m);
    if (pts.empty()) return distinctive(due);
    std::vector<uint8_t> rows;
    std::vector<int32_t> off;
    {
        PhaseTimer pt(&phase_ms[PH_LM_OBSROWS]);
        obs_rows(due, rows, off);
    }
    if (rows.empty()) {  // no descriptor changes: the plain search
        std::vector<int32_t> best;
        SLAM_CHECK(fuse_search(k, pts, best));
        fuse_replay(k, pts, best.data(), dirty);
        return ORBMI_OK;
    }
    const int nd = (int)due.size(), np = (int)pts.size();
    std::vector<orbmi_mappoint> rec(np);
    std::vector<uint8_t> in_kf(np);
    std::vector<int32_t> from(np, -1);
    for (int j = 0; j < np; j++) {
        rec[j] = fuse_record(pts[j]);
        in_kf[j] = mps[pts[j]].obs.count(k) ? 1 : 0;
        auto it = std::lower_bound(due.begin(), due.end(), pts[j]);  // (due ascending: a std::set's order)
        if (it != due.end() && *it == pts[j]) {
            const int d = (int)(it - due.begin());
            if (off[d + 1] > off[d]) from[j] = d;
        }
    }
    std::vector<int32_t> dbest(nd), best(np, -1), bd(np);
    std::vector<uint8_t> dout((size_t)nd * 32);
    for (int d = 0; d < nd; d++) std::memcpy(&dout[32 * d], mps[due[d]].desc, 32);
    const M4 tcw = kfs[k].tcw;
    const orbmi_frame_view v = kf_view(kfs[k], tcw.data());
    orbmi_matcher* mt = lmm();
    SLAM_CHECK(unlocked(ORBMI_SCHED_L_FUSE, k, [&] {
        PhaseTimer pt(&phase_ms[PH_LM_FUSE_CALL]);
        return orbmi_fuse_search_refresh(mt, rows.data(), off.data(), nd, dbest.data(), dout.data(), 1, &v,
                                         rec.data(), from.data(), in_kf.data(), np, 3.f, best.data(), bd.data());
    }));
    for (int d = 0; d < nd; d++)
        if (off[d + 1] > off[d]) std::memcpy(mps[due[d]].desc, &dout[32 * d], 32);
    fuse_replay(k, pts, best.data(), dirty);
    return ORBMI_OK;
}

// Fuse(target, the keyframe's points) for every target in order (src/LocalMapping.cc:620-628).
// The searches of all targets run in one orbmi_fuse_search_batch on the records as they are
// before the first target; a point's search depends only on its own record, its IsInKeyFrame
// and the target, so a target's batch result is the reference's wherever neither changed in
// the earlier targets' replays -- the points where one did (a Replace survivor's descriptor or
// observations) are searched again before that target's replay.  ComputeDistinctiveDescriptors
// of a survivor is done before the first read of its record (a survivor gains no observation
// from AddObservation before then: only listed points do, and a listed dirty point is
// recomputed before the target that could add one).
// `owed`: points whose descriptors CreateNewMapPoints left to compute -- computed in the same
// device call as the batched searches, which read them.
int orbmi_slam::fuse_targets(const std::vector<int>& targets, const std::vector<int>& list, std::set<int>& dirty,
                 const std::vector<int>& owed) {
    std::vector<int> pts;
    for (int m : list)
        if (m >= 0) pts.push_back(m);
    const int nt = (int)targets.size(), np = (int)pts.size();
    if (nt == 0 || np == 0) return distinctive(owed);
    PhaseTimer prep(&phase_ms[PH_LM_SIN_PREP]);
    fuse_touched.clear();
    std::vector<orbmi_mappoint> rec0(np);
    for (int j = 0; j < np; j++) rec0[j] = fuse_record(pts[j]);
    std::vector<uint8_t> in0((size_t)nt * np);
    std::vector<M4> tcw(nt);
    std::vector<orbmi_frame_view> views(nt);
    for (int t = 0; t < nt; t++) {
        for (int j = 0; j < np; j++) in0[(size_t)t * np + j] = mps[pts[j]].obs.count(targets[t]) ? 1 : 0;
        tcw[t] = kfs[targets[t]].tcw;
        views[t] = kf_view(kfs[targets[t]], tcw[t].data());
    }
    std::vector<int32_t> best((size_t)nt * np), dist((size_t)nt * np);
    orbmi_matcher* mt = lmm();
    // the owed descriptors (ascending ids, as created) and the records that take them
    std::vector<int> due;
    for (int m : owed)
        if (!mps[m].bad) due.push_back(m);
    std::vector<uint8_t> orows;
    std::vector<int32_t> ooff, ofrom;
    obs_rows(due, orows, ooff);
    const int nd = (int)due.size();
    std::vector<uint8_t> odesc;
    if (!orows.empty()) {
        ofrom.assign(np, -1);
        for (int j = 0; j < np; j++) {
            auto it = std::lower_bound(due.begin(), due.end(), pts[j]);
            if (it != due.end() && *it == pts[j]) {
                const int d = (int)(it - due.begin());
                if (ooff[d + 1] > ooff[d]) ofrom[j] = d;
            }
        }
        odesc.resize((size_t)nd * 32);
        for (int d = 0; d < nd; d++) std::memcpy(&odesc[32 * d], mps[due[d]].desc, 32);
    }
    prep.stop();
    SLAM_CHECK(unlocked(ORBMI_SCHED_L_FUSE_BATCH, -1, [&] {
        PhaseTimer pt(&phase_ms[PH_LM_FUSE_CALL]);
        if (orows.empty())
            return orbmi_fuse_search_batch(mt, nt, views.data(), rec0.data(), in0.data(), np, 3.f, best.data(),
                                           dist.data(), nullptr);
        std::vector<int32_t> dbest(nd);
        return orbmi_fuse_search_refresh(mt, orows.data(), ooff.data(), nd, dbest.data(), odesc.data(), nt,
                                         views.data(), rec0.data(), ofrom.data(), in0.data(), np, 3.f, best.data(),
                                         dist.data());
    }));
    if (!orows.empty()) {
        for (int d = 0; d < nd; d++)
            if (ooff[d + 1] > ooff[d]) std::memcpy(mps[due[d]].desc, &odesc[32 * d], 32);
        for (int j = 0; j < np; j++)
            if (ofrom[j] >= 0) std::memcpy(rec0[j].desc, &odesc[32 * ofrom[j]], 32);
    }
    std::map<int, int> listed;  // point -> its (first) position in pts
    for (int j = np - 1; j >= 0; j--) listed[pts[j]] = j;
    for (int t = 0; t < nt; t++) {
        const int kt = targets[t];
        std::vector<int> due;
        for (auto it = dirty.begin(); it != dirty.end();) {
            if (listed.count(*it)) {
                if (!mps[*it].bad) due.push_back(*it);
                it = dirty.erase(it);
            } else {
                ++it;
            }
        }
        if (!due.empty()) {
            // one device call: the due descriptors, and the searches of the listed records that
            // take them against this and every later target (their batch rows are stale)
            std::vector<uint8_t> rows;
            std::vector<int32_t> off;
            obs_rows(due, rows, off);
            const int nd = (int)due.size();
            std::vector<int> rj;  // positions in pts of the listed occurrences of due points
            std::vector<int32_t> from;
            for (int d = 0; d < nd; d++)
                for (int j = 0; j < np; j++)
                    if (pts[j] == due[d]) {
                        rj.push_back(j);
                        from.push_back(off[d + 1] > off[d] ? d : -1);
                    }
            const int nr = (int)rj.size(), ntr = nt - t;
            std::vector<orbmi_mappoint> rrec(std::max(nr, 1));
            std::vector<uint8_t> rin(std::max((size_t)nr * ntr, (size_t)1));
            std::vector<orbmi_frame_view> rv(views.begin() + t, views.end());
            for (int q = 0; q < nr; q++) {
                rrec[q] = fuse_record(pts[rj[q]]);
                for (int u = 0; u < ntr; u++) rin[(size_t)u * nr + q] = mps[pts[rj[q]]].obs.count(targets[t + u]) ? 1 : 0;
            }
            std::vector<int32_t> dbest(nd), bi((size_t)std::max(nr * ntr, 1)), bd((size_t)std::max(nr * ntr, 1));
            std::vector<uint8_t> dout((size_t)nd * 32);
            for (int d = 0; d < nd; d++) std::memcpy(&dout[32 * d], mps[due[d]].desc, 32);
            orbmi_matcher* mt2 = lmm();
            SLAM_CHECK(unlocked(ORBMI_SCHED_L_FUSE_REFRESH, t, [&] {
                PhaseTimer pt(&phase_ms[PH_LM_FUSE_CALL]);
                return orbmi_fuse_search_refresh(mt2, rows.empty() ? nullptr : rows.data(), off.data(), nd,
                                                 dbest.data(), dout.data(), ntr, rv.data(), rrec.data(),
                                                 from.data(), rin.data(), nr, 3.f, bi.data(), bd.data());
            }));
            for (int d = 0; d < nd; d++)
                if (off[d + 1] > off[d]) std::memcpy(mps[due[d]].desc, &dout[32 * d], 32);
            for (int q = 0; q < nr; q++) {
                rec0[rj[q]] = fuse_record(pts[rj[q]]);
                for (int u = 0; u < ntr; u++) best[(size_t)(t + u) * np + rj[q]] = bi[(size_t)u * nr + q];
            }
        }
        int32_t* row = best.data() + (size_t)t * np;
        std::vector<int> redo_pts, redo_j;
        PhaseTimer rt(&phase_ms[PH_LM_SIN_REDO]);
        // A record can change here only through an earlier target's replay (Replace, a new
        // observation: fuse_touched) -- Tracking creates points but changes no existing
        // point's position, normal, distances, flags or descriptor, and the refreshed
        // descriptors are in rec0 -- so only touched points are compared.  With recording on
        // (the parity tests) every point is compared too and a difference fails the call.
        for (int j = 0; j < np; j++) {
            const int m = pts[j];
            // the replay skips bad points and points already in the target (observations are
            // only gained here, so a point in the target now was in it or is skipped anyway)
            if (!recording && !fuse_touched.count(m)) continue;
            if (mps[m].bad || mps[m].obs.count(kt)) continue;
            const orbmi_mappoint r = fuse_record(m);
            if (std::memcmp(&r, &rec0[j], sizeof(r)) != 0) {
                if (!fuse_touched.count(m)) {
                    fprintf(stderr, "orbmi_slam: Fuse record of point %d changed untouched\n", m);
                    return ORBMI_E_STATE;
                }
                redo_pts.push_back(m);
                redo_j.push_back(j);
            }
        }
        rt.stop();
        if (!redo_pts.empty()) {
            std::vector<int32_t> b2;
            SLAM_CHECK(fuse_search(kt, redo_pts, b2));
            for (size_t q = 0; q < redo_j.size(); q++) row[redo_j[q]] = b2[q];
        }
        PhaseTimer rp(&phase_ms[PH_LM_SIN_REPLAY]);
        fuse_replay(kt, pts, row, dirty);
    }
    return ORBMI_OK;
}

// owed2 <- the keyframe's points, whose ComputeDistinctiveDescriptors (:656-667) the caller does
// -- in LocalBA's device window when that runs next.  UpdateNormalAndDepth and UpdateConnections
// do not read descriptors and are done here.
int orbmi_slam::search_in_neighbors(int k, const std::vector<int>& owed, std::vector<int>& owed2) {  // src/LocalMapping.cc:589-674, stereo: nn = 10
    std::vector<int> targets;
    const std::vector<int> neigh(kfs[k].covisible.begin(),
                                 kfs[k].covisible.begin() + std::min<size_t>(10, kfs[k].covisible.size()));
    for (int k1 : neigh) {
        if (kfs[k1].bad || kfs[k1].fuse_target_for_kf == k) continue;
        targets.push_back(k1);
        kfs[k1].fuse_target_for_kf = k;
        const std::vector<int> second(kfs[k1].covisible.begin(),
                                      kfs[k1].covisible.begin() + std::min<size_t>(5, kfs[k1].covisible.size()));
        for (int k2 : second) {
            if (kfs[k2].bad || kfs[k2].fuse_target_for_kf == k || k2 == k) continue;
            targets.push_back(k2);
        }
    }
    std::set<int> dirty;
    const std::vector<int> matches = kfs[k].mps;
    SLAM_CHECK(fuse_targets(targets, matches, dirty, owed));
    std::vector<int> cands;
    for (int t : targets)
        for (int m : kfs[t].mps) {
            if (m < 0 || mps[m].bad || mps[m].fuse_candidate_for_kf == k) continue;
            mps[m].fuse_candidate_for_kf = k;
            cands.push_back(m);
        }
    SLAM_CHECK(fuse(k, cands, dirty));
    dirty.clear();
    std::vector<int> upd;
    std::set<int> seen_pt;
    for (int m : kfs[k].mps)
        if (m >= 0 && !mps[m].bad && seen_pt.insert(m).second) upd.push_back(m);
    normals(upd);
    connections(k);
    owed2 = std::move(upd);
    return ORBMI_OK;
}

// Optimizer::LocalBundleAdjustment: the graph as src/Optimizer.cc:486-683 assembles it
// (system/optimizer.gather_local_ba), the optimisation on the GPU, the write-back (:776-805)
// `owed`: points whose ComputeDistinctiveDescriptors runs in the same device window as the
// optimisation (the descriptors written back with the poses)
int orbmi_slam::local_bundle_adjustment(int k, const std::vector<int>& owed) {
    PhaseTimer gt(&phase_ms[PH_LM_BA_GATHER]);
    std::vector<int> lkf{k};
    SeenSet& local_set = ba_local_mark;
    local_set.clear();
    local_set.insert(k);
    for (int c : kfs[k].covisible) {
        local_set.insert(c);
        if (!kfs[c].bad) lkf.push_back(c);
    }
    std::vector<int> lmp;
    SeenSet& seen_mp = ba_mp_mark;
    seen_mp.clear();
    for (int kk : lkf)
        for (int m : kfs[kk].mps)
            if (m >= 0 && !mps[m].bad && !seen_mp.count(m)) {
                seen_mp.insert(m);
                lmp.push_back(m);
            }
    std::vector<int> fixed;
    SeenSet& fixed_set = ba_fixed_mark;
    fixed_set.clear();
    for (int m : lmp)
        for (auto& o : mps[m].obs)
            if (!local_set.count(o.first) && !fixed_set.count(o.first)) {
                fixed_set.insert(o.first);
                if (!kfs[o.first].bad) fixed.push_back(o.first);
            }
    std::vector<int> all = lkf;
    all.insert(all.end(), fixed.begin(), fixed.end());
    std::vector<int> kidx(kfs.size(), -1);  // keyframe id -> its vertex
    for (int i = 0; i < (int)all.size(); i++) kidx[all[i]] = i;
    std::vector<orbmi_ba_keyframe> K(all.size());
    for (int i = 0; i < (int)all.size(); i++) {
        const KeyFrame& kf = kfs[all[i]];
        std::memcpy(K[i].tcw, kf.tcw.data(), sizeof(K[i].tcw));
        K[i].id = (uint32_t)kf.id;
        K[i].fixed = (i >= (int)lkf.size() || kf.id == 0) ? 1 : 0;
        K[i].fx = s.fx; K[i].fy = s.fy; K[i].cx = s.cx; K[i].cy = s.cy; K[i].bf = s.bf;
    }
    std::vector<orbmi_ba_point> P(lmp.size());
    for (int j = 0; j < (int)lmp.size(); j++) {
        const MapPoint& mp = mps[lmp[j]];
        std::memcpy(P[j].pos, mp.pos, sizeof(P[j].pos));
        P[j].id = (uint32_t)mp.id;
        P[j].bad = mp.bad ? 1 : 0;
    }
    std::vector<orbmi_ba_edge> E;
    std::vector<std::pair<int, int>> e_ref;  // (map point id, keyframe id) per edge
    for (int j = 0; j < (int)lmp.size(); j++)
        for (auto& o : mps[lmp[j]].obs) {
            const int vi = kidx[o.first];
            if (kfs[o.first].bad || vi < 0) continue;
            const KeyFrame& kf = kfs[o.first];
            const orbmi_keypoint& kp = kf.keys[o.second];
            E.push_back(orbmi_ba_edge{j, vi, kp.x, kp.y, kf.ur[o.second], inv_level_sigma2[kp.octave]});
            e_ref.push_back({lmp[j], o.first});
        }
    gt.stop();
    if (E.empty()) return distinctive(owed);
    std::vector<uint8_t> orows;
    std::vector<int32_t> ooff;
    {
        PhaseTimer pt(&phase_ms[PH_LM_OBSROWS]);
        obs_rows(owed, orows, ooff);
    }
    const int nod = (int)owed.size();
    std::vector<int32_t> obest(std::max(nod, 1));
    std::vector<uint8_t> oout((size_t)std::max(nod, 1) * 32);
    auto owed_call = [&]() -> int {
        if (orows.empty()) return ORBMI_OK;
        PhaseTimer pt(&phase_ms[PH_LM_DISTINCTIVE_CALL]);
        return orbmi_compute_distinctive_descriptors(lmm(), orows.data(), ooff.data(), nod, obest.data(), oout.data());
    };
    orbmi_ba_problem prob{(int)K.size(), (int)P.size(), (int)E.size(), K.data(), P.data(), E.data()};
    std::vector<float> tcw(K.size() * 16), pos(P.size() * 3 + 3);
    std::vector<uint8_t> erase(E.size());
    orbmi_ba_result res{};
    res.tcw = tcw.data();
    res.pos = pos.data();
    res.erase = erase.data();
    int rc;
    std::unique_lock<std::mutex> update_guard;  // held to the end of the write-back
    if (held_lock && on_mapping_thread) {  // tracking runs while the GPU solves
        hold_end();
        held_lock->unlock();
        rc = owed_call();
        if (!rc) {
            PhaseTimer ct(&phase_ms[PH_LM_BA_CALL]);
            rc = orbmi_local_bundle_adjustment(ba, &prob, &res, &abort_ba);
        }
        PhaseTimer lt(&phase_ms[PH_LM_LOCK]);
        update_guard = std::unique_lock<std::mutex>(update_mtx);  // (lock order: update, map)
        held_lock->lock();
        log_section(ORBMI_SCHED_L_BA, k);
    } else {
        rc = owed_call();
        PhaseTimer ct(&phase_ms[PH_LM_BA_CALL]);
        if (!rc) rc = orbmi_local_bundle_adjustment(ba, &prob, &res, nullptr);
    }
    SLAM_CHECK(rc);
    for (int j = 0; j < nod; j++)  // the owed descriptors (under the map lock again)
        if (ooff[j + 1] > ooff[j]) std::memcpy(mps[owed[j]].desc, &oout[32 * j], 32);
    PhaseTimer wb(&phase_ms[PH_LM_BA_WRITEBACK]);
    ba_calls++;
    if (res.aborted) ba_aborted++;
    else if (res.stop_check >= 0) ba_interrupted++;
    {
        int erased = 0;
        for (uint8_t x : erase) erased += x != 0;
        if (recording)
            ba_log.push_back(orbmi_slam_ba_record{k, res.stop_check, res.aborted, res.checks,
                                              {res.iterations[0], res.iterations[1]}, (int)E.size(), erased});
    }
    if (res.aborted) return ORBMI_OK;  // src/Optimizer.cc:685-687: no write-back
    for (size_t e = 0; e < E.size(); e++) {
        if (!erase[e]) continue;
        const int m = e_ref[e].first, kk = e_ref[e].second;
        auto it = mps[m].obs.find(kk);
        if (it != mps[m].obs.end() && kfs[kk].mps[it->second] == m) kfs[kk].mps[it->second] = -1;  // EraseMapPointMatch
        erase_observation(m, kk);
    }
    int n_local = 1;
    for (int c : kfs[k].covisible)
        if (!kfs[c].bad) n_local++;
    for (int i = 0; i < n_local; i++) std::memcpy(kfs[all[i]].tcw.data(), &tcw[16 * i], 16 * sizeof(float));
    for (int j = 0; j < (int)lmp.size(); j++) std::memcpy(mps[lmp[j]].pos, &pos[3 * j], 3 * sizeof(float));
    for (int m : lmp) update_normal_and_depth(m);
    return ORBMI_OK;
}
