// The map of the native SLAM loop, free of HIP: the pose helpers, KeyFrame and MapPoint as plain
// records, and struct Map with the bookkeeping of src/KeyFrame.cc and src/MapPoint.cc
// (observations, covisibility graph, spanning tree, SetBadFlag, Replace, UpdateNormalAndDepth)
// and LocalMapping's two cullings.  It reads nothing but kfs, mps, scale_factors and the depth
// threshold it is given, so a host program can drive it (tests/cpp/slam_map_check.cpp, compared
// with system.KeyFrame / system.MapPoint by tests/test_slam_map_cpu.py).  A KeyFrame's device
// pointers are carried here as plain pointers; this header never dereferences or frees them.
// orbmi_slam (slam.h) derives from Map; what logs, locks, times or calls the device stays there.
#pragma once

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <map>
#include <set>
#include <stdexcept>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/orbmi.h"

namespace orbmi {
namespace slam {

using M4 = std::array<float, 16>;

inline M4 eye4() {
    M4 m{};
    m[0] = m[5] = m[10] = m[15] = 1.f;
    return m;
}

// float32(float64(a) @ float64(b)), 4x4 row-major
inline M4 mul(const M4& a, const M4& b) {
    M4 o;
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) {
            double s = 0;
            for (int k = 0; k < 4; k++) s += (double)a[4 * r + k] * (double)b[4 * k + c];
            o[4 * r + c] = (float)s;
        }
    return o;
}

// Frame::UpdatePoseMatrices: Rwc = Rcw^T, Ow = -Rwc tcw; Twc as a 4x4
inline M4 pose_inverse(const M4& T) {
    M4 o = eye4();
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) o[4 * r + c] = T[4 * c + r];
    for (int r = 0; r < 3; r++) {
        double s = 0;
        for (int k = 0; k < 3; k++) s += (double)o[4 * r + k] * (double)T[4 * k + 3];
        o[4 * r + 3] = -(float)s;
    }
    return o;
}

inline void camera_center(const M4& T, float ow[3]) {
    const M4 i = pose_inverse(T);
    ow[0] = i[3]; ow[1] = i[7]; ow[2] = i[11];
}

// Converter::toQuaternion (src/Converter.cc:137-149): Eigen::Quaterniond(Matrix3d) -> x y z w
inline void quaternion_xyzw(const float R[9], float q_out[4]) {
    double m[3][3], q[4] = {0, 0, 0, 0};
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) m[r][c] = R[3 * r + c];
    double t = m[0][0] + m[1][1] + m[2][2];
    if (t > 0) {
        t = std::sqrt(t + 1.0);
        q[3] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (m[2][1] - m[1][2]) * t;
        q[1] = (m[0][2] - m[2][0]) * t;
        q[2] = (m[1][0] - m[0][1]) * t;
    } else {
        int i = m[1][1] > m[0][0] ? 1 : 0;
        if (m[2][2] > m[i][i]) i = 2;
        const int j = (i + 1) % 3, k = (i + 2) % 3;
        t = std::sqrt(m[i][i] - m[j][j] - m[k][k] + 1.0);
        q[i] = 0.5 * t;
        t = 0.5 / t;
        q[3] = (m[k][j] - m[j][k]) * t;
        q[j] = (m[j][i] + m[i][j]) * t;
        q[k] = (m[k][i] + m[i][k]) * t;
    }
    for (int k = 0; k < 4; k++) q_out[k] = (float)q[k];
}

// DBoW2::FeatureVector as CSR (orbmi_feature_vector)
struct FeatVec {
    bool valid = false;
    int words = 0;  // the BowVector's word count (kept for the per-keyframe state record)
    std::vector<uint32_t> node;
    std::vector<int32_t> off, feat;
    orbmi_feature_vector view() const {
        return orbmi_feature_vector{(int)node.size(), node.data(), off.data(), feat.data()};
    }
};

struct KeyFrame {
    int id = 0, frame_id = 0;
    double ts = 0;
    M4 tcw{};
    std::vector<orbmi_keypoint> keys;
    std::vector<uint8_t> desc;
    std::vector<float> ur, depth;
    std::vector<int> mps;        // map point id per keypoint, -1 = NULL
    FeatVec fv;
    std::vector<int> covisible;  // mvpOrderedConnectedKeyFrames
    std::map<int, int> conn;     // mConnectedKeyFrameWeights (keyframe id order)
    int parent = -1;
    std::vector<int> children;   // mspChildrens (iterated in id order)
    bool first_connection = true;
    bool bad = false;
    int fuse_target_for_kf = -1;  // mnFuseTargetForKF
    M4 tcp{};                    // mTcp, set when the keyframe turns bad
    // device copies of keys / desc / u_right (one block): the searches read the keyframe in place
    uint8_t* d_block = nullptr;
    const orbmi_keypoint* d_keys = nullptr;
    const uint8_t* d_desc = nullptr;
    const float* d_ur = nullptr;
    const float* d_depth = nullptr;
    const float* d_cos = nullptr;  // orbmi_stereo_parallax_cos per keypoint (CreateNewMapPoints)
};

// MapPoint::mObservations (keyframe id -> keypoint index, keyframe-id order) as a sorted flat
// vector: a map point has a handful of observations, and the tracking thread walks them for every
// matched point each frame (UpdateLocalKeyFrames), which node-based std::map made pointer chases
struct ObsMap {
    using Entry = std::pair<int, int>;
    std::vector<Entry> v;
    using iterator = std::vector<Entry>::iterator;
    using const_iterator = std::vector<Entry>::const_iterator;
    iterator begin() { return v.begin(); }
    iterator end() { return v.end(); }
    const_iterator begin() const { return v.begin(); }
    const_iterator end() const { return v.end(); }
    size_t size() const { return v.size(); }
    bool empty() const { return v.empty(); }
    void clear() { v.clear(); }
    iterator lower(int k) {
        return std::lower_bound(v.begin(), v.end(), k, [](const Entry& e, int x) { return e.first < x; });
    }
    const_iterator lower(int k) const {
        return std::lower_bound(v.begin(), v.end(), k, [](const Entry& e, int x) { return e.first < x; });
    }
    iterator find(int k) {
        auto it = lower(k);
        return it != v.end() && it->first == k ? it : v.end();
    }
    const_iterator find(int k) const {
        auto it = lower(k);
        return it != v.end() && it->first == k ? it : v.end();
    }
    size_t count(int k) const { return find(k) != v.end() ? 1 : 0; }
    int& operator[](int k) {
        auto it = lower(k);
        if (it == v.end() || it->first != k) it = v.insert(it, Entry{k, 0});
        return it->second;
    }
    const int& at(int k) const {
        auto it = find(k);
        if (it == v.end()) throw std::out_of_range("ObsMap::at");
        return it->second;
    }
    iterator erase(iterator it) { return v.erase(it); }
};

struct MapPoint {
    int id = 0;
    float pos[3] = {0, 0, 0};
    int ref_kf = -1;
    uint8_t desc[32] = {};
    float normal[3] = {0, 0, 0};
    float max_distance = 0, min_distance = 0;
    ObsMap obs;                  // keyframe id -> keypoint index (keyframe id order)
    int nobs = 0;
    bool bad = false;
    int first_kf_id = 0;         // mnFirstKFid
    int visible = 1, found = 1;  // mnVisible, mnFound
    int replaced = -1;           // mpReplaced
    int fuse_candidate_for_kf = -1;
};
// The mapping thread's device calls read keyframes' FeatureVectors through host pointers with the
// map lock released, while Tracking may append to `kfs`: a reallocation must move the elements
// (their heap arrays stay put), never copy and free them.
static_assert(std::is_nothrow_move_constructible<KeyFrame>::value, "kfs growth would copy keyframes");
static_assert(std::is_nothrow_move_constructible<FeatVec>::value, "FeatVec growth would copy");

// mnLastFrameSeen == current frame, as a generation stamp per map point (O(1) insert / test /
// clear instead of a std::set over thousands of points per frame)
struct SeenSet {
    std::vector<int> mark;
    int gen = 1;
    void clear() { gen++; }
    void insert(int m) {
        if (m >= (int)mark.size()) mark.resize(std::max<size_t>(2 * mark.size(), m + 1), 0);
        mark[m] = gen;
    }
    bool count(int m) const { return m < (int)mark.size() && mark[m] == gen; }
};

struct Map {
    std::vector<KeyFrame> kfs;         // index = keyframe id
    std::vector<MapPoint> mps;         // index = map point id
    std::vector<float> scale_factors;  // mvScaleFactors
    std::vector<int> recent_mps;       // mlpRecentAddedMapPoints

    void kf_ow(int k, float ow[3]) const { camera_center(kfs[k].tcw, ow); }

    int tracked_map_points(const KeyFrame& kf, int min_obs) const {  // KeyFrame::TrackedMapPoints
        int n = 0;
        for (int m : kf.mps)
            if (m >= 0 && !mps[m].bad && (min_obs <= 0 || mps[m].nobs >= min_obs)) n++;
        return n;
    }

    int get_weight(int k, int other) const {
        auto it = kfs[k].conn.find(other);
        return it == kfs[k].conn.end() ? 0 : it->second;
    }

    int keyframes_in_map() const {  // Map::KeyFramesInMap
        int n = 0;
        for (auto& k : kfs) n += !k.bad;
        return n;
    }

    int count_mappoints() const {
        int n = 0;
        for (auto& m : mps) n += !m.bad;
        return n;
    }

    // MapPoint::ComputeDistinctiveDescriptors for a batch of points (src/MapPoint.cc:247-316)
    // the observation descriptors of the points (CSR, mObservations order, bad keyframes left out)
    void obs_rows(const std::vector<int>& pts, std::vector<uint8_t>& rows, std::vector<int32_t>& off) const {
        rows.clear();
        off.assign(1, 0);
        for (int m : pts) {
            for (auto& o : mps[m].obs)
                if (!kfs[o.first].bad) rows.insert(rows.end(), &kfs[o.first].desc[32 * o.second], &kfs[o.first].desc[32 * o.second] + 32);
            off.push_back((int32_t)(rows.size() / 32));
        }
    }

    void sort_covisible(KeyFrame& kf) {  // heaviest first, ties to the higher id
        std::vector<std::pair<int, int>> p;
        for (auto& c : kf.conn) p.push_back({c.second, c.first});
        std::sort(p.begin(), p.end(), [](const std::pair<int, int>& a, const std::pair<int, int>& b) {
            return a.first != b.first ? a.first > b.first : a.second > b.second;
        });
        kf.covisible.clear();
        for (auto& x : p) kf.covisible.push_back(x.second);
    }

    void add_connection(int k, int other, int w) {  // KeyFrame::AddConnection + UpdateBestCovisibles
        kfs[k].conn[other] = w;
        sort_covisible(kfs[k]);
    }

    void erase_connection(int k, int other) {  // KeyFrame::EraseConnection + UpdateBestCovisibles
        if (kfs[k].conn.erase(other)) sort_covisible(kfs[k]);
    }

    void change_parent(int k, int p) {
        kfs[k].parent = p;
        auto& ch = kfs[p].children;
        if (std::find(ch.begin(), ch.end(), k) == ch.end()) ch.push_back(k);
    }

    void update_connections(int k) {  // KeyFrame::UpdateConnections (src/KeyFrame.cc:285-371)
        std::map<int, int> counter;
        for (int m : kfs[k].mps) {
            if (m < 0 || mps[m].bad) continue;
            for (auto& o : mps[m].obs)
                if (o.first != k) counter[o.first]++;
        }
        if (counter.empty()) return;
        const int th = 15;
        int nmax = 0, kfmax = -1;
        std::vector<std::pair<int, int>> pairs;  // (w, id)
        for (auto& c : counter) {
            const int w = c.second;
            if (w > nmax) { nmax = w; kfmax = c.first; }
            if (w >= th) {
                pairs.push_back({w, c.first});
                add_connection(c.first, k, w);
            }
        }
        if (pairs.empty()) {
            pairs.push_back({nmax, kfmax});
            add_connection(kfmax, k, nmax);
        }
        std::sort(pairs.begin(), pairs.end(), [](const std::pair<int, int>& a, const std::pair<int, int>& b) {
            return a.first != b.first ? a.first > b.first : a.second > b.second;
        });
        KeyFrame& kf = kfs[k];
        kf.conn = counter;
        kf.covisible.clear();
        for (auto& p : pairs) kf.covisible.push_back(p.second);
        if (kf.first_connection && kf.id != 0) {
            kf.parent = kf.covisible[0];
            kfs[kf.parent].children.push_back(k);
            kf.first_connection = false;
        }
    }

    void add_observation(int m, int k, int idx) {  // MapPoint::AddObservation
        MapPoint& mp = mps[m];
        if (mp.obs.count(k)) return;
        mp.obs[k] = idx;
        mp.nobs += kfs[k].ur[idx] >= 0 ? 2 : 1;
    }

    void erase_observation(int m, int k) {  // MapPoint::EraseObservation
        MapPoint& mp = mps[m];
        auto it = mp.obs.find(k);
        if (it == mp.obs.end()) return;
        const int idx = it->second;
        mp.obs.erase(it);
        mp.nobs -= kfs[k].ur[idx] >= 0 ? 2 : 1;
        if (mp.ref_kf == k && !mp.obs.empty()) mp.ref_kf = mp.obs.begin()->first;  // lowest id
        if (mp.nobs <= 2) set_bad(m);
    }

    void set_bad(int m) {  // MapPoint::SetBadFlag
        MapPoint& mp = mps[m];
        mp.bad = true;
        for (auto& o : mp.obs)
            if (kfs[o.first].mps[o.second] == m) kfs[o.first].mps[o.second] = -1;
        mp.obs.clear();
    }

    // MapPoint::Replace (src/MapPoint.cc:172-215): `other` takes over m's observations; m turns bad.
    // Returns true when other gained them (its descriptor is recomputed before the next search).
    bool replace(int m, int other) {
        if (m == other) return false;
        const ObsMap obs = mps[m].obs;
        mps[m].obs.clear();
        mps[m].bad = true;
        mps[m].replaced = other;
        for (auto& o : obs) {
            if (!mps[other].obs.count(o.first)) {
                kfs[o.first].mps[o.second] = other;  // KeyFrame::ReplaceMapPointMatch
                add_observation(other, o.first, o.second);
            } else {
                kfs[o.first].mps[o.second] = -1;     // KeyFrame::EraseMapPointMatch
            }
        }
        mps[other].found += mps[m].found;
        mps[other].visible += mps[m].visible;
        return true;
    }

    // MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:339-390), float32 arithmetic as
    // system.update_normals_and_depths (observing keyframes in id order)
    void update_normal_and_depth(int m) {
        MapPoint& mp = mps[m];
        if (mp.bad || mp.obs.empty()) return;
        float normal[3] = {0, 0, 0};
        for (auto& o : mp.obs) {
            float ow[3];
            kf_ow(o.first, ow);
            const float v[3] = {mp.pos[0] - ow[0], mp.pos[1] - ow[1], mp.pos[2] - ow[2]};
            const double n2 = ((double)v[0] * v[0] + (double)v[1] * v[1]) + (double)v[2] * v[2];
            const double inv = 1.0 / std::sqrt(n2);
            for (int r = 0; r < 3; r++) normal[r] = normal[r] + (float)((double)v[r] * inv);
        }
        const double ic = 1.0 / (double)mp.obs.size();
        for (int r = 0; r < 3; r++) mp.normal[r] = (float)((double)normal[r] * ic);
        float ow[3];
        kf_ow(mp.ref_kf, ow);
        const float pc[3] = {mp.pos[0] - ow[0], mp.pos[1] - ow[1], mp.pos[2] - ow[2]};
        const float dist = (float)std::sqrt(((double)pc[0] * pc[0] + (double)pc[1] * pc[1]) + (double)pc[2] * pc[2]);
        const KeyFrame& rk = kfs[mp.ref_kf];
        const int level = rk.keys[mp.obs.at(mp.ref_kf)].octave;
        mp.max_distance = dist * scale_factors[level];
        mp.min_distance = mp.max_distance / scale_factors[scale_factors.size() - 1];
    }

    void set_bad_keyframe(int k) {  // KeyFrame::SetBadFlag (src/KeyFrame.cc:467-559)
        if (kfs[k].id == 0) return;
        const std::map<int, int> conn = kfs[k].conn;
        for (auto& c : conn) erase_connection(c.first, k);
        for (int m : std::vector<int>(kfs[k].mps))
            if (m >= 0) erase_observation(m, k);
        kfs[k].conn.clear();
        kfs[k].covisible.clear();
        std::set<int> candidates{kfs[k].parent};
        std::vector<int> children = kfs[k].children;
        std::sort(children.begin(), children.end());
        while (!children.empty()) {
            bool cont = false;
            int best = -1, pc = -1, pp = -1;
            for (int c : children) {
                if (kfs[c].bad) continue;
                for (int cv : kfs[c].covisible)
                    for (int cand : candidates)
                        if (cv == cand) {
                            const int w = get_weight(c, cv);
                            if (w > best) { pc = c; pp = cv; best = w; cont = true; }
                        }
            }
            if (!cont) break;
            change_parent(pc, pp);
            candidates.insert(pc);
            children.erase(std::find(children.begin(), children.end(), pc));
            auto& own = kfs[k].children;
            own.erase(std::find(own.begin(), own.end(), pc));
        }
        const int parent = kfs[k].parent;
        for (int c : children) change_parent(c, parent);
        kfs[k].children.clear();
        auto& pch = kfs[parent].children;
        auto it = std::find(pch.begin(), pch.end(), k);
        if (it != pch.end()) pch.erase(it);
        kfs[k].tcp = mul(kfs[k].tcw, pose_inverse(kfs[parent].tcw));
        kfs[k].bad = true;
    }

    void keyframe_culling(int k, float th_depth) {  // src/LocalMapping.cc:775-841
        const std::vector<int> local = kfs[k].covisible;
        for (int kk : local) {
            const KeyFrame& kf = kfs[kk];
            if (kf.id == 0) continue;
            int n_mps = 0, n_red = 0;
            for (size_t i = 0; i < kf.mps.size(); i++) {
                const int m = kf.mps[i];
                if (m < 0 || mps[m].bad) continue;
                if (kf.depth[i] > th_depth || kf.depth[i] < 0) continue;
                n_mps++;
                if (mps[m].nobs > 3) {
                    const int level = kf.keys[i].octave;
                    int n = 0;
                    for (auto& o : mps[m].obs) {
                        if (o.first == kk) continue;
                        if (kfs[o.first].keys[o.second].octave <= level + 1 && ++n >= 3) break;
                    }
                    if (n >= 3) n_red++;
                }
            }
            if (n_red > 0.9 * n_mps) set_bad_keyframe(kk);
        }
    }

    void map_point_culling(int k) {  // src/LocalMapping.cc:219-263, stereo: nThObs = 3
        std::vector<int> keep;
        for (int m : recent_mps) {
            MapPoint& mp = mps[m];
            if (mp.bad) continue;
            if ((float)mp.found / (float)mp.visible < 0.25f) set_bad(m);  // GetFoundRatio
            else if (k - mp.first_kf_id >= 2 && mp.nobs <= 3) set_bad(m);
            else if (k - mp.first_kf_id >= 3) continue;
            else keep.push_back(m);
        }
        recent_mps = keep;
    }
};

}  // namespace slam
}  // namespace orbmi
