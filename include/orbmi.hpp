// orbmi.hpp — C++ host layer over include/orbmi.h, keeping the reference's class names and call
// shapes (include/ORBextractor.h:45-111, include/ORBmatcher.h:37-102, include/Optimizer.h:62) so a
// Tracking / LocalMapping port reads like the original.  Header-only; link liborbmi.so.
//
// Differences from the reference surface, all at the type level: images are (pointer, rows, cols,
// step) instead of cv::InputArray, keypoints are orbmi::KeyPoint (cv::KeyPoint field order, so
// a std::vector<cv::KeyPoint> can be reinterpreted), descriptors are N x 32 bytes, frames and
// map points cross as the flat views of orbmi.h.  INTEGRATION.md shows the cv::Mat adapter.
// Every call throws orbmi::Error on a non-OK status: there is no CPU fallback.
#ifndef ORBMI_HPP
#define ORBMI_HPP

#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "orbmi.h"

namespace orbmi {

class Error : public std::runtime_error {
public:
    Error(int status, const char* what) : std::runtime_error(std::string(what) + " failed: status " + std::to_string(status)),
                                          status_(status) {}
    int status() const { return status_; }

private:
    int status_;
};

inline void check(int rc, const char* what) {
    if (rc != ORBMI_OK) throw Error(rc, what);
}

using KeyPoint = orbmi_keypoint;
static_assert(sizeof(KeyPoint) == 28, "cv::KeyPoint layout");

// ORB_SLAM2::ORBextractor (include/ORBextractor.h:45-111)
class ORBextractor {
public:
    ORBextractor(int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST, int device = 0)
        : nfeatures_(nfeatures) {
        check(orbmi_extractor_create(device, nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, &h_),
              "orbmi_extractor_create");
    }
    ~ORBextractor() { orbmi_extractor_destroy(h_); }
    ORBextractor(const ORBextractor&) = delete;
    ORBextractor& operator=(const ORBextractor&) = delete;
    ORBextractor(ORBextractor&& o) noexcept : h_(std::exchange(o.h_, nullptr)), nfeatures_(o.nfeatures_) {}

    // ORBextractor::operator()(image, mask, keypoints, descriptors) (src/ORBextractor.cc:1043-1105):
    // u8 gray image, rows x cols, row pitch `step`.  Empty image -> no keypoints; no keypoints ->
    // empty descriptors (descriptors.release()).
    void operator()(const uint8_t* image, int rows, int cols, size_t step, std::vector<KeyPoint>& keypoints,
                    std::vector<uint8_t>& descriptors) {
        keypoints.clear();
        descriptors.clear();
        if (rows == 0 || cols == 0 || !image) return;
        int cap = nfeatures_ + 16 * GetLevels() + 64, n = 0;
        for (;;) {
            keypoints.resize(cap);
            descriptors.resize((size_t)cap * 32);
            const int rc = orbmi_extract(h_, image, rows, cols, step, keypoints.data(), descriptors.data(), cap, &n);
            if (rc == ORBMI_E_CAP) { cap = n; continue; }
            check(rc, "orbmi_extract");
            break;
        }
        keypoints.resize(n);
        descriptors.resize((size_t)n * 32);
    }

    int GetLevels() const { return orbmi_extractor_get_levels(h_); }
    float GetScaleFactor() const { return orbmi_extractor_get_scale_factor(h_); }
    std::vector<float> GetScaleFactors() const { return levels(orbmi_extractor_get_scale_factors); }
    std::vector<float> GetInverseScaleFactors() const { return levels(orbmi_extractor_get_inverse_scale_factors); }
    std::vector<float> GetScaleSigmaSquares() const { return levels(orbmi_extractor_get_scale_sigma_squares); }
    std::vector<float> GetInverseScaleSigmaSquares() const {
        return levels(orbmi_extractor_get_inverse_scale_sigma_squares);
    }

    // mvImagePyramid[level] of the last extraction (read by Frame::ComputeStereoMatches)
    std::vector<uint8_t> ImagePyramid(int level, int rows_max, int cols_max, int* width, int* height,
                                      bool padded = false, int item = 0) const {
        const int cw = cols_max + 64, ch = rows_max + 64;
        std::vector<uint8_t> out((size_t)cw * ch);
        check(orbmi_extractor_get_pyramid_level(h_, item, level, padded, out.data(), cw, width, height),
              "orbmi_extractor_get_pyramid_level");
        std::vector<uint8_t> tight((size_t)*width * *height);
        for (int y = 0; y < *height; y++)
            for (int x = 0; x < *width; x++) tight[(size_t)y * *width + x] = out[(size_t)y * cw + x];
        return tight;
    }

    orbmi_extractor* handle() const { return h_; }

private:
    template <class F>
    std::vector<float> levels(F fn) const {
        std::vector<float> v(GetLevels());
        check(fn(h_, v.data()), "orbmi_extractor_get_*");
        return v;
    }
    orbmi_extractor* h_ = nullptr;
    int nfeatures_;
};

// Frame::ComputeStereoMatches (src/Frame.cc:501-675) on the last extractions of left / right
inline void ComputeStereoMatches(ORBextractor& left, ORBextractor& right, float bf, float fx, int nLeft,
                                 std::vector<float>& mvuRight, std::vector<float>& mvDepth) {
    mvuRight.assign(nLeft, -1.0f);
    mvDepth.assign(nLeft, -1.0f);
    if (nLeft == 0) return;
    check(orbmi_compute_stereo_matches(left.handle(), 0, right.handle(), 0, bf, fx, mvuRight.data(), mvDepth.data(),
                                       nLeft),
          "orbmi_compute_stereo_matches");
}

// ORB_SLAM2::ORBmatcher (include/ORBmatcher.h:37-102).  Results are the reference's side
// effects as index arrays (see orbmi.h for the codes).
class ORBmatcher {
public:
    static const int TH_HIGH = 100, TH_LOW = 50, HISTO_LENGTH = 30;  // src/ORBmatcher.cc:37-39

    explicit ORBmatcher(float nnratio = 0.6f, bool checkOri = true, int device = 0)
        : mfNNratio(nnratio), mbCheckOrientation(checkOri) {
        check(orbmi_matcher_create(device, &h_), "orbmi_matcher_create");
    }
    ~ORBmatcher() { orbmi_matcher_destroy(h_); }
    ORBmatcher(const ORBmatcher&) = delete;
    ORBmatcher& operator=(const ORBmatcher&) = delete;

    // ORBmatcher::DescriptorDistance (src/ORBmatcher.cc:1901-1917): popcount of a ^ b
    static int DescriptorDistance(const uint8_t* a, const uint8_t* b) {
        int d = 0;
        for (int i = 0; i < 32; i += 8) {
            uint64_t x, y;
            __builtin_memcpy(&x, a + i, 8);
            __builtin_memcpy(&y, b + i, 8);
            d += __builtin_popcountll(x ^ y);
        }
        return d;
    }

    // Frame::isInFrustum over all points (src/Frame.cc:274-342)
    void IsInFrustum(const orbmi_frame_view& F, const std::vector<orbmi_mappoint>& mps, float viewingCosLimit,
                     std::vector<orbmi_mappoint_track>& track) {
        track.resize(mps.size());
        check(orbmi_is_in_frustum(h_, &F, mps.data(), (int)mps.size(), viewingCosLimit, track.data()),
              "orbmi_is_in_frustum");
    }

    // SearchByProjection(Frame&, const vector<MapPoint*>&, th) (src/ORBmatcher.cc:59-155)
    int SearchByProjection(const orbmi_frame_view& F, const std::vector<uint8_t>& occupied,
                           const std::vector<orbmi_mappoint>& mps, const std::vector<orbmi_mappoint_track>& track,
                           float th, std::vector<int32_t>& match) {
        match.assign(F.n, -1);
        int n = 0;
        check(orbmi_search_by_projection_local(h_, &F, occupied.data(), mps.data(), track.data(), (int)mps.size(), th,
                                               mfNNratio, match.data(), &n),
              "orbmi_search_by_projection_local");
        return n;
    }

    // Tracking::SearchLocalPoints (src/Tracking.cc:1345-1403): isInFrustum(0.5) + nnratio 0.8
    int SearchLocalPoints(const orbmi_frame_view& F, const std::vector<uint8_t>& occupied,
                          const std::vector<orbmi_mappoint>& mps, float th, std::vector<int32_t>& match,
                          int* nToMatch = nullptr) {
        match.assign(F.n, -1);
        int n = 0;
        check(orbmi_search_local_points(h_, &F, occupied.data(), mps.data(), (int)mps.size(), th, match.data(), &n,
                                        nToMatch),
              "orbmi_search_local_points");
        return n;
    }

    // SearchByProjection(Frame& CF, const Frame& LF, th, bMono) (src/ORBmatcher.cc:1540-1695)
    int SearchByProjection(const orbmi_frame_view& CF, const std::vector<uint8_t>& occupied, const orbmi_frame_view& LF,
                           const std::vector<orbmi_lastframe_point>& lfPoints, float th, bool bMono,
                           std::vector<int32_t>& match) {
        match.assign(CF.n, -1);
        int n = 0;
        check(orbmi_search_by_projection_last_frame(h_, &CF, occupied.data(), &LF, lfPoints.data(), th, bMono,
                                                    mbCheckOrientation, match.data(), &n),
              "orbmi_search_by_projection_last_frame");
        return n;
    }

    // SearchByBoW(KeyFrame*, Frame&, vector<MapPoint*>&) (src/ORBmatcher.cc:211-344)
    int SearchByBoW(const orbmi_frame_view& KF, const std::vector<uint8_t>& kfMapPointOk,
                    const orbmi_feature_vector& kfFeat, const orbmi_frame_view& F, const orbmi_feature_vector& fFeat,
                    std::vector<int32_t>& match) {
        match.assign(F.n, -1);
        int n = 0;
        check(orbmi_search_by_bow(h_, &KF, kfMapPointOk.data(), &kfFeat, &F, &fFeat, mfNNratio, mbCheckOrientation,
                                  match.data(), &n),
              "orbmi_search_by_bow");
        return n;
    }

    // SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12)
    // (src/ORBmatcher.cc:635-768): vpMatches12 as the KF2 keypoint index per KF1 keypoint, -1 none
    int SearchByBoW(const orbmi_frame_view& KF1, const std::vector<uint8_t>& mapPointOk1,
                    const orbmi_feature_vector& fv1, const orbmi_frame_view& KF2,
                    const std::vector<uint8_t>& mapPointOk2, const orbmi_feature_vector& fv2,
                    std::vector<int32_t>& match12) {
        match12.assign(KF1.n > 0 ? KF1.n : 1, -1);
        int n = 0;
        check(orbmi_search_by_bow_kf(h_, &KF1, mapPointOk1.data(), &fv1, &KF2, mapPointOk2.data(), &fv2, mfNNratio,
                                     mbCheckOrientation, match12.data(), &n),
              "orbmi_search_by_bow_kf");
        match12.resize(KF1.n);
        return n;
    }

    // SearchForTriangulation(KeyFrame*, KeyFrame*, cv::Mat F12, vector<pair<size_t,size_t>>&,
    // bool bOnlyStereo) (src/ORBmatcher.cc:783-975): the matched pairs in i1 order
    int SearchForTriangulation(const orbmi_frame_view& KF1, const std::vector<uint8_t>& hasMapPoint1,
                               const orbmi_feature_vector& fv1, const orbmi_frame_view& KF2,
                               const std::vector<uint8_t>& hasMapPoint2, const orbmi_feature_vector& fv2,
                               const float F12[9], std::vector<std::pair<size_t, size_t>>& vMatchedPairs,
                               bool bOnlyStereo) {
        std::vector<int32_t> m12(KF1.n > 0 ? KF1.n : 1, -1);
        int n = 0;
        check(orbmi_search_for_triangulation(h_, &KF1, hasMapPoint1.data(), &fv1, &KF2, hasMapPoint2.data(), &fv2, F12,
                                             bOnlyStereo, mbCheckOrientation, m12.data(), &n),
              "orbmi_search_for_triangulation");
        vMatchedPairs.clear();
        vMatchedPairs.reserve(n);
        for (int i = 0; i < KF1.n; i++)
            if (m12[i] >= 0) vMatchedPairs.emplace_back((size_t)i, (size_t)m12[i]);
        return n;
    }

    // The search of Fuse(KeyFrame*, const vector<MapPoint*>&, th) (src/ORBmatcher.cc:977-1127):
    // bestIdx[i] (-1 = no fusion), bestDist[i]; the caller replays the map updates in list order
    int FuseSearch(const orbmi_frame_view& KF, const std::vector<orbmi_mappoint>& mps,
                   const std::vector<uint8_t>& inKeyFrame, float th, std::vector<int32_t>& bestIdx,
                   std::vector<int32_t>& bestDist) {
        bestIdx.assign(mps.size(), -1);
        bestDist.assign(mps.size(), 256);
        int n = 0;
        check(orbmi_fuse_search(h_, &KF, mps.data(), inKeyFrame.empty() ? nullptr : inKeyFrame.data(), (int)mps.size(),
                                th, bestIdx.data(), bestDist.data(), &n),
              "orbmi_fuse_search");
        return n;
    }

    // The search of Fuse(KeyFrame*, cv::Mat Scw, const vector<MapPoint*>& vpPoints, float th,
    // vector<MapPoint*>& vpReplacePoint) (src/ORBmatcher.cc:1139-1269) for the keyframes of
    // LoopClosing::SearchAndFuse in one call: Scw = KFs.size() x 12 floats (rows 0-2 of each
    // keyframe's [sRcw | t]), inKeyFrame KFs.size() x mps.size() flags or empty; keyframe k's
    // results at bestIdx / bestDist[k * mps.size() ..), its count of bestIdx >= 0 at nFused[k].
    // The caller replays the map updates in list order, keyframe by keyframe
    void FuseSearch(const std::vector<orbmi_frame_view>& KFs, const float* Scw, const std::vector<orbmi_mappoint>& mps,
                    const std::vector<uint8_t>& inKeyFrame, float th, std::vector<int32_t>& bestIdx,
                    std::vector<int32_t>& bestDist, std::vector<int>& nFused) {
        const size_t total = KFs.size() * mps.size();
        if (!inKeyFrame.empty() && inKeyFrame.size() != total) throw Error(ORBMI_E_ARG, "ORBmatcher::FuseSearch(KFs, Scw)");
        bestIdx.assign(total, -1);
        bestDist.assign(total, 256);
        nFused.assign(KFs.size(), 0);
        check(orbmi_fuse_sim3_search_batch(h_, (int)KFs.size(), KFs.data(), Scw, mps.data(),
                                           inKeyFrame.empty() ? nullptr : inKeyFrame.data(), (int)mps.size(), th,
                                           bestIdx.data(), bestDist.data(), nFused.data()),
              "orbmi_fuse_sim3_search_batch");
    }

    // SearchBySim3(KeyFrame*, KeyFrame*, vector<MapPoint*>& vpMatches12, s12, R12, t12, th)
    // (src/ORBmatcher.cc:1285-1525): mps / hasMapPoint one record and flag per keypoint slot,
    // match12 as orbmi.h codes vpMatches12 (-1 none, >= 0 the KF2 slot, -2 a point without an index
    // in KF2), updated with the new matches.  Returns nFound.
    int SearchBySim3(const orbmi_frame_view& KF1, const std::vector<orbmi_mappoint>& mps1,
                     const std::vector<uint8_t>& hasMapPoint1, const orbmi_frame_view& KF2,
                     const std::vector<orbmi_mappoint>& mps2, const std::vector<uint8_t>& hasMapPoint2,
                     std::vector<int32_t>& match12, float s12, const float R12[9], const float t12[3], float th) {
        if ((int)mps1.size() != KF1.n || (int)hasMapPoint1.size() != KF1.n || (int)match12.size() != KF1.n ||
            (int)mps2.size() != KF2.n || (int)hasMapPoint2.size() != KF2.n)
            throw Error(ORBMI_E_ARG, "ORBmatcher::SearchBySim3");
        int n = 0;
        check(orbmi_search_by_sim3(h_, &KF1, mps1.data(), hasMapPoint1.data(), &KF2, mps2.data(), hasMapPoint2.data(), s12,
                                   R12, t12, th, match12.data(), &n, nullptr, nullptr),
              "orbmi_search_by_sim3");
        return n;
    }

    // SearchByProjection(KeyFrame*, cv::Mat Scw, const vector<MapPoint*>& vpPoints,
    // vector<MapPoint*>& vpMatched, int th) (src/ORBmatcher.cc:359-479): Scw = rows 0-2 of
    // [sRcw | t], matched one entry per keypoint slot of KF as orbmi.h codes vpMatched (-1 none,
    // >= 0 the index in mps, -2 a point that is not in mps), updated.  Returns nmatches.
    int SearchByProjection(const orbmi_frame_view& KF, const float Scw[12], const std::vector<orbmi_mappoint>& mps,
                           std::vector<int32_t>& matched, int th) {
        if ((int)matched.size() != KF.n) throw Error(ORBMI_E_ARG, "ORBmatcher::SearchByProjection(KF, Scw)");
        int n = 0;
        check(orbmi_search_by_projection_sim3(h_, &KF, Scw, mps.data(), (int)mps.size(), matched.data(), (float)th, &n),
              "orbmi_search_by_projection_sim3");
        return n;
    }

    // MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:247-316) for a batch of points
    void ComputeDistinctiveDescriptors(const std::vector<uint8_t>& obsDesc, const std::vector<int32_t>& obsOff,
                                       std::vector<int32_t>& best, std::vector<uint8_t>& descOut) {
        const int np = obsOff.empty() ? 0 : (int)obsOff.size() - 1;
        best.assign(np > 0 ? np : 1, -1);
        descOut.resize((size_t)(np > 0 ? np : 1) * 32);
        check(orbmi_compute_distinctive_descriptors(h_, obsDesc.data(), obsOff.data(), np, best.data(), descOut.data()),
              "orbmi_compute_distinctive_descriptors");
    }

    orbmi_matcher* handle() const { return h_; }

private:
    orbmi_matcher* h_ = nullptr;
    float mfNNratio;
    bool mbCheckOrientation;
};

// ORB_SLAM2::ORBVocabulary = DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB>
// (include/ORBVocabulary.h) on the device; transform() = TemplatedVocabulary::transform(
// features, BowVector&, FeatureVector&, levelsup), as Frame/KeyFrame::ComputeBoW call it.
class ORBVocabulary {
public:
    ORBVocabulary(const orbmi_vocabulary_desc& d, int device = 0) {
        check(orbmi_vocabulary_create(device, &d, &h_), "orbmi_vocabulary_create");
    }
    ~ORBVocabulary() { orbmi_vocabulary_destroy(h_); }
    ORBVocabulary(const ORBVocabulary&) = delete;
    ORBVocabulary& operator=(const ORBVocabulary&) = delete;

    struct BowVector { std::vector<uint32_t> word; std::vector<double> value; };
    struct FeatureVector {
        std::vector<uint32_t> node;
        std::vector<int32_t> off, feat;
        orbmi_feature_vector view() const {
            return orbmi_feature_vector{(int)node.size(), node.data(), off.data(), feat.data()};
        }
    };

    void transform(const uint8_t* desc, int n, BowVector& v, FeatureVector& fv, int levelsup) {
        const size_t cap = n > 0 ? (size_t)n : 1;
        v.word.resize(cap); v.value.resize(cap);
        fv.node.resize(cap); fv.off.resize(cap + 1); fv.feat.resize(cap);
        int counts[2] = {0, 0};
        check(orbmi_transform(h_, desc, n, nullptr, levelsup, v.word.data(), v.value.data(), fv.node.data(),
                              fv.off.data(), fv.feat.data(), counts),
              "orbmi_transform");
        v.word.resize(counts[0]); v.value.resize(counts[0]);
        fv.node.resize(counts[1]); fv.off.resize(counts[1] + 1); fv.feat.resize(fv.off.back());
    }

private:
    orbmi_vocabulary* h_ = nullptr;
};

// ORB_SLAM2::KeyFrameDatabase (include/KeyFrameDatabase.h) on the device, by keyframe id
// (pKF->mnId).  store() takes a keyframe's mBowVec once; add / erase are the reference's.  The
// covisibility graph stays the caller's: DetectLoopCandidates takes pKF->GetConnectedKeyFrames()
// as ids and GetBestCovisibilityKeyFrames(10) of every keyframe as a CSR indexed by id.
class KeyFrameDatabase {
public:
    enum ScoringType { L1_NORM = 0, L2_NORM = 1 };
    KeyFrameDatabase(int scoring, int maxKeyFrames, int maxWordsTotal, int device = 0) : cap_(maxKeyFrames) {
        check(orbmi_kfdb_create(device, scoring, maxKeyFrames, maxWordsTotal, &h_), "orbmi_kfdb_create");
    }
    ~KeyFrameDatabase() { orbmi_kfdb_destroy(h_); }
    KeyFrameDatabase(const KeyFrameDatabase&) = delete;
    KeyFrameDatabase& operator=(const KeyFrameDatabase&) = delete;
    orbmi_kfdb* handle() { return h_; }

    void store(int32_t mnId, const ORBVocabulary::BowVector& v) {
        check(orbmi_kfdb_store(h_, mnId, v.word.data(), v.value.data(), (int)v.word.size()), "orbmi_kfdb_store");
    }
    void add(int32_t mnId) { check(orbmi_kfdb_add(h_, mnId), "orbmi_kfdb_add"); }
    void erase(int32_t mnId) { check(orbmi_kfdb_erase(h_, mnId), "orbmi_kfdb_erase"); }
    void clear() { check(orbmi_kfdb_clear(h_), "orbmi_kfdb_clear"); }

    // mpVoc->score(v, mBowVec of each id) (DetectLoop's minScore loop, src/LoopClosing.cc:126-140)
    std::vector<double> score(const ORBVocabulary::BowVector& v, const std::vector<int32_t>& ids) {
        std::vector<double> s(ids.size());
        check(orbmi_kfdb_score(h_, v.word.data(), v.value.data(), (int)v.word.size(), ids.data(), (int)ids.size(),
                               s.data()),
              "orbmi_kfdb_score");
        return s;
    }

    // DetectLoopCandidates(pKF, minScore) (src/KeyFrameDatabase.cc:76-197) -> vpLoopCandidates as ids
    std::vector<int32_t> DetectLoopCandidates(const ORBVocabulary::BowVector& v, float minScore,
                                              const std::vector<int32_t>& connected,
                                              const std::vector<int32_t>& bestCovisOff,
                                              const std::vector<int32_t>& bestCovisIds) {
        std::vector<int32_t> out((size_t)cap_);
        int n = 0;
        check(orbmi_detect_loop_candidates(h_, v.word.data(), v.value.data(), (int)v.word.size(), minScore,
                                           connected.data(), (int)connected.size(), bestCovisOff.data(),
                                           bestCovisIds.data(), bestCovisOff.empty() ? 0 : (int)bestCovisOff.size() - 1,
                                           out.data(), cap_, &n),
              "orbmi_detect_loop_candidates");
        out.resize((size_t)n);
        return out;
    }

private:
    orbmi_kfdb* h_ = nullptr;
    int cap_;
};

// Optimizer::LocalBundleAdjustment (include/Optimizer.h:62) on the assembled local graph
// (src/Optimizer.cc:486-683 gathering; orbmi.h documents the arrays).  The handle keeps the
// device arena between calls; pbStopFlag is LocalMapping's mbAbortBA as an int flag.
class LocalBundleAdjuster {
public:
    struct Result {
        std::vector<float> tcw;       // nkf x 16
        std::vector<float> pos;       // npt x 3
        std::vector<uint8_t> erase;   // nedge
        int iterations[2] = {0, 0};
        double chi2[2] = {0, 0};
        bool aborted = false;
        int stop_check = -1;          // the first pbStopFlag check that found it raised (-1: none)
    };

    explicit LocalBundleAdjuster(int device = 0) { check(orbmi_ba_create(device, &h_), "orbmi_ba_create"); }
    ~LocalBundleAdjuster() { orbmi_ba_destroy(h_); }
    LocalBundleAdjuster(const LocalBundleAdjuster&) = delete;
    LocalBundleAdjuster& operator=(const LocalBundleAdjuster&) = delete;

    Result operator()(const std::vector<orbmi_ba_keyframe>& kfs, const std::vector<orbmi_ba_point>& pts,
                      const std::vector<orbmi_ba_edge>& edges, const volatile int* pbStopFlag = nullptr) {
        Result r;
        r.tcw.assign(kfs.size() * 16, 0.0f);
        r.pos.assign(pts.size() * 3, 0.0f);
        r.erase.assign(edges.size(), 0);
        orbmi_ba_problem p{(int)kfs.size(), (int)pts.size(), (int)edges.size(), kfs.data(), pts.data(), edges.data()};
        orbmi_ba_result out{r.tcw.data(), r.pos.data(), r.erase.data(), {0, 0}, {0, 0}, 0, -1, 0};
        check(orbmi_local_bundle_adjustment(h_, &p, &out, pbStopFlag), "orbmi_local_bundle_adjustment");
        r.iterations[0] = out.iterations[0];
        r.iterations[1] = out.iterations[1];
        r.chi2[0] = out.chi2[0];
        r.chi2[1] = out.chi2[1];
        r.aborted = out.aborted != 0;
        r.stop_check = out.stop_check;
        return r;
    }

    // the deterministic pbStopFlag of orbmi_ba_set_stop_at_check (k < 0: off)
    void SetStopAtCheck(int k) { check(orbmi_ba_set_stop_at_check(h_, k), "orbmi_ba_set_stop_at_check"); }

    orbmi_ba* handle() const { return h_; }

private:
    orbmi_ba* h_ = nullptr;
};

// The graph of Optimizer::BundleAdjustment (src/Optimizer.cc:78-200) over plain vectors, as
// orbmi_bundle_adjustment takes it, and what comes back (orbmi_gba_result).
struct BundleAdjustmentOutput {
    std::vector<float> Tcw;             // nkf x 16
    std::vector<float> pos;             // npt x 3
    std::vector<uint8_t> included;      // npt: !vbNotIncludedMP
    int iterations = 0, status = 0;     // status: ORBMI_GBA_* or'ed
    std::vector<int> trials;            // per iteration
    double chi2Initial = 0, chi2 = 0;
    int stop_check = -1, checks = 0;
};

// ORB_SLAM2::Sim3Solver (include/Sim3Solver.h:37-130, src/Sim3Solver.cc) over the flat arrays the
// reference's constructor builds (:62-103: mvX3Dc1 / mvX3Dc2, mvnMaxError1 / 2, mvnIndices1, mN1,
// mK1 / mK2).  The device computes every hypothesis (orbmi_sim3_ransac_batch); iterate replays the
// reference's best / return rule over them.  Several solvers share one launch through SolveBatch
// (the candidate loop of LoopClosing::ComputeSim3, src/LoopClosing.cc:349-398); a solver that was
// not part of a batch solves itself on its first iterate.  The arrays are copied.
class Sim3Solver {
public:
    Sim3Solver(std::vector<float> x3Dc1, std::vector<float> x3Dc2, std::vector<int32_t> maxError1,
               std::vector<int32_t> maxError2, std::vector<int32_t> indices1, int N1, const float K1[4],
               const float K2[4], bool bFixScale, uint64_t seed = 0)
        : x1_(std::move(x3Dc1)), x2_(std::move(x3Dc2)), e1_(std::move(maxError1)), e2_(std::move(maxError2)),
          idx1_(std::move(indices1)), mN1(N1), N((int)e1_.size()), mbFixScale(bFixScale), seed_(seed) {
        for (int k = 0; k < 4; k++) { k1_[k] = K1[k]; k2_[k] = K2[k]; }
        SetRansacParameters();  // :111
    }

    // :114-138
    void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300) {
        mRansacProb = probability;
        mRansacMinInliers = minInliers;
        maxIterations_ = maxIterations;
        check(orbmi_sim3_iterations(N, minInliers, probability, maxIterations, &mRansacMaxIts), "orbmi_sim3_iterations");
        mnIterations = 0;
        mnBestInliers = 0;
        best_ = -1;
        solved_ = false;
    }

    // Minimal sets to use instead of the library's sampler: mRansacMaxIts x 3 indices
    void SetTriples(std::vector<int32_t> triples) { triples_ = std::move(triples); solved_ = false; }

    // Every hypothesis of the solvers in one launch on the matcher's stream
    static void SolveBatch(ORBmatcher& matcher, const std::vector<Sim3Solver*>& solvers) {
        std::vector<orbmi_sim3_problem> P(solvers.size());
        std::vector<orbmi_sim3_hypotheses> R(solvers.size());
        for (size_t k = 0; k < solvers.size(); k++) {
            Sim3Solver& s = *solvers[k];
            const size_t H = (size_t)(s.mRansacMaxIts > 0 ? s.mRansacMaxIts : 1), words = ((size_t)s.N + 63) / 64;
            s.T12_.assign(12 * H, 0.0f); s.T21_.assign(12 * H, 0.0f); s.s_.assign(H, 0.0f);
            s.count_.assign(H, 0); s.mask_.assign(H * (words ? words : 1), 0);
            if (!s.triples_.empty() && s.triples_.size() < 3 * H) throw Error(ORBMI_E_ARG, "Sim3Solver::SetTriples");
            P[k] = orbmi_sim3_problem{s.N, s.x1_.data(), s.x2_.data(), s.e1_.data(), s.e2_.data(),
                                      {s.k1_[0], s.k1_[1], s.k1_[2], s.k1_[3]}, {s.k2_[0], s.k2_[1], s.k2_[2], s.k2_[3]},
                                      s.mbFixScale, s.mRansacProb, s.mRansacMinInliers, s.maxIterations_,
                                      s.triples_.empty() ? nullptr : s.triples_.data(), s.seed_};
            R[k] = orbmi_sim3_hypotheses{0, s.T12_.data(), s.T21_.data(), s.s_.data(), s.count_.data(), s.mask_.data()};
        }
        check(orbmi_sim3_ransac_batch(matcher.handle(), (int)solvers.size(), P.data(), R.data()), "orbmi_sim3_ransac_batch");
        for (Sim3Solver* s : solvers) s->solved_ = true;
    }

    // cv::Mat iterate(int nIterations, bool& bNoMore, vector<bool>& vbInliers, int& nInliers) (:140-220):
    // true and T12 (16 floats, row-major) when the reference returns a non-empty matrix
    bool iterate(ORBmatcher& matcher, int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers,
                 float T12[16]) {
        bNoMore = false;
        vbInliers.assign(mN1, false);
        nInliers = 0;
        if (N < mRansacMinInliers) {
            bNoMore = true;
            return false;
        }
        if (!solved_) SolveBatch(matcher, {this});
        const size_t words = ((size_t)N + 63) / 64;
        int nCurrentIterations = 0;
        while (mnIterations < mRansacMaxIts && nCurrentIterations < nIterations) {
            nCurrentIterations++;
            const int h = mnIterations++;
            if (count_[h] >= mnBestInliers) {
                mnBestInliers = count_[h];
                best_ = h;
                if (count_[h] > mRansacMinInliers) {
                    nInliers = count_[h];
                    for (int i = 0; i < N; i++)
                        if (mask_[h * words + (i >> 6)] >> (i & 63) & 1) vbInliers[idx1_[i]] = true;
                    for (int j = 0; j < 12; j++) T12[j] = T12_[12 * (size_t)h + j];
                    T12[12] = T12[13] = T12[14] = 0.0f;
                    T12[15] = 1.0f;
                    return true;
                }
            }
        }
        if (mnIterations >= mRansacMaxIts) bNoMore = true;
        return false;
    }

    // :222-226
    bool find(ORBmatcher& matcher, std::vector<bool>& vbInliers12, int& nInliers, float T12[16]) {
        bool bFlag;
        return iterate(matcher, mRansacMaxIts, bFlag, vbInliers12, nInliers, T12);
    }

    // mBestScale, mBestTranslation, mBestRotation (= sR12 / s, one float division per entry) of
    // the best hypothesis so far; valid after an iterate that ran at least one iteration
    float GetEstimatedScale() const { return s_[best_]; }
    void GetEstimatedTranslation(float t[3]) const {
        for (int r = 0; r < 3; r++) t[r] = T12_[12 * (size_t)best_ + 4 * r + 3];
    }
    void GetEstimatedRotation(float R[9]) const {
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) R[3 * r + c] = T12_[12 * (size_t)best_ + 4 * r + c] / s_[best_];
    }
    int GetIterations() const { return mRansacMaxIts; }

private:
    std::vector<float> x1_, x2_;
    std::vector<int32_t> e1_, e2_, idx1_, triples_;
    float k1_[4], k2_[4];
    int mN1, N;
    bool mbFixScale;
    uint64_t seed_;
    double mRansacProb = 0.99;
    int mRansacMinInliers = 6, mRansacMaxIts = 0, maxIterations_ = 300, mnIterations = 0, mnBestInliers = 0, best_ = -1;
    bool solved_ = false;
    std::vector<float> T12_, T21_, s_;
    std::vector<int32_t> count_;
    std::vector<uint64_t> mask_;
};

// Optimizer::OptimizeSim3 (src/Optimizer.cc:1145-1347) over the arrays the reference's assembly
// loop builds (:1198-1281): one problem per (candidate, hypothesis) pair, all of them in one launch
// on the matcher's stream.  OptimizeSim3() takes one; OptimizeSim3Batch() several, the caller
// taking the first in order with nIn >= 20 (src/LoopClosing.cc:399-420).
struct Sim3OptInput {
    std::vector<float> x3Dc1, x3Dc2;        // n x 3: R1w * P3D1w + t1w, R2w * P3D2w + t2w
    std::vector<float> obs1, obs2;          // n x 2: kpUn.pt of either keyframe
    std::vector<float> invSigma2_1, invSigma2_2;  // n: mvInvLevelSigma2[kpUn.octave]
    float K1[4], K2[4];                     // fx fy cx cy
    float th2 = 10.0f;
    bool bFixScale = false;
    float R12[9], t12[3], s12 = 1.0f;       // g2oS12 on entry
};

struct Sim3OptOutput {
    double q[4], t[3], s;                   // g2oS12 on return (q = x y z w)
    float sR[9], tf[3];                     // Converter::toCvMat(g2oS12)
    int nIn = 0, nBad = 0, iterations[2] = {0, 0};
    std::vector<uint8_t> inlier;            // 0 where the reference nulls vpMatches1
};

inline std::vector<Sim3OptOutput> OptimizeSim3Batch(ORBmatcher& matcher, const std::vector<Sim3OptInput>& in) {
    std::vector<orbmi_sim3_opt_problem> P(in.size());
    std::vector<orbmi_sim3_opt_result> R(in.size());
    std::vector<Sim3OptOutput> out(in.size());
    for (size_t k = 0; k < in.size(); k++) {
        const Sim3OptInput& I = in[k];
        const size_t n = I.invSigma2_1.size();
        if (I.x3Dc1.size() != 3 * n || I.x3Dc2.size() != 3 * n || I.obs1.size() != 2 * n || I.obs2.size() != 2 * n ||
            I.invSigma2_2.size() != n)
            throw Error(ORBMI_E_ARG, "OptimizeSim3");
        orbmi_sim3_opt_problem& p = P[k];
        p = orbmi_sim3_opt_problem{};
        p.n = (int32_t)n;
        p.x3d_c1 = I.x3Dc1.data(); p.x3d_c2 = I.x3Dc2.data();
        p.obs1 = I.obs1.data(); p.obs2 = I.obs2.data();
        p.inv_sigma2_1 = I.invSigma2_1.data(); p.inv_sigma2_2 = I.invSigma2_2.data();
        for (int j = 0; j < 4; j++) { p.k1[j] = I.K1[j]; p.k2[j] = I.K2[j]; }
        p.th2 = I.th2;
        p.fix_scale = I.bFixScale;
        for (int j = 0; j < 9; j++) p.R12[j] = I.R12[j];
        for (int j = 0; j < 3; j++) p.t12[j] = I.t12[j];
        p.s12 = I.s12;
        out[k].inlier.assign(n ? n : 1, 0);
        R[k] = orbmi_sim3_opt_result{};
        R[k].inlier = out[k].inlier.data();
    }
    check(orbmi_optimize_sim3_batch(matcher.handle(), (int)in.size(), P.data(), R.data()), "orbmi_optimize_sim3_batch");
    for (size_t k = 0; k < in.size(); k++) {
        Sim3OptOutput& o = out[k];
        for (int j = 0; j < 4; j++) o.q[j] = R[k].q[j];
        for (int j = 0; j < 3; j++) { o.t[j] = R[k].t[j]; o.tf[j] = R[k].t_f[j]; }
        for (int j = 0; j < 9; j++) o.sR[j] = R[k].sR[j];
        o.s = R[k].s;
        o.nIn = R[k].n_in;
        o.nBad = R[k].n_bad;
        o.iterations[0] = R[k].iterations[0];
        o.iterations[1] = R[k].iterations[1];
        o.inlier.resize(in[k].invSigma2_1.size());
    }
    return out;
}

// int Optimizer::OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale): returns nIn
inline int OptimizeSim3(ORBmatcher& matcher, const Sim3OptInput& in, Sim3OptOutput& out) {
    out = OptimizeSim3Batch(matcher, {in})[0];
    return out.nIn;
}

// Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:829-1118) over plain vectors: the pose graph
// as the reference builds it (orbmi_essential_graph_edges gives the edges from the map's arrays).
// A Sim3 is 8 doubles: q (x y z w), t, s.
struct EssentialGraphInput {
    std::vector<double> vertices;       // n x 8: vScw of every live keyframe
    int fixed = 0;                      // index of pLoopKF among them
    std::vector<int32_t> v0, v1;        // per edge: indices into vertices
    std::vector<double> measurements;   // per edge x 8: Sji
    bool bFixScale = true;
    int iterations = 20;
};

struct EssentialGraphOutput {
    std::vector<double> vertices;       // n x 8: the optimised Sim3s
    std::vector<float> Tcw;             // n x 16: [R | t / s], what pKFi->SetPose takes
    double chi2Before = 0, chi2After = 0;
    int iterations = 0, status = 0;     // status: ORBMI_EG_* or'ed
    std::vector<int> trials;            // per iteration
};

struct Optimizer {
    // void Optimizer::OptimizeEssentialGraph(pMap, pLoopKF, pCurKF, NonCorrectedSim3, CorrectedSim3,
    // LoopConnections, bFixScale), from the edge list on: optimize(20) and the SE3 pose recovery
    static EssentialGraphOutput OptimizeEssentialGraph(ORBmatcher& matcher, const EssentialGraphInput& in) {
        const size_t n = in.vertices.size() / 8, ne = in.v0.size();
        if (in.vertices.size() != 8 * n || n == 0 || in.v1.size() != ne || in.measurements.size() != 8 * ne)
            throw Error(ORBMI_E_ARG, "OptimizeEssentialGraph");
        orbmi_essgraph_problem p{};
        p.n_vertices = (int32_t)n;
        p.vertices = in.vertices.data();
        p.fixed = in.fixed;
        p.n_edges = (int32_t)ne;
        p.v0 = in.v0.data();
        p.v1 = in.v1.data();
        p.measurements = in.measurements.data();
        p.fix_scale = in.bFixScale;
        p.iterations = in.iterations;
        EssentialGraphOutput out;
        out.vertices.assign(8 * n, 0.0);
        out.Tcw.assign(16 * n, 0.0f);
        orbmi_essgraph_result r{};
        r.vertices = out.vertices.data();
        check(orbmi_optimize_essential_graph(matcher.handle(), &p, &r), "orbmi_optimize_essential_graph");
        check(orbmi_correct_points_sim3(matcher.handle(), 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr, (int)n,
                                        out.vertices.data(), out.Tcw.data()),
              "orbmi_correct_points_sim3");
        out.chi2Before = r.chi2_before;
        out.chi2After = r.chi2_after;
        out.iterations = r.iterations;
        out.status = r.status;
        out.trials.assign(r.trials, r.trials + r.iterations);
        return out;
    }

    // void Optimizer::BundleAdjustment(vpKFs, vpMP, nIterations, pbStopFlag, nLoopKF, bRobust) on the
    // assembled graph (src/Optimizer.cc:56-255, from the vertices and edges on); the write-back by
    // nLoopKF stays the caller's.  It runs on a LocalBundleAdjuster's handle.
    static BundleAdjustmentOutput BundleAdjustment(LocalBundleAdjuster& ba, const std::vector<orbmi_ba_keyframe>& kfs,
                                                   const std::vector<orbmi_ba_point>& pts, const std::vector<orbmi_ba_edge>& edges,
                                                   int nIterations = 5, const volatile int* pbStopFlag = nullptr,
                                                   bool bRobust = true) {
        BundleAdjustmentOutput out;
        out.Tcw.assign(kfs.size() * 16, 0.0f);
        out.pos.assign(pts.size() * 3, 0.0f);
        out.included.assign(pts.size(), 0);
        orbmi_ba_problem p{(int)kfs.size(), (int)pts.size(), (int)edges.size(), kfs.data(), pts.data(), edges.data()};
        orbmi_gba_result r{};
        r.tcw = out.Tcw.data();
        r.pos = out.pos.data();
        r.included = out.included.data();
        check(orbmi_bundle_adjustment(ba.handle(), &p, nIterations, bRobust ? 1 : 0, &r, pbStopFlag), "orbmi_bundle_adjustment");
        out.iterations = r.iterations;
        out.status = r.status;
        out.trials.assign(r.trials, r.trials + nIterations);
        out.chi2Initial = r.chi2_initial;
        out.chi2 = r.chi2;
        out.stop_check = r.stop_check;
        out.checks = r.checks;
        return out;
    }

    // void Optimizer::GlobalBundleAdjustemnt(pMap, nIterations, pbStopFlag, nLoopKF, bRobust)
    // (src/Optimizer.cc:47-53), the reference's spelling: BundleAdjustment over the whole map
    static BundleAdjustmentOutput GlobalBundleAdjustemnt(LocalBundleAdjuster& ba, const std::vector<orbmi_ba_keyframe>& kfs,
                                                         const std::vector<orbmi_ba_point>& pts,
                                                         const std::vector<orbmi_ba_edge>& edges, int nIterations = 5,
                                                         const volatile int* pbStopFlag = nullptr, bool bRobust = true) {
        return BundleAdjustment(ba, kfs, pts, edges, nIterations, pbStopFlag, bRobust);
    }

    // The map-point loop of CorrectLoop / OptimizeEssentialGraph (src/LoopClosing.cc:607-612,
    // src/Optimizer.cc:1105-1114): points n x 3, ref[i] indexes the two Sim3 tables (m x 8 each)
    static std::vector<float> CorrectPoints(ORBmatcher& matcher, const std::vector<float>& points, const std::vector<int32_t>& ref,
                                            const std::vector<double>& Srw, const std::vector<double>& correctedSwr) {
        const size_t n = ref.size();
        if (points.size() != 3 * n || Srw.size() != correctedSwr.size() || Srw.size() % 8) throw Error(ORBMI_E_ARG, "CorrectPoints");
        std::vector<float> out(3 * n ? 3 * n : 1);
        check(orbmi_correct_points_sim3(matcher.handle(), (int)n, points.data(), ref.data(), (int)(Srw.size() / 8), Srw.data(),
                                        correctedSwr.data(), out.data(), 0, nullptr, nullptr),
              "orbmi_correct_points_sim3");
        out.resize(3 * n);
        return out;
    }
};

// ORB_SLAM2::System for the RGB-D sensor (include/System.h:58-83, src/System.cc:161-210) over the
// native loop (orbmi_slam_create_rgbd / orbmi_slam_track_rgbd).  settings: the Tracking
// constructor's reads (src/Tracking.cc:53-143); rgbd: mDistCoef, mDepthMapFactor (already
// inverted) and mbRGB.  The vocabulary is borrowed.
class System {
public:
    System(const orbmi_slam_settings& settings, const orbmi_rgbd_settings& rgbd, orbmi_vocabulary* vocabulary = nullptr,
           int device = 0) {
        check(orbmi_slam_create_rgbd(&settings, &rgbd, device, vocabulary, &h_), "orbmi_slam_create_rgbd");
    }
    ~System() { orbmi_slam_destroy(h_); }
    System(const System&) = delete;
    System& operator=(const System&) = delete;

    // cv::Mat System::TrackRGBD(const cv::Mat& im, const cv::Mat& depthmap, const double& timestamp):
    // im = u8 with 1, 3 or 4 channels (im.data, im.channels(), im.step), depthmap = CV_32F
    // (ORBMI_DEPTH_F32) or CV_16U (ORBMI_DEPTH_U16) with its step in bytes.  Returns false while
    // not initialised / lost (the reference's empty Tcw); Tcw = 16 floats, row-major.
    bool TrackRGBD(const uint8_t* im, int channels, size_t imStep, const void* depthmap, int depthType, size_t depthStep,
                   int rows, int cols, double timestamp, float* Tcw) {
        int has = 0;
        check(orbmi_slam_track_rgbd(h_, im, channels, imStep, depthmap, depthType, depthStep, rows, cols, timestamp, Tcw,
                                    &has),
              "orbmi_slam_track_rgbd");
        return has != 0;
    }

    void SaveTrajectoryTUM(const std::string& filename) {
        check(orbmi_slam_save_trajectory_tum(h_, filename.c_str()), "orbmi_slam_save_trajectory_tum");
    }
    void SaveKeyFrameTrajectoryTUM(const std::string& filename) {
        check(orbmi_slam_save_keyframe_trajectory_tum(h_, filename.c_str()), "orbmi_slam_save_keyframe_trajectory_tum");
    }

    orbmi_slam* handle() const { return h_; }

private:
    orbmi_slam* h_ = nullptr;
};

// What Examples/Stereo/stereo_euroc.cc:92-93, 122-123 does with cv::initUndistortRectifyMap and
// cv::remap: both cameras' maps built once (left / right = LEFT / RIGHT.K, .D, .R, .P and the size
// from the settings file), then each raw pair remapped in one launch.  Images are 8-bit gray,
// host or device memory; the rectified images have the cameras' sizes.
class StereoRectifier {
public:
    StereoRectifier(const orbmi_rectify_camera& left, const orbmi_rectify_camera& right, int device = 0) {
        try {
            create(left, &l_, device);
            create(right, &r_, device);
        } catch (...) {
            orbmi_rectifier_destroy(l_);
            throw;
        }
    }
    ~StereoRectifier() {
        orbmi_rectifier_destroy(l_);
        orbmi_rectifier_destroy(r_);
    }
    StereoRectifier(const StereoRectifier&) = delete;
    StereoRectifier& operator=(const StereoRectifier&) = delete;

    // cv::remap(imLeft, imLeftRect, M1l, M2l, cv::INTER_LINEAR); cv::remap(imRight, imRightRect, M1r, M2r, ...)
    void operator()(const uint8_t* imLeft, const uint8_t* imRight, int rows, int cols, size_t step, uint8_t* imLeftRect,
                    uint8_t* imRightRect, size_t rectStep, void* stream = nullptr) {
        check(orbmi_remap_pair(l_, r_, imLeft, imRight, rows, cols, step, imLeftRect, imRightRect, rectStep, stream),
              "orbmi_remap_pair");
    }

    orbmi_rectifier* left() const { return l_; }
    orbmi_rectifier* right() const { return r_; }

private:
    static void create(const orbmi_rectify_camera& c, orbmi_rectifier** out, int device) {
        if (c.rows <= 0 || c.cols <= 0) throw Error(ORBMI_E_ARG, "StereoRectifier");
        std::vector<float> m1((size_t)c.rows * c.cols), m2(m1.size());
        check(orbmi_init_undistort_rectify_map(&c, m1.data(), m2.data()), "orbmi_init_undistort_rectify_map");
        check(orbmi_rectifier_create(device, m1.data(), m2.data(), c.rows, c.cols, out), "orbmi_rectifier_create");
    }
    orbmi_rectifier* l_ = nullptr;
    orbmi_rectifier* r_ = nullptr;
};

}  // namespace orbmi

#endif  // ORBMI_HPP
