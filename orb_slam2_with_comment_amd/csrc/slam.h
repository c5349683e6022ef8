// Native stereo SLAM host loop: System::TrackStereo, the stereo Tracking state machine and a
// synchronous LocalMapping around the MI355X operators of this library (include/orbmi.h).
// Internal: declares orbmi_slam once; its definitions are split by role over
//   slam.cpp (handle, reset, C entry points, writers)   slam_frame.cpp (Frame construction)
//   slam_tracking.cpp (Tracking)   slam_mapping.cpp (LocalMapping)   slam_map.h (the map, HIP-free)
//
//   System::TrackStereo        -> orbmi_slam_track_stereo         src/System.cc:110-159   slam.cpp
//   System::TrackRGBD          -> orbmi_slam_track_rgbd           src/System.cc:161-210
//   Frame::Frame (RGB-D)       -> Slam::frame_rgbd                src/Frame.cc:119-171    slam_frame.cpp
//   Tracking::Track (stereo)   -> Slam::track                     src/Tracking.cc:287-581 slam_tracking.cpp
//   StereoInitialization       -> Slam::stereo_initialization     src/Tracking.cc:584-636
//   TrackReferenceKeyFrame     -> Slam::track_reference_kf        src/Tracking.cc:871-917
//   TrackWithMotionModel       -> Slam::track_motion_model        src/Tracking.cc:997-1063
//   TrackLocalMap, UpdateLocalKeyFrames / Points, SearchLocalPoints src/Tracking.cc:1075-1104, 1345-1580
//   NeedNewKeyFrame / CreateNewKeyFrame                           src/Tracking.cc:1140-1330
//   LocalMapping::Run: ProcessNewKeyFrame, MapPointCulling, CreateNewMapPoints,
//     SearchInNeighbors (ORBmatcher::Fuse + replay), LocalBundleAdjustment, KeyFrameCulling
//                                                                 src/LocalMapping.cc:47-841  slam_mapping.cpp;
//     the two cullings in slam_map.h
//   KeyFrame::UpdateConnections, MapPoint bookkeeping             src/KeyFrame.cc, src/MapPoint.cc  slam_map.h (Map::)
//   Optimizer::LocalBundleAdjustment's graph assembly             src/Optimizer.cc:486-683  slam_mapping.cpp
//   System::SaveTrajectoryKITTI / TUM / SaveKeyFrameTrajectoryTUM src/System.cc:334-486   slam.cpp
//
// The same host logic as orb_slam2_with_comment_amd/system.py (which the tests also drive with
// the CPU oracle behind it); this native form is what --mode system measures.  Pose algebra in
// float32 with double accumulation (cv::Mat CV_32F products, src/Converter.cc); the
// deterministic replacements of the reference's pointer-ordered containers are the Python
// module's: keyframe-id order for std::map<KeyFrame*, ...>, covisibility ties to the higher id.
// Compiled with -ffp-contract=off: one rounding per float operation, as numpy does.
#pragma once

#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <deque>
#include <mutex>
#include <new>
#include <thread>

#include <hip/hip_runtime_api.h>

#include "../../include/orbmi_debug.h"
#include "rectifier.h"
#include "rgbd.h"
#include "slam_map.h"
#include "tri_geom.h"

namespace orbmi {
namespace slam {

struct TrackedFrame {
    int id = 0;
    double ts = 0;
    std::vector<orbmi_keypoint> keys;
    std::vector<uint8_t> desc;
    std::vector<float> ur, depth;
    bool has_tcw = false;
    M4 tcw{};
    std::vector<int> mps;        // mvpMapPoints (map point ids, -1)
    std::vector<uint8_t> outlier;
    int ref_kf = -1;
    FeatVec fv;
    int dslot = -1;              // device slot holding keys / desc / u_right (orbmi_slam::Dev)
    int n() const { return (int)keys.size(); }
};

enum { NO_IMAGES_YET = 0, NOT_INITIALIZED = 1, OK = 2, LOST = 3 };

// wall time per phase of orbmi_slam_track_stereo (orbmi_slam_get_phase_ms; names in orbmi_debug.h)
enum Phase { PH_FRAME, PH_LOCK, PH_LF_SEARCH, PH_LF_POSE, PH_LOCAL_UPDATE, PH_LOCAL_RECORDS, PH_FRUSTUM,
             PH_LOCAL_SEARCH, PH_LOCAL_POSE, PH_KEYFRAME, PH_TOTAL,
             // LocalMapping::Run per keyframe (either thread): ProcessNewKeyFrame, MapPointCulling,
             // CreateNewMapPoints, SearchInNeighbors, LocalBundleAdjustment, KeyFrameCulling, all
             PH_LM_PROCESS, PH_LM_CULL, PH_LM_CREATE, PH_LM_FUSE, PH_LM_BA, PH_LM_KFCULL, PH_LM_TOTAL,
             // inside them: the device calls of CreateNewMapPoints, of the Fuse searches, and of
             // ComputeDistinctiveDescriptors (each with its staging and read-back)
             PH_LM_CREATE_CALL, PH_LM_FUSE_CALL, PH_LM_DISTINCTIVE_CALL,
             // the mapping thread's host work, finer: waits to re-take the map lock after a device
             // call; SearchInNeighbors' set-up (targets, records), its per-target check of changed
             // records, its Fuse replays; UpdateNormalAndDepth loops; UpdateConnections; the
             // observation rows of ComputeDistinctiveDescriptors; LocalBA's graph assembly, its
             // device call, its write-back
             PH_LM_LOCK, PH_LM_SIN_PREP, PH_LM_SIN_REDO, PH_LM_SIN_REPLAY, PH_LM_NORMALS, PH_LM_CONNECTIONS,
             PH_LM_OBSROWS, PH_LM_BA_GATHER, PH_LM_BA_CALL, PH_LM_BA_WRITEBACK, PH_COUNT };
struct PhaseTimer {
    double* acc;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    explicit PhaseTimer(double* a) : acc(a) {}
    ~PhaseTimer() { stop(); }
    PhaseTimer(const PhaseTimer&) = delete;
    PhaseTimer& operator=(const PhaseTimer&) = delete;
    void move_to(double* a) {  // the time so far goes to the current accumulator, the rest to `a` (null: nowhere)
        const auto t1 = std::chrono::steady_clock::now();
        if (acc) *acc += std::chrono::duration<double, std::milli>(t1 - t0).count();
        acc = a;
        t0 = t1;
    }
    void stop() { move_to(nullptr); }
};

#define SLAM_CHECK(call)              \
    do {                              \
        const int rc_ = (call);       \
        if (rc_ != ORBMI_OK) return rc_; \
    } while (0)

// this thread's hold on its system's map_mtx when the GPU calls may release it (the mapping
// thread, and the tracking thread with the mapping thread running); null otherwise
extern thread_local std::unique_lock<std::mutex>* held_lock;
extern thread_local bool on_mapping_thread;

}  // namespace slam
}  // namespace orbmi

using namespace orbmi::slam;

struct orbmi_slam : Map {
    orbmi_slam_settings s{};
    // System(..., RGBD): mDistCoef / mDepthMapFactor / mbRGB, the camera as the undistortion takes
    // it, and the device copy of the frame's image and depth map
    bool rgbd = false;
    orbmi_rgbd_settings rs{};
    orbmi::UndistortCam ucam{};
    // orbmi_slam_create_stereo_rectify: TrackStereo takes raw images, frame_enqueue remaps them
    // with the left and right record tables before the extraction
    bool rectify = false;
    orbmi::RectifyTable rect[2];
    // mnMinX, mnMaxX, mnMinY, mnMaxY (Frame::ComputeImageBounds, src/Frame.cc:471-499), computed
    // once at creation as the reference does for its first Frame (mbInitialComputations)
    float bounds[4] = {0.f, 0.f, 0.f, 0.f};
    int device = 0;
    orbmi_extractor* left = nullptr;
    orbmi_extractor* right = nullptr;
    orbmi_matcher* matcher = nullptr;
    orbmi_pose* pose = nullptr;
    orbmi_ba* ba = nullptr;
    orbmi_vocabulary* voc = nullptr;
    std::vector<float> inv_level_sigma2;
    float log_scale_factor = 0;

    int state = NO_IMAGES_YET;
    int frame_count = 0;
    TrackedFrame last_frame;
    bool have_last = false;
    bool has_velocity = false;
    M4 velocity{};
    int ref_kf = -1;
    int last_kf_frame_id = 0, last_reloc_frame_id = 0;
    std::vector<int> local_kfs, local_mps;
    int matches_inliers = 0;
    SeenSet seen;  // mnLastFrameSeen == current frame
    SeenSet local_mark;           // UpdateLocalPoints' mnTrackReferenceForFrame
    SeenSet local_kf_mark;        // UpdateLocalKeyFrames' mnTrackReferenceForFrame
    // LocalBundleAdjustment's mnBALocalForKF / mnBAFixedForKF and its points' marks (the mapping
    // thread's; generation stamps instead of std::set)
    SeenSet ba_local_mark, ba_fixed_mark, ba_mp_mark;
    // the points whose Fuse search record a replay may have changed (fuse_targets' check)
    SeenSet fuse_touched;
    std::vector<int> kf_counter;  // UpdateLocalKeyFrames' keyframe counter (indexed by id)
    // mlRelativeFramePoses, mlpReferences, mlFrameTimes, mlbLost
    std::vector<M4> rel_poses;
    std::vector<int> references;
    std::vector<double> frame_times;
    std::vector<uint8_t> lost;
    std::vector<orbmi_slam_frame_stats> stats;
    int ba_calls = 0;
    // LocalMapping::Run outcomes (orbmi_slam_get_local_mapping_counts): jobs, SearchInNeighbors
    // and LocalBA skipped because a keyframe was queued (src/LocalMapping.cc:79-90), LocalBAs that
    // saw mbAbortBA while optimising / before starting
    int lm_jobs = 0, sin_skipped = 0, ba_skipped = 0, ba_interrupted = 0, ba_aborted = 0;
    int resets = 0;  // Tracking::Reset calls (lost with <= 5 keyframes in the map)
    std::vector<float> level_sigma2;  // mvLevelSigma2
    // Device-resident frames: the image pair goes up once, both images are extracted as one
    // batch with the stereo match behind them on the extractor's stream, and the outputs stay
    // in one of three slots (current frame, last frame, the next frame's extraction running
    // ahead), so the searches and the pose optimisations read the frames in place instead of
    // staging them per call; the host gets its copy of the left outputs with one read-back.
    static constexpr int kSlots = 3;
    struct Dev {
        uint8_t* img = nullptr;  // 2 x rows x cols
        size_t img_bytes = 0;
        uint8_t* h_img = nullptr;  // pinned staging of the pair
        int cap = 0;               // keypoints per item
        orbmi_keypoint* kps[kSlots] = {};
        uint8_t* desc[kSlots] = {};
        int* cnt[kSlots] = {};
        float* ur[kSlots] = {};
        float* dep[kSlots] = {};
        // A slot is chosen per extraction (free_slot): never the current frame's nor the last
        // frame's, which tracking reads on its stream while the next pair is extracted
        // the extraction enqueued ahead (orbmi_slam_track_stereo_ahead) and not yet collected
        struct Ahead { bool on = false; int slot = -1, rows = 0, cols = 0; size_t step = 0; const uint8_t *L = nullptr, *R = nullptr; } ahead;
        // pinned host mirror of a slot's left outputs
        orbmi_keypoint* h_kps = nullptr;
        uint8_t* h_desc = nullptr;
        int* h_cnt = nullptr;
        float* h_ur = nullptr;
        float* h_dep = nullptr;
    } dev;
    hipStream_t xstream = nullptr;  // the left extractor's stream
    // The next pair's Frame-constructor work (image staging, the extraction and stereo launches,
    // the read-back copies: frame_enqueue) runs on a helper thread while the tracking thread
    // tracks the current frame; track_stereo joins it before returning, so the caller's next
    // images are never read after the call.  ORBMI_SLAM_INLINE_FRAME=1: on the tracking thread.
    struct FrameWorker {
        std::thread th;
        std::mutex mtx;
        std::condition_variable cv;
        bool job = false, busy = false, quit = false;
        int rc = ORBMI_OK;
        const uint8_t *L = nullptr, *R = nullptr;
        int rows = 0, cols = 0;
        size_t step = 0;
        int slot = -1;
    } fw;
    const bool inline_frame = getenv("ORBMI_SLAM_INLINE_FRAME") != nullptr;
    void frame_worker_run();
    void frame_post(const uint8_t* L, const uint8_t* R, int rows, int cols, size_t step, int slot);
    int frame_join();
    void frame_worker_stop();
    // Device-resident tracking stages: TrackWithMotionModel (SearchByProjection(CF, LF) with the
    // retry gated on the device count, PoseOptimization on the device-held matches) and
    // TrackLocalMap (SearchLocalPoints, PoseOptimization over both match arrays) are each enqueued
    // on the tracking stream (the matcher's, shared with PoseOptimization) behind one upload of
    // the records the host builds, and read back with one synchronisation.  Host arrays are
    // pinned, so the copies are plain DMA.
    struct TrackBuf {
        size_t cap_kp = 0, cap_lf = 0, cap_rec = 0;
        // One device arena and its pinned host mirror, laid out so that each tracking stage moves
        // its inputs in one upload and its results in one read-back (every copy is a queue
        // packet of several microseconds on the stream):
        //   rec | mlf | occ | lfp | n | pose | out | m | tr
        // TrackWithMotionModel uploads occ .. n (n zeroed: the first search's gate) and reads
        // n .. m; TrackLocalMap uploads rec .. lfp and reads n .. tr.
        uint8_t* d_arena = nullptr;
        uint8_t* h_arena = nullptr;
        size_t arena_bytes = 0;
        // device
        orbmi_lastframe_point* d_lfp = nullptr;  // TWMM: the last frame's points / TLM: the current frame's
        orbmi_mappoint* d_rec = nullptr;         // TLM: the local map points
        orbmi_mappoint_track* d_tr = nullptr;
        int32_t* d_m = nullptr;                  // matches (TWMM: to LF keypoints; TLM: to local map points)
        int32_t* d_mlf = nullptr;                // TLM: keypoint -> its own point record (or -1)
        uint8_t* d_occ = nullptr;
        uint8_t* d_out = nullptr;                // mvbOutlier
        int* d_n = nullptr;                      // match count
        orbmi_pose_frame* d_pose = nullptr;
        // pinned host
        orbmi_lastframe_point* h_lfp = nullptr;
        orbmi_mappoint* h_rec = nullptr;
        orbmi_mappoint_track* h_tr = nullptr;
        int32_t* h_m = nullptr;
        int32_t* h_mlf = nullptr;
        uint8_t* h_occ = nullptr;
        uint8_t* h_out = nullptr;
        int* h_n = nullptr;
        orbmi_pose_frame* h_pose = nullptr;
    } tb;
    hipStream_t tstream = nullptr;  // the tracking stream (the matcher's)
    int track_buffers(size_t nkp, size_t nlf, size_t nrec);
    void free_track_buffers();
    int up_range(const void* from, const void* to);
    int down_range(void* from, const void* to);
    double phase_ms[PH_COUNT] = {};
    long phase_frames = 0;

    // ---- LocalMapping on its own thread (settings.async_local_mapping, src/LocalMapping.cc:47-128)
    // The map and the handles both threads call (matcher, vocabulary) are guarded by map_mtx:
    // Tracking holds it for Track() (the Frame constructor's extraction runs outside it), the
    // mapping thread for a keyframe's LocalMapping::Run except the LocalBundleAdjustment's GPU
    // solve, which -- as the reference's mMutexMapUpdate does (src/Optimizer.cc:776) -- locks
    // only for the graph assembly and the write-back, so tracking proceeds while it runs.
    std::mutex map_mtx;
    // mMutexMapUpdate (include/Map.h:66): Tracking holds it for the whole Track(), including the
    // windows in which it releases map_mtx for its GPU work; LocalBundleAdjustment's write-back of
    // poses and positions takes it first (src/Optimizer.cc:776), so no frame is tracked half
    // against the map before a LocalBA and half against the map after it.  Lock order: update_mtx,
    // then map_mtx.
    std::mutex update_mtx;
    std::mutex q_mtx;
    std::condition_variable q_cv, idle_cv;
    std::deque<int> lm_queue;   // mlNewKeyFrames
    bool lm_busy = false;       // !mbAcceptKeyFrames
    bool lm_quit = false;
    int lm_rc = ORBMI_OK;       // the first error of the mapping thread
    // mbAbortBA: written by the tracking thread (InterruptBA, InsertKeyFrame) and the mapping
    // thread, read by the mapping thread and by LocalBA's stop-flag mirror (orbmi_local_bundle_
    // adjustment reads it with an atomic load): every access is an atomic operation on this word
    int abort_ba = 0;
    // ORBMI_SLAM_NO_INTERRUPT=1 (experiment, tools/concur_breakdown.py): Tracking never raises
    // mbAbortBA, so every LocalBA the mapping thread starts runs to its end
    const bool no_interrupt = getenv("ORBMI_SLAM_NO_INTERRUPT") != nullptr;
    void set_abort_ba(int v) {
        if (v && no_interrupt) return;
        __atomic_store_n(&abort_ba, v, __ATOMIC_RELEASE);
    }
    std::thread lm_thread;
    bool async_lm() const { return s.async_local_mapping != 0; }
    // the schedule (orbmi_slam_get_schedule): every acquisition of map_mtx with the mapping thread
    // running, logged by the thread that took it (so map_mtx guards the log too)
    std::vector<orbmi_slam_event> sched;
    // the schedule, the LocalBA log and the per-keyframe state log are kept only when recording
    // is on (orbmi_slam_set_recording, before the first frame): a replay / test hook, not part of
    // the production path
    bool recording = false;
    void log_section(int label, int arg) {
        if (recording && async_lm()) sched.push_back(orbmi_slam_event{on_mapping_thread ? 1 : 0, label, arg});
        if (lock_profile && on_mapping_thread) { hold_label = label; hold_t0 = std::chrono::steady_clock::now(); }
    }
    // ORBMI_SLAM_LOCK_PROFILE=1 (development aid): how long the mapping thread holds the map lock
    // after each kind of acquisition (by schedule label), printed to stderr at destroy
    const bool lock_profile = getenv("ORBMI_SLAM_LOCK_PROFILE") != nullptr;
    int hold_label = -1;
    std::chrono::steady_clock::time_point hold_t0;
    std::map<int, std::pair<double, double>> hold_ms;  // label -> (sum, max) ms (mapping thread only)
    std::map<int, long> hold_n;
    void hold_end() {  // the mapping thread releases the map lock
        if (!lock_profile || !on_mapping_thread || hold_label < 0) return;
        const double d = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - hold_t0).count();
        auto& e = hold_ms[hold_label];
        e.first += d;
        e.second = std::max(e.second, d);
        hold_n[hold_label]++;
        hold_label = -1;
    }
    std::vector<orbmi_slam_ba_record> ba_log;  // orbmi_slam_get_local_ba_log (under map_mtx)
    // orbmi_slam_get_keyframe_state_log (under map_mtx): the map as LocalMapping left it after each
    // stage of a keyframe's job, so a replay names the first keyframe and stage whose map differs
    std::vector<orbmi_slam_kf_state> kf_state;
    static uint32_t fnv_mix(uint32_t h, uint32_t v) { return (h ^ v) * 16777619u; }
    static constexpr uint32_t kFnv0 = 2166136261u;
    uint32_t slot_hash(int k) const {  // the keyframe's map-point slots (ids, -1 empty)
        uint32_t h = kFnv0;
        for (int m : kfs[k].mps) h = fnv_mix(h, (uint32_t)m);
        return h;
    }
    void log_state(int k, int stage, int a, uint32_t b, uint32_t c) {
        if (!recording) return;
        const int at = async_lm() ? (int)sched.size() - 1 : -1;
        kf_state.push_back(orbmi_slam_kf_state{k, stage, at, a, (int32_t)b, (int32_t)c});
    }
    int fuse_ops = 0;  // map updates made by Fuse replays (Replace that moved observations, AddMapPoint)
    // KeyFrame::ComputeBoW for the mapping thread from the keyframe's HBM descriptors, in two
    // halves so that ProcessNewKeyFrame's ComputeDistinctiveDescriptors call runs while the
    // transform does: bow_begin enqueues the transform (device outputs) and the read-back of the
    // FeatureVector into pinned memory on the vocabulary's stream; bow_end waits and parses.
    struct BowAsync {
        uint8_t* d = nullptr;   // value f64[cap] | word u32[cap] | node u32[cap] | off i32[cap+1] | feat i32[cap] | counts i32[2]
        uint8_t* h = nullptr;   // pinned mirror of node .. counts
        int cap = 0, n = 0;
        hipStream_t stream = nullptr;
        bool pending = false;
    } bowa;
    size_t bow_tail_bytes(int cap) const { return (size_t)(3 * cap + 3) * 4; }
    // LocalMapping's GPU calls: on the mapping thread they use its own matcher and run with the
    // map lock released (their inputs are the caller's copies or the keyframes' HBM copies)
    orbmi_matcher* lm_matcher = nullptr;
    orbmi_matcher* lmm() const { return on_mapping_thread ? lm_matcher : matcher; }
    // `label`, `arg`: where the thread resumes, for the schedule (ORBMI_SCHED_*)
    template <class F>
    int unlocked(int label, int arg, F f) {
        if (!held_lock) return f();
        hold_end();
        held_lock->unlock();
        const int rc = f();
        if (on_mapping_thread) {
            PhaseTimer pt(&phase_ms[PH_LM_LOCK]);
            held_lock->lock();
        } else {
            PhaseTimer pt(&phase_ms[PH_LOCK]);
            held_lock->lock();
        }
        log_section(label, arg);
        return rc;
    }
    // the per-call staged path (ORBMI_SLAM_STAGED=1): every operator call stages its host inputs
    // and synchronises; the default enqueues a stage's operators behind one upload
    const bool staged_track = getenv("ORBMI_SLAM_STAGED") != nullptr;
    // System::Reset with the mapping thread running: LocalMapping::RequestReset drops the queued
    // keyframes (its ResetIfRequested, src/LocalMapping.cc:700-716; the keyframe in hand is
    // finished first) and the rest of Tracking::Reset waits for the next TrackStereo
    bool reset_pending = false;
    // the first device slot that is neither a nor b (kSlots = 3 leaves at least one)
    static int free_slot(int a, int b) {
        for (int k = 0; k < kSlots; k++)
            if (k != a && k != b) return k;
        return -1;
    }

    // ---- slam_frame.cpp ------------------------------------------------------------------------
    orbmi_frame_view view(const std::vector<orbmi_keypoint>& keys, const std::vector<uint8_t>& desc,
                          const std::vector<float>& ur, const float* tcw) const;
    orbmi_frame_view view(const TrackedFrame& f, const float* tcw) const;
    orbmi_frame_view kf_view(const KeyFrame& kf, const float* tcw) const;
    int ensure_slots();
    int image_buffers(size_t bytes);
    int read_back(int k, int counts);
    int frame_enqueue(const uint8_t* L, const uint8_t* R, int rows, int cols, size_t step, int k);
    int frame_collect(TrackedFrame& cf, int slot);
    int frame_stereo(TrackedFrame& cf, const uint8_t* L, const uint8_t* R, int rows, int cols, size_t step);
    int frame_rgbd(TrackedFrame& cf, const uint8_t* image, int channels, size_t image_step, const void* depth,
                   int depth_type, size_t depth_step, int rows, int cols);
    int frame_stereo_ahead(TrackedFrame& cf, const uint8_t* L, const uint8_t* R, int rows, int cols, size_t step,
                           const uint8_t* nL, const uint8_t* nR);
    void drop_ahead();
    void free_dev();
    int compute_bow(const std::vector<uint8_t>& desc, FeatVec& fv);
    int bow_begin(const uint8_t* d_desc, int n);
    int bow_end(FeatVec& fv);
    void free_bow_async();
    int new_keyframe(const TrackedFrame& cf);

    // ---- slam_tracking.cpp ---------------------------------------------------------------------
    int pose_optimization(const TrackedFrame& cf, const std::vector<int32_t>& match,
                          const std::vector<orbmi_lastframe_point>& lfp, M4& tcw_out, std::vector<uint8_t>& out);
    void create_points(int k, TrackedFrame& cf, const std::vector<int>& idx);
    int stereo_initialization(TrackedFrame& cf);
    bool need_new_keyframe(const TrackedFrame& cf, orbmi_slam_frame_stats& st);
    int create_new_keyframe(TrackedFrame& cf);
    void mp_records_into(const std::vector<int>& pts, orbmi_mappoint* rec) const;
    std::vector<orbmi_lastframe_point> lf_records(const std::vector<int>& lf_mps, const std::vector<uint8_t>* outlier) const;
    void lf_records_into(const std::vector<int>& lf_mps, const std::vector<uint8_t>* outlier,
                         orbmi_lastframe_point* rec) const;
    int discard_outliers(TrackedFrame& cf, const std::vector<uint8_t>& outlier);
    int track_reference_kf(TrackedFrame& cf, orbmi_slam_frame_stats& st, bool& ok);
    int track_motion_model(TrackedFrame& cf, orbmi_slam_frame_stats& st, bool& ok);
    int track_motion_model_staged(TrackedFrame& cf, orbmi_slam_frame_stats& st, bool& ok);
    int track_motion_model_dev(TrackedFrame& cf, orbmi_slam_frame_stats& st, bool& ok);
    void motion_model_result(TrackedFrame& cf, int n, const int32_t* m, const float* tcw, const uint8_t* out,
                             orbmi_slam_frame_stats& st, bool& ok);
    void update_local_keyframes(TrackedFrame& cf);
    void update_local_points();
    int track_local_map(TrackedFrame& cf, orbmi_slam_frame_stats& st, bool& ok);
    int track_local_map_staged(TrackedFrame& cf, orbmi_slam_frame_stats& st, bool& ok);
    int track_local_map_dev(TrackedFrame& cf, orbmi_slam_frame_stats& st, bool& ok);
    void mark_own_points(TrackedFrame& cf, uint8_t* occ);
    void local_map_result(TrackedFrame& cf, orbmi_slam_frame_stats& st, bool& ok);
    int track(TrackedFrame& cf);

    // ---- slam_mapping.cpp ----------------------------------------------------------------------
    void normals(const std::vector<int>& pts);
    void connections(int k);
    int distinctive(const std::vector<int>& pts);
    int insert_keyframe(int k);
    bool new_keyframes_queued();
    void lm_run();
    int wait_local_mapping();
    int local_mapping(int k);
    orbmi_tri_keyframe tri_view(const KeyFrame& kf) const;
    int create_pair(int k, int k2, const float ow1[3], float F12[9], bool& use);
    int add_triangulated(int k, int i1, int k2, int i2, const float x3d[3]);
    int create_new_map_points(int k, std::vector<int>& owed);
    int create_new_map_points_host(int k);
    orbmi_mappoint fuse_record(int m) const;
    int fuse_search(int k, const std::vector<int>& pts, std::vector<int32_t>& best);
    void fuse_replay(int k, const std::vector<int>& pts, const int32_t* best, std::set<int>& dirty);
    int fuse(int k, const std::vector<int>& list, std::set<int>& dirty);
    int fuse_targets(const std::vector<int>& targets, const std::vector<int>& list, std::set<int>& dirty,
                     const std::vector<int>& owed);
    int search_in_neighbors(int k, const std::vector<int>& owed, std::vector<int>& owed2);
    int local_bundle_adjustment(int k, const std::vector<int>& owed);

    // ---- slam.cpp ------------------------------------------------------------------------------
    void hold_report() const;
    void request_reset();
    int deferred_reset();
    int reset();
    std::vector<M4> frame_poses() const;
};
