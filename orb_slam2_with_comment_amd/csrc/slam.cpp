// The native SLAM loop's handle (slam.h): creation, destruction, Tracking::Reset, the C entry
// points (System::TrackStereo / TrackRGBD and the queries) and the trajectory writers.
#include "slam.h"

namespace orbmi {
namespace slam {
thread_local std::unique_lock<std::mutex>* held_lock = nullptr;
thread_local bool on_mapping_thread = false;
}  // namespace slam
}  // namespace orbmi

void orbmi_slam::hold_report() const {
    if (!lock_profile) return;
    for (const auto& kv : hold_ms)
        fprintf(stderr, "map-lock hold after label %d: n %ld  total %.3f ms  mean %.4f ms  max %.4f ms\n", kv.first,
                hold_n.at(kv.first), kv.second.first, kv.second.first / std::max(1L, hold_n.at(kv.first)),
                kv.second.second);
}

void orbmi_slam::request_reset() {
    std::lock_guard<std::mutex> g(q_mtx);
    lm_queue.clear();
    reset_pending = true;
}

// the deferred Tracking::Reset at the start of orbmi_slam_track_stereo (no lock held): the
// mapping thread finishes the keyframe in hand -- a LocalBA included, whose write-back takes
// update_mtx, free now -- then the map is cleared under both locks
int orbmi_slam::deferred_reset() {
    {
        std::unique_lock<std::mutex> g(q_mtx);
        idle_cv.wait(g, [&] { return lm_queue.empty() && !lm_busy; });
        reset_pending = false;
    }
    std::lock_guard<std::mutex> u(update_mtx);
    std::lock_guard<std::mutex> m(map_mtx);
    log_section(ORBMI_SCHED_T_RESET, -1);
    return reset();
}

// Tracking::Reset (src/Tracking.cc:1780-1826): the map, the tracking state, the frame /
// keyframe ids and the trajectory lists start over (the mapping thread is idle: synchronous
// mode, or deferred_reset)
int orbmi_slam::reset() {
    for (auto& kf : kfs)
        if (kf.d_block) (void)hipFree(kf.d_block);
    kfs.clear();
    mps.clear();
    recent_mps.clear();
    local_kfs.clear();
    local_mps.clear();
    kf_counter.assign(kf_counter.size(), 0);
    last_frame = TrackedFrame();
    have_last = false;
    has_velocity = false;
    ref_kf = -1;
    last_kf_frame_id = 0;
    last_reloc_frame_id = 0;
    matches_inliers = 0;
    frame_count = 0;  // Frame::nNextId = 0 (KeyFrame ids restart with the emptied map)
    state = NO_IMAGES_YET;
    rel_poses.clear();
    references.clear();
    frame_times.clear();
    lost.clear();
    return ORBMI_OK;
}

// the poses SaveTrajectory* write: Tcw = Tcr * Trw * Two per recorded frame
std::vector<M4> orbmi_slam::frame_poses() const {
    std::vector<M4> out;
    if (kfs.empty()) return out;
    const M4 Two = pose_inverse(kfs[0].tcw);  // the first keyframe (lowest id)
    for (size_t f = 0; f < rel_poses.size(); f++) {
        M4 Trw = eye4();
        int k = references[f];
        while (kfs[k].bad) {  // a culled reference keyframe: through its parent (Tcp)
            Trw = mul(Trw, kfs[k].tcp);
            k = kfs[k].parent;
        }
        Trw = mul(mul(Trw, kfs[k].tcw), Two);
        out.push_back(mul(rel_poses[f], Trw));
    }
    return out;
}

// CUs LocalMapping's stream leaves to Tracking (ORBMI_LM_RESERVE_CUS overrides)
constexpr int kLmReserveCus = 0;

// r: the RGB-D sensor's settings, NULL for the stereo sensor
static int slam_create(const orbmi_slam_settings* s, const orbmi_rgbd_settings* r, int device,
                       orbmi_vocabulary* vocabulary, orbmi_slam** out) {
    if (!s || !out || s->width <= 0 || s->height <= 0 || s->n_levels < 1 || s->n_levels > 16 || s->fx == 0.f)
        return ORBMI_E_ARG;
    if (r && ((r->ndist != 4 && r->ndist != 5) || s->fy == 0.f || s->height > 65535)) return ORBMI_E_ARG;
    *out = nullptr;
    orbmi_slam* h = new (std::nothrow) orbmi_slam();
    if (!h) return ORBMI_E_ARG;
    h->s = *s;
    h->device = device;
    h->voc = vocabulary;
    h->ucam = orbmi::UndistortCam{s->fx, s->fy, s->cx, s->cy, {0.f, 0.f, 0.f, 0.f, 0.f}};
    if (r) {
        h->rgbd = true;
        h->rs = *r;
        for (int k = 0; k < r->ndist; k++) h->ucam.dist[k] = r->dist[k];
    }
    // a stereo handle's frames are rectified (no distortion): 0, width, 0, height
    orbmi::image_bounds(h->ucam, s->height, s->width, h->bounds);
    int rc = orbmi_extractor_create(device, s->n_features, s->scale_factor, s->n_levels, s->ini_th_fast, s->min_th_fast,
                                    &h->left);
    if (!rc && !r) rc = orbmi_extractor_create(device, s->n_features, s->scale_factor, s->n_levels, s->ini_th_fast,
                                               s->min_th_fast, &h->right);
    if (!rc) {
        void* xs = nullptr;
        rc = orbmi_extractor_get_stream(h->left, &xs);
        h->xstream = (hipStream_t)xs;
    }
    if (!rc) rc = orbmi_matcher_create(device, &h->matcher);
    if (!rc && s->async_local_mapping) rc = orbmi_matcher_create(device, &h->lm_matcher);
    if (!rc && h->lm_matcher) {  // LocalMapping's stream kept off a few CUs (orbmi_matcher_reserve_cus)
        const char* v = getenv("ORBMI_LM_RESERVE_CUS");
        const int n = v ? atoi(v) : kLmReserveCus;
        if (n > 0) rc = orbmi_matcher_reserve_cus(h->lm_matcher, n);
    }
    if (!rc) rc = orbmi_pose_create(device, &h->pose);
    if (!rc) rc = orbmi_ba_create(device, &h->ba);
    // each thread's operators in order on one stream (Tracking: searches + PoseOptimization;
    // LocalMapping: searches + LocalBA), so the streams stay within the hardware queues
    if (!rc) rc = orbmi_pose_share_matcher_stream(h->pose, h->matcher);
    if (!rc) {
        void* ts = nullptr;
        rc = orbmi_matcher_get_stream(h->matcher, &ts);
        h->tstream = (hipStream_t)ts;
    }
    if (!rc) {
        void* st = nullptr;
        rc = orbmi_matcher_get_stream(h->lm_matcher ? h->lm_matcher : h->matcher, &st);
        if (!rc) rc = orbmi_ba_set_stream(h->ba, st);
    }
    if (!rc) {
        h->scale_factors.resize(s->n_levels);
        h->inv_level_sigma2.resize(s->n_levels);
        rc = orbmi_extractor_get_scale_factors(h->left, h->scale_factors.data());
        if (!rc) rc = orbmi_extractor_get_inverse_scale_sigma_squares(h->left, h->inv_level_sigma2.data());
        h->log_scale_factor = s->n_levels > 1 ? (float)std::log((double)h->scale_factors[1]) : 0.f;  // mfLogScaleFactor
        h->level_sigma2.resize(s->n_levels);
        for (int l = 0; l < s->n_levels; l++) h->level_sigma2[l] = h->scale_factors[l] * h->scale_factors[l];
    }
    if (rc) {
        orbmi_slam_destroy(h);
        return rc;
    }
    if (h->async_lm()) h->lm_thread = std::thread([h] { h->lm_run(); });
    *out = h;
    return ORBMI_OK;
}

extern "C" {

int orbmi_slam_create(const orbmi_slam_settings* s, int device, orbmi_vocabulary* vocabulary, orbmi_slam** out) {
    return slam_create(s, nullptr, device, vocabulary, out);
}

int orbmi_slam_create_rgbd(const orbmi_slam_settings* s, const orbmi_rgbd_settings* r, int device,
                           orbmi_vocabulary* vocabulary, orbmi_slam** out) {
    if (!r) return ORBMI_E_ARG;
    return slam_create(s, r, device, vocabulary, out);
}

int orbmi_slam_create_stereo_rectify(const orbmi_slam_settings* s, const orbmi_rectify_camera* left_cam,
                                     const orbmi_rectify_camera* right_cam, int device, orbmi_vocabulary* vocabulary,
                                     orbmi_slam** out) {
    if (!out) return ORBMI_E_ARG;
    *out = nullptr;
    const orbmi_rectify_camera* cams[2] = {left_cam, right_cam};
    for (const orbmi_rectify_camera* c : cams)
        if (!s || !orbmi::rectify::camera_ok(c) || c->cols != s->width || c->rows != s->height ||
            c->rows > orbmi::rectify::kMaxSource || c->cols > orbmi::rectify::kMaxSource)
            return ORBMI_E_ARG;
    orbmi_slam* h = nullptr;
    int rc = slam_create(s, nullptr, device, vocabulary, &h);
    if (rc) return rc;
    // initUndistortRectifyMap of both cameras, once (Examples/Stereo/stereo_euroc.cc:92-93)
    std::vector<float> m1((size_t)s->width * s->height), m2(m1.size());
    if (hipSetDevice(device) != hipSuccess) rc = ORBMI_E_HIP;
    for (int e = 0; e < 2 && !rc; e++) {
        rc = orbmi_init_undistort_rectify_map(cams[e], m1.data(), m2.data());
        if (!rc) rc = h->rect[e].upload(m1.data(), m2.data(), s->height, s->width);
    }
    if (rc) {
        orbmi_slam_destroy(h);
        return rc;
    }
    h->rectify = true;
    *out = h;
    return ORBMI_OK;
}

int orbmi_slam_wait_local_mapping(orbmi_slam* h) {
    if (!h) return ORBMI_E_ARG;
    return h->wait_local_mapping();
}

void orbmi_slam_destroy(orbmi_slam* h) {
    if (!h) return;
    if (h->lm_thread.joinable()) {  // RequestFinish: the queued keyframes are processed first
        {
            std::lock_guard<std::mutex> g(h->q_mtx);
            h->lm_quit = true;
        }
        h->q_cv.notify_all();
        h->lm_thread.join();
    }
    if (h->xstream) (void)hipStreamSynchronize(h->xstream);
    if (h->tstream) (void)hipStreamSynchronize(h->tstream);
    h->hold_report();
    h->free_dev();
    for (orbmi::RectifyTable& t : h->rect) t.release();
    h->free_track_buffers();
    orbmi_ba_destroy(h->ba);
    orbmi_pose_destroy(h->pose);
    orbmi_matcher_destroy(h->matcher);
    if (h->lm_matcher) orbmi_matcher_destroy(h->lm_matcher);
    for (auto& kf : h->kfs)
        if (kf.d_block) (void)hipFree(kf.d_block);
    orbmi_extractor_destroy(h->right);
    orbmi_extractor_destroy(h->left);
    delete h;
}

// Tracking::Track on a constructed frame, under the map locks
static int track_frame(orbmi_slam* h, TrackedFrame& cf, float* tcw_out, int* has_pose) {
    PhaseTimer lock_t(&h->phase_ms[PH_LOCK]);
    std::unique_lock<std::mutex> update_guard(h->update_mtx, std::defer_lock);
    if (h->async_lm()) update_guard.lock();
    std::unique_lock<std::mutex> map_guard(h->map_mtx);
    lock_t.stop();
    h->log_section(ORBMI_SCHED_T_FRAME, cf.id);
    // with the mapping thread running, Tracking's GPU calls release the map lock (their inputs
    // are this thread's copies); the reference's Tracking and LocalMapping likewise interleave
    struct Hold {
        explicit Hold(std::unique_lock<std::mutex>* l) { held_lock = l; }
        ~Hold() { held_lock = nullptr; }
    } hold(h->async_lm() ? &map_guard : nullptr);
    {
        std::lock_guard<std::mutex> g(h->q_mtx);
        if (h->lm_rc) return h->lm_rc;
    }
    const int n = cf.n();
    cf.mps.assign(n, -1);
    cf.outlier.assign(n, 0);
    h->frame_count++;
    SLAM_CHECK(h->track(cf));
    const TrackedFrame& lf = h->last_frame;
    if (has_pose) *has_pose = lf.has_tcw ? 1 : 0;
    if (tcw_out && lf.has_tcw) std::memcpy(tcw_out, lf.tcw.data(), 16 * sizeof(float));
    return ORBMI_OK;
}

static int track_stereo(orbmi_slam* h, const uint8_t* left, const uint8_t* right, int rows, int cols, size_t step,
                        double timestamp, const uint8_t* next_left, const uint8_t* next_right, bool ahead, float* tcw_out,
                        int* has_pose) {
    if (!h || !left || !right || rows <= 0 || cols <= 0 || step < (size_t)cols) return ORBMI_E_ARG;
    if (h->rgbd) return ORBMI_E_STATE;
    // the record tables are the cameras' size: another frame is refused before anything is touched
    if (h->rectify && (rows != h->rect[0].rows || cols != h->rect[0].cols)) return ORBMI_E_ARG;
    if (h->reset_pending) SLAM_CHECK(h->deferred_reset());  // (src/System.cc:139-146)
    TrackedFrame cf;
    cf.id = h->frame_count;
    cf.ts = timestamp;
    // Frame::Frame (stereo, src/Frame.cc:58-100): ORBextractor on both images, ComputeStereoMatches
    // (touches no map state: outside the map lock)
    PhaseTimer total(&h->phase_ms[PH_TOTAL]);
    h->phase_frames++;
    {
        PhaseTimer pt(&h->phase_ms[PH_FRAME]);
        int rc = ahead ? h->frame_stereo_ahead(cf, left, right, rows, cols, step, next_left, next_right)
                       : h->frame_stereo(cf, left, right, rows, cols, step);
        if (rc) {
            if (h->frame_join() != ORBMI_OK) h->drop_ahead();
            return rc;
        }
    }
    const int rc = track_frame(h, cf, tcw_out, has_pose);
    // the next pair's enqueue (frame_post) has finished before the call returns: the caller's
    // images are not read afterwards.  A failed enqueue leaves its slot and the pinned read-back
    // buffers partly written: the pair is dropped, so the next call extracts it again
    const int jrc = h->frame_join();
    if (jrc != ORBMI_OK) h->drop_ahead();
    return rc ? rc : jrc;
}

int orbmi_slam_track_stereo(orbmi_slam* h, const uint8_t* left, const uint8_t* right, int rows, int cols, size_t step,
                            double timestamp, float* tcw_out, int* has_pose) {
    return track_stereo(h, left, right, rows, cols, step, timestamp, nullptr, nullptr, false, tcw_out, has_pose);
}

int orbmi_slam_track_stereo_ahead(orbmi_slam* h, const uint8_t* left, const uint8_t* right, int rows, int cols,
                                  size_t step, double timestamp, const uint8_t* next_left, const uint8_t* next_right,
                                  float* tcw_out, int* has_pose) {
    return track_stereo(h, left, right, rows, cols, step, timestamp, next_left, next_right, true, tcw_out, has_pose);
}

int orbmi_slam_track_rgbd(orbmi_slam* h, const uint8_t* image, int channels, size_t image_step, const void* depth,
                          int depth_type, size_t depth_step, int rows, int cols, double timestamp, float* tcw_out,
                          int* has_pose) {
    if (!h || !image || !depth || rows <= 0 || cols <= 0 || (channels != 1 && channels != 3 && channels != 4) ||
        image_step < (size_t)cols * channels || (depth_type != ORBMI_DEPTH_F32 && depth_type != ORBMI_DEPTH_U16) ||
        depth_step < (size_t)cols * (depth_type == ORBMI_DEPTH_U16 ? 2 : 4) || rows > 65535)
        return ORBMI_E_ARG;
    if (!h->rgbd) return ORBMI_E_STATE;
    if (h->reset_pending) SLAM_CHECK(h->deferred_reset());  // (src/System.cc:190-197)
    TrackedFrame cf;
    cf.id = h->frame_count;
    cf.ts = timestamp;
    PhaseTimer total(&h->phase_ms[PH_TOTAL]);
    h->phase_frames++;
    {
        PhaseTimer pt(&h->phase_ms[PH_FRAME]);
        SLAM_CHECK(h->frame_rgbd(cf, image, channels, image_step, depth, depth_type, depth_step, rows, cols));
    }
    return track_frame(h, cf, tcw_out, has_pose);
}

int orbmi_slam_get_schedule(orbmi_slam* h, orbmi_slam_event* out, int capacity, int* n) {
    if (!h || !n) return ORBMI_E_ARG;
    std::lock_guard<std::mutex> map_guard(h->map_mtx);
    *n = (int)h->sched.size();
    if (capacity < *n) return ORBMI_E_CAP;
    if (*n) std::memcpy(out, h->sched.data(), sizeof(orbmi_slam_event) * (size_t)*n);
    return ORBMI_OK;
}

int orbmi_slam_get_local_mapping_counts(orbmi_slam* h, int* out, int n) {
    if (!h || !out || n < 0) return ORBMI_E_ARG;
    std::lock_guard<std::mutex> map_guard(h->map_mtx);
    const int v[5] = {h->lm_jobs, h->sin_skipped, h->ba_skipped, h->ba_interrupted, h->ba_aborted};
    for (int i = 0; i < n && i < 5; i++) out[i] = v[i];
    return ORBMI_OK;
}

int orbmi_slam_set_recording(orbmi_slam* h, int on) {
    if (!h) return ORBMI_E_ARG;
    std::lock_guard<std::mutex> map_guard(h->map_mtx);
    h->recording = on != 0;
    return ORBMI_OK;
}

int orbmi_slam_get_keyframe_state_log(orbmi_slam* h, orbmi_slam_kf_state* out, int capacity, int* n) {
    if (!h || !n) return ORBMI_E_ARG;
    std::lock_guard<std::mutex> map_guard(h->map_mtx);
    *n = (int)h->kf_state.size();
    if (capacity < *n) return ORBMI_E_CAP;
    if (*n) std::memcpy(out, h->kf_state.data(), sizeof(orbmi_slam_kf_state) * (size_t)*n);
    return ORBMI_OK;
}

int orbmi_slam_get_local_ba_log(orbmi_slam* h, orbmi_slam_ba_record* out, int capacity, int* n) {
    if (!h || !n) return ORBMI_E_ARG;
    std::lock_guard<std::mutex> map_guard(h->map_mtx);
    *n = (int)h->ba_log.size();
    if (capacity < *n) return ORBMI_E_CAP;
    if (*n) std::memcpy(out, h->ba_log.data(), sizeof(orbmi_slam_ba_record) * (size_t)*n);
    return ORBMI_OK;
}

int orbmi_slam_get_stats(orbmi_slam* h, int frame, orbmi_slam_frame_stats* out) {
    if (!h || !out || frame < 0 || frame >= (int)h->stats.size()) return ORBMI_E_ARG;
    std::lock_guard<std::mutex> map_guard(h->map_mtx);
    *out = h->stats[frame];
    return ORBMI_OK;
}

int orbmi_slam_get_counts(orbmi_slam* h, int* frames, int* keyframes, int* mappoints, int* local_ba_calls) {
    if (!h) return ORBMI_E_ARG;
    std::lock_guard<std::mutex> map_guard(h->map_mtx);
    if (frames) *frames = h->frame_count;
    if (keyframes) *keyframes = (int)h->kfs.size();
    if (mappoints) *mappoints = h->count_mappoints();
    if (local_ba_calls) *local_ba_calls = h->ba_calls;
    return ORBMI_OK;
}

int orbmi_slam_get_trajectory(orbmi_slam* h, float* tcw, double* timestamps, uint8_t* lost, int capacity, int* n) {
    if (!h || !n) return ORBMI_E_ARG;
    std::lock_guard<std::mutex> map_guard(h->map_mtx);
    const std::vector<M4> P = h->frame_poses();
    *n = (int)P.size();
    if (capacity < *n) return ORBMI_E_CAP;
    for (int f = 0; f < *n; f++) {
        if (tcw) std::memcpy(tcw + 16 * f, P[f].data(), 16 * sizeof(float));
        if (timestamps) timestamps[f] = h->frame_times[f];
        if (lost) lost[f] = h->lost[f];
    }
    return ORBMI_OK;
}

int orbmi_slam_save_trajectory_kitti(orbmi_slam* h, const char* path) {  // src/System.cc:433-486
    if (!h || !path) return ORBMI_E_ARG;
    std::lock_guard<std::mutex> map_guard(h->map_mtx);
    FILE* f = std::fopen(path, "w");
    if (!f) return ORBMI_E_ARG;
    for (const M4& T : h->frame_poses()) {
        const M4 W = pose_inverse(T);  // Rwc = Rcw^T, twc = -Rwc tcw
        std::fprintf(f, "%.9f %.9f %.9f %.9f %.9f %.9f %.9f %.9f %.9f %.9f %.9f %.9f\n", W[0], W[1], W[2], W[3], W[4],
                     W[5], W[6], W[7], W[8], W[9], W[10], W[11]);
    }
    std::fclose(f);
    return ORBMI_OK;
}

int orbmi_slam_save_trajectory_tum(orbmi_slam* h, const char* path) {  // src/System.cc:334-389
    if (!h || !path) return ORBMI_E_ARG;
    std::lock_guard<std::mutex> map_guard(h->map_mtx);
    FILE* f = std::fopen(path, "w");
    if (!f) return ORBMI_E_ARG;
    const std::vector<M4> P = h->frame_poses();
    for (size_t i = 0; i < P.size(); i++) {
        if (h->lost[i]) continue;
        const M4 W = pose_inverse(P[i]);
        const float R[9] = {W[0], W[1], W[2], W[4], W[5], W[6], W[8], W[9], W[10]};
        float q[4];
        quaternion_xyzw(R, q);
        std::fprintf(f, "%.6f %.9f %.9f %.9f %.9f %.9f %.9f %.9f\n", h->frame_times[i], W[3], W[7], W[11], q[0], q[1],
                     q[2], q[3]);
    }
    std::fclose(f);
    return ORBMI_OK;
}

int orbmi_slam_save_keyframe_trajectory_tum(orbmi_slam* h, const char* path) {  // src/System.cc:392-431
    if (!h || !path) return ORBMI_E_ARG;
    std::lock_guard<std::mutex> map_guard(h->map_mtx);
    FILE* f = std::fopen(path, "w");
    if (!f) return ORBMI_E_ARG;
    for (const KeyFrame& kf : h->kfs) {
        if (kf.bad) continue;
        const M4 W = pose_inverse(kf.tcw);
        const float R[9] = {W[0], W[1], W[2], W[4], W[5], W[6], W[8], W[9], W[10]};
        float q[4];
        quaternion_xyzw(R, q);
        std::fprintf(f, "%.6f %.7f %.7f %.7f %.7f %.7f %.7f %.7f\n", kf.ts, W[3], W[7], W[11], q[0], q[1], q[2], q[3]);
    }
    std::fclose(f);
    return ORBMI_OK;
}

int orbmi_slam_get_phase_ms(orbmi_slam* h, double* ms, int n, long* frames) {
    if (!h || !ms || n < 0) return ORBMI_E_ARG;
    for (int i = 0; i < n && i < PH_COUNT; i++) ms[i] = h->phase_ms[i];
    if (frames) *frames = h->phase_frames;
    return ORBMI_OK;
}

}  // extern "C"
