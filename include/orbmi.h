/*
 * orbmi — MI355X-native ORB front-end + local BA for ORB-SLAM2 (C ABI).
 *
 * Drop-in boundary for the hot path of AHzZ123/orb_slam2_with_comment.
 * Plain pointers and sizes only; every entry point cites the reference interface it replaces.
 * Host buffers are owned by the caller (capacity based); each handle owns its device
 * buffers, one HIP stream and the device-resident pyramid of its last extraction.
 * Distinct handles may be used concurrently from different host threads (the reference runs
 * the left and right ORBextractor on two std::threads, src/Frame.cc:78-81); one handle is not
 * re-entrant.  All functions return ORBMI_OK (0) or a negative orbmi_status.
 */
#ifndef ORBMI_H
#define ORBMI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum orbmi_status {
    ORBMI_OK = 0,
    ORBMI_E_ARG = -1,         /* bad argument (null pointer, bad size)            */
    ORBMI_E_HIP = -2,         /* HIP runtime / kernel launch failure              */
    ORBMI_E_CAP = -3,         /* caller capacity too small; *n_out = needed count */
    ORBMI_E_UNSUPPORTED = -4, /* geometry outside what the kernels are sized for  */
    ORBMI_E_STATE = -5        /* call order violated (e.g. stereo before extract) */
} orbmi_status;

/* Field order of cv::KeyPoint (pt.x, pt.y, size, angle, response, octave, class_id). */
typedef struct orbmi_keypoint {
    float x, y, size, angle, response;
    int32_t octave, class_id;
} orbmi_keypoint;

typedef struct orbmi_extractor orbmi_extractor;

/* ---- ORBextractor ------------------------------------------------------------------ */

/* ORBextractor::ORBextractor(int nfeatures, float scaleFactor, int nlevels, int iniThFAST,
 * int minThFAST)  include/ORBextractor.h:58-59, src/ORBextractor.cc:410-470.
 * `device` is the HIP device ordinal the handle's buffers and stream live on. */
int orbmi_extractor_create(int device, int nfeatures, float scale_factor, int nlevels,
                           int ini_th_fast, int min_th_fast, orbmi_extractor** out);
void orbmi_extractor_destroy(orbmi_extractor* h);

/* ORBextractor::operator()(image, mask, keypoints, descriptors)
 * include/ORBextractor.h:64-66, src/ORBextractor.cc:1043-1105.  `image` is host u8 gray,
 * rows x cols with row pitch `step` bytes.  Writes n keypoints (level-major, coordinates at
 * level 0) and n x 32 descriptor bytes.  rows == 0 or cols == 0 -> *n_out = 0 (reference
 * returns on an empty image).  capacity < n -> ORBMI_E_CAP with *n_out = n. */
int orbmi_extract(orbmi_extractor* h, const uint8_t* image, int rows, int cols, size_t step,
                  orbmi_keypoint* kps, uint8_t* desc, int capacity, int* n_out);

/* Batched, device-resident form (config 5 / throughput mode).  Image b is at
 * d_images + b*image_stride (device memory).  Outputs stay on the device: keypoint i of
 * image b at d_kps[b*capacity + i], its descriptor at d_desc + (b*capacity + i)*32, count at
 * d_counts[b] (counts above `capacity` mean truncated output).  Asynchronous: enqueued on
 * the handle's stream; call orbmi_extractor_synchronize() before reading. */
int orbmi_extract_batch_device(orbmi_extractor* h, const uint8_t* d_images, int batch, int rows,
                               int cols, size_t step, size_t image_stride, orbmi_keypoint* d_kps,
                               uint8_t* d_desc, int* d_counts, int capacity);
/* The same with the images in host memory (the reference's operator() takes a host cv::Mat;
 * src/Tracking.cc:168-205 builds the Frame from it): image b at images + b*image_stride, rows
 * contiguous (pitch = cols).  The bytes go to HBM by a copy kernel on the handle's stream that
 * reads pinned memory (hipHostMalloc / hipHostRegister) in place -- asynchronous, the host does
 * not wait; the caller keeps the images unchanged until the stream has passed the call
 * (orbmi_extractor_synchronize, or an event on orbmi_extractor_get_stream).  Pageable memory is
 * first copied into one of two pinned staging buffers of the handle (the host may then wait for
 * the copy kernel two calls back). */
int orbmi_extract_batch_host(orbmi_extractor* h, const uint8_t* images, int batch, int rows, int cols,
                             size_t image_stride, orbmi_keypoint* d_kps, uint8_t* d_desc, int* d_counts, int capacity);
int orbmi_extractor_synchronize(orbmi_extractor* h);
/* The handle's HIP stream (hipStream_t), for callers that order their own work after it. */
int orbmi_extractor_get_stream(orbmi_extractor* h, void** stream);

/* Getters  include/ORBextractor.h:68-90. `out` holds nlevels floats. */
int orbmi_extractor_get_levels(const orbmi_extractor* h);
float orbmi_extractor_get_scale_factor(const orbmi_extractor* h);
int orbmi_extractor_get_scale_factors(const orbmi_extractor* h, float* out);
int orbmi_extractor_get_inverse_scale_factors(const orbmi_extractor* h, float* out);
int orbmi_extractor_get_scale_sigma_squares(const orbmi_extractor* h, float* out);
int orbmi_extractor_get_inverse_scale_sigma_squares(const orbmi_extractor* h, float* out);
int orbmi_extractor_get_features_per_level(const orbmi_extractor* h, int* out);

/* ORBextractor::mvImagePyramid[level] (public, read by Frame::ComputeStereoMatches,
 * src/Frame.cc:508,598,610) of batch item `item` of the last extraction.  padded = 0 copies
 * the W_l x H_l interior, padded = 1 the (W_l+38) x (H_l+38) buffer with its 19-px
 * reflect-101 border.  out_step = destination row pitch; *w, *h receive the copied size. */
int orbmi_extractor_get_pyramid_level(orbmi_extractor* h, int item, int level, int padded,
                                      uint8_t* out, size_t out_step, int* w, int* hgt);

/* ---- Frame::ComputeStereoMatches ----------------------------------------------------- */

/* Frame::ComputeStereoMatches()  src/Frame.cc:501-675 on the device-resident keypoints,
 * descriptors and pyramids of the last extraction of (left, item_left) and
 * (right, item_right); both handles must be on the same device.  bf = Camera.bf, fx =
 * Camera.fx (mb = bf/fx).  Writes mvuRight / mvDepth (-1 = no match) for
 * the n_left left keypoints, in left keypoint order. */
int orbmi_compute_stereo_matches(orbmi_extractor* left, int item_left, orbmi_extractor* right,
                                 int item_right, float bf, float fx, float* u_right,
                                 float* depth, int n_left);

/* Device-resident form: d_u_right / d_depth hold capacity floats per item of the last
 * batch (item-major, same layout as orbmi_extract_batch_device outputs).  Stereo pairs are
 * (left item 2p, right item 2p+1) of ONE handle for p < batch/2.  Asynchronous. */
int orbmi_compute_stereo_matches_batch_device(orbmi_extractor* h, float bf, float fx,
                                              float* d_u_right, float* d_depth);

/* ---- RGB-D Frame: UndistortKeyPoints, ComputeImageBounds, ComputeStereoFromRGBD ----------- */

/* mK and mDistCoef (src/Tracking.cc:60-80): dist = k1 k2 p1 p2 [k3]; ndist = 4 or 5 (4: k3 = 0).
 * Undistortion is cv::undistortPoints(pts, pts, mK, mDistCoef, cv::Mat(), mK) restated (OpenCV
 * 3.x cvUndistortPoints: five fixed iterations in fp64), applied only when
 * dist[0] != 0 as the reference tests only k1 (src/Frame.cc:437, 473). */
typedef struct orbmi_camera {
    float fx, fy, cx, cy;
    float dist[5];
    int ndist;
} orbmi_camera;

#define ORBMI_DEPTH_F32 0          /* CV_32F depth map                                */
#define ORBMI_DEPTH_U16 1          /* CV_16U depth map (TUM: 5000 units per metre)    */

/* Frame::ComputeImageBounds (src/Frame.cc:471-499) for a rows x cols image: out = mnMinX, mnMaxX,
 * mnMinY, mnMaxY.  Host only, no GPU. */
int orbmi_compute_image_bounds(float fx, float fy, float cx, float cy, const float* dist, int ndist, int rows,
                               int cols, float out[4]);

/* Frame::UndistortKeyPoints + Frame::ComputeStereoFromRGBD (src/Frame.cc:434-469, 678-699) on the
 * device-resident keypoints of item `item` of the extractor's last extraction, on its stream.
 * depth: rows x cols depth map (host or device), ORBMI_DEPTH_F32 or ORBMI_DEPTH_U16, row pitch
 * depth_step_bytes; depth_factor = mDepthMapFactor (already inverted, src/Tracking.cc:143-147):
 * d = depth[(int)v][(int)u] * factor in float32 (a float32 map with factor 1 is taken as is).
 * keys_un[i] = the keypoint with pt undistorted (mvKeysUn); d > 0: depth_out[i] = d, u_right[i] =
 * keys_un[i].x - bf / d; otherwise both -1.  n = capacity of the outputs (host or device,
 * detected per call): fewer than the item's keypoints -> ORBMI_E_CAP. */
int orbmi_compute_stereo_from_rgbd(orbmi_extractor* h, int item, const void* depth, int depth_type,
                                   size_t depth_step_bytes, float depth_factor, int rows, int cols,
                                   const orbmi_camera* camera, float bf, orbmi_keypoint* keys_un, float* u_right,
                                   float* depth_out, int n);

/* The same on the caller's n raw keypoints (mvKeys; host or device), without extractor state, on
 * `device`.  A key whose truncated position (int)v, (int)u lies outside rows x cols gets
 * depth -1, u_right -1 and is copied unchanged; nothing is read out of bounds. */
int orbmi_compute_stereo_from_rgbd_keys(int device, const orbmi_keypoint* keys, int n, const void* depth,
                                        int depth_type, size_t depth_step_bytes, float depth_factor, int rows,
                                        int cols, const orbmi_camera* camera, float bf, orbmi_keypoint* keys_un,
                                        float* u_right, float* depth_out);

/* cvtColor(im, gray, CV_RGB2GRAY / CV_BGR2GRAY / CV_RGBA2GRAY / CV_BGRA2GRAY) of
 * Tracking::GrabImageRGBD (src/Tracking.cc:208-224): interleaved u8 with `channels` = 3 or 4
 * (alpha ignored), rgb = Camera.RGB (1: R first, 0: B first); gray = (R*4899 + G*9617 + B*1868 +
 * 8192) >> 14.  image / gray: host or device of `device`, row pitches in bytes. */
int orbmi_cvt_gray(int device, const uint8_t* image, size_t image_step, int channels, int rgb, int rows, int cols,
                   uint8_t* gray, size_t gray_step);

/* ---- Stereo rectification: cv::initUndistortRectifyMap + cv::remap ------------------------ */

/* One camera of a rig that is not factory-rectified, as the settings file gives it
 * (Examples/Stereo/stereo_euroc.cc:55-90: LEFT/RIGHT.K, .D, .R, .P, .height, .width), row-major
 * doubles.  D = k1 k2 p1 p2 [k3 [k4 k5 k6]] with nd = 4, 5 or 8 (thin-prism and tilt terms are
 * not built: any other nd is ORBMI_E_ARG).  rows x cols is the size of the rectified image. */
typedef struct orbmi_rectify_camera {
    double K[9];
    double D[8];
    int nd;
    double R[9];
    double P[12];
    int rows, cols;
} orbmi_rectify_camera;

/* cv::initUndistortRectifyMap(K, D, R, P.rowRange(0,3).colRange(0,3), Size(cols, rows), CV_32F,
 * map1, map2) (stereo_euroc.cc:92-93) restated from OpenCV 3.x's documented algorithm in fp64
 * (DESIGN.md 6r).  map1 / map2: rows x cols host floats, contiguous.  Host only, no GPU. */
int orbmi_init_undistort_rectify_map(const orbmi_rectify_camera* camera, float* map1, float* map2);

typedef struct orbmi_rectifier orbmi_rectifier;

/* The maps of one camera on `device`, converted once into cv::remap's fixed-point form
 * (coordinates rounded half-even to 1/32 pixel; a NaN or a coordinate beyond int32 range reads as
 * outside the source).  map1 / map2: rows x cols host floats, contiguous -- from
 * orbmi_init_undistort_rectify_map or any other source (they are not kept). */
int orbmi_rectifier_create(int device, const float* map1, const float* map2, int rows, int cols,
                           orbmi_rectifier** out);
void orbmi_rectifier_destroy(orbmi_rectifier* h);

/* cv::remap(src, dst, map1, map2, cv::INTER_LINEAR) (stereo_euroc.cc:122-123; BORDER_CONSTANT 0)
 * for 8-bit single-channel images: dst has the maps' size, src its own (at most 32767 in either
 * dimension, ORBMI_E_ARG beyond); pitches in bytes.  src / dst: host or device memory of the
 * handle's device (detected per call).  stream: a hipStream_t of the caller or NULL.  With a
 * stream the inputs are read after the work enqueued on it so far and the stream waits for the
 * outputs, and a call whose pointers are all device memory does not block; with NULL the outputs
 * are complete on return, and device inputs must be complete on entry: the handle's stream is
 * non-blocking and waits for no other stream, the legacy default stream included (synchronise
 * it first, as rectify.py does).  A refused call leaves the handle as it was. */
int orbmi_remap(orbmi_rectifier* h, const uint8_t* src, int src_rows, int src_cols, size_t src_step, uint8_t* dst,
                size_t dst_step, void* stream);
/* Both images of a pair in one launch (on the left handle's stream; both handles on one device).
 * The sources share a size and a pitch, the destinations a pitch; each has its handle's size. */
int orbmi_remap_pair(orbmi_rectifier* left, orbmi_rectifier* right, const uint8_t* src_left, const uint8_t* src_right,
                     int src_rows, int src_cols, size_t src_step, uint8_t* dst_left, uint8_t* dst_right, size_t dst_step,
                     void* stream);

/* ---- ORBmatcher ----------------------------------------------------------------------- */

/* Read-only view of the Frame members the matchers use (include/Frame.h).  Pointers may be
 * host or device memory of the matcher's device (detected per call).  keys_un = mvKeysUn,
 * u_right = mvuRight (NULL for monocular), desc = mDescriptors (n x 32), tcw = mTcw (4x4
 * row-major float, needed by the projection searches and isInFrustum).  A device tcw is read by
 * the kernels when they run (stream order), so it may be the output of an enqueued
 * orbmi_pose_optimization_frame (orbmi_pose_frame.tcw). */
typedef struct orbmi_frame_view {
    int n;
    const orbmi_keypoint* keys_un;
    const float* u_right;
    const uint8_t* desc;
    const float* tcw;
    float fx, fy, cx, cy;          /* Frame::fx, fy, cx, cy                         */
    float bf, mb;                  /* mbf, mb                                       */
    float min_x, max_x, min_y, max_y;      /* mnMinX, mnMaxX, mnMinY, mnMaxY        */
    float grid_w_inv, grid_h_inv;  /* mfGridElementWidthInv, mfGridElementHeightInv */
    int nlevels;
    const float* scale_factors;    /* mvScaleFactors (host or device, nlevels)      */
    float log_scale_factor;        /* mfLogScaleFactor                              */
    const int* n_device;           /* optional device count (e.g. the extractor's count
                                      output): the frame then has min(*n_device, n) keypoints
                                      and n is the capacity of keys_un/u_right/desc      */
} orbmi_frame_view;

/* MapPoint state read by Frame::isInFrustum (src/Frame.cc:274-342). flags: */
#define ORBMI_MP_BAD 1u            /* isBad()                                       */
#define ORBMI_MP_SEEN 2u           /* mnLastFrameSeen == current frame (already matched) */
#define ORBMI_MP_HAS_OBS 4u        /* Observations() > 0                            */
typedef struct orbmi_mappoint {
    float pos[3];                  /* GetWorldPos()                                 */
    float normal[3];               /* GetNormal()                                   */
    float max_distance;            /* mfMaxDistance (invariance = 1.2 x)            */
    float min_distance;            /* mfMinDistance (invariance = 0.8 x)            */
    uint32_t flags;
    uint8_t desc[32];              /* GetDescriptor()                               */
} orbmi_mappoint;

/* Output of isInFrustum: mbTrackInView, mTrackProjX/XR/Y, mnTrackScaleLevel, mTrackViewCos. */
typedef struct orbmi_mappoint_track {
    int32_t in_view;
    float proj_x, proj_xr, proj_y;
    int32_t level;
    float view_cos;
} orbmi_mappoint_track;

typedef struct orbmi_matcher orbmi_matcher;

/* ORBmatcher(float nnratio, bool checkOri) is stateless in the reference (include/ORBmatcher.h:
 * 40); the handle holds a device, a stream and scratch buffers. */
int orbmi_matcher_create(int device, orbmi_matcher** out);
void orbmi_matcher_destroy(orbmi_matcher* m);
/* Run the matcher on `ex`'s stream (the frame's keypoints/descriptors come from that
 * extraction): calls are then ordered behind it without host synchronisation, and a call whose
 * outputs are all device pointers with nmatches == NULL returns without waiting. */
int orbmi_matcher_share_stream(orbmi_matcher* m, orbmi_extractor* ex);
/* The handle's HIP stream (hipStream_t): its own, or the extractor's after share_stream. */
int orbmi_matcher_get_stream(orbmi_matcher* m, void** stream);
/* Keep the handle's own stream off `n` compute units (hipExtStreamCreateWithCUMask; the last n
 * bits of the device's CU mask cleared), so that work on other streams -- Tracking's one-
 * workgroup searches and PoseOptimization -- always finds free CUs beside a LocalMapping chain
 * (LocalBA, Fuse) that fills the device.  Call before the stream is shared or queried; n = 0
 * restores an unmasked stream.  ORBMI_E_STATE on a shared stream. */
int orbmi_matcher_reserve_cus(orbmi_matcher* m, int n);
/* Frame::AssignFeaturesToGrid (src/Frame.cc:232-247), run once per Frame as the Frame
 * constructor does (src/Frame.cc:98): builds the keypoint grid of F (device-resident keypoints
 * only, else ORBMI_E_ARG) on the handle's stream and pins it, so the searches on the same frame
 * (same keys / n / n_device / image bounds) skip their rebuild.  The pin ends with
 * orbmi_matcher_release_grid or when a search on another frame builds its grid; the caller
 * re-pins whenever the keypoints behind the pointers change (a new frame in the same buffers). */
int orbmi_matcher_assign_features_to_grid(orbmi_matcher* m, const orbmi_frame_view* F);
int orbmi_matcher_release_grid(orbmi_matcher* m);
/* The same grid built ahead, on another stream: Frame::AssignFeaturesToGrid of F (device arrays
 * only) into the handle's slot grid `slot` (0..3) on `stream` (hipStream_t; NULL = the handle's),
 * e.g. the extraction stream right after the Frame's keypoints, so the build leaves the tracking
 * chain.  The caller orders the searches that read the slot behind `stream` (an event), and the
 * next build of the slot behind those searches.  orbmi_matcher_pin_grid_slot then makes the
 * searches on F read that grid, pinned as above; ORBMI_E_STATE if the slot was built for another
 * frame (keys / n / n_device / image bounds). */
int orbmi_matcher_build_grid_slot(orbmi_matcher* m, const orbmi_frame_view* F, int slot, void* stream);
int orbmi_matcher_pin_grid_slot(orbmi_matcher* m, const orbmi_frame_view* F, int slot);

/* Frame::isInFrustum(pMP, viewingCosLimit) for n_mp points (src/Frame.cc:274-342) with
 * MapPoint::PredictScale (src/MapPoint.cc:421-436).  Points flagged BAD or SEEN are skipped
 * (in_view = 0) as in Tracking::SearchLocalPoints (src/Tracking.cc:1375-1379).  track: n_mp. */
int orbmi_is_in_frustum(orbmi_matcher* m, const orbmi_frame_view* F, const orbmi_mappoint* mps, int n_mp,
                        float viewing_cos_limit, orbmi_mappoint_track* track);

/* ORBmatcher::SearchByProjection(Frame& F, const vector<MapPoint*>& vpMapPoints, float th)
 * (src/ORBmatcher.cc:59-155), greedy in point order.  occupied[i] = F.mvpMapPoints[i] &&
 * Observations() > 0 on entry.  match_mp[i] (n entries) = index of the point newly assigned
 * to keypoint i, -1 otherwise.  Returns the count in *nmatches. */
int orbmi_search_by_projection_local(orbmi_matcher* m, const orbmi_frame_view* F, const uint8_t* occupied,
                                     const orbmi_mappoint* mps, const orbmi_mappoint_track* track, int n_mp,
                                     float th, float nnratio, int32_t* match_mp, int* nmatches);

/* Tracking::SearchLocalPoints (src/Tracking.cc:1345-1403) fused: isInFrustum(0.5) on every
 * point, then SearchByProjection(F, points, th) with nnratio 0.8.  *n_to_match = nToMatch. */
int orbmi_search_local_points(orbmi_matcher* m, const orbmi_frame_view* F, const uint8_t* occupied,
                              const orbmi_mappoint* mps, int n_mp, float th, int32_t* match_mp,
                              int* nmatches, int* n_to_match);
/* The same, also returning every point's isInFrustum outputs (mbTrackInView etc., n_mp entries;
 * host or device): the caller's IncreaseVisible for the points in view needs no second call. */
int orbmi_search_local_points_track(orbmi_matcher* m, const orbmi_frame_view* F, const uint8_t* occupied,
                                    const orbmi_mappoint* mps, int n_mp, float th, int32_t* match_mp,
                                    int* nmatches, int* n_to_match, orbmi_mappoint_track* track_out);

/* Last-frame map point view for SearchByProjection(CF, LF): one entry per LF keypoint. */
#define ORBMI_LF_HAS_MP 1u         /* LastFrame.mvpMapPoints[i] != NULL             */
#define ORBMI_LF_OUTLIER 2u        /* LastFrame.mvbOutlier[i]                       */
typedef struct orbmi_lastframe_point {
    float pos[3];                  /* pMP->GetWorldPos()                            */
    uint32_t flags;                /* ORBMI_LF_* | ORBMI_MP_HAS_OBS                 */
    uint8_t desc[32];              /* pMP->GetDescriptor()                          */
} orbmi_lastframe_point;

/* ORBmatcher::SearchByProjection(Frame& CF, const Frame& LF, float th, bool bMono)
 * (src/ORBmatcher.cc:1540-1695) incl. the rotation-consistency histogram when check_ori.
 * LF provides keys_un (octave = mvKeys[i].octave, angle = mvKeysUn[i].angle) and tcw.
 * match_lf[i] (CF.n entries) = LF keypoint index newly assigned to CF keypoint i, else -1. */
int orbmi_search_by_projection_last_frame(orbmi_matcher* m, const orbmi_frame_view* CF, const uint8_t* occupied,
                                          const orbmi_frame_view* LF, const orbmi_lastframe_point* lf_points,
                                          float th, int mono, int check_ori, int32_t* match_lf, int* nmatches);

/* DBoW2::FeatureVector as CSR: node ids ascending, feature indices of node k at
 * feat[off[k] .. off[k+1]) in insertion order (Thirdparty/DBoW2/DBoW2/FeatureVector.h:21-22). */
typedef struct orbmi_feature_vector {
    int nnodes;
    const uint32_t* node_id;
    const int32_t* off;            /* nnodes + 1 */
    const int32_t* feat;
} orbmi_feature_vector;

/* ORBmatcher::SearchByBoW(KeyFrame* pKF, Frame& F, vector<MapPoint*>& matches)
 * (src/ORBmatcher.cc:211-344).  kf_mp_ok[j] = pKF->GetMapPointMatches()[j] && !isBad().
 * KF keys_un supply angles (mvKeysUn), F keys_un supply angles of F.mvKeys.  match_kf[i]
 * (F.n entries) = KF keypoint index whose map point is assigned to F keypoint i, else -1. */
int orbmi_search_by_bow(orbmi_matcher* m, const orbmi_frame_view* KF, const uint8_t* kf_mp_ok,
                        const orbmi_feature_vector* kf_fv, const orbmi_frame_view* F,
                        const orbmi_feature_vector* f_fv, float nnratio, int check_ori, int32_t* match_kf,
                        int* nmatches);

/* ORBmatcher::SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12)
 * (src/ORBmatcher.cc:635-768), the form LoopClosing::ComputeSim3 calls (src/LoopClosing.cc:330).
 * ok1[j] / ok2[j] = the keyframe's GetMapPointMatches()[j] && !isBad() (both sides need a live
 * point, :671-675 and :687-693); fv1 / fv2 = the keyframes' mFeatVec; keys_un supply mvKeysUn's
 * angles.  Unlike the (KeyFrame, Frame) form a match needs bestDist1 < TH_LOW strictly (:711), and
 * the result is indexed by KF1's keypoint: match12[i1] (KF1.n entries, at least one) = the KF2
 * keypoint whose map point vpMatches12[i1] is, else -1.  This is the bow_matches row
 * compute_sim3 takes.  *nmatches = the return value.  n_device views are not accepted. */
int orbmi_search_by_bow_kf(orbmi_matcher* m, const orbmi_frame_view* KF1, const uint8_t* ok1,
                           const orbmi_feature_vector* fv1, const orbmi_frame_view* KF2, const uint8_t* ok2,
                           const orbmi_feature_vector* fv2, float nnratio, int check_ori, int32_t* match12,
                           int* nmatches);

/* ORBmatcher::SearchForTriangulation(KeyFrame* pKF1, KeyFrame* pKF2, cv::Mat F12,
 * vector<pair<size_t,size_t>>& vMatchedPairs, bool bOnlyStereo) (src/ORBmatcher.cc:783-975)
 * with CheckDistEpipolarLine (:173-196): KF1 / KF2 views need keys_un, u_right, desc, tcw, the
 * intrinsics and scale factors (mvLevelSigma2 = scale^2); has_mp[i] = pKF->GetMapPoint(i) !=
 * NULL; fv = the keyframes' mFeatVec; F12 = LocalMapping::ComputeF12 (3x3 row-major float, host
 * or device).  match12[i1] (KF1.n entries) = the KF2 keypoint paired with KF1 keypoint i1, else
 * -1 (vMatchedPairs = the pairs in i1 order); *nmatches = the return value.  The reference
 * never marks KF2 keypoints as used (vbMatched2 stays false), so one KF2 keypoint may pair with
 * several KF1 keypoints, as here. */
int orbmi_search_for_triangulation(orbmi_matcher* m, const orbmi_frame_view* KF1, const uint8_t* has_mp1,
                                   const orbmi_feature_vector* fv1, const orbmi_frame_view* KF2, const uint8_t* has_mp2,
                                   const orbmi_feature_vector* fv2, const float* F12, int only_stereo, int check_ori,
                                   int32_t* match12, int* nmatches);

/* SearchForTriangulation of one keyframe against npairs neighbours in one launch, as
 * LocalMapping::CreateNewMapPoints calls it in its loop over the best covisible keyframes
 * (src/LocalMapping.cc:326-384): pair j is (KF1, KF2[j]) with has_mp2[j], fv2[j] and
 * F12[9 j .. 9 j + 8]; its matches go to match12[j * KF1.n .. (j + 1) * KF1.n) and, when nmatches
 * is not NULL, its count to nmatches[j] (host, synchronises).  Per pair identical to
 * orbmi_search_for_triangulation; asynchronous when match12 is device memory and nmatches NULL. */
int orbmi_search_for_triangulation_batch(orbmi_matcher* m, const orbmi_frame_view* KF1, const uint8_t* has_mp1,
                                         const orbmi_feature_vector* fv1, int npairs, const orbmi_frame_view* KF2,
                                         const uint8_t* const* has_mp2, const orbmi_feature_vector* fv2,
                                         const float* F12, int only_stereo, int check_ori, int32_t* match12,
                                         int* nmatches);

/* ORBmatcher::Fuse(KeyFrame* pKF, const vector<MapPoint*>& vpMapPoints, float th)
 * (src/ORBmatcher.cc:977-1127), its search: for each of the n_mp candidate map points (in
 * vpMapPoints order; NULL entries left out by the caller, isBad() as ORBMI_MP_BAD, in_kf[i] =
 * IsInKeyFrame(pKF), in_kf may be NULL) the keyframe keypoint it fuses with: best_idx[i] (-1
 * when the point is skipped or its best distance exceeds TH_LOW = 50) and best_dist[i] (256
 * without a candidate).  The KF view needs keys_un, u_right (NULL = monocular), desc, tcw, the
 * intrinsics, bounds (mnMinX.., IsInImage) and scale factors.  The map updates stay with the
 * caller, replayed in list order as the reference does them: skip points that became bad or
 * joined pKF meanwhile; pMPinKF = pKF->GetMapPoint(best_idx[i]): if present and not bad,
 * Replace toward the point with more observations, otherwise AddObservation + AddMapPoint;
 * count nFused.  *ncandidates = the points with best_idx >= 0 (= nFused when
 * the replay skips none). */
int orbmi_fuse_search(orbmi_matcher* m, const orbmi_frame_view* KF, const orbmi_mappoint* mps, const uint8_t* in_kf,
                      int n_mp, float th, int32_t* best_idx, int32_t* best_dist, int* ncandidates);

/* The search of Fuse(pKFi, vpMapPointMatches) for every target keyframe of SearchInNeighbors
 * (src/LocalMapping.cc:631-641) in one launch: the same n_mp candidates against each of the nkf
 * keyframes kfs[k]; keyframe k's results at best_idx / best_dist[k * n_mp ..) (in_kf, when not
 * NULL, likewise nkf x n_mp) and its candidate count at ncandidates[k] (host, synchronises; may
 * be NULL).  Per keyframe identical to orbmi_fuse_search. */
int orbmi_fuse_search_batch(orbmi_matcher* m, int nkf, const orbmi_frame_view* kfs, const orbmi_mappoint* mps,
                            const uint8_t* in_kf, int n_mp, float th, int32_t* best_idx, int32_t* best_dist,
                            int* ncandidates);

/* SearchInNeighbors between two Fuse targets (src/LocalMapping.cc:620-628): the
 * ComputeDistinctiveDescriptors that MapPoint::Replace owes its survivors (src/MapPoint.cc:212),
 * then the Fuse searches of the records whose descriptor that changed -- one synchronisation.
 * orbmi_compute_distinctive_descriptors of nd points (obs_desc, obs_off, best, desc_out as
 * there; nd may be 0), then orbmi_fuse_search_batch of n_mp records against nkf keyframes
 * (kfs, in_kf, th, best_idx, best_dist as there), record i searched with descriptor
 * desc_out[desc_from[i]] when desc_from (may be NULL) has desc_from[i] >= 0.  `mps` is read,
 * not written. */
int orbmi_fuse_search_refresh(orbmi_matcher* m, const uint8_t* obs_desc, const int32_t* obs_off, int nd, int32_t* best,
                              uint8_t* desc_out, int nkf, const orbmi_frame_view* kfs, const orbmi_mappoint* mps,
                              const int32_t* desc_from, const uint8_t* in_kf, int n_mp, float th, int32_t* best_idx,
                              int32_t* best_dist);

/* MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:247-316) for np map points: the
 * observation descriptors of point p are rows obs_off[p] .. obs_off[p + 1] - 1 of obs_desc
 * (x 32 B), in mObservations order with bad keyframes left out by the caller (the reference
 * iterates a map keyed by KeyFrame*; the build orders by keyframe id).
 * best[p] = the row (within the point) of least median Hamming distance to the point's other
 * descriptors (sorted row incl. the self-distance, element 0.5 (N - 1)), first row on ties; -1
 * without observations.  desc_out[p] (32 B) = that descriptor (mDescriptor); left unchanged for
 * points without observations.  Arrays host or device; asynchronous when best and desc_out are
 * device memory. */
int orbmi_compute_distinctive_descriptors(orbmi_matcher* m, const uint8_t* obs_desc, const int32_t* obs_off, int np,
                                          int32_t* best, uint8_t* desc_out);

/* ---- DBoW2 vocabulary: Frame::ComputeBoW / KeyFrame::ComputeBoW ---- */

/* DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB> (Thirdparty/DBoW2/DBoW2/
 * TemplatedVocabulary.h) as flat arrays, nodes in id order (node 0 = root, as
 * loadFromTextFile builds them, :1338-1424): 32-B descriptor, children as CSR in insertion
 * order, word id (-1 for inner nodes) and weight (idf for TF_IDF) per node.  scoring and
 * weighting are DBoW2::ScoringType / WeightingType (BowVector.h:36-53). */
typedef struct orbmi_vocabulary_desc {
    int k, L;                      /* m_k, m_L                                               */
    int scoring, weighting;        /* L1_NORM .. DOT_PRODUCT; TF_IDF, TF, IDF, BINARY         */
    int nnodes;
    const uint8_t* desc;           /* nnodes x 32                                            */
    const int32_t* child_off;      /* nnodes + 1                                             */
    const int32_t* children;       /* child_off[nnodes] node ids                             */
    const int32_t* word_id;        /* nnodes                                                 */
    const double* weight;          /* nnodes                                                 */
} orbmi_vocabulary_desc;

typedef struct orbmi_vocabulary orbmi_vocabulary;
/* Upload a vocabulary (host arrays) to `device`; the handle owns a stream. */
int orbmi_vocabulary_create(int device, const orbmi_vocabulary_desc* d, orbmi_vocabulary** out);
void orbmi_vocabulary_destroy(orbmi_vocabulary* v);
int orbmi_vocabulary_synchronize(orbmi_vocabulary* v);
/* Run the handle on `ex`'s stream (like orbmi_matcher_share_stream): a keyframe's ComputeBoW then
 * follows its extraction on the extraction stream, beside the LocalBA on the mapper's stream. */
int orbmi_vocabulary_share_stream(orbmi_vocabulary* v, orbmi_extractor* ex);
/* Run the handle on a caller's HIP stream (hipStream_t, e.g. orbmi_matcher_get_stream's), or on
 * a new stream of its own when `stream` is NULL.  The stream must outlive its use here.  Every
 * stream a process creates beyond the device's hardware queues (GPU_MAX_HW_QUEUES) shares a
 * queue with another and serialises behind its work: an in-order chain of operators (the
 * LocalMapping thread's) belongs on one stream. */
int orbmi_vocabulary_set_stream(orbmi_vocabulary* v, void* stream);
/* The handle's HIP stream (hipStream_t): its own, or the extractor's after share_stream. */
int orbmi_vocabulary_get_stream(orbmi_vocabulary* v, void** stream);

/* TemplatedVocabulary::transform(features, BowVector& v, FeatureVector& fv, levelsup)
 * (TemplatedVocabulary.h:1126-1194, per feature :1217-1259) as Frame::ComputeBoW calls it
 * (levelsup = 4, src/Frame.cc:425-432): each of the n descriptors (n x 32 u8) descends the tree
 * (FORB::distance, first child wins ties); features whose word weight is 0 are skipped.
 * Outputs (capacity n each; fv_off n + 1): the BowVector as word ids ascending + values
 * (addWeight for TF / TF_IDF, addIfNotExist for IDF / BINARY, 1/size for TF without
 * normalisation, then normalize(L1 | L2) when the scoring asks for it, BowVector.cpp:34-86),
 * the FeatureVector as CSR (orbmi_feature_vector: node ids at level L - levelsup ascending,
 * feature indices ascending), counts[0] = words, counts[1] = nodes.  n_device (optional)
 * overrides n with a device-resident count <= n.  Arrays host or device; asynchronous on the
 * handle's stream when every output (counts included) is device memory.  n <= 8192.  Calls on
 * one handle from several threads are serialised (the reference's transform is const). */
int orbmi_transform(orbmi_vocabulary* v, const uint8_t* desc, int n, const int* n_device, int levelsup,
                    uint32_t* bow_word, double* bow_value, uint32_t* fv_node, int32_t* fv_off, int32_t* fv_feat,
                    int* counts);

/* Cross-stream matching of config 4 (build-defined; no reference counterpart, SURVEY.md §8(d)
 * "Config 4"): brute-force Hamming nearest neighbour of each of the nq query descriptors over
 * the nseg gathered train segments (segment s = rows [s*seg_capacity, s*seg_capacity +
 * seg_counts[s]) of train_desc; segment skip_seg is ignored, -1 = none).  Accepted when
 * best <= th and best < ratio * second best (second = 256 when absent); equal distances
 * resolve to the lowest row.  match[q] = global train row or -1.  nq_device as in
 * orbmi_frame_view.  Inputs host or device; asynchronous when all outputs are device memory and
 * nmatches == NULL. */
int orbmi_match_descriptors_segments(orbmi_matcher* m, const uint8_t* q_desc, int nq, const int* nq_device,
                                     const uint8_t* train_desc, int nseg, int seg_capacity,
                                     const int* seg_counts, int skip_seg, int th, float ratio,
                                     int32_t* match, int* nmatches);

/* ---- Optimizer::LocalBundleAdjustment ------------------------------------------------ */

/* The local-BA graph exactly as src/Optimizer.cc:483-683 builds it: local keyframes
 * (optimised unless id == 0), fixed observer keyframes, local map points (marginalised), one
 * edge per (point, keyframe) observation in the reference's insertion order (points in
 * lLocalMapPoints order, observations in map order).  Poses cross as float Tcw (cv::Mat
 * CV_32F), converted to double inside (src/Converter.cc:37-47). */
typedef struct orbmi_ba_keyframe {
    float tcw[16];                 /* KeyFrame::GetPose(), row-major 4x4                */
    uint32_t id;                   /* KeyFrame::mnId (vertex id)                         */
    int32_t fixed;                 /* fixed camera or mnId == 0                          */
    float fx, fy, cx, cy, bf;      /* KeyFrame::fx, fy, cx, cy, mbf                     */
} orbmi_ba_keyframe;

typedef struct orbmi_ba_point {
    float pos[3];                  /* MapPoint::GetWorldPos()                            */
    uint32_t id;                   /* MapPoint::mnId (vertex id = id + maxKFid + 1)       */
    int32_t bad;                   /* isBad() when the outlier loops run (:705, :747)     */
} orbmi_ba_point;

typedef struct orbmi_ba_edge {
    int32_t point, kf;             /* indices into the point / keyframe arrays           */
    float u, v;                    /* mvKeysUn[idx].pt                                   */
    float ur;                      /* mvuRight[idx]; < 0 -> EdgeSE3ProjectXYZ (mono)     */
    float inv_sigma2;              /* mvInvLevelSigma2[octave]                            */
} orbmi_ba_edge;

typedef struct orbmi_ba_problem {
    int nkf, npt, nedge;
    const orbmi_ba_keyframe* kfs;
    const orbmi_ba_point* pts;
    const orbmi_ba_edge* edges;
} orbmi_ba_problem;

typedef struct orbmi_ba_result {
    float* tcw;                    /* nkf x 16: optimised poses (fixed ones unchanged)    */
    float* pos;                    /* npt x 3                                            */
    uint8_t* erase;                /* nedge: 1 -> (KF, MP) pair goes to vToErase (:741-773) */
    int iterations[2];             /* optimize(5) / optimize(10) iterations run          */
    double chi2[2];                /* final activeRobustChi2 of both optimisations       */
    int aborted;                   /* stop flag seen before the first optimisation: no write-back */
    int stop_check;                /* index of the first pbStopFlag check that found the flag
                                    * raised (-1: none); numbering: orbmi_ba_set_stop_at_check */
    int checks;                    /* pbStopFlag checks made by the call                 */
} orbmi_ba_result;

typedef struct orbmi_ba orbmi_ba;
int orbmi_ba_create(int device, orbmi_ba** out);
void orbmi_ba_destroy(orbmi_ba* h);
/* Run the handle on a caller's HIP stream, or its own new one when `stream` is NULL (as
 * orbmi_vocabulary_set_stream). */
int orbmi_ba_set_stream(orbmi_ba* b, void* stream);
/* Deterministic pbStopFlag (test and schedule-replay hook; no counterpart in the reference):
 * in every later call on the handle the flag reads raised from its k-th check on (k < 0: off),
 * whatever `stop` holds.  The checks are the reads of pbStopFlag in the order the reference
 * evaluates them, numbered from 0:
 *   #0  src/Optimizer.cc:685 (raised: return before optimising, `aborted`, no write-back);
 *   SparseOptimizer::optimize's loop condition before each iteration while i < iterations
 *       (Thirdparty/g2o/g2o/core/sparse_optimizer.cpp:376; none when the graph has no vertex);
 *   the LM inner loop's condition after a rejected trial while qmax < 10
 *       (optimization_algorithm_levenberg.cpp:149, evaluated only when rho < 0);
 *   src/Optimizer.cc:689 (bDoMore) after optimize(5); then optimize(10)'s, as optimize(5)'s.
 * A flag raised by another thread is first seen at one of these checks, so a call with
 * k = result.stop_check of a concurrent run repeats that run exactly. */
int orbmi_ba_set_stop_at_check(orbmi_ba* b, int k);
/* Host hook (no counterpart in the reference): in every later call on the handle, fn(arg) runs
 * on the calling thread once the LocalBA's work has been enqueued and before the call waits for
 * it, so a caller can enqueue independent work of its own (e.g. the next keyframe's
 * ComputeBoW on another stream) beside the solve.  fn must not call back into this handle.
 * fn = NULL removes it. */
int orbmi_ba_set_enqueued_hook(orbmi_ba* b, void (*fn)(void*), void* arg);

/* Optimizer::LocalBundleAdjustment(pKF, pbStopFlag, pMap) (include/Optimizer.h:62,
 * src/Optimizer.cc:483-808) on the assembled graph: LM (g2o OptimizationAlgorithmLevenberg,
 * BlockSolver_6_3 Schur complement, Huber sqrt(5.991)/sqrt(7.815)) 5 iterations, outlier
 * levels, 10 iterations without kernels, erase list.  All arithmetic fp64 on the GPU.
 * `stop` (may be NULL) is read like pbStopFlag / mbAbortBA, at the checks listed under
 * orbmi_ba_set_stop_at_check.  Edges must come grouped by point with at most one per (point,
 * keyframe), as a map point's observations give them; otherwise ORBMI_E_ARG. */
int orbmi_local_bundle_adjustment(orbmi_ba* h, const orbmi_ba_problem* problem, orbmi_ba_result* result,
                                  const volatile int* stop);

/* ---- Optimizer::BundleAdjustment (global BA) ------------------------------------------ */

#define ORBMI_GBA_MAX_FREE_POSES 2048 /* optimised keyframes of one call; more: ORBMI_E_UNSUPPORTED */
#define ORBMI_GBA_MAX_ITERATIONS 64   /* `iterations` of one call (the length of `trials`)          */
#define ORBMI_GBA_TERMINATE 1    /* Levenberg stopped by a rule of its own (else: count or stop flag) */
#define ORBMI_GBA_SOLVE_FAILED 2 /* a damped solve met a pivot that is not a positive finite number  */
#define ORBMI_GBA_REJECTED 4     /* a trial was rejected and the estimates restored                  */

typedef struct orbmi_gba_result {
    float* tcw;                    /* nkf x 16; fixed keyframes and keyframes that no edge names
                                    * come back as given, bit for bit                            */
    float* pos;                    /* npt x 3; a point without an edge comes back as given      */
    uint8_t* included;             /* npt: !vbNotIncludedMP (the point has at least one edge)    */
    int iterations;                /* iterations of optimize() run                               */
    int trials[ORBMI_GBA_MAX_ITERATIONS]; /* Levenberg trials (qmax) of iteration k; 0 beyond     */
    double chi2_initial;           /* activeRobustChi2 at the first linearisation                */
    double chi2;                   /* activeRobustChi2 of the errors as the last trial left them */
    int stop_check;                /* index of the first stop-flag check that found it raised, -1: none */
    int checks;                    /* stop-flag checks made by the call                          */
    int status;                    /* ORBMI_GBA_* or'ed                                          */
    int n_free;                    /* pose blocks of the reduced camera system                   */
    int n_blocks;                  /* non-zero 6 x 6 blocks (i >= j) of S before elimination     */
    double phase_ms[4];            /* with ORBMI_GBA_PROFILE set in the environment: device time of
                                    * linearise, Schur, factor + solve, update + chi2; else 0   */
} orbmi_gba_result;

/* Optimizer::BundleAdjustment(vpKFs, vpMP, nIterations, pbStopFlag, nLoopKF, bRobust)
 * (src/Optimizer.cc:56-255) on the assembled graph: one optimize(iterations) of g2o's Levenberg over
 * BlockSolver_6_3, Huber sqrt(5.99) / sqrt(7.815) when `robust`, no outlier levels.  It runs on an
 * orbmi_ba handle and honours orbmi_ba_set_stream and orbmi_ba_set_stop_at_check.  `fixed` is taken
 * as given; orbmi_ba_point.bad is ignored (the caller leaves bad vertices out).  Edges grouped by
 * point with at most one per (point, keyframe), as orbmi_local_bundle_adjustment; else ORBMI_E_ARG.
 * The stop-flag checks, numbered from 0 in the order g2o reads them: optimize's loop condition
 * before each iteration while i < iterations, and the Levenberg inner loop's condition after a
 * rejected trial while qmax < 10.  There is none before or after the optimisation; whatever
 * estimate stands when the flag is seen is written back (skipping the map update is the caller's
 * rule).  The reduced camera system is dense and sized from the problem: any number of keyframes,
 * up to ORBMI_GBA_MAX_FREE_POSES optimised ones, checked before anything is allocated or
 * launched (ORBMI_E_UNSUPPORTED).  ORBMI_E_ARG: a NULL array, a negative count, iterations outside
 * [0, ORBMI_GBA_MAX_ITERATIONS], an edge index out of range.  Every loop is bounded: any input
 * terminates, with ORBMI_GBA_SOLVE_FAILED where a solve failed.  Synchronous; host arrays. */
int orbmi_bundle_adjustment(orbmi_ba* h, const orbmi_ba_problem* problem, int iterations, int robust,
                            orbmi_gba_result* result, const volatile int* stop);

/* ---- Optimizer::PoseOptimization ---------------------------------------------------- */

/* One unary edge: a keypoint i of the Frame with a MapPoint (mvpMapPoints[i] != NULL),
 * src/Optimizer.cc:296-375.  `index` is the caller's keypoint index (mvbOutlier slot). */
typedef struct orbmi_pose_obs {
    float Xw[3];                   /* MapPoint::GetWorldPos()                             */
    float u, v;                    /* mvKeysUn[i].pt                                      */
    float ur;                      /* mvuRight[i]; < 0 -> EdgeSE3ProjectXYZOnlyPose (mono)  */
    float inv_sigma2;              /* mvInvLevelSigma2[mvKeysUn[i].octave]                 */
    int32_t index;                 /* keypoint index i (returned untouched)               */
} orbmi_pose_obs;

/* One frame: its observations are obs[obs_begin, obs_begin + n_obs). */
typedef struct orbmi_pose_frame {
    float tcw[16];                 /* in: Frame::mTcw (row-major); out: optimised pose;
                                      unchanged when fewer than 3 observations (:378-379)  */
    float fx, fy, cx, cy, bf;      /* Frame::fx, fy, cx, cy, mbf                           */
    int32_t obs_begin, n_obs;
    int32_t inliers;               /* out: nInitialCorrespondences - nBad, the return value;
                                      -1 when n_obs exceeds the kernel's 4096 (device path) */
    int32_t iterations;            /* out: LM iterations run over the 4 rounds (diagnostic) */
} orbmi_pose_frame;

typedef struct orbmi_pose orbmi_pose;
int orbmi_pose_create(int device, orbmi_pose** out);
void orbmi_pose_destroy(orbmi_pose* h);

/* Optimizer::PoseOptimization(Frame*) (include/Optimizer.h:58, src/Optimizer.cc:257-481) on
 * `nframes` independent frames in one launch (one workgroup per frame): 4 rounds of
 * optimize(10) (g2o Levenberg, BlockSolver_6_3 + LinearSolverDense, Huber sqrt(5.991) /
 * sqrt(7.815) for the first 3 rounds) from the frame's initial pose, outliers re-classified
 * after each round (chi2 > 5.991 / 7.815, level 1).  outlier[k] receives mvbOutlier for obs k.
 * fp64 on the GPU.  `frames`, `obs` and `outlier` may be host or device pointers; device
 * pointers leave the work enqueued on the handle's stream (orbmi_pose_synchronize). */
int orbmi_pose_optimization(orbmi_pose* h, orbmi_pose_frame* frames, int nframes, const orbmi_pose_obs* obs,
                            int nobs, uint8_t* outlier);
int orbmi_pose_synchronize(orbmi_pose* h);
/* Run the handle on `ex`'s stream (like orbmi_matcher_share_stream): a tracked frame's
 * extraction, searches and pose optimisations are then ordered without host round trips. */
int orbmi_pose_share_stream(orbmi_pose* h, orbmi_extractor* ex);
/* Run the handle on the matcher's stream instead: the tracking stages (searches, pose
 * optimisations) then form one stream that can run beside the next frame's extraction. */
int orbmi_pose_share_matcher_stream(orbmi_pose* h, orbmi_matcher* m);
/* Bracket PoseOptimization kernels launched by orbmi_pose_optimization_frame[_track] with HIP
 * events on the handle's stream: every launch for on == 1, every on-th launch for on > 1 (each
 * timed event is a queue packet of a few microseconds on the stream: sampling keeps the
 * measurement from slowing what it measures), none for on <= 0; orbmi_pose_read_profile
 * synchronises and returns the summed device time (ms) and the number of timed launches since
 * the last read. */
int orbmi_pose_set_profiling(orbmi_pose* h, int on);
int orbmi_pose_read_profile(orbmi_pose* h, double* ms, long long* launches);

/* Frame::mvpMapPoints of the frame being tracked, as the matchers left it: keypoint i holds
 * local map point mps[match_mp[i]] when match_mp && match_mp[i] >= 0, otherwise last-frame
 * point lf_points[match_lf[i]] when match_lf && match_lf[i] >= 0, otherwise NULL.  The match
 * arrays are the outputs of orbmi_search_local_points / orbmi_search_by_projection_last_frame
 * (CF.n entries; -1 and -2 both mean NULL). */
typedef struct orbmi_frame_mappoints {
    int32_t* match_lf;
    const orbmi_lastframe_point* lf_points;
    int n_lf_points;               /* entries of lf_points (last frame's N)                */
    int32_t* match_mp;
    const orbmi_mappoint* mps;
    int n_mps;                     /* entries of mps                                       */
} orbmi_frame_mappoints;

/* Optimizer::PoseOptimization(Frame* pFrame) (include/Optimizer.h:58, src/Optimizer.cc:257-481)
 * with its edge assembly (:296-375): one unary edge per keypoint holding a map point, in
 * keypoint order, stereo when mvuRight[i] >= 0, information mvInvLevelSigma2[octave].  The
 * initial pose is F->tcw (host or device).  rec receives the optimised tcw, fx..bf, n_obs =
 * nInitialCorrespondences, inliers (the return value) and iterations; outlier[i] = mvbOutlier[i]
 * (F->n entries; 0 for keypoints without a map point).  inv_level_sigma2: host, F->nlevels
 * floats.  Every array may be host or device memory; with rec and outlier in device memory the
 * call is asynchronous on the handle's stream (F->n_device is then honoured). */
int orbmi_pose_optimization_frame(orbmi_pose* h, const orbmi_frame_view* F, const float* inv_level_sigma2,
                                  const orbmi_frame_mappoints* mp, orbmi_pose_frame* rec, uint8_t* outlier);

/* ---- Tracking (TrackWithMotionModel / TrackLocalMap bookkeeping) -------------------- */

/* The wider-window retry of Tracking::TrackWithMotionModel (src/Tracking.cc:1018-1023) with
 * the count kept on the device: when *nmatches_dev < min_matches, SearchByProjection(CF, LF,
 * th) runs as orbmi_search_by_projection_last_frame (match_lf rewritten, *nmatches_dev = its
 * count); otherwise nothing changes.  nmatches_dev must be device memory; asynchronous. */
int orbmi_search_by_projection_last_frame_if(orbmi_matcher* m, const orbmi_frame_view* CF,
                                             const uint8_t* occupied, const orbmi_frame_view* LF,
                                             const orbmi_lastframe_point* lf_points, float th, int mono,
                                             int check_ori, int32_t* match_lf, int* nmatches_dev,
                                             int min_matches);

/* Tracking's pass over mvpMapPoints after a PoseOptimization, on the device:
 * stage 0 = TrackWithMotionModel "Discard outliers" (src/Tracking.cc:1036-1058): outlier map
 *   points become NULL (their match entry -1); counts[0] = outliers removed (the reference's
 *   nmatches -= counts[0]), counts[1] = nmatchesMap (inliers whose point has Observations() > 0);
 *   occupied_out[i] = 1 when keypoint i keeps a point with observations (the `occupied` input of
 *   the local-map search).
 * stage 1 = TrackLocalMap statistics (src/Tracking.cc:1085-1104): counts[0] = mnMatchesInliers
 *   (non-outliers with Observations() > 0), counts[1] = outliers; with stereo (F->u_right set)
 *   outliers become NULL.  occupied_out may be NULL.
 * counts: 2 ints, host or device (device -> asynchronous). */
int orbmi_track_update_matches(orbmi_matcher* m, const orbmi_frame_view* F, int stage, const uint8_t* outlier,
                               const orbmi_frame_mappoints* mp, uint8_t* occupied_out, int* counts);

/* orbmi_pose_optimization_frame followed by orbmi_track_update_matches(stage) on its outlier
 * flags, in one launch on the pose handle's stream (Tracking::TrackWithMotionModel's
 * PoseOptimization + "Discard outliers", src/Tracking.cc:1033-1058, with stage 0; TrackLocalMap's
 * PoseOptimization + statistics, :1079-1104, with stage 1): the same results as the two calls.
 * Every array (rec, outlier, counts, occupied_out, the match arrays and point records of mp)
 * must be device memory: the call is asynchronous; ORBMI_E_ARG otherwise. */
int orbmi_pose_optimization_frame_track(orbmi_pose* h, const orbmi_frame_view* F, const float* inv_level_sigma2,
                                        const orbmi_frame_mappoints* mp, orbmi_pose_frame* rec, uint8_t* outlier,
                                        int stage, uint8_t* occupied_out, int* counts);

/* ---- LocalMapping host geometry (CreateNewMapPoints around SearchForTriangulation) ----- */

/* The KeyFrame members CreateNewMapPoints reads (host arrays): pose, mvKeysUn, mvuRight,
 * mvDepth, intrinsics, mbf, mb, mvLevelSigma2 and mvScaleFactors (nlevels entries). */
typedef struct orbmi_tri_keyframe {
    const float* tcw;              /* 4x4 row-major Tcw                                     */
    const orbmi_keypoint* keys_un;
    const float* u_right;
    const float* depth;
    float fx, fy, cx, cy, bf, mb;
    const float* level_sigma2;
    const float* scale_factors;
} orbmi_tri_keyframe;

/* LocalMapping::ComputeF12 (src/LocalMapping.cc:676-693): F12 = K1^-T [t12]x R12 K2^-1 (3x3
 * row-major float), the epipolar constraint SearchForTriangulation takes. */
int orbmi_compute_f12(const orbmi_tri_keyframe* kf1, const orbmi_tri_keyframe* kf2, float* F12);

/* CreateNewMapPoints' per-match geometry (src/LocalMapping.cc:385-575) for the n matched
 * keypoint pairs (idx1[k] of kf1, idx2[k] of kf2): ray parallax, linear triangulation or stereo
 * back-projection, positive depth in both cameras, reprojection error (5.991 / 7.8 sigma^2) and
 * scale consistency.  ok[k] = 1 with x3d[3k..3k+2] the new point's world position, else 0. */
int orbmi_triangulate_matches(const orbmi_tri_keyframe* kf1, const orbmi_tri_keyframe* kf2, const int32_t* idx1,
                              const int32_t* idx2, int n, float* x3d, uint8_t* ok);

/* cos(2 atan2(mb / 2, depth[i])) as float for n keypoints: CreateNewMapPoints' stereo parallax
 * of a stereo keypoint (src/LocalMapping.cc:409-412), a per-keyframe table for
 * orbmi_create_new_map_points. */
int orbmi_stereo_parallax_cos(float mb, const float* depth, int n, float* out);

/* LocalMapping::CreateNewMapPoints' searches and geometry (src/LocalMapping.cc:290-577) for one
 * keyframe and npairs neighbours (in the order the reference visits them, the baseline test
 * already applied), all on the device with one synchronisation: pair j's SearchForTriangulation
 * (as orbmi_search_for_triangulation with bOnlyStereo = false and the matcher's
 * mbCheckOrientation = false, ORBmatcher matcher(0.6, false) at :306) sees KF1's map points as
 * the pairs before it left them -- a KF1 keypoint whose match an earlier pair's triangulation
 * accepted counts as having a map point, exactly as in the reference's loop -- and the pair's
 * matches are then tested as orbmi_triangulate_matches does.
 * kf1 / kf2[j]: frame views (keys_un, u_right, desc host or device; tcw host); tri1 / tri2[j]:
 * the geometry, of which tcw, depth (host or device, n entries), the intrinsics, level_sigma2
 * and scale_factors (host, nlevels of the frame view) are read; cos1 / cos2[j]: the keyframe's
 * orbmi_stereo_parallax_cos table (host or device), or NULL to compute it here from a host depth.
 * has_mp1 / has_mp2[j]: the keyframes' map points on entry (not modified).
 * Outputs (host or device), row j * kf1->n + i for pair j and KF1 keypoint i: match12 = the
 * KF2 keypoint SearchForTriangulation paired with i, or -1; ok = 1 when the geometry accepted a
 * new map point; x3d[3 * row ..] = its world position (unspecified where ok = 0). */
int orbmi_create_new_map_points(orbmi_matcher* m, const orbmi_frame_view* kf1, const orbmi_tri_keyframe* tri1,
                                const float* cos1, const uint8_t* has_mp1, const orbmi_feature_vector* fv1,
                                int npairs, const orbmi_frame_view* kf2, const orbmi_tri_keyframe* tri2,
                                const float* const* cos2, const uint8_t* const* has_mp2,
                                const orbmi_feature_vector* fv2, const float* F12, int32_t* match12, uint8_t* ok,
                                float* x3d);

/* One LocalMapping::Run iteration for a new keyframe (src/LocalMapping.cc:47-128) as one call:
 * what the per-operator entries above do when called one after the other, staged once.  Every
 * array is device memory unless noted; every output is device memory (the call reads none of
 * them back), except the LocalBA result. */
typedef struct orbmi_lm_job {
    /* KeyFrame::ComputeBoW (ProcessNewKeyFrame, :152-160).  voc != NULL: orbmi_transform of
     * bow_desc (bow_n x 32) is issued here, and its sizes copied to counts_host behind it.
     * voc == NULL: the caller issued both ahead (on any stream).  Either way counts_event is
     * recorded (by the caller when voc == NULL, here otherwise) behind the copy of the two size
     * words to counts_host (pinned host memory): the call waits on that event only. */
    orbmi_vocabulary* voc;
    const uint8_t* bow_desc;
    int bow_n;
    uint32_t* bow_word;            /* the keyframe's BowVector / FeatureVector set, as          */
    double* bow_value;             /* orbmi_transform writes it (capacity bow_n)               */
    uint32_t* fv_node;
    int32_t* fv_off;
    int32_t* fv_feat;
    int* bow_counts;               /* device: words, nodes                                     */
    const int32_t* counts_host;    /* pinned host: words, nodes                                */
    void* counts_event;            /* hipEvent_t behind the copy to counts_host                */
    /* MapPoint::ComputeDistinctiveDescriptors of the keyframe's points (:162-190 and :662-674),
     * as orbmi_compute_distinctive_descriptors; run before CreateNewMapPoints and after Fuse. */
    const uint8_t* obs_desc;
    const int32_t* obs_off;
    int n_points;
    int32_t* best;
    uint8_t* desc_out;
    /* CreateNewMapPoints (:290-577), as orbmi_create_new_map_points; fv1 = the set above with
     * the node count read from counts_host. */
    const orbmi_frame_view* kf;
    const orbmi_tri_keyframe* tri;
    const float* cos;
    const uint8_t* has_mp;
    int nnb;                       /* neighbours (may be 0: no search, no batched Fuse)         */
    const orbmi_frame_view* kf2;
    const orbmi_tri_keyframe* tri2;
    const float* const* cos2;
    const uint8_t* const* has_mp2;
    const orbmi_feature_vector* fv2;
    const float* F12;              /* host, 9 x nnb                                             */
    int32_t* match12;              /* nnb x kf->n                                               */
    uint8_t* ok;
    float* x3d;
    /* SearchInNeighbors (:589-660): orbmi_fuse_search_batch(kf2[0..nnb), kf_points) into
     * best_idx / best_dist[0 .. nnb * n_kf_points), then orbmi_fuse_search(kf, target_points)
     * into the n_target_points entries behind them. */
    const orbmi_mappoint* kf_points;
    int n_kf_points;
    const orbmi_mappoint* target_points;
    int n_target_points;
    float fuse_th;                 /* 3.0 in the reference                                      */
    int32_t* best_idx;
    int32_t* best_dist;
    /* Optimizer::LocalBundleAdjustment (:89-90), as orbmi_local_bundle_adjustment. */
    const orbmi_ba_problem* problem;
    orbmi_ba_result* result;
    const volatile int* stop;
    /* optional diagnostics: 4 hipEvent_t recorded on the matcher's stream behind ComputeBoW +
     * the first ComputeDistinctiveDescriptors, CreateNewMapPoints, the Fuse searches and the
     * second ComputeDistinctiveDescriptors (NULL: none) */
    void* const* stage_events;
} orbmi_lm_job;

typedef struct orbmi_lm_job_result {
    int bow_words, fv_nodes;       /* sizes of the keyframe's BowVector / FeatureVector         */
    int failed_stage;              /* -1, or the stage that returned the error: 0 ComputeBoW,
                                    * 1 / 4 ComputeDistinctiveDescriptors, 2 CreateNewMapPoints,
                                    * 3 Fuse, 5 LocalBundleAdjustment                           */
} orbmi_lm_job_result;

/* LocalMapping::Run's body for one keyframe (src/LocalMapping.cc:47-128, the calls it replaces:
 * ProcessNewKeyFrame :59, CreateNewMapPoints :65, SearchInNeighbors :70, LocalBundleAdjustment
 * :89-90) on the matcher's stream, in the reference's order, LocalBA through `ba` (run it on the
 * matcher's stream, orbmi_ba_set_stream, for an in-order chain).  The host tables of all the
 * searches (pair table, KF2 sides, Fuse keyframes) are validated and built inside the call and go
 * to the device in one copy into one arena generation.  The only host waits are counts_event
 * (the FeatureVector's node count sizes the triangulation search) and LocalBA's own.  Returns
 * when LocalBA has returned; the first failing stage's code otherwise (failed_stage), with
 * nothing left pending in the matcher's arena.  ba's enqueued hook fires as in
 * orbmi_local_bundle_adjustment. */
int orbmi_local_mapping_job(orbmi_matcher* m, orbmi_ba* ba, const orbmi_lm_job* job, orbmi_lm_job_result* result);

/* ---- System::TrackStereo: the native stereo SLAM host loop ---------------------------- */

/* The Tracking constructor's view of a settings file (src/Tracking.cc:53-143) for a rectified
 * stereo rig: Camera.fx/fy/cx/cy, Camera.bf, mThDepth = bf * ThDepth / fx, mMinFrames = 0,
 * mMaxFrames = fps, the image size and the ORBextractor parameters. */
typedef struct orbmi_slam_settings {
    float fx, fy, cx, cy, bf;
    float th_depth;
    int min_frames, max_frames;
    int width, height;
    int n_features;
    float scale_factor;
    int n_levels, ini_th_fast, min_th_fast;
    int local_ba;                  /* 1: LocalMapping runs LocalBundleAdjustment (:89-90)      */
    int local_mapping;             /* 1: and CreateNewMapPoints, SearchInNeighbors, KeyFrameCulling */
    int async_local_mapping;       /* 1: LocalMapping on its own thread, concurrent with Tracking as
                                      in the reference (keyframe decisions then depend on timing);
                                      0: synchronous after each keyframe (deterministic) */
} orbmi_slam_settings;

/* Per tracked frame: Tracking's counters (-1 = the stage did not run). track: 0 none, 1
 * TrackWithMotionModel, 2 TrackReferenceKeyFrame (the last one tried). */
typedef struct orbmi_slam_frame_stats {
    int frame, n, state, init, track;
    int lf_matches, bow_matches, nmatches_map, local_map_points, local_matches, inliers;
    int need_kf, keyframes, mappoints;
    int reset; /* 1: the frame was lost with <= 5 keyframes in the map and the system reset
                * (src/Tracking.cc:540-551); the map and the trajectory lists start over */
} orbmi_slam_frame_stats;

typedef struct orbmi_slam orbmi_slam;

/* System(strSettingsFile, STEREO) + Tracking + a synchronous LocalMapping
 * (src/System.cc:36-107, src/Tracking.cc:53-143, src/LocalMapping.cc:47-128) on `device`: the
 * map (keyframes, map points, covisibility, spanning tree) is kept natively, every per-keypoint
 * operator is the MI355X one of this library.  vocabulary (may be NULL: TrackReferenceKeyFrame
 * then fails with ORBMI_E_STATE) is borrowed and must outlive the handle. */
int orbmi_slam_create(const orbmi_slam_settings* s, int device, orbmi_vocabulary* vocabulary, orbmi_slam** out);
/* System::Shutdown's wait for LocalMapping (src/System.cc:300-314): returns when no keyframe is
 * queued or being processed (immediately in synchronous mode); the mapping thread's first error. */
int orbmi_slam_wait_local_mapping(orbmi_slam* h);
void orbmi_slam_destroy(orbmi_slam* h);

/* System::TrackStereo(imLeft, imRight, timestamp) (src/System.cc:110-159): host u8 gray images
 * (rows x cols, row pitch step).  tcw_out (16 floats, may be NULL) receives mCurrentFrame.mTcw;
 * *has_pose = 0 while not initialised / lost (empty Tcw). */
int orbmi_slam_track_stereo(orbmi_slam* h, const uint8_t* left, const uint8_t* right, int rows, int cols, size_t step,
                            double timestamp, float* tcw_out, int* has_pose);

/* orbmi_slam_track_stereo for drivers that have the next pair at hand (a stereo_kitti loop over
 * image files): as the plain call, and then the next pair's Frame constructor (upload, ORB
 * extraction of both images, ComputeStereoMatches) is enqueued to run on the GPU while this frame
 * is tracked.  The next call must pass that pair as left/right -- the same buffers, unmodified,
 * same geometry -- to use it (any other pair is extracted as usual); next_left / next_right NULL:
 * nothing ahead.  The extraction depends on the images only, so every result is the plain call's.
 * The next pair is copied and enqueued by a helper thread of the handle while this frame is
 * tracked, and that work has finished when the call returns: next_left / next_right are not
 * read after it (ORBMI_SLAM_INLINE_FRAME=1: on the calling thread, before tracking). */
int orbmi_slam_track_stereo_ahead(orbmi_slam* h, const uint8_t* left, const uint8_t* right, int rows, int cols,
                                  size_t step, double timestamp, const uint8_t* next_left,
                                  const uint8_t* next_right, float* tcw_out, int* has_pose);

/* orbmi_slam_create for a rig whose images are not rectified (Examples/Stereo/stereo_euroc.cc:
 * 55-137): both maps are built once, and orbmi_slam_track_stereo / _ahead then take the raw
 * images -- each pair is uploaded, remapped on the device (one launch) into the buffer the
 * extractor reads, and the Frame constructor continues as on a plain handle.  Both cameras'
 * sizes must equal s->width x s->height (ORBMI_E_ARG and no handle otherwise); a frame of
 * another size returns ORBMI_E_ARG and leaves the handle usable.  s describes the rectified
 * rig (Camera.fx ... = LEFT.P). */
int orbmi_slam_create_stereo_rectify(const orbmi_slam_settings* s, const orbmi_rectify_camera* left_cam,
                                     const orbmi_rectify_camera* right_cam, int device,
                                     orbmi_vocabulary* vocabulary, orbmi_slam** out);

/* System(strSettingsFile, RGBD): what Tracking reads for an RGB-D sensor beyond
 * orbmi_slam_settings -- mDistCoef (ndist = 4 or 5), mDepthMapFactor already inverted
 * (src/Tracking.cc:143-147) and mbRGB. */
typedef struct orbmi_rgbd_settings {
    float dist[5];
    int ndist;
    float depth_map_factor;
    int rgb;
} orbmi_rgbd_settings;

/* orbmi_slam_create for the RGB-D sensor: one ORBextractor, the image bounds of the distorted
 * camera (orbmi_compute_image_bounds) computed once.  Everything after the Frame constructor is the
 * stereo handle's (the reference takes the same branches for RGBD as for STEREO). */
int orbmi_slam_create_rgbd(const orbmi_slam_settings* s, const orbmi_rgbd_settings* r, int device,
                           orbmi_vocabulary* vocabulary, orbmi_slam** out);

/* System::TrackRGBD(im, depthmap, timestamp) (src/System.cc:161-210, Tracking::GrabImageRGBD):
 * image = host u8 with `channels` 1, 3 or 4 (row pitch image_step bytes), depth = host depth map
 * (ORBMI_DEPTH_F32 / ORBMI_DEPTH_U16, row pitch depth_step bytes), both rows x cols.  Outputs as
 * orbmi_slam_track_stereo.  ORBMI_E_STATE on a stereo handle; the stereo calls return
 * ORBMI_E_STATE on an RGB-D handle. */
int orbmi_slam_track_rgbd(orbmi_slam* h, const uint8_t* image, int channels, size_t image_step, const void* depth,
                          int depth_type, size_t depth_step, int rows, int cols, double timestamp, float* tcw_out,
                          int* has_pose);

/* The counters of the `frame`-th TrackStereo call (0-based; the record stays across a reset,
 * while frame ids restart); ORBMI_E_ARG past the last call. */
int orbmi_slam_get_stats(orbmi_slam* h, int frame, orbmi_slam_frame_stats* out);
/* frames since the last reset (Frame::nNextId), keyframes, non-bad map points, LocalBundleAdjustment calls */
int orbmi_slam_get_counts(orbmi_slam* h, int* frames, int* keyframes, int* mappoints, int* local_ba_calls);
/* The poses SaveTrajectoryKITTI / TUM write (src/System.cc:334-486): per recorded frame Tcw =
 * Tcr * Trw * Two (16 floats), its timestamp and mlbLost.  capacity < n -> ORBMI_E_CAP, *n set. */
int orbmi_slam_get_trajectory(orbmi_slam* h, float* tcw, double* timestamps, uint8_t* lost, int capacity, int* n);
/* System::SaveTrajectoryKITTI / SaveTrajectoryTUM / SaveKeyFrameTrajectoryTUM. */
int orbmi_slam_save_trajectory_kitti(orbmi_slam* h, const char* path);
int orbmi_slam_save_trajectory_tum(orbmi_slam* h, const char* path);
int orbmi_slam_save_keyframe_trajectory_tum(orbmi_slam* h, const char* path);

/* ---- LoopClosing::ComputeSim3: Sim3Solver ------------------------------------------- */

/* One Sim3Solver after its constructor's filtering (src/Sim3Solver.cc:62-103): the n kept
 * correspondences.  x3d_c1 / x3d_c2 = mvX3Dc1 / mvX3Dc2 (n x 3, camera frames), max_err1 /
 * max_err2 = mvnMaxError1 / 2 (9.210 * sigma2 truncated to an integer, as the reference's
 * vector<size_t> stores it), k1 / k2 = fx fy cx cy of mK1 / mK2, fix_scale = mbFixScale; then the
 * arguments of SetRansacParameters (:114-138).  The arrays may be host or device memory.
 * triples: the minimal sets, iterations x 3 indices into the n correspondences (host memory,
 * iterations = orbmi_sim3_iterations), or NULL to draw them as orbmi_sim3_sample_triples does
 * from (seed, the solver's position in the batch, the iteration). */
typedef struct orbmi_sim3_problem {
    int32_t n;
    const float* x3d_c1;
    const float* x3d_c2;
    const int32_t* max_err1;
    const int32_t* max_err2;
    float k1[4], k2[4];
    int32_t fix_scale;
    double probability;
    int32_t min_inliers;
    int32_t max_iterations;
    const int32_t* triples;
    uint64_t seed;
} orbmi_sim3_problem;

/* Every hypothesis of one solver: what iteration h of Sim3Solver::iterate (:160-213) computes
 * before it compares with the best.  iterations (out) = mRansacMaxIts after SetRansacParameters,
 * 0 when n < min_inliers (iterate returns bNoMore at once, :147-151).  The arrays (host or device
 * memory, room for max_iterations hypotheses) receive per hypothesis h: rows 0-2 of mT12i and
 * mT21i (row-major 3x4), ms12i, mnInliersi, and mvbInliersi as a bitmask of (n + 63) / 64 64-bit
 * words (bit i & 63 of word i >> 6 = correspondence i). */
typedef struct orbmi_sim3_hypotheses {
    int32_t iterations;
    float* T12;
    float* T21;
    float* s;
    int32_t* count;
    uint64_t* mask;
} orbmi_sim3_hypotheses;

/* ComputeSim3 (:239-351) and CheckInliers (:354-378) for every iteration of `nsolvers` solvers in
 * one launch on the matcher handle's stream (the candidate loop of LoopClosing::ComputeSim3,
 * src/LoopClosing.cc:349-398, runs 5 iterations per candidate per round, sequentially).  The
 * caller replays iterate's best / return rule over the arrays (orbmi::Sim3Solver in orbmi.hpp).
 * ORBMI_E_ARG before anything is launched: n < 3 (with n >= min_inliers), an index of `triples`
 * outside [0, n), a NULL array.  Host outputs are complete on return; with every output in
 * device memory the call is asynchronous. */
int orbmi_sim3_ransac_batch(orbmi_matcher* m, int nsolvers, const orbmi_sim3_problem* problems,
                            orbmi_sim3_hypotheses* results);
/* SetRansacParameters' iteration count (:125-135); 0 when n < min_inliers.  Host only. */
int orbmi_sim3_iterations(int n, int min_inliers, double probability, int max_iterations, int* out);
/* The minimal sets of :167-185 (draw, swap with the back, pop; three times) from the library's
 * counter-based generator (csrc/sim3_horn.h): out = iterations x 3.  Host only. */
int orbmi_sim3_sample_triples(uint64_t seed, int solver, int n, int iterations, int32_t* out);
/* mvnMaxError's entry for one level (:87-88): (size_t)(9.210 * sigma2).  Host only. */
int orbmi_sim3_max_error(float sigma2, int32_t* out);

/* ---- LoopClosing::ComputeSim3: ORBmatcher::SearchBySim3 ------------------------------ */

/* ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th) (src/ORBmatcher.cc:
 * 1285-1525): KF1's map points searched in KF2 and KF2's in KF1 under the Sim3 (s12, R12, t12:
 * camera 2 -> camera 1; R12 = 9 floats row-major, t12 = 3 floats, host memory), then the mutual
 * agreement check.  mps1 / mps2: one orbmi_mappoint per keypoint slot of KF1 / KF2
 * (GetMapPointMatches), has_mp1 / has_mp2[i] = GetMapPoint(i) != NULL.  match12 (KF1.n entries,
 * read and written) on entry: -1 = vpMatches12[i] NULL, >= 0 = vpMatches12[i]->
 * GetIndexInKeyFrame(pKF2), -2 = matched to a point without an index in KF2; on exit the new
 * matches are added (match12[i1] = the KF2 slot whose point vpMatches12[i1] becomes).  *nfound =
 * the return value.  vn_match1 (KF1.n) / vn_match2 (KF2.n): vnMatch1 / vnMatch2 before the
 * agreement check, optional (NULL).  Both directions project with KF1's fx, fy, cx, cy, as the
 * reference does (:1289-1292 used at :1363 and :1447); the keyframes' poses are host memory.
 * ORBMI_E_UNSUPPORTED above 16384 keypoints, as orbmi_fuse_search. */
int orbmi_search_by_sim3(orbmi_matcher* m, const orbmi_frame_view* KF1, const orbmi_mappoint* mps1,
                         const uint8_t* has_mp1, const orbmi_frame_view* KF2, const orbmi_mappoint* mps2,
                         const uint8_t* has_mp2, float s12, const float* R12, const float* t12, float th,
                         int32_t* match12, int* nfound, int32_t* vn_match1, int32_t* vn_match2);

/* ---- LoopClosing::ComputeSim3: ORBmatcher::SearchByProjection(KF, Scw) --------------- */

/* ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) (src/ORBmatcher.cc:359-479):
 * the n points of mps (vpPoints, the loop keyframe's neighbourhood) projected into KF under the
 * Sim3 Scw (rows 0-2 of [sRcw | t], 12 floats row-major, host memory) and matched to its
 * keypoints.  matched (KF.n entries, host memory, read and written) codes vpMatched: -1 = NULL,
 * >= 0 = the index in mps of the matched point, -2 = a point that is not in mps; a point already
 * in it is skipped (spAlreadyFound), an occupied keypoint is never taken, and a keypoint taken by
 * an earlier point of the list is skipped by later ones, as in the reference's loop.  *nmatches =
 * the return value.  The pose of KF is not read.  ORBMI_E_ARG: an entry of matched outside
 * [-2, n); ORBMI_E_UNSUPPORTED above 16384 keypoints, as orbmi_fuse_search. */
int orbmi_search_by_projection_sim3(orbmi_matcher* m, const orbmi_frame_view* KF, const float* Scw,
                                    const orbmi_mappoint* mps, int n, int32_t* matched, float th, int* nmatches);

/* ---- LoopClosing::SearchAndFuse: ORBmatcher::Fuse(KF, Scw) --------------------------- */

/* ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (src/ORBmatcher.cc:1139-1269), its
 * search, for the nkf keyframes of LoopClosing::SearchAndFuse in one launch: the same n_mp points
 * (vpPoints, the loop map points) projected into keyframe kfs[k] under its own Sim3
 * Scw[12 k .. 12 k + 11] (rows 0-2 of [sRcw | t], row-major, host memory) and compared with its
 * keypoints.  in_kf (nkf x n_mp, may be NULL): in_kf[k * n_mp + i] = vpPoints[i]->IsInKeyFrame(
 * kfs[k]) (spAlreadyFound); isBad() as ORBMI_MP_BAD.  best_idx[k * n_mp + i] = the keypoint of
 * least descriptor distance in the window (the first in the reference's visit order on ties) when
 * that distance is <= TH_LOW = 50, else -1; best_dist[k * n_mp + i] = that distance, 256 without
 * a candidate (orbmi_fuse_search's convention).  Unlike orbmi_fuse_search there is no chi2 gate
 * on the reprojection error; unlike orbmi_search_by_projection_sim3 a keypoint that already holds
 * a map point is a candidate and two points may choose one keypoint.  nfused[k] (host, may be
 * NULL) = the points of keyframe k with best_idx >= 0.  The keyframes' poses are not read.  The
 * map updates (:1247-1266) are the caller's replay of best_idx in list order.
 * ORBMI_E_ARG: a NULL array that is needed, a negative count, Scw in device memory, or an Scw
 * whose first row has norm 0 or is not finite -- checked before anything is launched or written.
 * nkf == 0 or n_mp == 0: ORBMI_OK, nothing launched or written.  ORBMI_E_UNSUPPORTED above 16384
 * keypoints, as orbmi_fuse_search. */
int orbmi_fuse_sim3_search_batch(orbmi_matcher* m, int nkf, const orbmi_frame_view* kfs, const float* Scw,
                                 const orbmi_mappoint* mps, const uint8_t* in_kf, int n_mp, float th,
                                 int32_t* best_idx, int32_t* best_dist, int* nfused);

/* ---- LoopClosing::ComputeSim3: Optimizer::OptimizeSim3 ------------------------------- */

/* One OptimizeSim3 problem after the reference's assembly loop (src/Optimizer.cc:1198-1281): the n
 * kept correspondences.  x3d_c1 / x3d_c2 (n x 3): the points in their own camera frames, computed
 * in float as R1w * P3D1w + t1w / R2w * P3D2w + t2w; obs1 / obs2 (n x 2): kpUn.pt of either
 * keyframe; inv_sigma2_1 / 2 (n): mvInvLevelSigma2[kpUn.octave] of either side; k1 / k2 = fx fy cx
 * cy of pKF1->mK / pKF2->mK; th2 and fix_scale the arguments; R12, t12, s12 the initial estimate
 * as g2o::Sim3(Matrix3d, Vector3d, double) takes it.  The arrays may be host or device memory. */
typedef struct orbmi_sim3_opt_problem {
    int32_t n;
    const float* x3d_c1;
    const float* x3d_c2;
    const float* obs1;
    const float* obs2;
    const float* inv_sigma2_1;
    const float* inv_sigma2_2;
    float k1[4], k2[4];
    float th2;
    int32_t fix_scale;
    float R12[9], t12[3], s12;
} orbmi_sim3_opt_problem;

/* g2oS12 on return: q (x y z w), t, s; sR / t_f as Converter::toCvMat(g2o::Sim3) rounds them to
 * float.  n_in = the return value (0 on the early return at nCorrespondences - nBad < 10, where
 * the transform is the one passed in), n_bad = nBad of the first chi2 pass, iterations = the
 * Levenberg iterations either optimize() ran.  inlier (n, host or device memory, required when
 * n > 0): 0 where the reference nulls vpMatches1; chi2 (n x 2, optional): e12 / e21's chi2 as
 * last tested. */
typedef struct orbmi_sim3_opt_result {
    double q[4], t[3], s;
    float sR[9], t_f[3];
    int32_t n_in, n_bad;
    int32_t iterations[2];
    uint8_t* inlier;
    double* chi2;
} orbmi_sim3_opt_result;

/* Optimizer::OptimizeSim3 (src/Optimizer.cc:1145-1347) for `nproblems` independent problems in one
 * launch on the matcher handle's stream, one workgroup each: optimize(5), the chi2 pass,
 * optimize(5 or 10) with the Huber kernels still on, the second chi2 pass; numeric Jacobians as
 * BaseBinaryEdge::linearizeOplus computes them.  The candidate loop of LoopClosing::ComputeSim3
 * (src/LoopClosing.cc:399-420) takes the first problem in order with n_in >= 20.  A pair whose
 * chi2 is NaN counts as an outlier, so a non-finite estimate returns n_in = 0.  ORBMI_E_ARG before
 * anything is launched: a NULL table, n < 0, a NULL array of a problem with n > 0. */
int orbmi_optimize_sim3_batch(orbmi_matcher* m, int nproblems, const orbmi_sim3_opt_problem* problems,
                              orbmi_sim3_opt_result* results);

/* ---- LoopClosing::DetectLoop: the KeyFrameDatabase ----------------------------------- */

/* KeyFrameDatabase (src/KeyFrameDatabase.cc:33-197) restated forward: instead of the inverted
 * file (one std::list<KeyFrame*> per word) every keyframe's BowVector sits in a slot of one
 * device arena, word ids ascending, and a query intersects the query vector with every indexed
 * slot at once.  Slots are numbered in the order of orbmi_kfdb_store.  `scoring` is DBoW2's
 * ScoringType (BowVector.h:45-53): L1_NORM (0) and L2_NORM (1), else ORBMI_E_UNSUPPORTED.
 * max_keyframes slots and max_words_total words are allocated here; a store beyond either
 * returns ORBMI_E_CAP.  Keyframe ids are in [0, 2^24).  Calls on one handle are serialised. */
typedef struct orbmi_kfdb orbmi_kfdb;
int orbmi_kfdb_create(int device, int scoring, int max_keyframes, int max_words_total, orbmi_kfdb** out);
void orbmi_kfdb_destroy(orbmi_kfdb* db);
/* KeyFrameDatabase::clear (:69-73) and the stored vectors with it: no slot is left. */
int orbmi_kfdb_clear(orbmi_kfdb* db);
/* Copy keyframe kf_id's mBowVec (n words ascending, n <= 8192, host or device arrays) into the
 * arena.  A host vector that is not strictly ascending returns ORBMI_E_ARG; for a device vector
 * (orbmi_transform's device outputs, ready on the device when the call is made) ascending order
 * is a precondition: a violation gives wrong counts, never an access outside the vector.  An id
 * stored before returns ORBMI_E_STATE.  The keyframe is not indexed yet. */
int orbmi_kfdb_store(orbmi_kfdb* db, int32_t kf_id, const uint32_t* word, const double* value, int n);
/* KeyFrameDatabase::add (:40-46) / erase (:48-67) of a stored keyframe (unknown id: ORBMI_E_ARG).
 * add gives the keyframe the next value of the handle's add counter: its position in every list
 * of the reference's inverted file (add appends, erase keeps the others' order).  Adding an
 * indexed keyframe returns ORBMI_E_STATE (the reference would list it twice); erasing one that is
 * not indexed does nothing.  The stored vector stays after erase, for orbmi_kfdb_score. */
int orbmi_kfdb_add(orbmi_kfdb* db, int32_t kf_id);
int orbmi_kfdb_erase(orbmi_kfdb* db, int32_t kf_id);
/* out_score[i] = mpVoc->score(query, mBowVec of kf_ids[i]) (L1Scoring / L2Scoring::score,
 * Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-120) in double, the reference's sum term by term in
 * ascending word order: DetectLoop's minScore loop (src/LoopClosing.cc:126-140).  Any stored id,
 * indexed or not; an unknown id returns ORBMI_E_ARG.  The query (nq <= 8192 words ascending) may
 * be host or device memory, kf_ids and out_score are host memory. */
int orbmi_kfdb_score(orbmi_kfdb* db, const uint32_t* q_word, const double* q_value, int nq, const int32_t* kf_ids,
                     int n, double* out_score);

/* One query's per-slot result (host arrays of max_keyframes entries each, any may be NULL). */
typedef struct orbmi_kfdb_query_result {
    int32_t n_slots;       /* out: slots in use                                                   */
    int32_t max_common;    /* out: maxCommonWords (:113-118)                                      */
    int32_t min_common;    /* out: (int)(maxCommonWords * 0.8f) (:120)                            */
    int32_t* kf_id;        /* the slot's keyframe                                                 */
    int32_t* common;       /* mnLoopWords; 0: not indexed, connected, or nothing shared           */
    uint32_t* first_word;  /* the smallest shared word id (0xFFFFFFFF where common = 0)           */
    uint64_t* add_seq;     /* the slot's add counter value                                        */
    double* score;         /* mpVoc->score where common > min_common (:129-133), 0 elsewhere      */
} orbmi_kfdb_query_result;

/* The device part of KeyFrameDatabase::DetectLoopCandidates (:76-139) for the query vector of
 * pKF: connected_ids = pKF->GetConnectedKeyFrames() (host memory; ids without a slot are
 * ignored).  lKFsSharingWords is the slots with common > 0 in ascending (first_word, add_seq). */
int orbmi_kfdb_query(orbmi_kfdb* db, const uint32_t* q_word, const double* q_value, int nq,
                     const int32_t* connected_ids, int n_connected, orbmi_kfdb_query_result* out);

/* KeyFrameDatabase::DetectLoopCandidates(pKF, minScore) (:76-197): the query above, then on the
 * host the minScore filter, the accumulation over each survivor's GetBestCovisibilityKeyFrames(10)
 * and the 0.75 * bestAccScore cut (:141-196).  The covisibility graph is the caller's:
 * best_covis_ids[best_covis_off[k] .. best_covis_off[k + 1]) = GetBestCovisibilityKeyFrames(10)
 * of keyframe id k in its order, for k < n_covis_kf (a keyframe past the table has none).
 * out_ids (capacity out_capacity) receives vpLoopCandidates in the reference's order, *n_out
 * their number; more than out_capacity returns ORBMI_E_CAP with *n_out = the number needed. */
int orbmi_detect_loop_candidates(orbmi_kfdb* db, const uint32_t* q_word, const double* q_value, int nq,
                                 float min_score, const int32_t* connected_ids, int n_connected,
                                 const int32_t* best_covis_off, const int32_t* best_covis_ids, int n_covis_kf,
                                 int32_t* out_ids, int out_capacity, int* n_out);

/* ---- LoopClosing::CorrectLoop: Optimizer::OptimizeEssentialGraph --------------------- */

/* A Sim3 here is 8 doubles: the rotation q (x y z w, Eigen's coefficient order), t, s. */

/* The graph OptimizeEssentialGraph reads, as host arrays indexed by keyframe id (n_ids =
 * nMaxKFid + 1; ids may have gaps: live[id] = 0).  Tcw: 4x4 row-major float per id; parent: the
 * spanning-tree parent or -1; loop_* / cov_* / lc_*: GetLoopEdges, GetCovisiblesByWeight(100) (in
 * that function's order) and LoopConnections as CSR over the ids (off has n_ids + 1 entries),
 * lc_weight the GetWeight of each listed pair; corrected / noncorrected: the CorrectedSim3 and
 * NonCorrectedSim3 maps as (id, Sim3) lists; loop_id / cur_id: pLoopKF and pCurKF. */
typedef struct orbmi_essgraph_input {
    int32_t n_ids;
    const uint8_t* live;
    const float* Tcw;
    const int32_t* parent;
    const int32_t* loop_off;
    const int32_t* loop_ids;
    const int32_t* cov_off;
    const int32_t* cov_ids;
    int32_t n_corrected;
    const int32_t* corrected_ids;
    const double* corrected;
    int32_t n_noncorrected;
    const int32_t* noncorrected_ids;
    const double* noncorrected;
    const int32_t* lc_off;
    const int32_t* lc_ids;
    const int32_t* lc_weight;
    int32_t loop_id, cur_id;
} orbmi_essgraph_input;

/* The edge list of OptimizeEssentialGraph (src/Optimizer.cc:862-1053), on the host: vScw (n_ids x
 * 8; the identity where no keyframe lives) = the corrected Sim3 where there is one, else
 * Sim3(Rcw, tcw, 1); then the LoopConnections edges ((i, j) skipped when (i != cur || j != loop)
 * and weight < 100, every listed direction its own edge), then per keyframe the parent edge, the
 * loop edges to a smaller id, and the covisibility edges to a smaller id that is not the parent,
 * a child, a loop-edge partner or a pair the LoopConnections inserted.  v0 = i, v1 = j (keyframe
 * ids), measurement = Sjw * Swi with NonCorrectedSim3 taking precedence on the normal edges.
 * Wherever the reference iterates a container keyed by KeyFrame* the order here is ascending
 * keyframe id.  At most n_live + the three CSR lengths edges; more than max_edges returns
 * ORBMI_E_CAP with *n_edges = the number needed.  ORBMI_E_ARG: a NULL array, an id out of range
 * or naming a keyframe that does not live, offsets that do not ascend. */
int orbmi_essential_graph_edges(const orbmi_essgraph_input* graph, int max_edges, int32_t* v0, int32_t* v1,
                                double* measurements, double* vScw, int* n_edges);

/* One pose graph: n_vertices VertexSim3Expmap (vertices: n_vertices x 8, the initial estimates),
 * vertex `fixed` held, n_edges EdgeSim3 with identity information between vertices v0[e] and
 * v1[e] (indices into `vertices`), measurements n_edges x 8.  iterations <= 32 (the reference:
 * 20).  profile != 0 brackets the phases with HIP events (and waits for each). */
typedef struct orbmi_essgraph_problem {
    int32_t n_vertices;
    const double* vertices;
    int32_t fixed;
    int32_t n_edges;
    const int32_t* v0;
    const int32_t* v1;
    const double* measurements;
    int32_t fix_scale;
    int32_t iterations;
    int32_t profile;
} orbmi_essgraph_problem;

#define ORBMI_EG_TERMINATE 1    /* Levenberg stopped by a rule of its own (else: ran to the count) */
#define ORBMI_EG_SOLVE_FAILED 2 /* a damped solve met a pivot that is not a positive finite number */
#define ORBMI_EG_REJECTED 4     /* a trial was rejected and the estimates restored                 */

/* vertices (n_vertices x 8, host memory): the optimised estimates; chi2 before the first and after
 * the last accepted step; iterations = outer Levenberg iterations, trials[k] the solves of
 * iteration k; status = ORBMI_EG_* or'ed; phase_ms: linearisation, assembly, factor + solve,
 * update, summed over the call (profile only). */
typedef struct orbmi_essgraph_result {
    double* vertices;
    double chi2_before, chi2_after;
    int32_t iterations;
    int32_t status;
    int32_t trials[32];
    float phase_ms[4];
} orbmi_essgraph_result;

/* optimizer.optimize(iterations) of OptimizeEssentialGraph (src/Optimizer.cc:1055-1057) on the
 * matcher handle's stream: numeric Jacobians as BaseBinaryEdge::linearizeOplus computes them, H
 * and b gathered in edge order, OptimizationAlgorithmLevenberg::solve with setUserLambdaInit(1e-16)
 * and a block-sparse LDL^T in a minimum-degree order; the Levenberg decisions are taken on the
 * host from one small read-back per trial.  A vertex no edge names is returned as given, and a
 * graph with nothing to optimise returns 0 iterations with ORBMI_EG_TERMINATE.  Every loop is
 * bounded by the reference's counts, so non-finite input terminates too (its status carries
 * ORBMI_EG_SOLVE_FAILED).  ORBMI_E_ARG before anything is launched: a NULL array, n_vertices < 1,
 * `fixed` or an edge's vertex out of range, v0 == v1, iterations outside [0, 32]. */
int orbmi_optimize_essential_graph(orbmi_matcher* m, const orbmi_essgraph_problem* problem, orbmi_essgraph_result* result);

/* The two arithmetic loops of CorrectLoop (src/LoopClosing.cc:607-628) and the tail of
 * OptimizeEssentialGraph (src/Optimizer.cc:1069-1114): out_points[i] (float) =
 * Swr_corrected[ref[i]].map(Srw[ref[i]].map((double)points[i])), ref[i] in [0, n_ref) naming the
 * point's reference keyframe in the two Sim3 tables (n_ref x 8 each); out_tcw[k] (4x4 row-major
 * float) = [R | t * (1. / s)] of poses[k] (n_poses x 8).  Host arrays.  UpdateNormalAndDepth stays
 * the caller's.  ORBMI_E_ARG before the launch: a NULL array, a ref outside the tables. */
int orbmi_correct_points_sim3(orbmi_matcher* m, int n_points, const float* points, const int32_t* ref, int n_ref,
                              const double* Srw, const double* Swr_corrected, float* out_points, int n_poses,
                              const double* poses, float* out_tcw);

/* ---- per-stage timing (HIP events on the handle's stream) ---------------------------- */

/* Kernel stages of one handle; each is a single kernel launch (resize: one per level). */
typedef enum orbmi_stage {
    ORBMI_STAGE_PYR_LEVEL0 = 0,
    ORBMI_STAGE_PYR_RESIZE = 1,
    ORBMI_STAGE_FAST = 2,
    ORBMI_STAGE_OCTREE = 3,
    ORBMI_STAGE_DESCRIBE = 4,
    ORBMI_STAGE_STEREO_ROWS = 5,
    ORBMI_STAGE_STEREO_MATCH = 6,
    ORBMI_STAGE_STEREO_FILTER = 7,
    ORBMI_STAGE_BLUR = 8,          /* GaussianBlur 7x7 of every level (ORBextractor.cc:1085-1086) */
    ORBMI_NUM_STAGES = 16
} orbmi_stage;

/* Bracket every launch of the stages in `stage_mask` (bit s = stage s) with HIP events. */
int orbmi_set_profiling(orbmi_extractor* h, unsigned stage_mask);
/* Synchronise, then add the elapsed device time (ms) and launch count of every bracketed
 * launch since the last call into ms[s], launches[s] (ORBMI_NUM_STAGES entries each). */
int orbmi_read_profile(orbmi_extractor* h, double* ms, long long* launches);

#ifdef __cplusplus
}
#endif
#endif /* ORBMI_H */
