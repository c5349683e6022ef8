// Frame construction of the native SLAM loop (slam.h): the device slots, the frame worker,
// stereo and RGB-D extraction, BoW (synchronous and asynchronous) and the keyframes' HBM copies.
#include "slam.h"

void orbmi_slam::frame_worker_run() {
    (void)hipSetDevice(device);  // the current device is per thread
    std::unique_lock<std::mutex> g(fw.mtx);
    for (;;) {
        fw.cv.wait(g, [this] { return fw.job || fw.quit; });
        if (fw.quit) return;
        fw.job = false;
        g.unlock();
        const int rc = frame_enqueue(fw.L, fw.R, fw.rows, fw.cols, fw.step, fw.slot);
        g.lock();
        fw.rc = rc;
        fw.busy = false;
        fw.cv.notify_all();
    }
}

void orbmi_slam::frame_post(const uint8_t* L, const uint8_t* R, int rows, int cols, size_t step, int slot) {
    std::lock_guard<std::mutex> g(fw.mtx);
    if (!fw.th.joinable()) fw.th = std::thread([this] { frame_worker_run(); });
    fw.L = L; fw.R = R; fw.rows = rows; fw.cols = cols; fw.step = step; fw.slot = slot;
    fw.job = true;
    fw.busy = true;
    fw.rc = ORBMI_OK;
    fw.cv.notify_all();
}

int orbmi_slam::frame_join() {  // the posted enqueue finished; its status
    std::unique_lock<std::mutex> g(fw.mtx);
    fw.cv.wait(g, [this] { return !fw.busy; });
    const int rc = fw.rc;
    fw.rc = ORBMI_OK;
    return rc;
}

void orbmi_slam::frame_worker_stop() {
    if (!fw.th.joinable()) return;
    (void)frame_join();
    {
        std::lock_guard<std::mutex> g(fw.mtx);
        fw.quit = true;
        fw.cv.notify_all();
    }
    fw.th.join();
}

// ---- Frame views (include/Frame.h members the matchers read) --------------------------
orbmi_frame_view orbmi_slam::view(const std::vector<orbmi_keypoint>& keys, const std::vector<uint8_t>& desc,
                      const std::vector<float>& ur, const float* tcw) const {
    orbmi_frame_view v{};
    v.n = (int)keys.size();
    v.keys_un = keys.data();
    v.u_right = ur.data();
    v.desc = desc.data();
    v.tcw = tcw;
    v.fx = s.fx; v.fy = s.fy; v.cx = s.cx; v.cy = s.cy; v.bf = s.bf;
    v.mb = s.bf / s.fx;
    v.min_x = bounds[0]; v.max_x = bounds[1]; v.min_y = bounds[2]; v.max_y = bounds[3];
    v.grid_w_inv = 64.f / (bounds[1] - bounds[0]);  // (src/Frame.cc:101-102, 155-156)
    v.grid_h_inv = 48.f / (bounds[3] - bounds[2]);
    v.nlevels = (int)scale_factors.size();
    v.scale_factors = scale_factors.data();
    v.log_scale_factor = log_scale_factor;
    v.n_device = nullptr;
    return v;
}

orbmi_frame_view orbmi_slam::view(const TrackedFrame& f, const float* tcw) const {
    orbmi_frame_view v = view(f.keys, f.desc, f.ur, tcw);
    if (f.dslot >= 0) {  // the frame's arrays in HBM (left item of its slot)
        v.keys_un = dev.kps[f.dslot];
        v.desc = dev.desc[f.dslot];
        v.u_right = dev.ur[f.dslot];
    }
    return v;
}

// the device slots and the pinned read-back buffers, on first use
int orbmi_slam::ensure_slots() {
    if (dev.kps[0]) return ORBMI_OK;
    const int cap = s.n_features + 16 * s.n_levels + 64;
    dev.cap = cap;
    for (int k = 0; k < kSlots; k++) {
        if (hipMalloc((void**)&dev.kps[k], 2 * (size_t)cap * sizeof(orbmi_keypoint)) != hipSuccess ||
            hipMalloc((void**)&dev.desc[k], 2 * (size_t)cap * 32) != hipSuccess ||
            hipMalloc((void**)&dev.cnt[k], 2 * sizeof(int)) != hipSuccess ||
            hipMalloc((void**)&dev.ur[k], 2 * (size_t)cap * sizeof(float)) != hipSuccess ||
            hipMalloc((void**)&dev.dep[k], 2 * (size_t)cap * sizeof(float)) != hipSuccess)
            return ORBMI_E_HIP;
    }
    if (hipHostMalloc((void**)&dev.h_kps, (size_t)cap * sizeof(orbmi_keypoint), hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc((void**)&dev.h_desc, (size_t)cap * 32, hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc((void**)&dev.h_cnt, 2 * sizeof(int), hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc((void**)&dev.h_ur, (size_t)cap * sizeof(float), hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc((void**)&dev.h_dep, (size_t)cap * sizeof(float), hipHostMallocDefault) != hipSuccess)
        return ORBMI_E_HIP;
    return ORBMI_OK;
}

// the device image buffer and its pinned staging, grown to `bytes`
int orbmi_slam::image_buffers(size_t bytes) {
    if (bytes <= dev.img_bytes) return ORBMI_OK;
    if (dev.img) (void)hipFree(dev.img);
    if (dev.h_img) (void)hipHostFree(dev.h_img);
    dev.img = nullptr;
    dev.h_img = nullptr;
    dev.img_bytes = 0;
    if (hipMalloc((void**)&dev.img, bytes) != hipSuccess) return ORBMI_E_HIP;
    if (hipHostMalloc((void**)&dev.h_img, bytes, hipHostMallocDefault) != hipSuccess) return ORBMI_E_HIP;
    dev.img_bytes = bytes;
    return ORBMI_OK;
}

// slot k's left outputs into the pinned mirror, on the extractor's stream (`counts`: 2 for a pair)
int orbmi_slam::read_back(int k, int counts) {
    const int cap = dev.cap;
    if (hipMemcpyAsync(dev.h_cnt, dev.cnt[k], counts * sizeof(int), hipMemcpyDeviceToHost, xstream) != hipSuccess ||
        hipMemcpyAsync(dev.h_kps, dev.kps[k], (size_t)cap * sizeof(orbmi_keypoint), hipMemcpyDeviceToHost, xstream) !=
            hipSuccess ||
        hipMemcpyAsync(dev.h_desc, dev.desc[k], (size_t)cap * 32, hipMemcpyDeviceToHost, xstream) != hipSuccess ||
        hipMemcpyAsync(dev.h_ur, dev.ur[k], (size_t)cap * sizeof(float), hipMemcpyDeviceToHost, xstream) != hipSuccess ||
        hipMemcpyAsync(dev.h_dep, dev.dep[k], (size_t)cap * sizeof(float), hipMemcpyDeviceToHost, xstream) != hipSuccess)
        return ORBMI_E_HIP;
    return ORBMI_OK;
}

// Frame::Frame (stereo, src/Frame.cc:58-100): ORBextractor on both images (one batch on the
// left handle) and ComputeStereoMatches into device slot k, enqueued on the extractor's stream
// with the read-back of the left outputs into pinned memory (frame_collect waits)
int orbmi_slam::frame_enqueue(const uint8_t* L, const uint8_t* R, int rows, int cols, size_t step, int k) {
    if (k < 0 || k >= kSlots) return ORBMI_E_ARG;
    const size_t img = (size_t)rows * cols;
    // a rectifying handle stages the raw pair behind the pair the extractor reads (image_buffers
    // sizes the pinned mirror like the device buffer: of the mirror only the first 2 * img bytes
    // are used, the raw pair's)
    const size_t raw = rectify ? 2 * img : 0;
    SLAM_CHECK(image_buffers(raw + 2 * img));
    SLAM_CHECK(ensure_slots());
    for (int r = 0; r < rows; r++) {
        std::memcpy(dev.h_img + (size_t)r * cols, L + (size_t)r * step, cols);
        std::memcpy(dev.h_img + img + (size_t)r * cols, R + (size_t)r * step, cols);
    }
    if (hipMemcpyAsync(dev.img + raw, dev.h_img, 2 * img, hipMemcpyHostToDevice, xstream) != hipSuccess) return ORBMI_E_HIP;
    if (rectify) {  // cv::remap of both images (Examples/Stereo/stereo_euroc.cc:122-123), one launch
        orbmi::RemapImage im[2];
        for (int e = 0; e < 2; e++)
            im[e] = orbmi::RemapImage{rect[e].d_rec, dev.img + raw + e * img, dev.img + e * img, rows, cols, rows, cols,
                                      (unsigned)cols, (unsigned)cols};
        SLAM_CHECK(orbmi::remap_run(xstream, im, 2));
    }
    const int cap = dev.cap;
    SLAM_CHECK(orbmi_extract_batch_device(left, dev.img, 2, rows, cols, cols, img, dev.kps[k], dev.desc[k], dev.cnt[k],
                                          cap));
    SLAM_CHECK(orbmi_compute_stereo_matches_batch_device(left, s.bf, s.fx, dev.ur[k], dev.dep[k]));
    return read_back(k, 2);
}

// the enqueued extraction's host copies into cf (waits for the extractor's stream)
int orbmi_slam::frame_collect(TrackedFrame& cf, int slot) {
    if (hipStreamSynchronize(xstream) != hipSuccess) return ORBMI_E_HIP;
    const int n = std::min(dev.h_cnt[0], dev.cap);
    cf.keys.assign(dev.h_kps, dev.h_kps + n);
    cf.desc.assign(dev.h_desc, dev.h_desc + (size_t)n * 32);
    cf.ur.assign(dev.h_ur, dev.h_ur + n);
    cf.depth.assign(dev.h_dep, dev.h_dep + n);
    cf.dslot = slot;
    // new keypoints behind a slot's pointers: a grid pinned on an older frame there is stale.
    // Frame::AssignFeaturesToGrid (src/Frame.cc:98) then runs once for the frame, on the
    // tracking stream: its searches (the last-frame search, the retry, SearchLocalPoints)
    // reuse that grid instead of building one each
    SLAM_CHECK(orbmi_matcher_release_grid(matcher));
    const orbmi_frame_view v = view(cf, nullptr);
    return orbmi_matcher_assign_features_to_grid(matcher, &v);
}

int orbmi_slam::frame_stereo(TrackedFrame& cf, const uint8_t* L, const uint8_t* R, int rows, int cols, size_t step) {
    // a pair enqueued ahead and not asked for (a plain call after an ahead one): it shares the
    // pinned read-back buffers, so it is drained and dropped first
    if (dev.ahead.on) {
        dev.ahead.on = false;
        if (hipStreamSynchronize(xstream) != hipSuccess) return ORBMI_E_HIP;
    }
    // the last frame's slot is read by this frame's tracking: extract into another one
    const int slot = free_slot(last_frame.dslot, -1);
    SLAM_CHECK(frame_enqueue(L, R, rows, cols, step, slot));
    return frame_collect(cf, slot);
}

// Frame::Frame (RGB-D, src/Frame.cc:119-171) behind Tracking::GrabImageRGBD's conversions
// (src/Tracking.cc:208-230): the image and the depth map go up once (pinned staging: gray or
// colour image, then the depth rows), cvtColor when the image has channels, ORBextractor as a
// batch of one, UndistortKeyPoints + ComputeStereoFromRGBD in place on the slot's keypoints
// (the slot then holds mvKeysUn, all Tracking reads), and the read-back of frame_enqueue --
// all on the extractor's stream.
int orbmi_slam::frame_rgbd(TrackedFrame& cf, const uint8_t* image, int channels, size_t image_step, const void* depth,
               int depth_type, size_t depth_step, int rows, int cols) {
    const size_t img = (size_t)rows * cols, es = depth_type == ORBMI_DEPTH_U16 ? 2 : 4;
    const size_t in_img = img * channels, in_depth = (in_img + 15) & ~(size_t)15, in_bytes = in_depth + img * es;
    // dev.img: [gray | staged input (image, depth)]; dev.h_img mirrors the staged input
    const size_t o_in = (img + 255) & ~(size_t)255;
    SLAM_CHECK(image_buffers(o_in + in_bytes));
    SLAM_CHECK(ensure_slots());
    const int k = free_slot(last_frame.dslot, -1);  // the last frame's slot is read by this frame's tracking
    const size_t row_bytes = (size_t)cols * channels;
    for (int r = 0; r < rows; r++) {
        std::memcpy(dev.h_img + (size_t)r * row_bytes, image + (size_t)r * image_step, row_bytes);
        std::memcpy(dev.h_img + in_depth + (size_t)r * cols * es, (const uint8_t*)depth + (size_t)r * depth_step,
                    (size_t)cols * es);
    }
    uint8_t* d_in = dev.img + o_in;
    if (hipMemcpyAsync(d_in, dev.h_img, in_bytes, hipMemcpyHostToDevice, xstream) != hipSuccess) return ORBMI_E_HIP;
    const uint8_t* d_gray = d_in;
    if (channels > 1) {
        SLAM_CHECK(orbmi::cvt_gray_run(xstream, d_in, row_bytes, channels, rs.rgb ? 1 : 0, rows, cols, dev.img, cols));
        d_gray = dev.img;
    }
    const int cap = dev.cap;
    SLAM_CHECK(orbmi_extract_batch_device(left, d_gray, 1, rows, cols, cols, img, dev.kps[k], dev.desc[k], dev.cnt[k],
                                          cap));
    SLAM_CHECK(orbmi::rgbd_frame_run(xstream, dev.kps[k], dev.cnt[k], cap, d_in + in_depth, depth_type, cols * es,
                                     rs.depth_map_factor, rows, cols, ucam, s.bf, dev.kps[k], dev.ur[k], dev.dep[k]));
    SLAM_CHECK(read_back(k, 1));
    return frame_collect(cf, k);
}

// orbmi_slam_track_stereo_ahead: the Frame constructor of this pair from the extraction
// enqueued by the previous call when it was for the same pair (same buffers and geometry),
// else now; then the next pair's extraction is enqueued to run while this frame is tracked.
// Extraction depends on the images only, so the frame is the one the plain call builds.
int orbmi_slam::frame_stereo_ahead(TrackedFrame& cf, const uint8_t* L, const uint8_t* R, int rows, int cols, size_t step,
                       const uint8_t* nL, const uint8_t* nR) {
    Dev::Ahead& a = dev.ahead;
    if (a.on && a.L == L && a.R == R && a.rows == rows && a.cols == cols && a.step == step) {
        a.on = false;
        SLAM_CHECK(frame_collect(cf, a.slot));
    } else {
        if (a.on && hipStreamSynchronize(xstream) != hipSuccess) return ORBMI_E_HIP;  // a pair not asked for
        a.on = false;
        SLAM_CHECK(frame_stereo(cf, L, R, rows, cols, step));
    }
    if (nL && nR) {
        // tracking this frame reads cf's slot and the last frame's while the next pair is
        // extracted; the next call then tracks a.slot against cf's
        a.slot = free_slot(cf.dslot, last_frame.dslot);
        if (inline_frame) SLAM_CHECK(frame_enqueue(nL, nR, rows, cols, step, a.slot));
        else frame_post(nL, nR, rows, cols, step, a.slot);  // joined before the call returns
        a.on = true;
        a.L = nL;
        a.R = nR;
        a.rows = rows;
        a.cols = cols;
        a.step = step;
    }
    return ORBMI_OK;
}

// forget the pair enqueued ahead (its extraction drained first)
void orbmi_slam::drop_ahead() {
    if (dev.ahead.on && xstream) (void)hipStreamSynchronize(xstream);
    dev.ahead.on = false;
    dev.ahead.slot = -1;
}

void orbmi_slam::free_dev() {
    frame_worker_stop();
    free_bow_async();
    if (dev.ahead.on && xstream) (void)hipStreamSynchronize(xstream);
    for (int k = 0; k < kSlots; k++) {
        (void)hipFree(dev.kps[k]);
        (void)hipFree(dev.desc[k]);
        (void)hipFree(dev.cnt[k]);
        (void)hipFree(dev.ur[k]);
        (void)hipFree(dev.dep[k]);
    }
    (void)hipFree(dev.img);
    (void)hipHostFree(dev.h_img);
    (void)hipHostFree(dev.h_kps);
    (void)hipHostFree(dev.h_desc);
    (void)hipHostFree(dev.h_cnt);
    (void)hipHostFree(dev.h_ur);
    (void)hipHostFree(dev.h_dep);
    dev = Dev{};
}

// ---- backend operators ------------------------------------------------------------------
int orbmi_slam::compute_bow(const std::vector<uint8_t>& desc, FeatVec& fv) {
    if (!voc) return ORBMI_E_STATE;  // TrackReferenceKeyFrame needs the vocabulary
    const int n = (int)(desc.size() / 32), cap = std::max(n, 1);
    std::vector<uint32_t> word(cap), node(cap);
    std::vector<double> value(cap);
    std::vector<int32_t> off(cap + 1), feat(cap);
    int counts[2] = {0, 0};
    SLAM_CHECK(orbmi_transform(voc, desc.data(), n, nullptr, 4, word.data(), value.data(), node.data(), off.data(),
                               feat.data(), counts));
    const int nn = counts[1];
    fv.words = counts[0];
    fv.node.assign(node.begin(), node.begin() + nn);
    fv.off.assign(off.begin(), off.begin() + nn + 1);
    fv.feat.assign(feat.begin(), feat.begin() + off[nn]);
    fv.valid = true;
    return ORBMI_OK;
}

int orbmi_slam::bow_begin(const uint8_t* d_desc, int n) {
    BowAsync& b = bowa;
    if (n > b.cap) {
        if (b.d) (void)hipFree(b.d);
        if (b.h) (void)hipHostFree(b.h);
        b.d = b.h = nullptr;
        b.cap = 0;
        const int cap = std::max(n, 2048);
        if (hipMalloc((void**)&b.d, (size_t)cap * 12 + bow_tail_bytes(cap)) != hipSuccess) return ORBMI_E_HIP;
        if (hipHostMalloc((void**)&b.h, bow_tail_bytes(cap), hipHostMallocDefault) != hipSuccess) return ORBMI_E_HIP;
        b.cap = cap;
    }
    void* vs = nullptr;
    SLAM_CHECK(orbmi_vocabulary_get_stream(voc, &vs));
    b.stream = (hipStream_t)vs;
    b.n = n;
    const int cap = b.cap;
    double* value = (double*)b.d;
    uint32_t* word = (uint32_t*)(b.d + (size_t)cap * 8);
    uint8_t* tail = b.d + (size_t)cap * 12;
    uint32_t* node = (uint32_t*)tail;
    int32_t* off = (int32_t*)(node + cap);
    int32_t* feat = off + cap + 1;
    int* counts = (int*)(feat + cap);
    SLAM_CHECK(orbmi_transform(voc, d_desc, n, nullptr, 4, word, value, node, off, feat, counts));
    if (hipMemcpyAsync(b.h, tail, bow_tail_bytes(cap), hipMemcpyDeviceToHost, b.stream) != hipSuccess)
        return ORBMI_E_HIP;
    b.pending = true;
    return ORBMI_OK;
}

int orbmi_slam::bow_end(FeatVec& fv) {
    BowAsync& b = bowa;
    if (!b.pending) return ORBMI_E_STATE;
    b.pending = false;
    if (hipStreamSynchronize(b.stream) != hipSuccess) return ORBMI_E_HIP;
    const int cap = b.cap;
    const uint32_t* node = (const uint32_t*)b.h;
    const int32_t* off = (const int32_t*)(node + cap);
    const int32_t* feat = off + cap + 1;
    const int* counts = (const int*)(feat + cap);
    const int nn = counts[1];
    if (nn < 0 || nn > b.n || off[nn] > b.n) return ORBMI_E_STATE;
    fv.words = counts[0];
    fv.node.assign(node, node + nn);
    fv.off.assign(off, off + nn + 1);
    fv.feat.assign(feat, feat + off[nn]);
    fv.valid = true;
    return ORBMI_OK;
}

void orbmi_slam::free_bow_async() {
    if (bowa.pending && bowa.stream) (void)hipStreamSynchronize(bowa.stream);
    if (bowa.d) (void)hipFree(bowa.d);
    if (bowa.h) (void)hipHostFree(bowa.h);
    bowa = BowAsync{};
}

// ---- keyframes and map points -------------------------------------------------------------
int orbmi_slam::new_keyframe(const TrackedFrame& cf) {
    KeyFrame kf;
    kf.id = (int)kfs.size();
    kf.frame_id = cf.id;
    kf.ts = cf.ts;
    kf.tcw = cf.tcw;
    kf.keys = cf.keys;
    kf.desc = cf.desc;
    kf.ur = cf.ur;
    kf.depth = cf.depth;
    kf.mps = cf.mps;
    kf.fv = cf.fv;
    // the keyframe's arrays in HBM, copied once (from the frame's device slot when it has one)
    const size_t n = kf.keys.size(), bk = n * sizeof(orbmi_keypoint), bd = n * 32, bu = n * sizeof(float);
    std::vector<float> dc(2 * n);  // depth, then the stereo parallax table
    const float mb = s.bf / s.fx;
    for (size_t i = 0; i < n; i++) {
        dc[i] = kf.depth[i];
        dc[n + i] = kf.ur[i] >= 0 ? orbmi::tri::stereo_parallax_cos(mb, kf.depth[i]) : 0.f;
    }
    if (n > 0 && hipMalloc((void**)&kf.d_block, bk + bd + 3 * bu) == hipSuccess) {
        const bool dslot = cf.dslot >= 0;
        const hipMemcpyKind kind = dslot ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
        const void* sk = dslot ? (const void*)dev.kps[cf.dslot] : (const void*)kf.keys.data();
        const void* sd = dslot ? (const void*)dev.desc[cf.dslot] : (const void*)kf.desc.data();
        const void* su = dslot ? (const void*)dev.ur[cf.dslot] : (const void*)kf.ur.data();
        // four copies in stream order on the tracking stream (idle here: the frame's stages
        // were read back), one wait -- instead of four blocking copies
        const hipStream_t cs = tstream;
        if (hipMemcpyAsync(kf.d_block, sk, bk, kind, cs) == hipSuccess &&
            hipMemcpyAsync(kf.d_block + bk, sd, bd, kind, cs) == hipSuccess &&
            hipMemcpyAsync(kf.d_block + bk + bd, su, bu, kind, cs) == hipSuccess &&
            hipMemcpyAsync(kf.d_block + bk + bd + bu, dc.data(), 2 * bu, hipMemcpyHostToDevice, cs) == hipSuccess &&
            hipStreamSynchronize(cs) == hipSuccess) {
            kf.d_keys = (const orbmi_keypoint*)kf.d_block;
            kf.d_desc = kf.d_block + bk;
            kf.d_ur = (const float*)(kf.d_block + bk + bd);
            kf.d_depth = (const float*)(kf.d_block + bk + bd + bu);
            kf.d_cos = (const float*)(kf.d_block + bk + bd + 2 * bu);
        }
    }
    kfs.push_back(std::move(kf));
    return (int)kfs.size() - 1;
}

// KeyFrame view for the searches: its HBM copy when there is one; tcw points at `tcw_copy`
// (the caller's copy: the keyframe's own pose may move while the map lock is released)
orbmi_frame_view orbmi_slam::kf_view(const KeyFrame& kf, const float* tcw) const {
    orbmi_frame_view v = view(kf.keys, kf.desc, kf.ur, tcw);
    if (kf.d_keys) {
        v.keys_un = kf.d_keys;
        v.desc = kf.d_desc;
        v.u_right = kf.d_ur;
    }
    return v;
}
