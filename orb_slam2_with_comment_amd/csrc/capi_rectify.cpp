// C ABI of stereo rectification (include/orbmi.h): the host map builder, the rectifier handle
// and cv::remap of one image or a pair.
#include <new>

#include "capi_stage.h"
#include "rectifier.h"

// The handle's stream and staging arena are a matcher's (capi_stage.h stages through it); none
// of the matcher's search buffers is ever allocated.
struct orbmi_rectifier {
    orbmi_matcher st;
    orbmi::RectifyTable tab;
    hipEvent_t ev_in = nullptr, ev_out = nullptr;  // the caller's stream handed over to the handle's, and back
};

namespace {

using orbmi::RemapImage;
using orbmi::Stage;

struct Side {
    orbmi_rectifier* h;
    const uint8_t* src;
    int src_rows, src_cols;
    size_t src_step;
    uint8_t* dst;
    size_t dst_step;
};

bool side_ok(const Side& s) {
    return s.h && s.h->tab.d_rec && orbmi::remap_source_ok(s.src, s.src_rows, s.src_cols, s.src_step) && s.dst &&
           s.dst_step >= (size_t)s.h->tab.cols && s.dst_step <= 0xFFFFFFFFu;
}

// bytes of a pitched image from its first to its last pixel
size_t span(int rows, int cols, size_t step) { return (size_t)(rows - 1) * step + (size_t)cols; }

RemapImage stage_side(Stage& s, const Side& d) {
    const orbmi::RectifyTable& t = d.h->tab;
    RemapImage I{};
    I.rec = t.d_rec;
    I.src = s.in(d.src, span(d.src_rows, d.src_cols, d.src_step));
    // a host destination with padded rows goes up first: the read-back covers whole rows, and the
    // padding keeps the caller's bytes
    const size_t n = span(t.rows, t.cols, d.dst_step);
    I.dst = d.dst_step == (size_t)t.cols ? s.out(d.dst, n) : s.inout(d.dst, n);
    I.src_rows = d.src_rows; I.src_cols = d.src_cols;
    I.dst_rows = t.rows; I.dst_cols = t.cols;
    I.src_step = (unsigned)d.src_step; I.dst_step = (unsigned)d.dst_step;
    return I;
}

// n sides on sides[0]'s stream.  stream (hipStream_t of the caller, may be NULL): the inputs are
// read after the work enqueued on it so far, and it waits for the outputs
int remap_sides(const Side* sides, int n, void* stream) {
    for (int k = 0; k < n; k++)
        if (!side_ok(sides[k]) || sides[k].h->st.m.device != sides[0].h->st.m.device) return ORBMI_E_ARG;
    orbmi_rectifier* h = sides[0].h;
    Stage s(&h->st);
    if (s.rc) return s.rc;
    hipStream_t user = (hipStream_t)stream;
    if (user) {
        ORBMI_HIP(hipEventRecord(h->ev_in, user));
        ORBMI_HIP(hipStreamWaitEvent(s.m.ls(), h->ev_in, 0));
    }
    RemapImage im[2];
    for (int k = 0; k < n; k++) im[k] = stage_side(s, sides[k]);
    if (s.rc) return s.rc;
    int rc = orbmi::remap_run(s.m.ls(), im, n);
    if (rc) return rc;
    if ((rc = s.finish())) return rc;
    if (user) {
        ORBMI_HIP(hipEventRecord(h->ev_out, s.m.ls()));
        ORBMI_HIP(hipStreamWaitEvent(user, h->ev_out, 0));
    } else {
        ORBMI_HIP(hipStreamSynchronize(s.m.ls()));  // no stream to order device outputs on: they are ready on return
    }
    return ORBMI_OK;
}

}  // namespace

extern "C" {

int orbmi_init_undistort_rectify_map(const orbmi_rectify_camera* camera, float* map1, float* map2) {
    return orbmi::rectify::init_undistort_rectify_map(camera, map1, map2);
}

int orbmi_rectifier_create(int device, const float* map1, const float* map2, int rows, int cols, orbmi_rectifier** out) {
    if (!out) return ORBMI_E_ARG;
    *out = nullptr;
    if (!map1 || !map2 || rows <= 0 || cols <= 0) return ORBMI_E_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return ORBMI_E_HIP;
    orbmi_rectifier* h = new (std::nothrow) orbmi_rectifier();
    if (!h) return ORBMI_E_ARG;
    h->st.m.device = device;
    int rc = ORBMI_OK;
    if (hipSetDevice(device) != hipSuccess || orbmi::stream_create(&h->st.m.stream, "EXTRACTOR") != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_in, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_out, hipEventDisableTiming) != hipSuccess)
        rc = ORBMI_E_HIP;
    if (!rc) rc = h->tab.upload(map1, map2, rows, cols);
    if (rc) {
        orbmi_rectifier_destroy(h);
        return rc;
    }
    *out = h;
    return ORBMI_OK;
}

void orbmi_rectifier_destroy(orbmi_rectifier* h) {
    if (!h) return;
    h->st.m.release();  // waits for the stream, frees the arena
    h->tab.release();
    if (h->ev_in) (void)hipEventDestroy(h->ev_in);
    if (h->ev_out) (void)hipEventDestroy(h->ev_out);
    delete h;
}

int orbmi_remap(orbmi_rectifier* h, const uint8_t* src, int src_rows, int src_cols, size_t src_step, uint8_t* dst,
                size_t dst_step, void* stream) {
    const Side s{h, src, src_rows, src_cols, src_step, dst, dst_step};
    return remap_sides(&s, 1, stream);
}

int orbmi_remap_pair(orbmi_rectifier* left, orbmi_rectifier* right, const uint8_t* src_left, const uint8_t* src_right,
                     int src_rows, int src_cols, size_t src_step, uint8_t* dst_left, uint8_t* dst_right, size_t dst_step,
                     void* stream) {
    const Side s[2] = {{left, src_left, src_rows, src_cols, src_step, dst_left, dst_step},
                       {right, src_right, src_rows, src_cols, src_step, dst_right, dst_step}};
    return remap_sides(s, 2, stream);
}

}  // extern "C"
