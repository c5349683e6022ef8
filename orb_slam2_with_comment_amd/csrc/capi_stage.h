// The staging scope of one call into the matcher's C interface (capi_match.cpp, capi_mapping.cpp,
// capi_loop.cpp).  Host only.  Inputs and outputs may live in host or device memory; host arrays
// go through the handle's arena (matcher_arena.cpp) and its pinned mirror.
#pragma once
#include <algorithm>
#include <initializer_list>
#include <vector>

#include "matcher.h"

struct orbmi_matcher {
    orbmi::Matcher m;
};

namespace orbmi {

// Copy a small array to the host wherever it lives (a device array: one blocking copy).
template <class T>
int to_host(const T* p, size_t n, T* out) {
    if (on_device(p)) ORBMI_HIP(hipMemcpy(out, p, n * sizeof(T), hipMemcpyDeviceToHost));
    else memcpy(out, p, n * sizeof(T));
    return ORBMI_OK;
}

// Total rows of a CSR offset array of n + 1 entries: its last entry, wherever it lives.
inline int csr_total(const int32_t* off, int n, int* total) { return to_host(off + n, 1, total); }

// Constructed at the top of an entry, after its argument checks.  The first failure (allocation,
// copy, argument) sticks in rc: every later call is a no-op that returns null, so an entry tests
// rc once before its launch and cannot launch with a null staged pointer.  A call that returns
// before finish() leaves nothing pending in the arena: the destructor drops the upload range
// and the read-backs.
struct Stage {
    Matcher& m;
    int rc = ORBMI_OK;
    bool done = false;
    struct Out { void* user; void* dev; size_t bytes; };
    std::vector<Out> outs;

    // reset = false: an entry that takes device arrays only, stages nothing and leaves the arena
    // and what is pending in it alone (the slot grids: built beside another call's staging)
    explicit Stage(orbmi_matcher* h, bool reset = true) : m(h->m), done(!reset) {
        if (hipSetDevice(m.device) != hipSuccess) rc = ORBMI_E_HIP;
        else if (reset) m.arena_reset();
    }
    ~Stage() {
        if (!done) { m.up = Matcher::PendUp{}; m.pend.clear(); }
    }
    Stage(const Stage&) = delete;
    Stage& operator=(const Stage&) = delete;

    int fail(int code) {
        if (!rc) rc = code;
        return rc;
    }

    // Uninitialised device memory of this call (at least one element).
    template <class T>
    T* scratch(size_t n) {
        if (rc) return nullptr;
        T* d = (T*)m.stage(std::max(n, (size_t)1) * sizeof(T));
        if (!d) fail(ORBMI_E_HIP);
        return d;
    }

    // Stage and upload host memory, unconditionally.
    template <class T>
    T* upload(const T* src, size_t n) {
        T* d = scratch<T>(n);
        if (d && m.h2d(d, src, n * sizeof(T)) != hipSuccess) fail(ORBMI_E_HIP);
        return rc ? nullptr : d;
    }
    template <class T>
    T* put(const std::vector<T>& v) { return upload(v.data(), v.size()); }

    // Device view of an input array: an empty array, a null pointer and a device pointer pass
    // through, host memory is staged.
    template <class T>
    const T* in(const T* p, size_t n) {
        if (rc) return nullptr;
        if (!p || n == 0 || on_device(p)) return p;
        return upload(p, n);
    }

    // Device view of an output array; a host array is read back by finish().
    template <class T>
    T* out(T* p, size_t n) {
        if (rc) return nullptr;
        if (on_device(p)) return p;
        T* d = scratch<T>(n);
        if (d) outs.push_back(Out{p, d, n * sizeof(T)});
        return d;
    }

    // An array updated in place: a host array goes up now and comes back with finish().
    template <class T>
    T* inout(T* p, size_t n) {
        T* d = out(p, n);
        if (d && d != p && m.h2d(d, p, n * sizeof(T)) != hipSuccess) fail(ORBMI_E_HIP);
        return rc ? nullptr : d;
    }

    // The handle's four per-call counters, zeroed in stream order.
    int* scalars() {
        if (rc) return nullptr;
        if (fail(ensure_buf(&m.d_scalars, &m.cap_scalars, 4))) return nullptr;
        if (hipMemsetAsync(m.d_scalars, 0, 4 * sizeof(int), m.ls()) != hipSuccess) fail(ORBMI_E_HIP);
        return rc ? nullptr : m.d_scalars;
    }

    // Frame view resolved to device pointers; the pose and the scale table travel by value.
    DevFrame frame(const orbmi_frame_view* v, bool need_pose) {
        DevFrame F;
        memset(&F, 0, sizeof(F));
        if (rc) return F;
        if (!v || v->n < 0 || (v->n > 0 && (!v->keys_un || !v->desc)) || v->nlevels < 1 || v->nlevels > kMaxLevels ||
            !v->scale_factors || (v->n_device && !on_device(v->n_device)) || (need_pose && !v->tcw)) {
            fail(ORBMI_E_ARG);
            return F;
        }
        F.n = v->n;
        F.n_dev = v->n_device;
        F.keys = in(v->keys_un, (size_t)v->n);
        F.u_right = in(v->u_right, v->u_right ? (size_t)v->n : 0);
        F.desc = in(v->desc, (size_t)v->n * 32);
        if (rc) return F;
        if (need_pose) {
            if (on_device(v->tcw)) F.tcw_dev = v->tcw;  // read by the kernels in stream order
            else memcpy(F.tcw, v->tcw, sizeof(F.tcw));
        }
        if (fail(to_host(v->scale_factors, (size_t)v->nlevels, F.scale))) return F;
        F.fx = v->fx; F.fy = v->fy; F.cx = v->cx; F.cy = v->cy; F.bf = v->bf; F.mb = v->mb;
        F.min_x = v->min_x; F.max_x = v->max_x; F.min_y = v->min_y; F.max_y = v->max_y;
        F.grid_w_inv = v->grid_w_inv; F.grid_h_inv = v->grid_h_inv;
        F.nlevels = v->nlevels;
        F.log_scale_factor = v->log_scale_factor;
        return F;
    }

    DevFV fv(const orbmi_feature_vector* v) {
        DevFV d{0, nullptr, nullptr, nullptr};
        if (rc) return d;
        if (!v || v->nnodes < 0) {
            fail(ORBMI_E_ARG);
            return d;
        }
        d.nnodes = v->nnodes;
        if (v->nnodes == 0) return d;
        // the feature count is needed only to stage a host feature list (a device one is used in
        // place: no read-back)
        int total = 0;
        if (!on_device(v->feat) && fail(csr_total(v->off, v->nnodes, &total))) return d;
        d.node_id = in(v->node_id, (size_t)v->nnodes);
        d.off = in(v->off, (size_t)v->nnodes + 1);
        d.feat = in(v->feat, (size_t)total);
        return d;
    }

    struct Count { int* user; const int* dev; int n = 1; };

    // Copy the host-bound outputs and the counts asked for (user != nullptr) back and wait.  A
    // call whose outputs are all device pointers and that asks for no count returns without
    // waiting.
    int finish(std::initializer_list<Count> counts = {}) {
        if (rc) return rc;
        bool wait = false;
        ORBMI_HIP(m.flush_up());
        if (m.up_err != hipSuccess) return ORBMI_E_HIP;
        for (Out& o : outs)
            if (o.bytes) { ORBMI_HIP(m.d2h(o.user, o.dev, o.bytes)); wait = true; }
        for (const Count& c : counts)
            if (c.user && c.dev) { ORBMI_HIP(m.d2h(c.user, c.dev, sizeof(int) * (size_t)c.n)); wait = true; }
        if (wait) ORBMI_HIP(hipStreamSynchronize(m.ls()));
        m.d2h_flush();
        done = true;
        return ORBMI_OK;
    }
};

// The keyframe table of a batched Fuse search, staged and uploaded (capi_mapping.cpp).
struct FuseTable {
    int nkf = 0, n = 0, ncap = 0;
    FuseKF* d_k = nullptr;
    int* d_cnt = nullptr;
    int* d_bi = nullptr;
    int* d_bd = nullptr;
};
// frames: the keyframes' views already resolved, or nullptr; view_pose: the search projects with
// the views' poses (false: Fuse(KF, Scw), whose poses are the caller's); d_in: nkf rows of n_mp
// IsInKeyFrame flags on the device, or nullptr
int fuse_table(Stage& s, int nkf, const orbmi_frame_view* kfs, const DevFrame* frames, bool view_pose, const uint8_t* d_in,
               int n_mp, int32_t* best_idx, int32_t* best_dist, FuseTable* T);

}  // namespace orbmi
