// C ABI of the matchers (include/orbmi.h, "ORBmatcher" section).  Inputs may live in host
// or device memory; host arrays are staged through a per-handle device arena.
#include <algorithm>
#include <cstring>
#include <new>

#include "matcher.h"
#include "essgraph_edges.h"
#include "essgraph_launch.h"
#include "sim3.h"
#include "sim3_horn.h"
#include "tri_geom.h"

using orbmi::DevFrame;
using orbmi::DevFV;
using orbmi::Matcher;
using orbmi::FuseKF;
using orbmi::TriPair;

struct orbmi_matcher {
    Matcher m;
};

hipStream_t orbmi_extractor_stream_(orbmi_extractor* ex);  // capi_extract.cpp

namespace orbmi {

void* Matcher::stage(size_t bytes) {
    bytes = (bytes + 255) & ~(size_t)255;
    std::vector<Block>& arena = gens[gen].blocks;
    for (Block& b : arena)
        if (b.size - b.used >= bytes) { void* p = b.p + b.used; b.used += bytes; return p; }
    Block b{nullptr, std::max(bytes, (size_t)(4 << 20)), 0, nullptr};
    if (hipMalloc((void**)&b.p, b.size) != hipSuccess) return nullptr;
    if (hipHostMalloc((void**)&b.h, b.size, hipHostMallocDefault) != hipSuccess) {
        (void)hipFree(b.p);
        return nullptr;
    }
    b.used = bytes;
    arena.push_back(b);
    return b.p;
}

uint8_t* Matcher::mirror(const void* d) {
    const uint8_t* q = (const uint8_t*)d;
    for (Block& b : gens[gen].blocks)
        if (q >= b.p && q < b.p + b.size) return b.h + (q - b.p);
    return nullptr;
}

hipError_t Matcher::flush_up() {
    if (!up.n) return hipSuccess;
    const hipError_t e = hipMemcpyAsync(up.d, up.h, up.n, hipMemcpyHostToDevice, stream);
    up.n = 0;
    if (e != hipSuccess && up_err == hipSuccess) up_err = e;
    return e;
}

hipError_t Matcher::h2d(void* d, const void* src, size_t bytes) {
    if (!bytes) return hipSuccess;
    uint8_t* h = mirror(d);
    if (!h) return hipMemcpyAsync(d, src, bytes, hipMemcpyHostToDevice, ls());
    memcpy(h, src, bytes);
    // the allocation right after the pending range (stage() rounds to 256 B; the gap is the
    // previous allocation's padding): extend the range, else send it and start a new one
    const size_t end = (up.n + 255) & ~(size_t)255;
    if (up.n && (uint8_t*)d == up.d + end && h == up.h + end) {
        up.n = end + bytes;
        return hipSuccess;
    }
    const hipError_t e = flush_up();
    up = PendUp{(uint8_t*)d, h, bytes};
    return e;
}

hipError_t Matcher::d2h(void* user, const void* d, size_t bytes) {
    if (!bytes) return hipSuccess;
    uint8_t* h = mirror(d);
    if (!h) return hipMemcpyAsync(user, d, bytes, hipMemcpyDeviceToHost, ls());
    pend.push_back(Pend{user, h, bytes});
    return hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, ls());
}

void Matcher::d2h_flush() {
    for (const Pend& p : pend) memcpy(p.user, p.mirror, p.bytes);
    pend.clear();
}

void Matcher::arena_reset() {
    (void)flush_up();  // (nothing is left pending by a finished call; kept for safety)
    up_err = hipSuccess;
    // the generation just used may still be read by the work enqueued so far: mark it with an
    // event, move on, and wait only for the generation about to be reused
    bool used = false;
    for (Block& b : gens[gen].blocks) used |= b.used > 0;
    if (used) {
        if (!gens[gen].ev && hipEventCreateWithFlags(&gens[gen].ev, hipEventDisableTiming) != hipSuccess) {
            gens[gen].ev = nullptr;
            (void)hipStreamSynchronize(stream);  // no event: fall back to a full wait
        } else if (gens[gen].ev) {
            (void)hipEventRecord(gens[gen].ev, stream);
            gens[gen].pending = true;
        }
        gen = (gen + 1) % kArenaGens;
    }
    Gen& g = gens[gen];
    if (g.pending) {
        (void)hipEventSynchronize(g.ev);
        g.pending = false;
    }
    for (Block& b : g.blocks) b.used = 0;
    pend.clear();
}

void Matcher::release() {
    (void)hipSetDevice(device);
    if (stream) (void)flush_up();
    if (own_stream && stream) (void)hipStreamSynchronize(stream);
    if (!own_stream && stream) (void)hipStreamSynchronize(stream);  // staged inputs may still be read
    void* ptrs[] = {d_cell_start, d_cell_list, d_kp_cell, d_mcell_start, d_mcell_list, d_mkp_cell, d_cand, d_ncand, d_top,
                    d_res, d_bin_of, d_hist, d_scalars, d_track};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    for (GridSlot& g : gslot) {
        if (g.cs) (void)hipFree(g.cs);
        if (g.cl) (void)hipFree(g.cl);
        if (g.kc) (void)hipFree(g.kc);
        g = GridSlot{};
    }
    for (Gen& g : gens) {
        for (Block& b : g.blocks) {
            (void)hipFree(b.p);
            if (b.h) (void)hipHostFree(b.h);
        }
        g.blocks.clear();
        if (g.ev) (void)hipEventDestroy(g.ev);
        g.ev = nullptr;
        g.pending = false;
    }
    if (stream && own_stream) (void)hipStreamDestroy(stream);
    stream = nullptr;
}

}  // namespace orbmi

namespace {

bool on_device(const void* p) {
    if (!p) return false;
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged;
}

// Device view of an input array (copied into the arena when it is host memory).
template <class T>
const T* dev_in(Matcher& m, const T* p, size_t n, int* rc) {
    if (!p || n == 0) return p;
    if (on_device(p)) return p;
    T* d = (T*)m.stage(n * sizeof(T));
    if (!d || m.h2d(d, p, n * sizeof(T)) != hipSuccess) {
        *rc = ORBMI_E_HIP;
        return nullptr;
    }
    return d;
}

struct OutBuf {
    void* user = nullptr;
    void* dev = nullptr;
    size_t bytes = 0;
};

template <class T>
T* dev_out(Matcher& m, T* p, size_t n, std::vector<OutBuf>& outs) {
    if (on_device(p)) return p;
    T* d = (T*)m.stage(std::max(n, (size_t)1) * sizeof(T));
    outs.push_back(OutBuf{p, d, n * sizeof(T)});
    return d;
}

// Copy host-bound outputs back and synchronise; fully device-resident calls (every output a
// device pointer, counts not requested) return without waiting.
int finish(Matcher& m, std::vector<OutBuf>& outs, int* nmatches_dev, int* nmatches, int* extra_dev = nullptr,
           int* extra = nullptr) {
    bool wait = false;
    ORBMI_HIP(m.flush_up());
    if (m.up_err != hipSuccess) return ORBMI_E_HIP;
    for (OutBuf& o : outs)
        if (o.bytes) { ORBMI_HIP(m.d2h(o.user, o.dev, o.bytes)); wait = true; }
    int tmp[2] = {0, 0};
    if (nmatches && nmatches_dev) { ORBMI_HIP(hipMemcpyAsync(&tmp[0], nmatches_dev, sizeof(int), hipMemcpyDeviceToHost, m.ls())); wait = true; }
    if (extra && extra_dev) { ORBMI_HIP(hipMemcpyAsync(&tmp[1], extra_dev, sizeof(int), hipMemcpyDeviceToHost, m.ls())); wait = true; }
    if (wait) ORBMI_HIP(hipStreamSynchronize(m.ls()));
    m.d2h_flush();
    if (nmatches) *nmatches = tmp[0];
    if (extra) *extra = tmp[1];
    return ORBMI_OK;
}

// finish() for the batched entries, whose counts are an array of n (user_counts == nullptr: not
// asked for)
int finish_counts(Matcher& m, std::vector<OutBuf>& outs, int* user_counts, const int* dev_counts, int n) {
    bool wait = false;
    ORBMI_HIP(m.flush_up());
    if (m.up_err != hipSuccess) return ORBMI_E_HIP;
    for (OutBuf& o : outs)
        if (o.bytes) { ORBMI_HIP(m.d2h(o.user, o.dev, o.bytes)); wait = true; }
    if (user_counts) {
        ORBMI_HIP(m.d2h(user_counts, dev_counts, sizeof(int) * (size_t)n));
        wait = true;
    }
    if (wait) ORBMI_HIP(hipStreamSynchronize(m.ls()));
    m.d2h_flush();
    return ORBMI_OK;
}

// Scw = [sRcw | t] into T = [Rcw | tcw] and the camera centre Ow (src/ORBmatcher.cc:368-374,
// :1148-1153), float: scw = sqrt(row 0 . row 0) (the dot product in double, rounded to float),
// Rcw = sRcw / scw, tcw = t / scw, Ow = -Rcw^T tcw.  Returns scw; what a degenerate one means is
// the caller's business.
float decompose_scw(const float* Scw, float T[12], float Ow[3]) {
    const float scw = (float)sqrt(((double)Scw[0] * Scw[0] + (double)Scw[1] * Scw[1]) + (double)Scw[2] * Scw[2]);
    for (int k = 0; k < 12; k++) T[k] = Scw[k] / scw;
    for (int c = 0; c < 3; c++) Ow[c] = -((T[c] * T[3] + T[4 + c] * T[7]) + T[8 + c] * T[11]);
    return scw;
}

int read_small(const float* p, int n, float* out) {
    if (on_device(p)) {
        ORBMI_HIP(hipMemcpy(out, p, n * sizeof(float), hipMemcpyDeviceToHost));
    } else {
        memcpy(out, p, n * sizeof(float));
    }
    return ORBMI_OK;
}

int make_frame(Matcher& m, const orbmi_frame_view* v, DevFrame* F, bool need_pose) {
    if (!v || v->n < 0 || (v->n > 0 && (!v->keys_un || !v->desc))) return ORBMI_E_ARG;
    if (v->nlevels < 1 || v->nlevels > orbmi::kMaxLevels || !v->scale_factors) return ORBMI_E_ARG;
    int rc = 0;
    memset(F, 0, sizeof(*F));
    F->n = v->n;
    F->n_dev = v->n_device;
    if (F->n_dev && !on_device(F->n_dev)) return ORBMI_E_ARG;
    F->keys = dev_in(m, v->keys_un, (size_t)v->n, &rc);
    F->u_right = dev_in(m, v->u_right, v->u_right ? (size_t)v->n : 0, &rc);
    F->desc = dev_in(m, v->desc, (size_t)v->n * 32, &rc);
    if (rc) return rc;
    if (need_pose) {
        if (!v->tcw) return ORBMI_E_ARG;
        if (on_device(v->tcw)) F->tcw_dev = v->tcw;  // read by the kernels in stream order
        else memcpy(F->tcw, v->tcw, sizeof(F->tcw));
    }
    if ((rc = read_small(v->scale_factors, v->nlevels, F->scale))) return rc;
    F->fx = v->fx; F->fy = v->fy; F->cx = v->cx; F->cy = v->cy; F->bf = v->bf; F->mb = v->mb;
    F->min_x = v->min_x; F->max_x = v->max_x; F->min_y = v->min_y; F->max_y = v->max_y;
    F->grid_w_inv = v->grid_w_inv; F->grid_h_inv = v->grid_h_inv;
    F->nlevels = v->nlevels;
    F->log_scale_factor = v->log_scale_factor;
    return ORBMI_OK;
}

int make_fv(Matcher& m, const orbmi_feature_vector* v, DevFV* d) {
    if (!v || v->nnodes < 0) return ORBMI_E_ARG;
    int rc = 0;
    d->nnodes = v->nnodes;
    if (v->nnodes == 0) { d->node_id = nullptr; d->off = nullptr; d->feat = nullptr; return ORBMI_OK; }
    // total features = off[nnodes], needed only to stage a host feature list (a device one is
    // used in place: no read-back)
    int total = 0;
    if (!on_device(v->feat)) {
        if (on_device(v->off)) ORBMI_HIP(hipMemcpy(&total, v->off + v->nnodes, sizeof(int), hipMemcpyDeviceToHost));
        else total = v->off[v->nnodes];
    }
    d->node_id = dev_in(m, v->node_id, (size_t)v->nnodes, &rc);
    d->off = dev_in(m, v->off, (size_t)v->nnodes + 1, &rc);
    d->feat = dev_in(m, v->feat, (size_t)total, &rc);
    return rc;
}

int scalars(Matcher& m) {
    int rc = orbmi::ensure_buf(&m.d_scalars, &m.cap_scalars, 4);
    if (rc) return rc;
    ORBMI_HIP(hipMemsetAsync(m.d_scalars, 0, 4 * sizeof(int), m.ls()));
    return ORBMI_OK;
}

// CreateNewMapPoints in two halves, shared by orbmi_create_new_map_points and
// orbmi_local_mapping_job: cnmp_stage validates the pairs and stages everything that does not
// depend on KF1's FeatureVector (frames, triangulation sides, the pair table and the KF2 sides
// in one upload), cnmp_launch enqueues the searches and the geometry.
struct CnmpPlan {
    DevFrame K1;
    const uint8_t* has1 = nullptr;
    orbmi::tri::Side S1;
    int npairs = 0;
    std::vector<DevFrame> KF2;  // the neighbours' frames (the batched Fuse of a job reuses them)
    TriPair* d_pairs = nullptr;
    const orbmi::tri::Side* d_S2 = nullptr;
    int* d_match = nullptr;
    uint8_t* d_ok = nullptr;
    float* d_x3d = nullptr;
};

int cnmp_stage(Matcher& m, const orbmi_frame_view* kf1, const orbmi_tri_keyframe* tri1, const float* cos1,
               const uint8_t* has_mp1, int npairs, const orbmi_frame_view* kf2, const orbmi_tri_keyframe* tri2,
               const float* const* cos2, const uint8_t* const* has_mp2, const orbmi_feature_vector* fv2,
               const float* F12, int32_t* match12, uint8_t* ok, float* x3d, std::vector<OutBuf>& outs, CnmpPlan* P) {
    if (!kf1 || !tri1 || !has_mp1 || !kf1->u_right || npairs <= 0 || !kf2 || !tri2 || !has_mp2 || !fv2 || !F12 ||
        !match12 || !ok || !x3d)
        return ORBMI_E_ARG;
    int rc;
    DevFrame& K1 = P->K1;
    if ((rc = make_frame(m, kf1, &K1, true))) return rc;
    const size_t n1 = (size_t)std::max(K1.n, 1);
    P->has1 = dev_in(m, has_mp1, n1, &rc);
    if (rc) return rc;
    std::vector<std::vector<float>> cos_tmp;  // tables computed here (copied into the arena's mirror at once)
    cos_tmp.reserve((size_t)npairs + 1);
    // the triangulation side of a keyframe: keys / u_right from its frame view (device), the rest
    // from its tri view
    auto side = [&](const orbmi_tri_keyframe* T, const orbmi_frame_view* v, const DevFrame& D, const float* cs,
                    orbmi::tri::Side* S) -> int {
        if (!T->tcw || !T->depth || !T->level_sigma2 || !T->scale_factors || on_device(T->level_sigma2) ||
            on_device(T->scale_factors) || v->nlevels > orbmi::tri::kLevels)
            return ORBMI_E_ARG;
        orbmi::tri::make_side(*T, v->nlevels, S);
        S->keys = D.keys;
        S->ur = D.u_right;
        int r = 0;
        S->depth = dev_in(m, T->depth, (size_t)D.n, &r);
        if (r) return r;
        if (!cs) {
            if (on_device(T->depth)) return ORBMI_E_ARG;
            cos_tmp.emplace_back((size_t)std::max(D.n, 1));
            if ((r = orbmi_stereo_parallax_cos(T->mb, T->depth, D.n, cos_tmp.back().data()))) return r;
            cs = cos_tmp.back().data();
        }
        S->cos_stereo = dev_in(m, cs, (size_t)D.n, &r);
        return r;
    };
    if ((rc = side(tri1, kf1, K1, cos1, &P->S1))) return rc;
    std::vector<orbmi::tri::Side> S2(npairs);
    std::vector<TriPair> pairs(npairs);
    const bool F_dev = on_device(F12);
    std::vector<float> Fh((size_t)9 * npairs);
    if (F_dev) ORBMI_HIP(hipMemcpy(Fh.data(), F12, Fh.size() * sizeof(float), hipMemcpyDeviceToHost));
    else memcpy(Fh.data(), F12, Fh.size() * sizeof(float));
    P->KF2.resize(npairs);
    for (int j = 0; j < npairs; j++) {
        TriPair& T = pairs[j];
        memset(&T, 0, sizeof(T));
        if (!kf2[j].u_right || !has_mp2[j]) return ORBMI_E_ARG;
        if ((rc = make_frame(m, &kf2[j], &T.KF2, true))) return rc;
        P->KF2[j] = T.KF2;
        if ((rc = make_fv(m, &fv2[j], &T.fv2))) return rc;
        T.has_mp2 = dev_in(m, has_mp2[j], (size_t)std::max(T.KF2.n, 1), &rc);
        if (rc) return rc;
        for (int q = 0; q < 9; q++) T.F12.m[q] = Fh[9 * j + q];
        if ((rc = side(&tri2[j], &kf2[j], T.KF2, cos2 ? cos2[j] : nullptr, &S2[j]))) return rc;
    }
    P->npairs = npairs;
    P->d_match = dev_out(m, match12, (size_t)K1.n * npairs, outs);
    P->d_ok = dev_out(m, ok, (size_t)K1.n * npairs, outs);
    P->d_x3d = dev_out(m, x3d, (size_t)3 * K1.n * npairs, outs);
    if (!P->d_match || !P->d_ok || !P->d_x3d) return ORBMI_E_HIP;
    if ((rc = orbmi::tri_pairs_prepare(m, K1, npairs, pairs.data(), P->d_match))) return rc;
    // the pair table and the KF2 sides go up in one copy
    const size_t o_s2 = (sizeof(TriPair) * npairs + 255) & ~(size_t)255;
    const size_t tab_bytes = o_s2 + sizeof(orbmi::tri::Side) * npairs;
    std::vector<uint8_t> tab(tab_bytes);
    memcpy(tab.data(), pairs.data(), sizeof(TriPair) * npairs);
    memcpy(tab.data() + o_s2, S2.data(), sizeof(orbmi::tri::Side) * npairs);
    uint8_t* d_tab = (uint8_t*)m.stage(tab_bytes);
    if (!d_tab) return ORBMI_E_HIP;
    ORBMI_HIP(m.h2d(d_tab, tab.data(), tab_bytes));
    P->d_pairs = (TriPair*)d_tab;
    P->d_S2 = (const orbmi::tri::Side*)(d_tab + o_s2);
    return ORBMI_OK;
}

int cnmp_launch(Matcher& m, const CnmpPlan& P, const DevFV& f1) {
    return orbmi::launch_create_points(m, P.K1, P.has1, f1, P.npairs, nullptr, P.d_pairs, P.S1, P.d_S2, P.d_match, P.d_ok,
                                       P.d_x3d);
}

// The batched Fuse search in the same two halves: fuse_batch_stage builds and uploads the
// keyframe table (frames: the keyframes' views already resolved, or nullptr), fuse_batch_launch
// enqueues the grids and the search.
struct FusePlan {
    int nkf = 0, n = 0, ncap = 0;
    FuseKF* d_k = nullptr;
    int* d_cnt = nullptr;
    const orbmi_mappoint* d_mps = nullptr;
    int* d_bi = nullptr;
    int* d_bd = nullptr;
};

int fuse_batch_stage(Matcher& m, int nkf, const orbmi_frame_view* kfs, const DevFrame* frames, const orbmi_mappoint* mps,
                     const uint8_t* in_kf, int n_mp, int32_t* best_idx, int32_t* best_dist, std::vector<OutBuf>& outs,
                     FusePlan* P) {
    int rc = 0;
    std::vector<FuseKF> K(nkf);
    P->d_mps = dev_in(m, mps, (size_t)n_mp, &rc);
    const uint8_t* d_in = dev_in(m, in_kf, in_kf ? (size_t)std::max(n_mp, 1) * nkf : 0, &rc);
    if (rc) return rc;
    for (int k = 0; k < nkf; k++) {
        memset(&K[k], 0, sizeof(FuseKF));
        if (frames) K[k].F = frames[k];
        else if ((rc = make_frame(m, &kfs[k], &K[k].F, true))) return rc;
        K[k].in_kf = d_in ? d_in + (size_t)k * n_mp : nullptr;
    }
    P->nkf = nkf;
    P->n = n_mp;
    P->d_k = (FuseKF*)m.stage(sizeof(FuseKF) * nkf);
    P->d_cnt = (int*)m.stage(sizeof(int) * nkf);
    P->d_bi = dev_out(m, best_idx, (size_t)n_mp * nkf, outs);
    P->d_bd = dev_out(m, best_dist, (size_t)n_mp * nkf, outs);
    if (!P->d_k || !P->d_cnt) return ORBMI_E_HIP;
    if ((rc = orbmi::fuse_multi_prepare(m, nkf, K.data(), n_mp, P->d_bi, P->d_bd, P->d_cnt, &P->ncap))) return rc;
    ORBMI_HIP(m.h2d(P->d_k, K.data(), sizeof(FuseKF) * nkf));
    return ORBMI_OK;
}

int fuse_batch_launch(Matcher& m, const FusePlan& P, float th) {
    return orbmi::launch_fuse_multi(m, P.nkf, nullptr, P.d_k, P.d_mps, P.n, th, P.d_bi, P.d_bd, P.d_cnt, P.ncap);
}

}  // namespace

extern "C" {

int orbmi_matcher_create(int device, orbmi_matcher** out) {
    if (!out) return ORBMI_E_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return ORBMI_E_HIP;
    orbmi_matcher* h = new (std::nothrow) orbmi_matcher();
    if (!h) return ORBMI_E_ARG;
    h->m.device = device;
    if (hipSetDevice(device) != hipSuccess || orbmi::stream_create(&h->m.stream, "MATCHER") != hipSuccess) {
        delete h;
        return ORBMI_E_HIP;
    }
    *out = h;
    return ORBMI_OK;
}

int orbmi_matcher_share_stream(orbmi_matcher* h, orbmi_extractor* ex) {
    if (!h || !ex) return ORBMI_E_ARG;
    Matcher& m = h->m;
    hipStream_t s = orbmi_extractor_stream_(ex);
    if (!s) return ORBMI_E_STATE;
    ORBMI_HIP(hipSetDevice(m.device));
    ORBMI_HIP(hipStreamSynchronize(m.stream));
    if (m.own_stream) ORBMI_HIP(hipStreamDestroy(m.stream));
    m.stream = s;
    m.own_stream = false;
    return ORBMI_OK;
}

int orbmi_matcher_reserve_cus(orbmi_matcher* h, int n) {
    if (!h || n < 0) return ORBMI_E_ARG;
    Matcher& m = h->m;
    if (!m.own_stream) return ORBMI_E_STATE;
    ORBMI_HIP(hipSetDevice(m.device));
    int ncu = 0;
    ORBMI_HIP(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, m.device));
    if (n >= ncu) return ORBMI_E_ARG;
    hipStream_t s = nullptr;
    if (n == 0) {
        ORBMI_HIP(orbmi::stream_create(&s, "MATCHER"));
    } else {
        std::vector<uint32_t> mask((size_t)(ncu + 31) / 32, 0u);
        for (int c = 0; c < ncu - n; c++) mask[c >> 5] |= 1u << (c & 31);
        ORBMI_HIP(hipExtStreamCreateWithCUMask(&s, (uint32_t)mask.size(), mask.data()));
    }
    (void)hipStreamSynchronize(m.stream);
    (void)hipStreamDestroy(m.stream);
    m.stream = s;
    return ORBMI_OK;
}

int orbmi_matcher_assign_features_to_grid(orbmi_matcher* h, const orbmi_frame_view* v) {
    if (!h || !v || (v->n > 0 && !on_device(v->keys_un))) return ORBMI_E_ARG;
    Matcher& m = h->m;
    ORBMI_HIP(hipSetDevice(m.device));
    m.arena_reset();
    DevFrame F;
    int rc;
    if ((rc = make_frame(m, v, &F, false))) return rc;
    if ((rc = orbmi::pin_grid(m, F))) return rc;
    ORBMI_HIP(hipGetLastError());
    return ORBMI_OK;
}

int orbmi_matcher_build_grid_slot(orbmi_matcher* h, const orbmi_frame_view* v, int slot, void* stream) {
    if (!h || !v || slot < 0 || slot >= orbmi::Matcher::kGridSlots || (v->n > 0 && !on_device(v->keys_un)) ||
        (v->n > 0 && !on_device(v->desc)) || (v->u_right && !on_device(v->u_right)))
        return ORBMI_E_ARG;
    Matcher& m = h->m;
    ORBMI_HIP(hipSetDevice(m.device));
    DevFrame F;
    int rc;
    if ((rc = make_frame(m, v, &F, false))) return rc;  // device arrays: nothing staged
    hipStream_t s = stream ? (hipStream_t)stream : m.ls();
    if ((rc = orbmi::build_grid_slot(m, F, slot, s))) return rc;
    ORBMI_HIP(hipGetLastError());
    return ORBMI_OK;
}

int orbmi_matcher_pin_grid_slot(orbmi_matcher* h, const orbmi_frame_view* v, int slot) {
    if (!h || !v || slot < 0 || slot >= orbmi::Matcher::kGridSlots || (v->n > 0 && !on_device(v->keys_un)))
        return ORBMI_E_ARG;
    Matcher& m = h->m;
    ORBMI_HIP(hipSetDevice(m.device));
    DevFrame F;
    int rc;
    if ((rc = make_frame(m, v, &F, false))) return rc;
    return orbmi::pin_grid_slot(m, F, slot);
}

int orbmi_matcher_release_grid(orbmi_matcher* h) {
    if (!h) return ORBMI_E_ARG;
    h->m.grid_pinned = false;
    return ORBMI_OK;
}

int orbmi_matcher_get_stream(orbmi_matcher* h, void** stream) {
    if (!h || !stream) return ORBMI_E_ARG;
    *stream = (void*)h->m.stream;
    return ORBMI_OK;
}

void orbmi_matcher_destroy(orbmi_matcher* h) {
    if (!h) return;
    h->m.release();
    delete h;
}

int orbmi_is_in_frustum(orbmi_matcher* h, const orbmi_frame_view* v, const orbmi_mappoint* mps, int n_mp,
                        float viewing_cos_limit, orbmi_mappoint_track* track) {
    if (!h || n_mp < 0 || (n_mp > 0 && (!mps || !track))) return ORBMI_E_ARG;
    Matcher& m = h->m;
    ORBMI_HIP(hipSetDevice(m.device));
    m.arena_reset();
    DevFrame F;
    int rc;
    if ((rc = make_frame(m, v, &F, true))) return rc;
    const orbmi_mappoint* d_mps = dev_in(m, mps, (size_t)n_mp, &rc);
    if (rc) return rc;
    std::vector<OutBuf> outs;
    orbmi_mappoint_track* d_tr = dev_out(m, track, (size_t)n_mp, outs);
    if ((rc = orbmi::launch_frustum(m, F, d_mps, n_mp, viewing_cos_limit, d_tr, nullptr))) return rc;
    ORBMI_HIP(hipGetLastError());
    return finish(m, outs, nullptr, nullptr);
}

int orbmi_search_by_projection_local(orbmi_matcher* h, const orbmi_frame_view* v, const uint8_t* occupied,
                                     const orbmi_mappoint* mps, const orbmi_mappoint_track* track, int n_mp,
                                     float th, float nnratio, int32_t* match_mp, int* nmatches) {
    if (!h || !occupied || !match_mp || n_mp < 0 || (n_mp > 0 && (!mps || !track))) return ORBMI_E_ARG;
    Matcher& m = h->m;
    ORBMI_HIP(hipSetDevice(m.device));
    m.arena_reset();
    DevFrame F;
    int rc;
    if ((rc = make_frame(m, v, &F, false))) return rc;
    const uint8_t* d_occ = dev_in(m, occupied, (size_t)std::max(F.n, 1), &rc);
    const orbmi_mappoint* d_mps = dev_in(m, mps, (size_t)n_mp, &rc);
    const orbmi_mappoint_track* d_tr = dev_in(m, track, (size_t)n_mp, &rc);
    if (rc) return rc;
    if ((rc = scalars(m))) return rc;
    std::vector<OutBuf> outs;
    int* d_out = dev_out(m, match_mp, (size_t)F.n, outs);
    if ((rc = orbmi::launch_local_search(m, F, d_occ, d_mps, d_tr, n_mp, th, nnratio, d_out, m.d_scalars))) return rc;
    ORBMI_HIP(hipGetLastError());
    return finish(m, outs, m.d_scalars, nmatches);
}

int orbmi_search_local_points(orbmi_matcher* h, const orbmi_frame_view* v, const uint8_t* occupied,
                              const orbmi_mappoint* mps, int n_mp, float th, int32_t* match_mp, int* nmatches,
                              int* n_to_match) {
    return orbmi_search_local_points_track(h, v, occupied, mps, n_mp, th, match_mp, nmatches, n_to_match, nullptr);
}

int orbmi_search_local_points_track(orbmi_matcher* h, const orbmi_frame_view* v, const uint8_t* occupied,
                                    const orbmi_mappoint* mps, int n_mp, float th, int32_t* match_mp, int* nmatches,
                                    int* n_to_match, orbmi_mappoint_track* track_out) {
    if (!h || !occupied || !match_mp || n_mp < 0 || (n_mp > 0 && !mps)) return ORBMI_E_ARG;
    Matcher& m = h->m;
    ORBMI_HIP(hipSetDevice(m.device));
    m.arena_reset();
    DevFrame F;
    int rc;
    if ((rc = make_frame(m, v, &F, true))) return rc;
    const uint8_t* d_occ = dev_in(m, occupied, (size_t)std::max(F.n, 1), &rc);
    const orbmi_mappoint* d_mps = dev_in(m, mps, (size_t)n_mp, &rc);
    if (rc) return rc;
    // k_greedy stores the match count (slot 0) unconditionally; only the nToMatch counter (slot 1,
    // atomics in k_frustum) needs zeroing, and only when the caller asks for it
    if ((rc = n_to_match ? scalars(m) : orbmi::ensure_buf(&m.d_scalars, &m.cap_scalars, 4))) return rc;
    std::vector<OutBuf> outs;
    orbmi_mappoint_track* d_tr = nullptr;
    if (track_out) {  // the isInFrustum outputs go to the caller (host: copied back with the matches)
        d_tr = dev_out(m, track_out, (size_t)std::max(n_mp, 1), outs);
    } else {
        if ((rc = orbmi::ensure_buf(&m.d_track, &m.cap_track, (size_t)std::max(n_mp, 1)))) return rc;
        d_tr = m.d_track;
    }
    int* d_out = dev_out(m, match_mp, (size_t)F.n, outs);
    // Tracking::SearchLocalPoints: isInFrustum(pMP, 0.5); ORBmatcher matcher(0.8)
#ifdef ORBMI_FRUSTUM_SEPARATE  // A/B builds (ORBMI_CFLAGS): k_frustum as its own launch ahead of the search
    if ((rc = orbmi::launch_frustum(m, F, d_mps, n_mp, 0.5f, d_tr, n_to_match ? m.d_scalars + 1 : nullptr))) return rc;
    if ((rc = orbmi::launch_local_search(m, F, d_occ, d_mps, d_tr, n_mp, th, 0.8f, d_out, m.d_scalars))) return rc;
#else
    // (isInFrustum runs inside the search's candidate kernel, which writes d_tr)
    if ((rc = orbmi::launch_local_search(m, F, d_occ, d_mps, d_tr, n_mp, th, 0.8f, d_out, m.d_scalars, d_tr, 0.5f,
                                         n_to_match ? m.d_scalars + 1 : nullptr)))
        return rc;
#endif
    ORBMI_HIP(hipGetLastError());
    int ntm = 0;  // read back (and waited for) only when the caller asks for it
    rc = finish(m, outs, m.d_scalars, nmatches, m.d_scalars + 1, n_to_match ? &ntm : nullptr);
    if (n_to_match) *n_to_match = ntm;
    return rc;
}

int orbmi_search_by_projection_last_frame(orbmi_matcher* h, const orbmi_frame_view* cf, const uint8_t* occupied,
                                          const orbmi_frame_view* lf, const orbmi_lastframe_point* lf_points,
                                          float th, int mono, int check_ori, int32_t* match_lf, int* nmatches) {
    if (!h || !occupied || !match_lf || !lf || (lf->n > 0 && !lf_points)) return ORBMI_E_ARG;
    Matcher& m = h->m;
    ORBMI_HIP(hipSetDevice(m.device));
    m.arena_reset();
    DevFrame CF, LF;
    int rc;
    if ((rc = make_frame(m, cf, &CF, true))) return rc;
    if ((rc = make_frame(m, lf, &LF, true))) return rc;
    const uint8_t* d_occ = dev_in(m, occupied, (size_t)std::max(CF.n, 1), &rc);
    const orbmi_lastframe_point* d_lfp = dev_in(m, lf_points, (size_t)LF.n, &rc);
    if (rc) return rc;
    if ((rc = scalars(m))) return rc;
    std::vector<OutBuf> outs;
    int* d_out = dev_out(m, match_lf, (size_t)CF.n, outs);
    if ((rc = orbmi::launch_lastframe_search(m, CF, d_occ, LF, d_lfp, th, mono, check_ori, d_out, m.d_scalars)))
        return rc;
    ORBMI_HIP(hipGetLastError());
    return finish(m, outs, m.d_scalars, nmatches);
}

int orbmi_search_by_projection_last_frame_if(orbmi_matcher* h, const orbmi_frame_view* cf, const uint8_t* occupied,
                                             const orbmi_frame_view* lf, const orbmi_lastframe_point* lf_points,
                                             float th, int mono, int check_ori, int32_t* match_lf, int* nmatches_dev,
                                             int min_matches) {
    if (!h || !occupied || !match_lf || !lf || (lf->n > 0 && !lf_points) || !on_device(nmatches_dev)) return ORBMI_E_ARG;
    Matcher& m = h->m;
    ORBMI_HIP(hipSetDevice(m.device));
    m.arena_reset();
    DevFrame CF, LF;
    int rc;
    if ((rc = make_frame(m, cf, &CF, true))) return rc;
    if ((rc = make_frame(m, lf, &LF, true))) return rc;
    const uint8_t* d_occ = dev_in(m, occupied, (size_t)std::max(CF.n, 1), &rc);
    const orbmi_lastframe_point* d_lfp = dev_in(m, lf_points, (size_t)LF.n, &rc);
    if (rc) return rc;
    std::vector<OutBuf> outs;
    int* d_out = dev_out(m, match_lf, (size_t)CF.n, outs);
    if ((rc = orbmi::launch_lastframe_search(m, CF, d_occ, LF, d_lfp, th, mono, check_ori, d_out, nmatches_dev,
                                             nmatches_dev, min_matches)))
        return rc;
    ORBMI_HIP(hipGetLastError());
    return finish(m, outs, nullptr, nullptr);
}

int orbmi_track_update_matches(orbmi_matcher* h, const orbmi_frame_view* f, int stage, const uint8_t* outlier,
                               const orbmi_frame_mappoints* mp, uint8_t* occupied_out, int* counts) {
    if (!h || !f || !outlier || !mp || !counts || (stage != 0 && stage != 1)) return ORBMI_E_ARG;
    if ((mp->match_lf && (!mp->lf_points || mp->n_lf_points < 0)) || (mp->match_mp && (!mp->mps || mp->n_mps < 0)))
        return ORBMI_E_ARG;
    Matcher& m = h->m;
    ORBMI_HIP(hipSetDevice(m.device));
    m.arena_reset();
    DevFrame F;
    int rc;
    if ((rc = make_frame(m, f, &F, false))) return rc;
    // the match arrays are updated in place: host arrays go through the arena and back
    std::vector<OutBuf> outs;
    const size_t n = (size_t)std::max(F.n, 1);
    int* d_lf = nullptr;
    int* d_mp = nullptr;
    if (mp->match_lf) {
        d_lf = const_cast<int*>(dev_in(m, (const int*)mp->match_lf, n, &rc));
        if (!on_device(mp->match_lf)) outs.push_back(OutBuf{mp->match_lf, d_lf, n * sizeof(int)});
    }
    if (mp->match_mp) {
        d_mp = const_cast<int*>(dev_in(m, (const int*)mp->match_mp, n, &rc));
        if (!on_device(mp->match_mp)) outs.push_back(OutBuf{mp->match_mp, d_mp, n * sizeof(int)});
    }
    const uint8_t* d_outl = dev_in(m, outlier, n, &rc);
    const orbmi_lastframe_point* d_lfp = mp->match_lf ? dev_in(m, mp->lf_points, (size_t)mp->n_lf_points, &rc) : nullptr;
    const orbmi_mappoint* d_mps = mp->match_mp ? dev_in(m, mp->mps, (size_t)mp->n_mps, &rc) : nullptr;
    if (rc) return rc;
    uint8_t* d_occ = occupied_out ? dev_out(m, occupied_out, n, outs) : nullptr;
    int* d_cnt = dev_out(m, counts, 2, outs);
    if ((rc = orbmi::launch_track_update(m, F, stage, d_outl, d_lf, d_lfp, mp->n_lf_points, d_mp, d_mps,
                                                mp->n_mps, d_occ, d_cnt))) return rc;
    ORBMI_HIP(hipGetLastError());
    return finish(m, outs, nullptr, nullptr);
}

int orbmi_search_by_bow(orbmi_matcher* h, const orbmi_frame_view* kf, const uint8_t* kf_mp_ok,
                        const orbmi_feature_vector* kf_fv, const orbmi_frame_view* f,
                        const orbmi_feature_vector* f_fv, float nnratio, int check_ori, int32_t* match_kf,
                        int* nmatches) {
    if (!h || !kf_mp_ok || !match_kf) return ORBMI_E_ARG;
    Matcher& m = h->m;
    ORBMI_HIP(hipSetDevice(m.device));
    m.arena_reset();
    DevFrame KF, F;
    DevFV kfv, fv;
    int rc;
    if ((rc = make_frame(m, kf, &KF, false))) return rc;
    if ((rc = make_frame(m, f, &F, false))) return rc;
    if ((rc = make_fv(m, kf_fv, &kfv))) return rc;
    if ((rc = make_fv(m, f_fv, &fv))) return rc;
    const uint8_t* d_ok = dev_in(m, kf_mp_ok, (size_t)std::max(KF.n, 1), &rc);
    if (rc) return rc;
    if ((rc = scalars(m))) return rc;
    std::vector<OutBuf> outs;
    int* d_out = dev_out(m, match_kf, (size_t)F.n, outs);
    if ((rc = orbmi::launch_bow(m, KF, d_ok, kfv, F, fv, nnratio, check_ori, d_out, m.d_scalars))) return rc;
    ORBMI_HIP(hipGetLastError());
    return finish(m, outs, m.d_scalars, nmatches);
}

int orbmi_search_by_bow_kf(orbmi_matcher* h, const orbmi_frame_view* kf1, const uint8_t* ok1,
                           const orbmi_feature_vector* fv1, const orbmi_frame_view* kf2, const uint8_t* ok2,
                           const orbmi_feature_vector* fv2, float nnratio, int check_ori, int32_t* match12,
                           int* nmatches) {
    if (!h || !kf1 || !kf2 || !match12 || (kf1->n > 0 && !ok1) || (kf2->n > 0 && !ok2)) return ORBMI_E_ARG;
    if (kf1->n_device || kf2->n_device) return ORBMI_E_ARG;  // keyframes: host-known counts
    Matcher& m = h->m;
    ORBMI_HIP(hipSetDevice(m.device));
    m.arena_reset();
    DevFrame K1, K2;
    DevFV f1, f2;
    int rc;
    if ((rc = make_frame(m, kf1, &K1, false))) return rc;
    if ((rc = make_frame(m, kf2, &K2, false))) return rc;
    if ((rc = make_fv(m, fv1, &f1))) return rc;
    if ((rc = make_fv(m, fv2, &f2))) return rc;
    const uint8_t* d_ok1 = dev_in(m, ok1, (size_t)K1.n, &rc);
    const uint8_t* d_ok2 = dev_in(m, ok2, (size_t)K2.n, &rc);
    if (rc) return rc;
    if ((rc = scalars(m))) return rc;
    int* d_matched2 = (int*)m.stage((size_t)std::max(K2.n, 1) * sizeof(int));  // vbMatched2
    if (!d_matched2) return ORBMI_E_HIP;
    std::vector<OutBuf> outs;
    int* d_out = dev_out(m, match12, (size_t)K1.n, outs);
    if ((rc = orbmi::launch_bow_kf(m, K1, d_ok1, f1, K2, d_ok2, f2, nnratio, check_ori, d_out, d_matched2,
                                   m.d_scalars)))
        return rc;
    ORBMI_HIP(hipGetLastError());
    return finish(m, outs, m.d_scalars, nmatches);
}

int orbmi_match_descriptors_segments(orbmi_matcher* h, const uint8_t* q_desc, int nq, const int* nq_device,
                                     const uint8_t* train_desc, int nseg, int seg_capacity, const int* seg_counts,
                                     int skip_seg, int th, float ratio, int32_t* match, int* nmatches) {
    if (!h || nq < 0 || nseg < 0 || seg_capacity < 0 || (nq > 0 && (!q_desc || !match))) return ORBMI_E_ARG;
    if ((long long)nseg * seg_capacity > 0xFFFFFFFLL) return ORBMI_E_UNSUPPORTED;
    if (nseg * seg_capacity > 0 && (!train_desc || !seg_counts)) return ORBMI_E_ARG;
    if (nq_device && !on_device(nq_device)) return ORBMI_E_ARG;
    Matcher& m = h->m;
    ORBMI_HIP(hipSetDevice(m.device));
    m.arena_reset();
    int rc = 0;
    const uint8_t* d_q = dev_in(m, q_desc, (size_t)nq * 32, &rc);
    const uint8_t* d_t = dev_in(m, train_desc, (size_t)nseg * seg_capacity * 32, &rc);
    const int* d_cnt = dev_in(m, seg_counts, (size_t)nseg, &rc);
    if (rc) return rc;
    if ((rc = scalars(m))) return rc;
    std::vector<OutBuf> outs;
    int* d_out = dev_out(m, match, (size_t)nq, outs);
    if (nseg * seg_capacity == 0 && nq > 0) ORBMI_HIP(hipMemsetAsync(d_out, 0xFF, (size_t)nq * sizeof(int), m.ls()));
    else if ((rc = orbmi::launch_xmatch(m, d_q, nq, nq_device, d_t, nseg, seg_capacity, d_cnt, skip_seg, th, ratio,
                                        d_out, m.d_scalars)))
        return rc;
    ORBMI_HIP(hipGetLastError());
    return finish(m, outs, m.d_scalars, nmatches);
}

int orbmi_compute_distinctive_descriptors(orbmi_matcher* h, const uint8_t* obs_desc, const int32_t* obs_off, int np,
                                          int32_t* best, uint8_t* desc_out) {
    if (!h || np < 0 || (np > 0 && (!obs_off || !best || !desc_out))) return ORBMI_E_ARG;
    if (np == 0) return ORBMI_OK;
    Matcher& m = h->m;
    ORBMI_HIP(hipSetDevice(m.device));
    m.arena_reset();
    // the row count is needed only to stage host descriptors (a device array is used in place)
    int total = 0;
    const bool desc_dev = on_device(obs_desc);
    if (!desc_dev) {
        if (on_device(obs_off)) ORBMI_HIP(hipMemcpy(&total, obs_off + np, sizeof(int), hipMemcpyDeviceToHost));
        else total = obs_off[np];
        if (total < 0 || (total > 0 && !obs_desc)) return ORBMI_E_ARG;
    }
    int rc = 0;
    const uint8_t* d_desc = desc_dev ? obs_desc : dev_in(m, obs_desc, (size_t)total * 32, &rc);
    const int* d_off = dev_in(m, obs_off, (size_t)np + 1, &rc);
    if (rc) return rc;
    std::vector<OutBuf> outs;
    int* d_best = dev_out(m, best, (size_t)np, outs);
    uint8_t* d_out = dev_out(m, desc_out, (size_t)np * 32, outs);
    if (!on_device(desc_out)) ORBMI_HIP(m.h2d(d_out, desc_out, (size_t)np * 32));
    if ((rc = orbmi::launch_distinctive(m, d_desc, d_off, np, d_best, d_out))) return rc;
    return finish(m, outs, nullptr, nullptr);
}

int orbmi_search_for_triangulation(orbmi_matcher* h, const orbmi_frame_view* kf1, const uint8_t* has_mp1,
                                   const orbmi_feature_vector* fv1, const orbmi_frame_view* kf2, const uint8_t* has_mp2,
                                   const orbmi_feature_vector* fv2, const float* F12, int only_stereo, int check_ori,
                                   int32_t* match12, int* nmatches) {
    if (!kf2 || !has_mp2 || !fv2 || !F12) return ORBMI_E_ARG;
    const uint8_t* mp2[1] = {has_mp2};
    return orbmi_search_for_triangulation_batch(h, kf1, has_mp1, fv1, 1, kf2, mp2, fv2, F12, only_stereo, check_ori,
                                                match12, nmatches);
}

int orbmi_search_for_triangulation_batch(orbmi_matcher* h, const orbmi_frame_view* kf1, const uint8_t* has_mp1,
                                         const orbmi_feature_vector* fv1, int npairs, const orbmi_frame_view* kf2,
                                         const uint8_t* const* has_mp2, const orbmi_feature_vector* fv2,
                                         const float* F12, int only_stereo, int check_ori, int32_t* match12,
                                         int* nmatches) {
    if (!h || !has_mp1 || !fv1 || !kf1 || !kf1->u_right || npairs < 0 || (npairs > 0 && (!kf2 || !has_mp2 || !fv2 ||
                                                                                      !F12 || !match12)))
        return ORBMI_E_ARG;
    if (npairs == 0) return ORBMI_OK;
    Matcher& m = h->m;
    ORBMI_HIP(hipSetDevice(m.device));
    m.arena_reset();
    DevFrame K1;
    DevFV f1;
    int rc;
    if ((rc = make_frame(m, kf1, &K1, true))) return rc;
    if ((rc = make_fv(m, fv1, &f1))) return rc;
    const uint8_t* d_mp1 = dev_in(m, has_mp1, (size_t)std::max(K1.n, 1), &rc);
    if (rc) return rc;
    std::vector<TriPair> pairs(npairs);
    const bool F_dev = on_device(F12);
    std::vector<float> Fh((size_t)9 * npairs);
    if (F_dev) ORBMI_HIP(hipMemcpy(Fh.data(), F12, Fh.size() * sizeof(float), hipMemcpyDeviceToHost));
    else memcpy(Fh.data(), F12, Fh.size() * sizeof(float));
    int* d_counts = nullptr;
    if (nmatches) d_counts = (int*)m.stage((size_t)npairs * sizeof(int));
    for (int j = 0; j < npairs; j++) {
        TriPair& P = pairs[j];
        memset(&P, 0, sizeof(P));
        if (!kf2[j].u_right || !has_mp2[j]) return ORBMI_E_ARG;
        if ((rc = make_frame(m, &kf2[j], &P.KF2, true))) return rc;
        if ((rc = make_fv(m, &fv2[j], &P.fv2))) return rc;
        P.has_mp2 = dev_in(m, has_mp2[j], (size_t)std::max(P.KF2.n, 1), &rc);
        if (rc) return rc;
        for (int q = 0; q < 9; q++) P.F12.m[q] = Fh[9 * j + q];
        P.nmatches = d_counts ? d_counts + j : nullptr;
    }
    TriPair* d_pairs = (TriPair*)m.stage(sizeof(TriPair) * npairs);
    std::vector<OutBuf> outs;
    int* d_out = dev_out(m, match12, (size_t)K1.n * npairs, outs);
    if (!d_pairs || !d_out) return ORBMI_E_HIP;
    if ((rc = orbmi::launch_triangulation(m, K1, d_mp1, f1, npairs, pairs.data(), d_pairs, only_stereo, check_ori,
                                          d_out)))
        return rc;
    return finish_counts(m, outs, nmatches, d_counts, npairs);
}

int orbmi_create_new_map_points(orbmi_matcher* h, const orbmi_frame_view* kf1, const orbmi_tri_keyframe* tri1,
                                const float* cos1, const uint8_t* has_mp1, const orbmi_feature_vector* fv1,
                                int npairs, const orbmi_frame_view* kf2, const orbmi_tri_keyframe* tri2,
                                const float* const* cos2, const uint8_t* const* has_mp2,
                                const orbmi_feature_vector* fv2, const float* F12, int32_t* match12, uint8_t* ok,
                                float* x3d) {
    if (!h || !kf1 || !tri1 || !has_mp1 || !fv1 || !kf1->u_right || npairs < 0 ||
        (npairs > 0 && (!kf2 || !tri2 || !has_mp2 || !fv2 || !F12 || !match12 || !ok || !x3d)))
        return ORBMI_E_ARG;
    if (npairs == 0) return ORBMI_OK;
    Matcher& m = h->m;
    ORBMI_HIP(hipSetDevice(m.device));
    m.arena_reset();
    DevFV f1;
    int rc;
    if ((rc = make_fv(m, fv1, &f1))) return rc;
    CnmpPlan P;
    std::vector<OutBuf> outs;
    if ((rc = cnmp_stage(m, kf1, tri1, cos1, has_mp1, npairs, kf2, tri2, cos2, has_mp2, fv2, F12, match12, ok, x3d, outs,
                         &P)))
        return rc;
    if ((rc = cnmp_launch(m, P, f1))) return rc;
    return finish(m, outs, nullptr, nullptr);
}

int orbmi_fuse_search(orbmi_matcher* h, const orbmi_frame_view* kf, const orbmi_mappoint* mps, const uint8_t* in_kf,
                      int n_mp, float th, int32_t* best_idx, int32_t* best_dist, int* ncandidates) {
    if (!h || !kf || n_mp < 0 || (n_mp > 0 && (!mps || !best_idx || !best_dist))) return ORBMI_E_ARG;
    Matcher& m = h->m;
    ORBMI_HIP(hipSetDevice(m.device));
    m.arena_reset();
    DevFrame F;
    int rc;
    if ((rc = make_frame(m, kf, &F, true))) return rc;
    const orbmi_mappoint* d_mps = dev_in(m, mps, (size_t)n_mp, &rc);
    const uint8_t* d_in = dev_in(m, in_kf, in_kf ? (size_t)std::max(n_mp, 1) : 0, &rc);
    if (rc) return rc;
    if (ncandidates && (rc = scalars(m))) return rc;  // the count only when asked for
    std::vector<OutBuf> outs;
    int* d_bi = dev_out(m, best_idx, (size_t)n_mp, outs);
    int* d_bd = dev_out(m, best_dist, (size_t)n_mp, outs);
    int* d_cnt = ncandidates ? m.d_scalars : nullptr;
    if ((rc = orbmi::launch_fuse(m, F, d_mps, d_in, n_mp, th, d_bi, d_bd, d_cnt))) return rc;
    return finish(m, outs, d_cnt, ncandidates);
}

int orbmi_fuse_search_batch(orbmi_matcher* h, int nkf, const orbmi_frame_view* kfs, const orbmi_mappoint* mps,
                            const uint8_t* in_kf, int n_mp, float th, int32_t* best_idx, int32_t* best_dist,
                            int* ncandidates) {
    if (!h || nkf < 0 || n_mp < 0 || (nkf > 0 && !kfs) || (nkf > 0 && n_mp > 0 && (!mps || !best_idx || !best_dist)))
        return ORBMI_E_ARG;
    if (nkf == 0) return ORBMI_OK;
    Matcher& m = h->m;
    ORBMI_HIP(hipSetDevice(m.device));
    m.arena_reset();
    int rc = 0;
    FusePlan P;
    std::vector<OutBuf> outs;
    if ((rc = fuse_batch_stage(m, nkf, kfs, nullptr, mps, in_kf, n_mp, best_idx, best_dist, outs, &P))) return rc;
    if ((rc = fuse_batch_launch(m, P, th))) return rc;
    return finish_counts(m, outs, ncandidates, P.d_cnt, nkf);
}

int orbmi_fuse_search_refresh(orbmi_matcher* h, const uint8_t* obs_desc, const int32_t* obs_off, int nd, int32_t* best,
                              uint8_t* desc_out, int nkf, const orbmi_frame_view* kfs, const orbmi_mappoint* mps,
                              const int32_t* desc_from, const uint8_t* in_kf, int n_mp, float th, int32_t* best_idx,
                              int32_t* best_dist) {
    if (!h || nd < 0 || nkf < 0 || n_mp < 0 || (nd > 0 && (!obs_off || !best || !desc_out)) ||
        (nkf > 0 && !kfs) || (nkf > 0 && n_mp > 0 && (!mps || !best_idx || !best_dist)))
        return ORBMI_E_ARG;
    Matcher& m = h->m;
    ORBMI_HIP(hipSetDevice(m.device));
    m.arena_reset();
    int rc = 0;
    std::vector<OutBuf> outs;
    // ComputeDistinctiveDescriptors of the nd due points
    uint8_t* d_dout = nullptr;
    if (nd > 0) {
        int total = 0;
        if (on_device(obs_off)) ORBMI_HIP(hipMemcpy(&total, obs_off + nd, sizeof(int), hipMemcpyDeviceToHost));
        else total = obs_off[nd];
        if (total < 0 || (total > 0 && !obs_desc)) return ORBMI_E_ARG;
        const uint8_t* d_desc = dev_in(m, obs_desc, (size_t)total * 32, &rc);
        const int* d_off = dev_in(m, obs_off, (size_t)nd + 1, &rc);
        if (rc) return rc;
        int* d_best = dev_out(m, best, (size_t)nd, outs);
        d_dout = dev_out(m, desc_out, (size_t)nd * 32, outs);
        if (!on_device(desc_out))
            ORBMI_HIP(m.h2d(d_dout, desc_out, (size_t)nd * 32));
        if ((rc = orbmi::launch_distinctive(m, d_desc, d_off, nd, d_best, d_dout))) return rc;
    }
    // the Fuse searches on records patched with the new descriptors
    if (nkf > 0 && n_mp > 0) {
        orbmi_mappoint* d_mps = (orbmi_mappoint*)m.stage(sizeof(orbmi_mappoint) * n_mp);
        if (!d_mps) return ORBMI_E_HIP;
        if (on_device(mps))
            ORBMI_HIP(hipMemcpyAsync(d_mps, mps, sizeof(orbmi_mappoint) * n_mp, hipMemcpyDeviceToDevice, m.ls()));
        else
            ORBMI_HIP(m.h2d(d_mps, mps, sizeof(orbmi_mappoint) * n_mp));
        if (desc_from && nd > 0) {
            const int* d_from = dev_in(m, desc_from, (size_t)n_mp, &rc);
            if (rc) return rc;
            if ((rc = orbmi::launch_patch_desc(m, d_mps, d_from, d_dout, n_mp))) return rc;
        }
        const uint8_t* d_in = dev_in(m, in_kf, in_kf ? (size_t)n_mp * nkf : 0, &rc);
        if (rc) return rc;
        std::vector<FuseKF> K(nkf);
        for (int k = 0; k < nkf; k++) {
            memset(&K[k], 0, sizeof(FuseKF));
            if ((rc = make_frame(m, &kfs[k], &K[k].F, true))) return rc;
            K[k].in_kf = d_in ? d_in + (size_t)k * n_mp : nullptr;
        }
        FuseKF* d_k = (FuseKF*)m.stage(sizeof(FuseKF) * nkf);
        int* d_cnt = (int*)m.stage(sizeof(int) * nkf);
        int* d_bi = dev_out(m, best_idx, (size_t)n_mp * nkf, outs);
        int* d_bd = dev_out(m, best_dist, (size_t)n_mp * nkf, outs);
        if (!d_k || !d_cnt) return ORBMI_E_HIP;
        if ((rc = orbmi::launch_fuse_multi(m, nkf, K.data(), d_k, d_mps, n_mp, th, d_bi, d_bd, d_cnt))) return rc;
    }
    return finish(m, outs, nullptr, nullptr);
}

int orbmi_local_mapping_job(orbmi_matcher* h, orbmi_ba* ba, const orbmi_lm_job* J, orbmi_lm_job_result* R) {
    if (!h || !ba || !J || !R) return ORBMI_E_ARG;
    R->bow_words = R->fv_nodes = 0;
    R->failed_stage = -1;
    auto fail = [R](int stage, int rc) { R->failed_stage = stage; return rc; };
    const int np = J->n_points, nnb = J->nnb, n_kp = J->n_kf_points, n_tp = J->n_target_points;
    if (!J->kf || !J->problem || !J->result || !J->counts_host || !J->counts_event || !J->fv_node || !J->fv_off ||
        !J->fv_feat || np < 0 || nnb < 0 || n_kp < 0 || n_tp < 0 || (np > 0 && (!J->obs_off || !J->best || !J->desc_out)) ||
        (nnb > 0 && n_kp > 0 && (!J->kf_points || !J->best_idx || !J->best_dist)) ||
        (n_tp > 0 && (!J->target_points || !J->best_idx || !J->best_dist)))
        return ORBMI_E_ARG;
    if (J->voc && (J->bow_n < 0 || !J->bow_counts || !J->bow_word || !J->bow_value)) return fail(0, ORBMI_E_ARG);
    Matcher& m = h->m;
    ORBMI_HIP(hipSetDevice(m.device));
    m.arena_reset();  // the job's one arena generation
    // an error leaves nothing pending in the arena: staged uploads and read-backs are dropped
    struct Pending {
        Matcher& m;
        bool done = false;
        ~Pending() {
            if (!done) { m.up = Matcher::PendUp{}; m.pend.clear(); }
        }
    } pending{m};
    auto mark = [&](int k) {  // a stage boundary for the caller's timeline (diagnostics)
        if (J->stage_events && J->stage_events[k]) (void)hipEventRecord((hipEvent_t)J->stage_events[k], m.ls());
    };
    int rc;
    // ---- ProcessNewKeyFrame: ComputeBoW (unless issued ahead) + ComputeDistinctiveDescriptors
    hipEvent_t counts_ev = (hipEvent_t)J->counts_event;
    if (J->voc) {
        if ((rc = orbmi_transform(J->voc, J->bow_desc, J->bow_n, nullptr, 4, J->bow_word, J->bow_value, J->fv_node,
                                  J->fv_off, J->fv_feat, J->bow_counts)))
            return fail(0, rc);
        void* vs = nullptr;
        if ((rc = orbmi_vocabulary_get_stream(J->voc, &vs))) return fail(0, rc);
        if ((hipStream_t)vs != m.stream && (rc = orbmi_vocabulary_synchronize(J->voc))) return fail(0, rc);
        if (hipMemcpyAsync(const_cast<int32_t*>(J->counts_host), J->bow_counts, 2 * sizeof(int), hipMemcpyDeviceToHost,
                           m.stream) != hipSuccess ||
            hipEventRecord(counts_ev, m.stream) != hipSuccess)
            return fail(0, ORBMI_E_HIP);
    }
    // enqueued first, so the stream is busy while the host builds the searches' tables
    const uint8_t* d_obs = nullptr;
    const int* d_off = nullptr;
    std::vector<OutBuf> outs;
    int* d_best = nullptr;
    uint8_t* d_dsc = nullptr;
    if (np > 0) {
        if (!on_device(J->obs_desc) && J->obs_desc) return fail(1, ORBMI_E_ARG);  // (its row count is not read back here)
        rc = 0;
        d_obs = J->obs_desc;
        d_off = dev_in(m, J->obs_off, (size_t)np + 1, &rc);
        if (rc) return fail(1, rc);
        d_best = dev_out(m, J->best, (size_t)np, outs);
        d_dsc = dev_out(m, J->desc_out, (size_t)np * 32, outs);
        if (!on_device(J->desc_out) && hipSuccess != m.h2d(d_dsc, J->desc_out, (size_t)np * 32)) return fail(1, ORBMI_E_HIP);
        if ((rc = orbmi::launch_distinctive(m, d_obs, d_off, np, d_best, d_dsc))) return fail(1, rc);
    }
    mark(0);
    // ---- every search's host tables: validated, built and staged now, one upload
    CnmpPlan cn;
    FusePlan fb;
    DevFrame KF;
    if (nnb > 0) {
        if ((rc = cnmp_stage(m, J->kf, J->tri, J->cos, J->has_mp, nnb, J->kf2, J->tri2, J->cos2, J->has_mp2, J->fv2, J->F12,
                             J->match12, J->ok, J->x3d, outs, &cn)))
            return fail(2, rc);
        if ((rc = fuse_batch_stage(m, nnb, J->kf2, cn.KF2.data(), J->kf_points, nullptr, n_kp, J->best_idx, J->best_dist,
                                   outs, &fb)))
            return fail(3, rc);
        KF = cn.K1;
    } else if ((rc = make_frame(m, J->kf, &KF, true))) {
        return fail(3, rc);
    }
    const size_t o = (size_t)nnb * n_kp;  // Fuse(keyframe, targets' points) behind the targets' rows
    rc = 0;
    const orbmi_mappoint* d_tp = dev_in(m, J->target_points, (size_t)n_tp, &rc);
    if (rc) return fail(3, rc);
    int* d_bi = dev_out(m, J->best_idx ? J->best_idx + o : nullptr, (size_t)n_tp, outs);
    int* d_bd = dev_out(m, J->best_dist ? J->best_dist + o : nullptr, (size_t)n_tp, outs);
    // ---- the FeatureVector's node count sizes SearchForTriangulation: the one host wait ahead of LocalBA
    if (hipEventSynchronize(counts_ev) != hipSuccess) return fail(0, ORBMI_E_HIP);
    const int nw = J->counts_host[0], nn = J->counts_host[1];
    if (nw < 0 || nn < 0) return fail(0, ORBMI_E_STATE);
    R->bow_words = nw;
    R->fv_nodes = nn;
    // ---- CreateNewMapPoints
    if (nnb > 0) {
        const DevFV f1{nn, nn ? J->fv_node : nullptr, nn ? J->fv_off : nullptr, nn ? J->fv_feat : nullptr};
        if ((rc = cnmp_launch(m, cn, f1))) return fail(2, rc);
    }
    mark(1);
    // ---- SearchInNeighbors: Fuse(target, keyframe's points) per target, Fuse(keyframe, targets' points)
    if (nnb > 0 && (rc = fuse_batch_launch(m, fb, J->fuse_th))) return fail(3, rc);
    if ((rc = orbmi::launch_fuse(m, KF, d_tp, nullptr, n_tp, J->fuse_th, d_bi, d_bd, nullptr))) return fail(3, rc);
    mark(2);
    // ---- ComputeDistinctiveDescriptors of the keyframe's points after fusion
    if (np > 0 && (rc = orbmi::launch_distinctive(m, d_obs, d_off, np, d_best, d_dsc))) return fail(4, rc);
    mark(3);
    if ((rc = finish(m, outs, nullptr, nullptr))) return fail(4, rc);
    pending.done = true;
    // ---- LocalBundleAdjustment (in stream order behind the searches when ba runs on this stream)
    if ((rc = orbmi_local_bundle_adjustment(ba, J->problem, J->result, J->stop))) return fail(5, rc);
    return ORBMI_OK;
}

int orbmi_sim3_ransac_batch(orbmi_matcher* h, int nsolvers, const orbmi_sim3_problem* problems,
                            orbmi_sim3_hypotheses* results) {
    if (!h || nsolvers < 0 || (nsolvers > 0 && (!problems || !results))) return ORBMI_E_ARG;
    // everything is validated before anything is staged or launched
    std::vector<int> its((size_t)nsolvers);
    int max_its = 0;
    for (int k = 0; k < nsolvers; k++) {
        const orbmi_sim3_problem& P = problems[k];
        if (P.n < 0 || P.min_inliers < 0 || P.max_iterations < 0) return ORBMI_E_ARG;
        its[k] = orbmi::sim3_iterations(P.n, P.min_inliers, P.probability, P.max_iterations);
        if (its[k] == 0) continue;
        const orbmi_sim3_hypotheses& R = results[k];
        if (P.n < 3 || !P.x3d_c1 || !P.x3d_c2 || !P.max_err1 || !P.max_err2 || !R.T12 || !R.T21 || !R.s || !R.count ||
            !R.mask)
            return ORBMI_E_ARG;
        if (P.triples) {
            if (on_device(P.triples)) return ORBMI_E_ARG;
            for (int j = 0; j < 3 * its[k]; j++)
                if (P.triples[j] < 0 || P.triples[j] >= P.n) return ORBMI_E_ARG;
        }
        max_its = std::max(max_its, its[k]);
    }
    for (int k = 0; k < nsolvers; k++) results[k].iterations = its[k];
    if (max_its == 0) return ORBMI_OK;
    Matcher& m = h->m;
    ORBMI_HIP(hipSetDevice(m.device));
    m.arena_reset();
    int rc = 0;
    std::vector<OutBuf> outs;
    std::vector<orbmi::Sim3Dev> T((size_t)nsolvers);
    std::vector<int32_t> tri, avail;
    for (int k = 0; k < nsolvers; k++) {
        const orbmi_sim3_problem& P = problems[k];
        orbmi::Sim3Dev& D = T[k];
        memset(&D, 0, sizeof(D));
        D.n = P.n;
        D.iterations = its[k];
        if (its[k] == 0) continue;
        const size_t n = (size_t)P.n, H = (size_t)its[k], words = (n + 63) / 64;
        D.fix_scale = P.fix_scale;
        D.x1 = dev_in(m, P.x3d_c1, 3 * n, &rc);
        D.x2 = dev_in(m, P.x3d_c2, 3 * n, &rc);
        D.e1 = dev_in(m, P.max_err1, n, &rc);
        D.e2 = dev_in(m, P.max_err2, n, &rc);
        memcpy(D.k1, P.k1, sizeof(D.k1));
        memcpy(D.k2, P.k2, sizeof(D.k2));
        if (P.triples) {
            D.triples = dev_in(m, P.triples, 3 * H, &rc);
        } else {
            tri.resize(3 * H);
            avail.resize(n);
            for (int it = 0; it < its[k]; it++)
                orbmi::sim3_sample_triple(P.seed, k, it, P.n, avail.data(), tri.data() + 3 * (size_t)it);
            D.triples = dev_in(m, (const int32_t*)tri.data(), 3 * H, &rc);  // copied into the arena's mirror at once
        }
        if (rc) return rc;
        const orbmi_sim3_hypotheses& R = results[k];
        D.T12 = dev_out(m, R.T12, 12 * H, outs);
        D.T21 = dev_out(m, R.T21, 12 * H, outs);
        D.s = dev_out(m, R.s, H, outs);
        D.count = dev_out(m, R.count, H, outs);
        D.mask = dev_out(m, R.mask, H * words, outs);
        if (!D.T12 || !D.T21 || !D.s || !D.count || !D.mask) return ORBMI_E_HIP;
    }
    const orbmi::Sim3Dev* d_T = dev_in(m, (const orbmi::Sim3Dev*)T.data(), (size_t)nsolvers, &rc);
    if (rc) return rc;
    if ((rc = orbmi::launch_sim3_ransac(m, nsolvers, d_T, max_its))) return rc;
    return finish(m, outs, nullptr, nullptr);
}

int orbmi_search_by_sim3(orbmi_matcher* h, const orbmi_frame_view* kf1, const orbmi_mappoint* mps1, const uint8_t* has_mp1,
                         const orbmi_frame_view* kf2, const orbmi_mappoint* mps2, const uint8_t* has_mp2, float s12,
                         const float* R12, const float* t12, float th, int32_t* match12, int* nfound, int32_t* vn_match1,
                         int32_t* vn_match2) {
    if (!h || !kf1 || !kf2 || !R12 || !t12 || kf1->n < 0 || kf2->n < 0 || (kf1->n > 0 && (!mps1 || !has_mp1 || !match12)) ||
        (kf2->n > 0 && (!mps2 || !has_mp2)) || on_device(R12) || on_device(t12))
        return ORBMI_E_ARG;
    if (nfound) *nfound = 0;
    Matcher& m = h->m;
    ORBMI_HIP(hipSetDevice(m.device));
    m.arena_reset();
    int rc = 0;
    orbmi::Sim3Side S[2];
    memset(S, 0, sizeof(S));
    DevFrame K1, K2;
    if ((rc = make_frame(m, kf1, &K1, true)) || (rc = make_frame(m, kf2, &K2, true))) return rc;
    if (K1.tcw_dev || K2.tcw_dev) return ORBMI_E_ARG;  // the poses travel by value
    const size_t n1 = (size_t)kf1->n, n2 = (size_t)kf2->n;
    S[0].F = K2; S[0].n_src = kf1->n;
    S[1].F = K1; S[1].n_src = kf2->n;
    S[0].mps = dev_in(m, mps1, n1, &rc); S[0].has = dev_in(m, has_mp1, n1, &rc);
    S[1].mps = dev_in(m, mps2, n2, &rc); S[1].has = dev_in(m, has_mp2, n2, &rc);
    if (rc) return rc;
    memcpy(S[0].Tcw, K1.tcw, sizeof(S[0].Tcw));
    memcpy(S[1].Tcw, K2.tcw, sizeof(S[1].Tcw));
    // sR12 = s12 * R12, sR21 = (1.0 / s12) * R12^T, t21 = -sR21 * t12 (:1304-1308): the scalar a
    // double, the matrix float, one rounding to float per entry; the products float, left to right
    const double inv = 1.0 / (double)s12;
    float sR21[9];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            S[1].S[4 * r + c] = (float)((double)s12 * (double)R12[3 * r + c]);
            sR21[3 * r + c] = (float)(inv * (double)R12[3 * c + r]);
            S[0].S[4 * r + c] = sR21[3 * r + c];
        }
    for (int r = 0; r < 3; r++) {
        S[1].S[4 * r + 3] = t12[r];
        S[0].S[4 * r + 3] = -((sR21[3 * r] * t12[0] + sR21[3 * r + 1] * t12[1]) + sR21[3 * r + 2] * t12[2]);
    }
    for (int k = 0; k < 2; k++) { S[k].fx = kf1->fx; S[k].fy = kf1->fy; S[k].cx = kf1->cx; S[k].cy = kf1->cy; }
    std::vector<OutBuf> outs;
    int* d_m12 = dev_out(m, match12, n1, outs);
    if (!on_device(match12) && n1) ORBMI_HIP(m.h2d(d_m12, match12, n1 * sizeof(int32_t)));
    S[0].vn = vn_match1 ? dev_out(m, vn_match1, n1, outs) : (int*)m.stage(std::max(n1, (size_t)1) * sizeof(int));
    S[1].vn = vn_match2 ? dev_out(m, vn_match2, n2, outs) : (int*)m.stage(std::max(n2, (size_t)1) * sizeof(int));
    uint8_t* d_already2 = (uint8_t*)m.stage(std::max(n2, (size_t)1));
    orbmi::Sim3Side* d_S = (orbmi::Sim3Side*)m.stage(sizeof(S));
    if (!d_m12 || !S[0].vn || !S[1].vn || !d_already2 || !d_S) return ORBMI_E_HIP;
    if ((rc = scalars(m))) return rc;
    if ((rc = orbmi::launch_search_by_sim3(m, S, d_S, d_m12, d_already2, th, m.d_scalars))) return rc;
    return finish(m, outs, m.d_scalars, nfound);
}

int orbmi_search_by_projection_sim3(orbmi_matcher* h, const orbmi_frame_view* kf, const float* Scw, const orbmi_mappoint* mps,
                                    int n, int32_t* matched, float th, int* nmatches) {
    if (!h || !kf || !Scw || n < 0 || kf->n < 0 || (n > 0 && !mps) || (kf->n > 0 && !matched) || on_device(Scw) ||
        on_device(matched))
        return ORBMI_E_ARG;
    const int nk = kf->n, cap = Matcher::kCandCap;
    for (int k = 0; k < nk; k++)
        if (matched[k] < -2 || matched[k] >= n) return ORBMI_E_ARG;
    if (nmatches) *nmatches = 0;
    if (n == 0 || nk == 0) return ORBMI_OK;
    Matcher& m = h->m;
    ORBMI_HIP(hipSetDevice(m.device));
    m.arena_reset();
    int rc = 0;
    DevFrame F;
    if ((rc = make_frame(m, kf, &F, false))) return rc;
    orbmi::ProjSim3Args a;
    memset(&a, 0, sizeof(a));
    (void)decompose_scw(Scw, a.T, a.Ow);  // (no test of scw here: a degenerate Scw finds nothing)
    // spAlreadyFound and the occupied keypoints
    std::vector<uint8_t> skip((size_t)n, 0), occ((size_t)nk, 0);
    for (int k = 0; k < nk; k++) {
        if (matched[k] >= 0) skip[matched[k]] = 1;
        occ[k] = matched[k] != -1;
    }
    a.mps = dev_in(m, mps, (size_t)n, &rc);
    a.skip = dev_in(m, (const uint8_t*)skip.data(), (size_t)n, &rc);
    uint8_t* d_occ = (uint8_t*)m.stage((size_t)nk);
    a.list = (unsigned long long*)m.stage((size_t)n * cap * sizeof(unsigned long long));
    a.count = (int*)m.stage((size_t)n * sizeof(int));
    a.best = (unsigned long long*)m.stage((size_t)n * sizeof(unsigned long long));
    if (rc || !d_occ || !a.list || !a.count || !a.best) return rc ? rc : ORBMI_E_HIP;
    ORBMI_HIP(m.h2d(d_occ, occ.data(), (size_t)nk));
    a.occ = d_occ;
    a.first = 0;
    a.n = n;
    a.th = th;
    ORBMI_HIP(hipMemsetAsync(a.count, 0, (size_t)n * sizeof(int), m.ls()));
    if ((rc = orbmi::launch_proj_sim3(m, F, a))) return rc;
    std::vector<unsigned long long> list((size_t)n * cap);
    std::vector<int> count((size_t)n);
    ORBMI_HIP(hipMemcpyAsync(count.data(), a.count, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, m.ls()));
    ORBMI_HIP(hipMemcpyAsync(list.data(), a.list, list.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, m.ls()));
    ORBMI_HIP(hipStreamSynchronize(m.ls()));
    // the reference's loop in list order: the best unclaimed keypoint, accepted at <= TH_LOW, which
    // is the best unclaimed among the candidates <= TH_LOW
    int found = 0;
    for (int i = 0; i < n; i++) {
        if (count[i] == 0) continue;
        int idx = -1;
        if (count[i] <= cap) {
            unsigned long long* L = &list[(size_t)i * cap];
            std::sort(L, L + count[i]);
            for (int k = 0; k < count[i] && idx < 0; k++)
                if (!occ[L[k] & 0xFFFFF]) idx = (int)(L[k] & 0xFFFFF);
        } else {  // the list overflowed: enumerate this point again against the claims so far
            orbmi::ProjSim3Args b = a;
            b.first = i;
            b.n = 1;
            ORBMI_HIP(m.h2d(d_occ, occ.data(), (size_t)nk));
            ORBMI_HIP(hipMemsetAsync(a.count + i, 0, sizeof(int), m.ls()));
            if ((rc = orbmi::launch_proj_sim3(m, F, b))) return rc;
            unsigned long long best = ~0ull;
            ORBMI_HIP(hipMemcpyAsync(&best, a.best + i, sizeof(best), hipMemcpyDeviceToHost, m.ls()));
            ORBMI_HIP(hipStreamSynchronize(m.ls()));
            if (best != ~0ull && (int)(best >> 40) <= orbmi::TH_LOW) idx = (int)(best & 0xFFFFF);
        }
        if (idx < 0) continue;
        matched[idx] = i;
        occ[idx] = 1;
        found++;
    }
    if (nmatches) *nmatches = found;
    return ORBMI_OK;
}

int orbmi_fuse_sim3_search_batch(orbmi_matcher* h, int nkf, const orbmi_frame_view* kfs, const float* Scw,
                                 const orbmi_mappoint* mps, const uint8_t* in_kf, int n_mp, float th, int32_t* best_idx,
                                 int32_t* best_dist, int* nfused) {
    if (!h || nkf < 0 || n_mp < 0 || (nkf > 0 && (!kfs || !Scw || on_device(Scw))) ||
        (nkf > 0 && n_mp > 0 && (!mps || !best_idx || !best_dist)))
        return ORBMI_E_ARG;
    // one decomposed Scw per keyframe
    std::vector<orbmi::FuseSim3Pose> poses((size_t)nkf);
    for (int k = 0; k < nkf; k++) {
        const float scw = decompose_scw(Scw + 12 * (size_t)k, poses[k].T, poses[k].Ow);
        if (!(scw > 0.0f) || !std::isfinite(scw)) return ORBMI_E_ARG;
    }
    if (nkf == 0 || n_mp == 0) return ORBMI_OK;
    Matcher& m = h->m;
    ORBMI_HIP(hipSetDevice(m.device));
    m.arena_reset();
    int rc = 0;
    const orbmi_mappoint* d_mps = dev_in(m, mps, (size_t)n_mp, &rc);
    const uint8_t* d_in = dev_in(m, in_kf, in_kf ? (size_t)n_mp * nkf : 0, &rc);
    if (rc) return rc;
    std::vector<FuseKF> K(nkf);
    for (int k = 0; k < nkf; k++) {
        memset(&K[k], 0, sizeof(FuseKF));
        if ((rc = make_frame(m, &kfs[k], &K[k].F, false))) return rc;  // the pose is Scw's
        K[k].in_kf = d_in ? d_in + (size_t)k * n_mp : nullptr;
    }
    FuseKF* d_k = (FuseKF*)m.stage(sizeof(FuseKF) * nkf);
    orbmi::FuseSim3Pose* d_p = (orbmi::FuseSim3Pose*)m.stage(sizeof(orbmi::FuseSim3Pose) * nkf);
    int* d_cnt = (int*)m.stage(sizeof(int) * nkf);
    std::vector<OutBuf> outs;
    int* d_bi = dev_out(m, best_idx, (size_t)n_mp * nkf, outs);
    int* d_bd = dev_out(m, best_dist, (size_t)n_mp * nkf, outs);
    if (!d_k || !d_p || !d_cnt || !d_bi || !d_bd) return ORBMI_E_HIP;
    int ncap = 0;
    if ((rc = orbmi::fuse_multi_prepare(m, nkf, K.data(), n_mp, d_bi, d_bd, d_cnt, &ncap))) return rc;
    ORBMI_HIP(m.h2d(d_k, K.data(), sizeof(FuseKF) * nkf));
    ORBMI_HIP(m.h2d(d_p, poses.data(), sizeof(orbmi::FuseSim3Pose) * nkf));
    if ((rc = orbmi::launch_fuse_sim3(m, nkf, d_k, d_p, d_mps, n_mp, th, ncap))) return rc;
    return finish_counts(m, outs, nfused, d_cnt, nkf);
}

namespace {

bool sim3_opt_args_ok(const orbmi_sim3_opt_problem& P) {
    if (P.n < 0) return false;
    return P.n == 0 || (P.x3d_c1 && P.x3d_c2 && P.obs1 && P.obs2 && P.inv_sigma2_1 && P.inv_sigma2_2);
}

// Stage one problem; inlier / chi2 are device arrays of n and 2 n entries
int sim3_opt_stage(Matcher& m, const orbmi_sim3_opt_problem& P, uint8_t* inlier, double* chi2, orbmi::Sim3OptDev* D) {
    int rc = 0;
    memset(D, 0, sizeof(*D));
    const size_t n = (size_t)P.n;
    D->n = P.n;
    D->fix_scale = P.fix_scale != 0;
    D->th2 = P.th2;
    D->x1 = dev_in(m, P.x3d_c1, 3 * n, &rc);
    D->x2 = dev_in(m, P.x3d_c2, 3 * n, &rc);
    D->o1 = dev_in(m, P.obs1, 2 * n, &rc);
    D->o2 = dev_in(m, P.obs2, 2 * n, &rc);
    D->w1 = dev_in(m, P.inv_sigma2_1, n, &rc);
    D->w2 = dev_in(m, P.inv_sigma2_2, n, &rc);
    memcpy(D->k1, P.k1, sizeof(D->k1));
    memcpy(D->k2, P.k2, sizeof(D->k2));
    memcpy(D->R, P.R12, sizeof(D->R));
    memcpy(D->t, P.t12, sizeof(D->t));
    D->s = P.s12;
    D->inlier = inlier;
    D->chi2 = chi2;
    return rc;
}

}  // namespace

int orbmi_optimize_sim3_batch(orbmi_matcher* h, int nproblems, const orbmi_sim3_opt_problem* problems,
                              orbmi_sim3_opt_result* results) {
    if (!h || nproblems < 0 || (nproblems > 0 && (!problems || !results))) return ORBMI_E_ARG;
    for (int k = 0; k < nproblems; k++)
        if (!sim3_opt_args_ok(problems[k]) || (problems[k].n > 0 && !results[k].inlier)) return ORBMI_E_ARG;
    if (nproblems == 0) return ORBMI_OK;
    Matcher& m = h->m;
    ORBMI_HIP(hipSetDevice(m.device));
    m.arena_reset();
    int rc = 0;
    std::vector<OutBuf> outs;
    std::vector<orbmi::Sim3OptDev> T((size_t)nproblems);
    std::vector<orbmi::Sim3OptOut> O((size_t)nproblems);
    for (int k = 0; k < nproblems; k++) {
        const size_t n = (size_t)problems[k].n;
        uint8_t* d_in = n ? dev_out(m, results[k].inlier, n, outs) : (uint8_t*)m.stage(1);
        double* d_chi = n && results[k].chi2 ? dev_out(m, results[k].chi2, 2 * n, outs)
                                             : (double*)m.stage(std::max(2 * n, (size_t)1) * sizeof(double));
        if (!d_in || !d_chi) return ORBMI_E_HIP;
        if ((rc = sim3_opt_stage(m, problems[k], d_in, d_chi, &T[k]))) return rc;
    }
    const orbmi::Sim3OptDev* d_T = dev_in(m, (const orbmi::Sim3OptDev*)T.data(), (size_t)nproblems, &rc);
    if (rc) return rc;
    orbmi::Sim3OptOut* d_O = dev_out(m, O.data(), (size_t)nproblems, outs);
    if (!d_O) return ORBMI_E_HIP;
    if ((rc = orbmi::launch_sim3_opt(m, nproblems, d_T, d_O))) return rc;
    if ((rc = finish(m, outs, nullptr, nullptr))) return rc;  // O is host memory: the call has waited
    for (int k = 0; k < nproblems; k++) {
        orbmi_sim3_opt_result& R = results[k];
        memcpy(R.q, O[k].q, sizeof(R.q));
        memcpy(R.t, O[k].t, sizeof(R.t));
        R.s = O[k].s;
        memcpy(R.sR, O[k].sR, sizeof(R.sR));
        memcpy(R.t_f, O[k].t_f, sizeof(R.t_f));
        R.n_in = O[k].n_in;
        R.n_bad = O[k].n_bad;
        R.iterations[0] = O[k].iterations[0];
        R.iterations[1] = O[k].iterations[1];
    }
    return ORBMI_OK;
}

int orbmi_debug_sim3_opt_linearize(orbmi_matcher* h, const orbmi_sim3_opt_problem* problem, double* H, double* b,
                                   double* chi2) {
    if (!h || !problem || !H || !b || !chi2 || !sim3_opt_args_ok(*problem)) return ORBMI_E_ARG;
    double lin[57] = {};
    if (problem->n > 0) {
        Matcher& m = h->m;
        ORBMI_HIP(hipSetDevice(m.device));
        m.arena_reset();
        int rc = 0;
        std::vector<OutBuf> outs;
        const size_t n = (size_t)problem->n;
        uint8_t* d_in = (uint8_t*)m.stage(n);
        double* d_chi = (double*)m.stage(2 * n * sizeof(double));
        if (!d_in || !d_chi) return ORBMI_E_HIP;
        orbmi::Sim3OptDev T;
        if ((rc = sim3_opt_stage(m, *problem, d_in, d_chi, &T))) return rc;
        const orbmi::Sim3OptDev* d_T = dev_in(m, (const orbmi::Sim3OptDev*)&T, 1, &rc);
        if (rc) return rc;
        double* d_lin = dev_out(m, (double*)lin, 57, outs);
        if (!d_lin) return ORBMI_E_HIP;
        if ((rc = orbmi::launch_sim3_opt_linearize(m, d_T, d_lin))) return rc;
        if ((rc = finish(m, outs, nullptr, nullptr))) return rc;
    }
    memcpy(H, lin, 49 * sizeof(double));
    memcpy(b, lin + 49, 7 * sizeof(double));
    *chi2 = lin[56];
    return ORBMI_OK;
}

}  // extern "C"

namespace {

static_assert(sizeof(orbmi::Sim3d) == 8 * sizeof(double), "a Sim3 is 8 doubles in the C interface");

bool essgraph_args_ok(const orbmi_essgraph_problem& P) {
    if (P.n_vertices < 1 || !P.vertices || P.n_edges < 0 || P.iterations < 0 || P.iterations > 32) return false;
    if (P.fixed < 0 || P.fixed >= P.n_vertices) return false;
    return P.n_edges == 0 || (P.v0 && P.v1 && P.measurements);
}

std::vector<orbmi::EgEdge> essgraph_edges_of(const orbmi_essgraph_problem& P) {
    std::vector<orbmi::EgEdge> E((size_t)P.n_edges);
    for (int e = 0; e < P.n_edges; e++) {
        E[e].v0 = P.v0[e];
        E[e].v1 = P.v1[e];
        memcpy(&E[e].C, P.measurements + 8 * (size_t)e, sizeof(orbmi::Sim3d));
    }
    return E;
}

template <class T>
T* essgraph_put(Matcher& m, const std::vector<T>& v, int* rc) {
    T* d = (T*)m.stage(std::max(v.size(), (size_t)1) * sizeof(T));
    if (!d || m.h2d(d, v.data(), v.size() * sizeof(T)) != hipSuccess) *rc = ORBMI_E_HIP;
    return d;
}

// One call's device state: the plan's tables, the edges and two copies of the estimates
struct EssgraphCall {
    orbmi::EgPlan plan;
    orbmi::EgDev D;
    orbmi::Sim3d *est = nullptr, *trial = nullptr;
};

int essgraph_stage(Matcher& m, const orbmi_essgraph_problem& P, const std::vector<orbmi::EgEdge>& E, EssgraphCall* C) {
    C->plan = orbmi::eg_plan(P.n_vertices, P.fixed, P.n_edges, E.data());
    const orbmi::EgPlan& Q = C->plan;
    if (!orbmi::eg_plan_ok(Q)) return ORBMI_E_ARG;  // every table index against its array, before any launch
    int rc = 0;
    orbmi::EgDev& D = C->D;
    memset(&D, 0, sizeof(D));
    D.nv = Q.nv; D.ne = Q.ne; D.nf = Q.nf; D.nl = Q.nl;
    D.fix_scale = P.fix_scale != 0;
    D.edges = essgraph_put(m, E, &rc);
    D.vert_of = essgraph_put(m, Q.vert_of, &rc);
    D.col_ptr = essgraph_put(m, Q.col_ptr, &rc);
    D.row_of = essgraph_put(m, Q.row_of, &rc);
    D.upd_ptr = essgraph_put(m, Q.upd_ptr, &rc);
    D.upd = essgraph_put(m, Q.upd, &rc);
    D.asm_ptr = essgraph_put(m, Q.asm_ptr, &rc);
    D.asm_ent = essgraph_put(m, Q.asm_ent, &rc);
    auto doubles = [&](size_t n) { return (double*)m.stage(std::max(n, (size_t)1) * sizeof(double)); };
    D.recs = doubles((size_t)Q.ne * orbmi::kEgRec);
    D.Hd = doubles((size_t)Q.nf * 49); D.Ho = doubles((size_t)Q.nl * 49); D.b = doubles((size_t)Q.nf * 7);
    D.Ld = doubles((size_t)Q.nf * 49); D.Lo = doubles((size_t)Q.nl * 49); D.x = doubles((size_t)Q.nf * 7);
    D.y = doubles((size_t)Q.nf * 7);
    D.chi2 = doubles((size_t)Q.ne);
    D.out = doubles(orbmi::kEgOut);
    const size_t vb = (size_t)P.n_vertices * sizeof(orbmi::Sim3d);
    C->est = (orbmi::Sim3d*)m.stage(vb);
    C->trial = (orbmi::Sim3d*)m.stage(vb);
    if (rc || !D.recs || !D.Hd || !D.Ho || !D.b || !D.Ld || !D.Lo || !D.x || !D.y || !D.chi2 || !D.out || !C->est || !C->trial)
        return ORBMI_E_HIP;
    if (m.h2d(C->est, P.vertices, vb) != hipSuccess || m.h2d(C->trial, P.vertices, vb) != hipSuccess) return ORBMI_E_HIP;
    ORBMI_HIP(m.flush_up());
    if (m.up_err != hipSuccess) return ORBMI_E_HIP;
    // fill blocks are never written by the assembly
    if (Q.nl) ORBMI_HIP(hipMemsetAsync(D.Ho, 0, (size_t)Q.nl * 49 * sizeof(double), m.ls()));
    return ORBMI_OK;
}

// HIP events around one phase of a profiled call
struct EssgraphTimer {
    Matcher& m;
    bool on;
    hipEvent_t a = nullptr, b = nullptr;
    EssgraphTimer(Matcher& m_, bool on_) : m(m_), on(on_) {
        if (on && (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess)) on = false;
    }
    ~EssgraphTimer() {
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
    }
    void begin() { if (on) (void)hipEventRecord(a, m.ls()); }
    void end(float* acc) {
        if (!on) return;
        float ms = 0;
        if (hipEventRecord(b, m.ls()) == hipSuccess && hipEventSynchronize(b) == hipSuccess &&
            hipEventElapsedTime(&ms, a, b) == hipSuccess)
            *acc += ms;
    }
};

}  // namespace

extern "C" {

int orbmi_essential_graph_edges(const orbmi_essgraph_input* g, int max_edges, int32_t* v0, int32_t* v1,
                                double* measurements, double* vScw, int* n_edges) {
    if (!g || !n_edges || !vScw || max_edges < 0 || (max_edges > 0 && (!v0 || !v1 || !measurements))) return ORBMI_E_ARG;
    orbmi::EgGraphIn G;
    G.n_ids = g->n_ids;
    G.live = g->live; G.Tcw = g->Tcw; G.parent = g->parent;
    G.loop_off = g->loop_off; G.loop_ids = g->loop_ids;
    G.cov_off = g->cov_off; G.cov_ids = g->cov_ids;
    G.n_corrected = g->n_corrected; G.corrected_ids = g->corrected_ids; G.corrected = (const orbmi::Sim3d*)g->corrected;
    G.n_noncorrected = g->n_noncorrected; G.noncorrected_ids = g->noncorrected_ids;
    G.noncorrected = (const orbmi::Sim3d*)g->noncorrected;
    G.lc_off = g->lc_off; G.lc_ids = g->lc_ids; G.lc_weight = g->lc_weight;
    G.loop_id = g->loop_id; G.cur_id = g->cur_id;
    if (!orbmi::eg_graph_args_ok(G)) return ORBMI_E_ARG;
    std::vector<orbmi::EgGraphEdge> E;
    std::vector<orbmi::Sim3d> S;
    orbmi::eg_graph_edges(G, &E, &S);
    memcpy(vScw, S.data(), S.size() * sizeof(orbmi::Sim3d));
    *n_edges = (int)E.size();
    if ((int)E.size() > max_edges) return ORBMI_E_CAP;
    for (size_t e = 0; e < E.size(); e++) {
        v0[e] = E[e].v0;
        v1[e] = E[e].v1;
        memcpy(measurements + 8 * e, &E[e].S, sizeof(orbmi::Sim3d));
    }
    return ORBMI_OK;
}

int orbmi_optimize_essential_graph(orbmi_matcher* h, const orbmi_essgraph_problem* problem, orbmi_essgraph_result* result) {
    if (!h || !problem || !result || !result->vertices || !essgraph_args_ok(*problem)) return ORBMI_E_ARG;
    const orbmi_essgraph_problem& P = *problem;
    const std::vector<orbmi::EgEdge> E = essgraph_edges_of(P);
    if (!orbmi::eg_args_ok(P.n_vertices, P.fixed, P.n_edges, E.data())) return ORBMI_E_ARG;
    orbmi_essgraph_result& R = *result;
    R.chi2_before = R.chi2_after = 0;
    R.iterations = 0;
    R.status = 0;
    memset(R.trials, 0, sizeof(R.trials));
    memset(R.phase_ms, 0, sizeof(R.phase_ms));
    const size_t vb = (size_t)P.n_vertices * sizeof(orbmi::Sim3d);
    Matcher& m = h->m;
    ORBMI_HIP(hipSetDevice(m.device));
    m.arena_reset();
    EssgraphCall C;
    int rc = essgraph_stage(m, P, E, &C);
    if (rc) return rc;
    if (C.plan.nf == 0 || P.n_edges == 0 || P.iterations == 0) {  // nothing to optimise
        memmove(R.vertices, P.vertices, vb);
        R.status = ORBMI_EG_TERMINATE;
        ORBMI_HIP(hipStreamSynchronize(m.ls()));
        return ORBMI_OK;
    }
    const orbmi::EgDev& D = C.D;
    EssgraphTimer T(m, P.profile != 0);
    orbmi::S3oLm L{};
    double out[orbmi::kEgOut];
    auto read_out = [&]() -> int {
        ORBMI_HIP(hipMemcpyAsync(out, D.out, sizeof(out), hipMemcpyDeviceToHost, m.ls()));
        ORBMI_HIP(hipStreamSynchronize(m.ls()));
        return ORBMI_OK;
    };
    bool stopped = false;
    for (int it = 0; it < P.iterations; it++) {
        T.begin();
        if ((rc = orbmi::launch_eg_linearize(m, D, C.est))) return rc;
        T.end(&R.phase_ms[0]);
        T.begin();
        if ((rc = orbmi::launch_eg_assemble(m, D))) return rc;
        T.end(&R.phase_ms[1]);
        if ((rc = read_out())) return rc;
        if (it == 0) R.chi2_before = out[orbmi::kEgOutChi];
        orbmi::eg_lm_begin(L, it, out[orbmi::kEgOutChi]);
        bool more;
        do {
            T.begin();
            if ((rc = orbmi::launch_eg_factor_solve(m, D, L.lambda))) return rc;
            T.end(&R.phase_ms[2]);
            if ((rc = read_out())) return rc;
            const bool ok2 = out[orbmi::kEgOutFail] == 0;
            const double scale = ok2 ? out[orbmi::kEgOutScale] : 0.0;
            double tempChi = 0;
            if (ok2) {
                T.begin();
                if ((rc = orbmi::launch_eg_update(m, D, C.est, C.trial))) return rc;
                T.end(&R.phase_ms[3]);
                if ((rc = read_out())) return rc;
                tempChi = out[orbmi::kEgOutChi];
            } else {
                R.status |= ORBMI_EG_SOLVE_FAILED;
            }
            if (orbmi::eg_lm_trial(L, ok2, tempChi, scale, &more)) std::swap(C.est, C.trial);  // the step is kept
            else R.status |= ORBMI_EG_REJECTED;  // est still holds the accepted estimates
        } while (more);
        R.trials[it] = L.qmax;
        R.iterations++;
        if (orbmi::s3o_lm_end(L)) {
            stopped = true;
            break;
        }
    }
    if (stopped) R.status |= ORBMI_EG_TERMINATE;
    R.chi2_after = L.currentChi;
    ORBMI_HIP(hipMemcpyAsync(R.vertices, C.est, vb, hipMemcpyDeviceToHost, m.ls()));
    ORBMI_HIP(hipStreamSynchronize(m.ls()));
    return ORBMI_OK;
}

int orbmi_debug_essgraph_linearize(orbmi_matcher* h, const orbmi_essgraph_problem* problem, int32_t* dims,
                                   int32_t* vert_of, int32_t* col_ptr, int32_t* row_of, double* Hd, double* Ho,
                                   double* b, double* chi2) {
    if (!h || !problem || !dims || !essgraph_args_ok(*problem)) return ORBMI_E_ARG;
    const orbmi_essgraph_problem& P = *problem;
    const std::vector<orbmi::EgEdge> E = essgraph_edges_of(P);
    if (!orbmi::eg_args_ok(P.n_vertices, P.fixed, P.n_edges, E.data())) return ORBMI_E_ARG;
    if (!vert_of) {
        const orbmi::EgPlan Q = orbmi::eg_plan(P.n_vertices, P.fixed, P.n_edges, E.data());
        dims[0] = Q.nf;
        dims[1] = Q.nl;
        return ORBMI_OK;
    }
    if (!col_ptr || !row_of || !Hd || !Ho || !b || !chi2) return ORBMI_E_ARG;
    Matcher& m = h->m;
    ORBMI_HIP(hipSetDevice(m.device));
    m.arena_reset();
    EssgraphCall C;
    int rc = essgraph_stage(m, P, E, &C);
    if (rc) return rc;
    const orbmi::EgPlan& Q = C.plan;
    dims[0] = Q.nf;
    dims[1] = Q.nl;
    memcpy(vert_of, Q.vert_of.data(), Q.vert_of.size() * sizeof(int32_t));
    memcpy(col_ptr, Q.col_ptr.data(), Q.col_ptr.size() * sizeof(int32_t));
    memcpy(row_of, Q.row_of.data(), Q.row_of.size() * sizeof(int32_t));
    *chi2 = 0;
    if (Q.ne > 0) {
        if ((rc = orbmi::launch_eg_linearize(m, C.D, C.est))) return rc;
        if ((rc = orbmi::launch_eg_assemble(m, C.D))) return rc;
        ORBMI_HIP(hipMemcpyAsync(chi2, C.D.out + orbmi::kEgOutChi, sizeof(double), hipMemcpyDeviceToHost, m.ls()));
        if (Q.nf) {
            ORBMI_HIP(hipMemcpyAsync(Hd, C.D.Hd, (size_t)Q.nf * 49 * sizeof(double), hipMemcpyDeviceToHost, m.ls()));
            ORBMI_HIP(hipMemcpyAsync(b, C.D.b, (size_t)Q.nf * 7 * sizeof(double), hipMemcpyDeviceToHost, m.ls()));
        }
        if (Q.nl) ORBMI_HIP(hipMemcpyAsync(Ho, C.D.Ho, (size_t)Q.nl * 49 * sizeof(double), hipMemcpyDeviceToHost, m.ls()));
    }
    ORBMI_HIP(hipStreamSynchronize(m.ls()));
    return ORBMI_OK;
}

int orbmi_correct_points_sim3(orbmi_matcher* h, int n_points, const float* points, const int32_t* ref, int n_ref,
                              const double* Srw, const double* Swr_corrected, float* out_points, int n_poses,
                              const double* poses, float* out_tcw) {
    if (!h || n_points < 0 || n_ref < 0 || n_poses < 0) return ORBMI_E_ARG;
    if (n_points > 0 && (!points || !ref || !Srw || !Swr_corrected || !out_points || n_ref < 1)) return ORBMI_E_ARG;
    if (n_poses > 0 && (!poses || !out_tcw)) return ORBMI_E_ARG;
    for (int i = 0; i < n_points; i++)
        if (ref[i] < 0 || ref[i] >= n_ref) return ORBMI_E_ARG;
    if (n_points == 0 && n_poses == 0) return ORBMI_OK;
    Matcher& m = h->m;
    ORBMI_HIP(hipSetDevice(m.device));
    m.arena_reset();
    int rc = 0;
    std::vector<OutBuf> outs;
    const float* d_p = dev_in(m, points, 3 * (size_t)n_points, &rc);
    const int32_t* d_r = dev_in(m, ref, (size_t)n_points, &rc);
    const orbmi::Sim3d* d_a = dev_in(m, (const orbmi::Sim3d*)Srw, n_points ? (size_t)n_ref : 0, &rc);
    const orbmi::Sim3d* d_b = dev_in(m, (const orbmi::Sim3d*)Swr_corrected, n_points ? (size_t)n_ref : 0, &rc);
    const orbmi::Sim3d* d_s = dev_in(m, (const orbmi::Sim3d*)poses, (size_t)n_poses, &rc);
    if (rc) return rc;
    float* d_op = n_points ? dev_out(m, out_points, 3 * (size_t)n_points, outs) : nullptr;
    float* d_ot = n_poses ? dev_out(m, out_tcw, 16 * (size_t)n_poses, outs) : nullptr;
    if ((n_points && !d_op) || (n_poses && !d_ot)) return ORBMI_E_HIP;
    if ((rc = orbmi::launch_eg_correct(m, n_points, d_p, d_r, d_a, d_b, d_op, n_poses, d_s, d_ot))) return rc;
    return finish(m, outs, nullptr, nullptr);
}

int orbmi_debug_greedy_stats(unsigned long long* out, int reset) {
    if (!out) return ORBMI_E_ARG;
    return orbmi::greedy_stats(out, reset);
}

int orbmi_debug_greedy_cycles(unsigned long long* out, int reset) {
    if (!out) return ORBMI_E_ARG;
    return orbmi::greedy_cycles(out, reset);
}

}  // extern "C"
