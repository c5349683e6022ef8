// KeyFrameDatabase on the device (orbmi_kfdb_*): LoopClosing::DetectLoop's database half.
//
// The reference (src/KeyFrameDatabase.cc:76-139) walks an inverted file of std::list<KeyFrame*>
// per word, bumps mnLoopWords per hit and then scores the survivors one after another with a
// sequential merge of two std::maps.  Here every keyframe's BowVector is stored forward (word ids
// ascending + values) in one arena, and one query intersects the query vector with every indexed
// slot at once: k_kfdb_common counts the shared words per slot (mnLoopWords), their smallest id
// (the key of the reference's list order, kfdb_select.h) and the maximum count; k_kfdb_score
// reads that maximum from device memory and sums the score terms of the slots above the
// threshold.  The sum is the reference's: one fp64 add per shared word in ascending word order
// (a wave-uniform loop over the set bits of each chunk's ballot), no FMA (-ffp-contract=off).
// The tails (-s/2, 1 - sqrt(1 - s)) and everything after :139 run on the host (kfdb_select.h).
#include <algorithm>
#include <mutex>
#include <vector>

#include "kfdb_select.h"
#include "orbmi_common.h"
#include "wave_ops.h"

namespace orbmi {

constexpr int kKfdbMaxQuery = 8192;     // orbmi_transform's limit on a BowVector
constexpr int kKfdbMaxId = 1 << 24;
constexpr int kKfdbMaxBlocks = 1024;

struct KfdbSlot {  // device record
    int off, len, indexed, pad;
};

// lower_bound of w in the ascending q[0, nq); the index is in [0, nq]
__device__ inline int kfdb_lower_bound(const uint32_t* q, int nq, uint32_t w) {
    int lo = 0, hi = nq;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (q[mid] < w) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__device__ inline void kfdb_stage_query(uint32_t* sq, const uint32_t* __restrict__ q_word, int nq) {
    for (int i = threadIdx.x; i < nq; i += blockDim.x) sq[i] = q_word[i];
    __syncthreads();
}

// mnLoopWords, the smallest shared word and maxCommonWords (:86-118).  One wave per slot,
// grid-stride; the slot's words 64 at a time, one word per lane, searched in the query (LDS).
__global__ __launch_bounds__(256) void k_kfdb_common(int nslots, const KfdbSlot* __restrict__ slots,
                                                     const uint32_t* __restrict__ words, int arena_words,
                                                     const uint32_t* __restrict__ q_word, int nq,
                                                     const int* __restrict__ conn, int nconn,
                                                     int* __restrict__ common, uint32_t* __restrict__ first_word,
                                                     int* __restrict__ max_common) {
    __shared__ uint32_t sq[kKfdbMaxQuery];
    nq = min(nq, kKfdbMaxQuery);
    kfdb_stage_query(sq, q_word, nq);
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = gridDim.x * 4;
    int wave_max = 0;
    for (int slot = wave; slot < nslots; slot += nwaves) {
        const KfdbSlot s = slots[slot];
        bool skip = !s.indexed;
        if (!skip && nconn > 0) {  // spConnectedKeyFrames.count(pKFi): a sorted list of slots
            int lo = 0, hi = nconn;
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (conn[mid] < slot) lo = mid + 1; else hi = mid; }
            skip = lo < nconn && conn[lo] == slot;
        }
        int count = 0;
        uint32_t first = 0xFFFFFFFFu;
        if (!skip) {
            const int off = max(s.off, 0);
            const int len = min(s.len, arena_words - off);  // never past the arena
            for (int base = 0; base < len; base += 64) {
                const int i = base + lane;
                bool hit = false;
                uint32_t w = 0;
                if (i < len) {
                    w = words[off + i];
                    const int j = kfdb_lower_bound(sq, nq, w);
                    hit = j < nq && sq[j] == w;
                }
                count += __popcll(__ballot(hit));
                if (hit) first = min(first, w);
            }
            first = (uint32_t)wave_min_u64((unsigned long long)first);
        }
        if (lane == 0) {
            common[slot] = count;
            first_word[slot] = first;
        }
        wave_max = max(wave_max, count);
    }
    if (lane == 0 && wave_max > 0) atomicMax(max_common, wave_max);
}

// The sum over the shared words of mpVoc->score(query, slot) (ScoringObject.cpp:34-59 / :84-109),
// before its tail.  list != nullptr: the n listed slots (orbmi_kfdb_score); else every slot with
// common > (int)(max_common * 0.8f), 0 written elsewhere (:120-133).
__global__ __launch_bounds__(256) void k_kfdb_score(int n, const int* __restrict__ list, int nslots,
                                                    const KfdbSlot* __restrict__ slots,
                                                    const uint32_t* __restrict__ words,
                                                    const double* __restrict__ values, int arena_words,
                                                    const uint32_t* __restrict__ q_word,
                                                    const double* __restrict__ q_value, int nq, int l2,
                                                    const int* __restrict__ common,
                                                    const int* __restrict__ max_common, int* __restrict__ max_out,
                                                    double* __restrict__ sum_out) {
    __shared__ uint32_t sq[kKfdbMaxQuery];
    nq = min(nq, kKfdbMaxQuery);
    kfdb_stage_query(sq, q_word, nq);
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = gridDim.x * 4;
    int min_common = 0;
    if (!list) {
        const int mc = *max_common;
        min_common = (int)((float)mc * 0.8f);
        if (blockIdx.x == 0 && threadIdx.x == 0) *max_out = mc;
    }
    for (int item = wave; item < n; item += nwaves) {
        const int slot = list ? list[item] : item;
        if ((unsigned)slot >= (unsigned)nslots) continue;  // the host wrote the list; checked all the same
        if (!list && common[slot] <= min_common) {
            if (lane == 0) sum_out[item] = 0.0;
            continue;
        }
        const KfdbSlot s = slots[slot];
        const int off = max(s.off, 0);
        const int len = min(s.len, arena_words - off);
        double acc = 0.0;  // the same in every lane
        for (int base = 0; base < len; base += 64) {
            const int i = base + lane;
            bool hit = false;
            double term = 0.0;
            if (i < len) {
                const uint32_t w = words[off + i];
                const int j = kfdb_lower_bound(sq, nq, w);
                hit = j < nq && sq[j] == w;
                if (hit) {
                    const double vi = q_value[j], wi = values[off + i];  // v1 = the query, v2 = the keyframe
                    term = l2 ? vi * wi : fabs(vi - wi) - fabs(vi) - fabs(wi);
                }
            }
            unsigned long long mask = __ballot(hit);
            while (mask) {  // lane order = ascending word order: the reference's sequential sum
                const int l = __builtin_amdgcn_readfirstlane((int)__builtin_ctzll(mask));
                mask &= mask - 1;
                acc += readlane_d(term, l);
            }
        }
        if (lane == 0) sum_out[item] = acc;
    }
}

}  // namespace orbmi

using namespace orbmi;

struct orbmi_kfdb {
    int device = 0, scoring = 0, max_kf = 0, max_words = 0;
    hipStream_t stream = nullptr;
    std::mutex mu;
    // device: the arena and the slot table
    uint32_t* d_word = nullptr;
    double* d_value = nullptr;
    KfdbSlot* d_slot = nullptr;
    // device: one query's inputs (in) and outputs (res), each with a pinned host mirror so that a
    // query is one upload, two kernels and one read-back
    uint8_t* d_in = nullptr; uint8_t* h_in = nullptr; size_t in_bytes = 0;
    uint8_t* d_res = nullptr; uint8_t* h_res = nullptr; size_t res_bytes = 0;
    // host
    struct Slot { int32_t kf_id; int off, len; bool indexed; uint64_t add_seq; };
    std::vector<Slot> slots;
    std::vector<int32_t> slot_of_id;
    int words_used = 0;
    uint64_t add_counter = 0;
};

namespace {

using orbmi::on_device;  // orbmi_common.h

// layout of the query upload: [max_common 16 B][q_value nq f64][q_word nq u32][list n i32]
struct InLayout { size_t value, word, list, total; };
InLayout in_layout(int nq, int nlist) {
    InLayout L;
    L.value = 16;
    L.word = L.value + (size_t)nq * sizeof(double);
    L.list = L.word + (size_t)nq * sizeof(uint32_t);
    L.total = L.list + (size_t)nlist * sizeof(int32_t);
    return L;
}
// layout of the result: [max_common 16 B][sum n f64][common n i32][first_word n u32]
struct ResLayout { size_t sum, common, first, total; };
ResLayout res_layout(int n) {
    ResLayout L;
    L.sum = 16;
    L.common = L.sum + (size_t)n * sizeof(double);
    L.first = L.common + (size_t)n * sizeof(int32_t);
    L.total = L.first + (size_t)n * sizeof(uint32_t);
    return L;
}

int slot_of(const orbmi_kfdb* db, int32_t id) {
    if (id < 0 || (size_t)id >= db->slot_of_id.size()) return -1;
    return db->slot_of_id[(size_t)id];
}

int grid_for(int items) { return std::max(1, std::min((items + 3) / 4, kKfdbMaxBlocks)); }

// Upload the query (and a list of slots) into d_in; device query arrays are copied in place.
int stage_query(orbmi_kfdb* db, const uint32_t* q_word, const double* q_value, int nq, const std::vector<int>& list,
                InLayout* Lout) {
    const InLayout L = in_layout(nq, (int)list.size());
    *Lout = L;
    const bool dev = nq > 0 && on_device(q_word);
    if (nq > 0 && dev != on_device(q_value)) return ORBMI_E_ARG;
    memset(db->h_in, 0, 16);
    if (!list.empty()) memcpy(db->h_in + L.list, list.data(), list.size() * sizeof(int));
    if (nq > 0 && !dev) {
        for (int i = 1; i < nq; i++)
            if (q_word[i] <= q_word[i - 1]) return ORBMI_E_ARG;
        memcpy(db->h_in + L.value, q_value, (size_t)nq * sizeof(double));
        memcpy(db->h_in + L.word, q_word, (size_t)nq * sizeof(uint32_t));
        ORBMI_HIP(hipMemcpyAsync(db->d_in, db->h_in, L.total, hipMemcpyHostToDevice, db->stream));
    } else {
        ORBMI_HIP(hipMemcpyAsync(db->d_in, db->h_in, 16, hipMemcpyHostToDevice, db->stream));
        if (!list.empty())
            ORBMI_HIP(hipMemcpyAsync(db->d_in + L.list, db->h_in + L.list, list.size() * sizeof(int),
                                     hipMemcpyHostToDevice, db->stream));
        if (nq > 0) {
            ORBMI_HIP(hipMemcpyAsync(db->d_in + L.value, q_value, (size_t)nq * sizeof(double), hipMemcpyDeviceToDevice,
                                     db->stream));
            ORBMI_HIP(hipMemcpyAsync(db->d_in + L.word, q_word, (size_t)nq * sizeof(uint32_t), hipMemcpyDeviceToDevice,
                                     db->stream));
        }
    }
    return ORBMI_OK;
}

// The device part of a query; afterwards h_res holds the result (sums with their tails applied).
int run_query(orbmi_kfdb* db, const uint32_t* q_word, const double* q_value, int nq, const int32_t* connected_ids,
              int n_connected, int* max_common) {
    if (nq < 0 || nq > kKfdbMaxQuery || n_connected < 0 || (nq > 0 && (!q_word || !q_value)) ||
        (n_connected > 0 && !connected_ids))
        return nq > kKfdbMaxQuery ? ORBMI_E_UNSUPPORTED : ORBMI_E_ARG;
    const int n = (int)db->slots.size();
    *max_common = 0;
    if (n == 0) return ORBMI_OK;
    std::vector<int> conn;
    for (int i = 0; i < n_connected; i++) {
        const int s = slot_of(db, connected_ids[i]);
        if (s >= 0) conn.push_back(s);
    }
    std::sort(conn.begin(), conn.end());
    conn.erase(std::unique(conn.begin(), conn.end()), conn.end());
    InLayout I;
    int rc;
    if ((rc = stage_query(db, q_word, q_value, nq, conn, &I))) return rc;
    const ResLayout R = res_layout(n);
    int* d_max = (int*)db->d_in;
    const uint32_t* dq_word = (const uint32_t*)(db->d_in + I.word);
    const double* dq_value = (const double*)(db->d_in + I.value);
    int* d_common = (int*)(db->d_res + R.common);
    hipLaunchKernelGGL(k_kfdb_common, dim3(grid_for(n)), dim3(256), 0, db->stream, n, db->d_slot, db->d_word,
                       db->max_words, dq_word, nq, (const int*)(db->d_in + I.list), (int)conn.size(), d_common,
                       (uint32_t*)(db->d_res + R.first), d_max);
    hipLaunchKernelGGL(k_kfdb_score, dim3(grid_for(n)), dim3(256), 0, db->stream, n, (const int*)nullptr, n,
                       db->d_slot, db->d_word, db->d_value, db->max_words, dq_word, dq_value, nq,
                       db->scoring == 1 ? 1 : 0, d_common, d_max, (int*)db->d_res, (double*)(db->d_res + R.sum));
    ORBMI_HIP(hipGetLastError());
    ORBMI_HIP(hipMemcpyAsync(db->h_res, db->d_res, R.total, hipMemcpyDeviceToHost, db->stream));
    ORBMI_HIP(hipStreamSynchronize(db->stream));
    *max_common = *(const int*)db->h_res;
    const int min_common = kfdb_min_common(*max_common);
    double* sum = (double*)(db->h_res + R.sum);
    const int* common = (const int*)(db->h_res + R.common);
    for (int i = 0; i < n; i++) sum[i] = common[i] > min_common ? kfdb_score_tail(db->scoring, sum[i]) : 0.0;
    return ORBMI_OK;
}

void fill_result(orbmi_kfdb* db, int max_common, orbmi_kfdb_query_result* out, std::vector<int32_t>* ids,
                 std::vector<uint64_t>* seq) {
    const int n = (int)db->slots.size();
    const ResLayout R = res_layout(n);
    if (out) {
        out->n_slots = n;
        out->max_common = max_common;
        out->min_common = kfdb_min_common(max_common);
        if (n && out->common) memcpy(out->common, db->h_res + R.common, (size_t)n * sizeof(int32_t));
        if (n && out->first_word) memcpy(out->first_word, db->h_res + R.first, (size_t)n * sizeof(uint32_t));
        if (n && out->score) memcpy(out->score, db->h_res + R.sum, (size_t)n * sizeof(double));
        for (int i = 0; i < n; i++) {
            if (out->kf_id) out->kf_id[i] = db->slots[(size_t)i].kf_id;
            if (out->add_seq) out->add_seq[i] = db->slots[(size_t)i].add_seq;
        }
    }
    if (ids) {
        ids->resize((size_t)n);
        seq->resize((size_t)n);
        for (int i = 0; i < n; i++) {
            (*ids)[(size_t)i] = db->slots[(size_t)i].kf_id;
            (*seq)[(size_t)i] = db->slots[(size_t)i].add_seq;
        }
    }
}

void kfdb_free(orbmi_kfdb* db) {
    if (db->d_word) (void)hipFree(db->d_word);
    if (db->d_value) (void)hipFree(db->d_value);
    if (db->d_slot) (void)hipFree(db->d_slot);
    if (db->d_in) (void)hipFree(db->d_in);
    if (db->d_res) (void)hipFree(db->d_res);
    if (db->h_in) (void)hipHostFree(db->h_in);
    if (db->h_res) (void)hipHostFree(db->h_res);
    if (db->stream) (void)hipStreamDestroy(db->stream);
    delete db;
}

int set_indexed(orbmi_kfdb* db, int slot, bool on) {
    const int v = on ? 1 : 0;
    ORBMI_HIP(hipMemcpyAsync(&db->d_slot[slot].indexed, &v, sizeof(int), hipMemcpyHostToDevice, db->stream));
    ORBMI_HIP(hipStreamSynchronize(db->stream));  // v is a local
    return ORBMI_OK;
}

}  // namespace

extern "C" {

int orbmi_kfdb_create(int device, int scoring, int max_keyframes, int max_words_total, orbmi_kfdb** out) {
    if (!out || max_keyframes < 1 || max_words_total < 1) return ORBMI_E_ARG;
    if (scoring < 0 || scoring > 5) return ORBMI_E_ARG;
    if (scoring > 1) return ORBMI_E_UNSUPPORTED;  // CHI_SQUARE, KL, BHATTACHARYYA, DOT_PRODUCT
    ORBMI_HIP(hipSetDevice(device));
    orbmi_kfdb* db = new orbmi_kfdb;
    db->device = device; db->scoring = scoring; db->max_kf = max_keyframes; db->max_words = max_words_total;
    db->in_bytes = in_layout(kKfdbMaxQuery, max_keyframes).total;
    db->res_bytes = res_layout(max_keyframes).total;
    hipError_t e = stream_create(&db->stream, "MATCHER");
    if (e == hipSuccess) e = hipMalloc((void**)&db->d_word, (size_t)max_words_total * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void**)&db->d_value, (size_t)max_words_total * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&db->d_slot, (size_t)max_keyframes * sizeof(KfdbSlot));
    if (e == hipSuccess) e = hipMalloc((void**)&db->d_in, db->in_bytes);
    if (e == hipSuccess) e = hipMalloc((void**)&db->d_res, db->res_bytes);
    if (e == hipSuccess) e = hipHostMalloc((void**)&db->h_in, db->in_bytes, hipHostMallocDefault);
    if (e == hipSuccess) e = hipHostMalloc((void**)&db->h_res, db->res_bytes, hipHostMallocDefault);
    if (e != hipSuccess) {
        fprintf(stderr, "orbmi: orbmi_kfdb_create failed: %s\n", hipGetErrorString(e));
        kfdb_free(db);
        return ORBMI_E_HIP;
    }
    *out = db;
    return ORBMI_OK;
}

void orbmi_kfdb_destroy(orbmi_kfdb* db) {
    if (!db) return;
    (void)hipSetDevice(db->device);
    if (db->stream) (void)hipStreamSynchronize(db->stream);
    kfdb_free(db);
}

int orbmi_kfdb_clear(orbmi_kfdb* db) {
    if (!db) return ORBMI_E_ARG;
    std::lock_guard<std::mutex> lock(db->mu);
    db->slots.clear();
    db->slot_of_id.clear();
    db->words_used = 0;
    db->add_counter = 0;
    return ORBMI_OK;
}

int orbmi_kfdb_store(orbmi_kfdb* db, int32_t kf_id, const uint32_t* word, const double* value, int n) {
    if (!db || kf_id < 0 || kf_id >= kKfdbMaxId || n < 0 || (n > 0 && (!word || !value))) return ORBMI_E_ARG;
    if (n > kKfdbMaxQuery) return ORBMI_E_UNSUPPORTED;
    std::lock_guard<std::mutex> lock(db->mu);
    ORBMI_HIP(hipSetDevice(db->device));
    if (slot_of(db, kf_id) >= 0) return ORBMI_E_STATE;
    const bool dev = n > 0 && on_device(word);
    if (n > 0 && dev != on_device(value)) return ORBMI_E_ARG;
    if (!dev)
        for (int i = 1; i < n; i++)
            if (word[i] <= word[i - 1]) return ORBMI_E_ARG;
    if ((int)db->slots.size() >= db->max_kf || n > db->max_words - db->words_used) return ORBMI_E_CAP;
    const int slot = (int)db->slots.size(), off = db->words_used;
    const KfdbSlot rec{off, n, 0, 0};
    const hipMemcpyKind kind = dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    if (n > 0) {
        ORBMI_HIP(hipMemcpyAsync(db->d_word + off, word, (size_t)n * sizeof(uint32_t), kind, db->stream));
        ORBMI_HIP(hipMemcpyAsync(db->d_value + off, value, (size_t)n * sizeof(double), kind, db->stream));
    }
    ORBMI_HIP(hipMemcpyAsync(&db->d_slot[slot], &rec, sizeof(rec), hipMemcpyHostToDevice, db->stream));
    ORBMI_HIP(hipStreamSynchronize(db->stream));  // the caller's arrays and rec are free again
    db->slots.push_back(orbmi_kfdb::Slot{kf_id, off, n, false, 0});
    if ((size_t)kf_id >= db->slot_of_id.size()) db->slot_of_id.resize((size_t)kf_id + 1, -1);
    db->slot_of_id[(size_t)kf_id] = slot;
    db->words_used += n;
    return ORBMI_OK;
}

int orbmi_kfdb_add(orbmi_kfdb* db, int32_t kf_id) {
    if (!db) return ORBMI_E_ARG;
    std::lock_guard<std::mutex> lock(db->mu);
    const int slot = slot_of(db, kf_id);
    if (slot < 0) return ORBMI_E_ARG;
    if (db->slots[(size_t)slot].indexed) return ORBMI_E_STATE;
    ORBMI_HIP(hipSetDevice(db->device));
    int rc;
    if ((rc = set_indexed(db, slot, true))) return rc;
    db->slots[(size_t)slot].indexed = true;
    db->slots[(size_t)slot].add_seq = ++db->add_counter;
    return ORBMI_OK;
}

int orbmi_kfdb_erase(orbmi_kfdb* db, int32_t kf_id) {
    if (!db) return ORBMI_E_ARG;
    std::lock_guard<std::mutex> lock(db->mu);
    const int slot = slot_of(db, kf_id);
    if (slot < 0) return ORBMI_E_ARG;
    if (!db->slots[(size_t)slot].indexed) return ORBMI_OK;
    ORBMI_HIP(hipSetDevice(db->device));
    int rc;
    if ((rc = set_indexed(db, slot, false))) return rc;
    db->slots[(size_t)slot].indexed = false;
    return ORBMI_OK;
}

int orbmi_kfdb_score(orbmi_kfdb* db, const uint32_t* q_word, const double* q_value, int nq, const int32_t* kf_ids,
                     int n, double* out_score) {
    if (!db || nq < 0 || n < 0 || (nq > 0 && (!q_word || !q_value)) || (n > 0 && (!kf_ids || !out_score)))
        return ORBMI_E_ARG;
    if (nq > kKfdbMaxQuery) return ORBMI_E_UNSUPPORTED;
    std::lock_guard<std::mutex> lock(db->mu);
    ORBMI_HIP(hipSetDevice(db->device));
    std::vector<int> list((size_t)n);
    for (int i = 0; i < n; i++)
        if ((list[(size_t)i] = slot_of(db, kf_ids[i])) < 0) return ORBMI_E_ARG;
    const int nslots = (int)db->slots.size();
    for (int done = 0; done < n; done += db->max_kf) {  // the list buffers hold max_keyframes entries
        const int m = std::min(n - done, db->max_kf);
        const std::vector<int> part(list.begin() + done, list.begin() + done + m);
        InLayout I;
        int rc;
        if ((rc = stage_query(db, q_word, q_value, nq, part, &I))) return rc;
        const ResLayout R = res_layout(m);
        hipLaunchKernelGGL(k_kfdb_score, dim3(grid_for(m)), dim3(256), 0, db->stream, m,
                           (const int*)(db->d_in + I.list), nslots, db->d_slot, db->d_word, db->d_value, db->max_words,
                           (const uint32_t*)(db->d_in + I.word), (const double*)(db->d_in + I.value), nq,
                           db->scoring == 1 ? 1 : 0, (const int*)nullptr, (const int*)nullptr, (int*)nullptr,
                           (double*)(db->d_res + R.sum));
        ORBMI_HIP(hipGetLastError());
        ORBMI_HIP(hipMemcpyAsync(db->h_res + R.sum, db->d_res + R.sum, (size_t)m * sizeof(double),
                                 hipMemcpyDeviceToHost, db->stream));
        ORBMI_HIP(hipStreamSynchronize(db->stream));
        const double* sum = (const double*)(db->h_res + R.sum);
        for (int i = 0; i < m; i++) out_score[done + i] = kfdb_score_tail(db->scoring, sum[i]);
    }
    return ORBMI_OK;
}

int orbmi_kfdb_query(orbmi_kfdb* db, const uint32_t* q_word, const double* q_value, int nq,
                     const int32_t* connected_ids, int n_connected, orbmi_kfdb_query_result* out) {
    if (!db || !out) return ORBMI_E_ARG;
    std::lock_guard<std::mutex> lock(db->mu);
    ORBMI_HIP(hipSetDevice(db->device));
    int max_common = 0, rc;
    if ((rc = run_query(db, q_word, q_value, nq, connected_ids, n_connected, &max_common))) return rc;
    fill_result(db, max_common, out, nullptr, nullptr);
    return ORBMI_OK;
}

int orbmi_detect_loop_candidates(orbmi_kfdb* db, const uint32_t* q_word, const double* q_value, int nq,
                                 float min_score, const int32_t* connected_ids, int n_connected,
                                 const int32_t* best_covis_off, const int32_t* best_covis_ids, int n_covis_kf,
                                 int32_t* out_ids, int out_capacity, int* n_out) {
    if (!db || !n_out || out_capacity < 0 || (out_capacity > 0 && !out_ids) || n_covis_kf < 0 ||
        (n_covis_kf > 0 && !best_covis_off))
        return ORBMI_E_ARG;
    std::lock_guard<std::mutex> lock(db->mu);
    ORBMI_HIP(hipSetDevice(db->device));
    *n_out = 0;
    int max_common = 0, rc;
    if ((rc = run_query(db, q_word, q_value, nq, connected_ids, n_connected, &max_common))) return rc;
    const int n = (int)db->slots.size();
    if (n == 0) return ORBMI_OK;
    std::vector<int32_t> ids;
    std::vector<uint64_t> seq;
    fill_result(db, max_common, nullptr, &ids, &seq);
    const ResLayout R = res_layout(n);
    KfdbSlots S;
    S.n = n; S.kf_id = ids.data(); S.add_seq = seq.data();
    S.common = (const int32_t*)(db->h_res + R.common);
    S.first_word = (const uint32_t*)(db->h_res + R.first);
    S.score = (const double*)(db->h_res + R.sum);
    S.min_common = kfdb_min_common(max_common);
    KfdbGraph G;
    G.slot_of_id = db->slot_of_id.data(); G.n_ids = (int)db->slot_of_id.size();
    G.covis_off = best_covis_off; G.covis_ids = best_covis_ids; G.n_covis_kf = n_covis_kf;
    const std::vector<int32_t> cand = kfdb_select(S, G, min_score);
    *n_out = (int)cand.size();
    if ((int)cand.size() > out_capacity) return ORBMI_E_CAP;
    if (!cand.empty()) memcpy(out_ids, cand.data(), cand.size() * sizeof(int32_t));
    return ORBMI_OK;
}

}  // extern "C"
