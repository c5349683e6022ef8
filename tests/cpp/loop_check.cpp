// Stand-alone host program over csrc/kfdb_select.h (no HIP): the host tail of
// KeyFrameDatabase::DetectLoopCandidates and the score tails on cases written by
// tests/test_loop_cpu.py, and a scalar inverted-file DetectLoopCandidates for tools/loop_bench.py
// to time on the host (a plain port of the algorithm for comparison, not the reference program).
//
//   loop_check select IN OUT    the case in IN -> OUT: int32 count, the candidate ids, int32 count,
//                               the sharing order (keyframe ids)
//   loop_check tail IN OUT      n doubles -> n L1 tails, n L2 tails
//   loop_check invfile IN REPS  build the inverted file from IN, run the query REPS times, print
//                               the candidates and the median microseconds per query
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <list>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "kfdb_select.h"

namespace {

struct Reader {
    std::vector<unsigned char> b;
    size_t o = 0;
    bool ok = true;
    explicit Reader(const char* path) {
        FILE* f = fopen(path, "rb");
        if (!f) { ok = false; return; }
        fseek(f, 0, SEEK_END);
        const long n = ftell(f);
        fseek(f, 0, SEEK_SET);
        b.resize(n > 0 ? (size_t)n : 0);
        if (n > 0 && fread(b.data(), 1, (size_t)n, f) != (size_t)n) ok = false;
        fclose(f);
    }
    template <class T>
    std::vector<T> take(size_t n) {
        std::vector<T> v(n);
        if (o + n * sizeof(T) > b.size()) { ok = false; return v; }
        if (n) memcpy(v.data(), b.data() + o, n * sizeof(T));
        o += n * sizeof(T);
        return v;
    }
};

template <class T>
void put(FILE* f, const std::vector<T>& v) {
    if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f);
}

int fail(const char* what) {
    fprintf(stderr, "loop_check: %s\n", what);
    return 2;
}

int run_select(const char* in, const char* out) {
    Reader r(in);
    if (!r.ok) return fail("cannot read the case");
    const std::vector<int32_t> head = r.take<int32_t>(5);  // n, min_common, n_ids, n_covis_kf, ncovis
    const std::vector<float> min_score = r.take<float>(1);
    if (!r.ok || head[0] < 0 || head[2] < 0 || head[3] < 0 || head[4] < 0) return fail("bad header");
    const size_t n = (size_t)head[0];
    const std::vector<int32_t> kf_id = r.take<int32_t>(n), common = r.take<int32_t>(n);
    const std::vector<uint32_t> first = r.take<uint32_t>(n);
    const std::vector<uint64_t> seq = r.take<uint64_t>(n);
    const std::vector<double> score = r.take<double>(n);
    const std::vector<int32_t> slot_of_id = r.take<int32_t>((size_t)head[2]);
    const std::vector<int32_t> off = r.take<int32_t>((size_t)head[3] + 1), ids = r.take<int32_t>((size_t)head[4]);
    if (!r.ok) return fail("short case");
    for (size_t k = 0; k + 1 < off.size(); k++)
        if (off[k] < 0 || off[k] > off[k + 1] || off[k + 1] > head[4]) return fail("bad CSR");
    orbmi::KfdbSlots S;
    S.n = (int)n; S.kf_id = kf_id.data(); S.common = common.data(); S.first_word = first.data();
    S.add_seq = seq.data(); S.score = score.data(); S.min_common = head[1];
    orbmi::KfdbGraph G;
    G.slot_of_id = slot_of_id.data(); G.n_ids = head[2]; G.covis_off = off.data(); G.covis_ids = ids.data();
    G.n_covis_kf = head[3];
    const std::vector<int32_t> cand = orbmi::kfdb_select(S, G, min_score[0]);
    std::vector<int32_t> order;
    for (int s : orbmi::kfdb_sharing_order(S)) order.push_back(kf_id[(size_t)s]);
    FILE* f = fopen(out, "wb");
    if (!f) return fail("cannot write");
    put(f, std::vector<int32_t>{(int32_t)cand.size()});
    put(f, cand);
    put(f, std::vector<int32_t>{(int32_t)order.size()});
    put(f, order);
    fclose(f);
    return 0;
}

int run_tail(const char* in, const char* out) {
    Reader r(in);
    if (!r.ok) return fail("cannot read the sums");
    const std::vector<double> s = r.take<double>(r.b.size() / sizeof(double));
    std::vector<double> t;
    for (int scoring = 0; scoring < 2; scoring++)
        for (double v : s) t.push_back(orbmi::kfdb_score_tail(scoring, v));
    FILE* f = fopen(out, "wb");
    if (!f) return fail("cannot write");
    put(f, t);
    fclose(f);
    return 0;
}

// ---- a scalar inverted-file database, for the host timing ---------------------------------------

struct HostKF {
    std::vector<uint32_t> word;
    std::vector<double> value;
    long query = -1;
    int words = 0;
    float score = 0.f;
};

double host_score(int scoring, const HostKF& a, const HostKF& b) {
    size_t i = 0, j = 0;
    double s = 0;
    while (i < a.word.size() && j < b.word.size()) {
        if (a.word[i] == b.word[j]) {
            const double vi = a.value[i], wi = b.value[j];
            s += scoring == 0 ? fabs(vi - wi) - fabs(vi) - fabs(wi) : vi * wi;
            i++; j++;
        } else if (a.word[i] < b.word[j]) {
            i = (size_t)(std::lower_bound(a.word.begin() + (long)i, a.word.end(), b.word[j]) - a.word.begin());
        } else {
            j = (size_t)(std::lower_bound(b.word.begin() + (long)j, b.word.end(), a.word[i]) - b.word.begin());
        }
    }
    return orbmi::kfdb_score_tail(scoring, s);
}

int run_invfile(const char* in, int reps) {
    Reader r(in);
    if (!r.ok) return fail("cannot read the database");
    // scoring, nkf, nwords_vocab, nq, n_connected, ncovis ; min_score ; per keyframe: n, words, values ;
    // the query ; connected ids ; covis_off (nkf + 1), covis_ids
    const std::vector<int32_t> head = r.take<int32_t>(6);
    const std::vector<float> min_score = r.take<float>(1);
    if (!r.ok || head[1] < 0 || head[2] < 1 || head[3] < 0 || head[4] < 0 || head[5] < 0) return fail("bad header");
    const int scoring = head[0], nkf = head[1];
    std::vector<HostKF> kfs((size_t)nkf);
    std::vector<std::list<int>> inverted((size_t)head[2]);
    for (int k = 0; k < nkf; k++) {
        const std::vector<int32_t> n = r.take<int32_t>(1);
        if (!r.ok || n[0] < 0) return fail("short database");
        kfs[(size_t)k].word = r.take<uint32_t>((size_t)n[0]);
        kfs[(size_t)k].value = r.take<double>((size_t)n[0]);
        for (uint32_t w : kfs[(size_t)k].word) {
            if (w >= (uint32_t)head[2]) return fail("word outside the vocabulary");
            inverted[w].push_back(k);
        }
    }
    HostKF q;
    q.word = r.take<uint32_t>((size_t)head[3]);
    q.value = r.take<double>((size_t)head[3]);
    const std::vector<int32_t> conn = r.take<int32_t>((size_t)head[4]);
    const std::vector<int32_t> off = r.take<int32_t>((size_t)nkf + 1), cov = r.take<int32_t>((size_t)head[5]);
    if (!r.ok) return fail("short database");
    for (uint32_t w : q.word)
        if (w >= (uint32_t)head[2]) return fail("word outside the vocabulary");
    for (int k = 0; k < nkf; k++)
        if (off[(size_t)k] < 0 || off[(size_t)k] > off[(size_t)k + 1] || off[(size_t)k + 1] > head[5]) return fail("bad CSR");
    for (int32_t c : cov)
        if (c < 0 || c >= nkf) return fail("bad covisible id");
    const std::set<int> connected(conn.begin(), conn.end());
    std::vector<double> us;
    std::vector<int> result;
    for (int rep = 0; rep < std::max(reps, 1); rep++) {
        const auto t0 = std::chrono::steady_clock::now();
        const long qid = rep;
        std::list<int> sharing;
        for (uint32_t w : q.word)
            for (int k : inverted[w]) {
                HostKF& kf = kfs[(size_t)k];
                if (kf.query != qid) {
                    kf.words = 0;
                    if (!connected.count(k)) { kf.query = qid; sharing.push_back(k); }
                }
                kf.words++;
            }
        result.clear();
        if (!sharing.empty()) {
            int maxc = 0;
            for (int k : sharing) maxc = std::max(maxc, kfs[(size_t)k].words);
            const int minc = orbmi::kfdb_min_common(maxc);
            std::list<std::pair<float, int>> scored, acc;
            for (int k : sharing)
                if (kfs[(size_t)k].words > minc) {
                    const float si = (float)host_score(scoring, q, kfs[(size_t)k]);
                    kfs[(size_t)k].score = si;
                    if (si >= min_score[0]) scored.push_back({si, k});
                }
            float best_acc = min_score[0];
            for (const auto& e : scored) {
                float best = e.first, a = e.first;
                int bk = e.second;
                for (int i = off[(size_t)e.second]; i < off[(size_t)e.second + 1]; i++) {
                    const HostKF& k2 = kfs[(size_t)cov[(size_t)i]];
                    if (k2.query == qid && k2.words > minc) {
                        a += k2.score;
                        if (k2.score > best) { bk = cov[(size_t)i]; best = k2.score; }
                    }
                }
                acc.push_back({a, bk});
                if (a > best_acc) best_acc = a;
            }
            const float keep = 0.75f * best_acc;
            std::set<int> added;
            for (const auto& e : acc)
                if (e.first > keep && !added.count(e.second)) { result.push_back(e.second); added.insert(e.second); }
        }
        us.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
    }
    std::sort(us.begin(), us.end());
    printf("candidates");
    for (int k : result) printf(" %d", k);
    printf("\nmedian_us %.3f min_us %.3f max_us %.3f reps %zu\n", us[us.size() / 2], us.front(), us.back(), us.size());
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 4 && !strcmp(argv[1], "select")) return run_select(argv[2], argv[3]);
    if (argc == 4 && !strcmp(argv[1], "tail")) return run_tail(argv[2], argv[3]);
    if (argc == 4 && !strcmp(argv[1], "invfile")) return run_invfile(argv[2], atoi(argv[3]));
    fprintf(stderr, "usage: loop_check select|tail IN OUT | invfile IN REPS\n");
    return 2;
}
