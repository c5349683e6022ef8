// Host half of KeyFrameDatabase::DetectLoopCandidates (src/KeyFrameDatabase.cc:107-196) and the
// tails of DBoW2's L1 / L2 scores, over the per-slot arrays a database query returns.  No HIP in
// here: tests/cpp/loop_check.cpp runs it stand-alone.
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace orbmi {

// minCommonWords = maxCommonWords * 0.8f (:120): int -> float, one float product, truncation
inline int kfdb_min_common(int max_common) { return (int)((float)max_common * 0.8f); }

// What follows the sum over the shared words in L1Scoring::score (ScoringObject.cpp:65) and
// L2Scoring::score (:114-117); scoring 0 = L1_NORM, 1 = L2_NORM
inline double kfdb_score_tail(int scoring, double sum) {
    if (scoring == 0) return -sum / 2.0;
    if (sum >= 1) return 1.0;
    return 1.0 - sqrt(1.0 - sum);
}

struct KfdbSlots {  // one query's result, per slot
    int n = 0;
    const int32_t* kf_id = nullptr;
    const int32_t* common = nullptr;       // mnLoopWords (0: not in lKFsSharingWords)
    const uint32_t* first_word = nullptr;  // smallest shared word
    const uint64_t* add_seq = nullptr;     // position in every posting list
    const double* score = nullptr;         // mpVoc->score where common > min_common
    int min_common = 0;
};

struct KfdbGraph {  // id -> slot, and GetBestCovisibilityKeyFrames(10) per keyframe id as CSR
    const int32_t* slot_of_id = nullptr;
    int n_ids = 0;
    const int32_t* covis_off = nullptr;
    const int32_t* covis_ids = nullptr;
    int n_covis_kf = 0;
};

// lKFsSharingWords: the reference pushes a keyframe where it first meets it, at its smallest
// shared word, at its place in that word's list: ascending (first_word, add_seq)
inline std::vector<int> kfdb_sharing_order(const KfdbSlots& s) {
    std::vector<int> order;
    for (int i = 0; i < s.n; i++)
        if (s.common[i] > 0) order.push_back(i);
    std::sort(order.begin(), order.end(), [&](int a, int b) {
        if (s.first_word[a] != s.first_word[b]) return s.first_word[a] < s.first_word[b];
        return s.add_seq[a] < s.add_seq[b];
    });
    return order;
}

// :107-196 -> vpLoopCandidates (keyframe ids in the reference's order)
inline std::vector<int32_t> kfdb_select(const KfdbSlots& s, const KfdbGraph& g, float min_score) {
    std::vector<int32_t> out;
    const std::vector<int> order = kfdb_sharing_order(s);
    if (order.empty()) return out;
    struct SM { float score; int slot; };
    std::vector<SM> score_and_match;  // lScoreAndMatch
    for (int slot : order) {
        if (s.common[slot] > s.min_common) {
            const float si = (float)s.score[slot];
            if (si >= min_score) score_and_match.push_back(SM{si, slot});
        }
    }
    if (score_and_match.empty()) return out;
    std::vector<SM> acc_and_match;  // lAccScoreAndMatch
    float best_acc = min_score;
    for (const SM& e : score_and_match) {
        float best = e.score, acc = e.score;
        int best_slot = e.slot;
        const int32_t id = s.kf_id[e.slot];
        if (id >= 0 && id < g.n_covis_kf) {
            for (int k = g.covis_off[id]; k < g.covis_off[id + 1]; k++) {
                const int32_t id2 = g.covis_ids[k];
                if (id2 < 0 || id2 >= g.n_ids) continue;
                const int s2 = g.slot_of_id[id2];
                // mnLoopQuery == pKF->mnId && mnLoopWords > minCommonWords (:159)
                if (s2 < 0 || s2 >= s.n || s.common[s2] <= s.min_common) continue;
                const float sc2 = (float)s.score[s2];  // mLoopScore
                acc += sc2;
                if (sc2 > best) { best_slot = s2; best = sc2; }
            }
        }
        acc_and_match.push_back(SM{acc, best_slot});
        if (acc > best_acc) best_acc = acc;
    }
    const float min_to_retain = 0.75f * best_acc;
    std::vector<uint8_t> added((size_t)s.n, 0);  // spAlreadyAddedKF
    for (const SM& e : acc_and_match) {
        if (e.score > min_to_retain && !added[e.slot]) {
            out.push_back(s.kf_id[e.slot]);
            added[e.slot] = 1;
        }
    }
    return out;
}

}  // namespace orbmi
