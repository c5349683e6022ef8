// The edge list of Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:862-1053) over arrays indexed
// by keyframe id.  No HIP in here: tests/cpp/essgraph_check.cpp runs it stand-alone.
//
// The reference walks std::map<KeyFrame*, ...> and std::set<KeyFrame*> in pointer order, which no
// two runs share.  Everywhere a pointer order is meant the order here is ascending keyframe id:
// the keyframes of the map, the keys and the sets of LoopConnections, and a keyframe's loop edges.
// GetCovisiblesByWeight(100) keeps the order its caller lists.  The order only sets the order in
// which the edges are summed.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <set>
#include <utility>
#include <vector>

#include "sim3_opt.h"

namespace orbmi {

struct EgGraphIn {
    int n_ids = 0;                      // nMaxKFid + 1
    const uint8_t* live = nullptr;      // n_ids: the keyframe exists and is not bad
    const float* Tcw = nullptr;         // n_ids x 16, row-major 4x4
    const int32_t* parent = nullptr;    // n_ids, -1: none
    const int32_t* loop_off = nullptr;  // n_ids + 1: GetLoopEdges as CSR
    const int32_t* loop_ids = nullptr;
    const int32_t* cov_off = nullptr;   // n_ids + 1: GetCovisiblesByWeight(100), in that function's order
    const int32_t* cov_ids = nullptr;
    int n_corrected = 0;                // CorrectedSim3
    const int32_t* corrected_ids = nullptr;
    const Sim3d* corrected = nullptr;
    int n_noncorrected = 0;             // NonCorrectedSim3
    const int32_t* noncorrected_ids = nullptr;
    const Sim3d* noncorrected = nullptr;
    const int32_t* lc_off = nullptr;    // n_ids + 1: LoopConnections as CSR, with GetWeight of each pair
    const int32_t* lc_ids = nullptr;
    const int32_t* lc_weight = nullptr;
    int loop_id = -1, cur_id = -1;
};

struct EgGraphEdge {
    int32_t v0, v1;  // keyframe ids
    Sim3d S;         // the measurement
};

inline bool eg_graph_args_ok(const EgGraphIn& G) {
    const int n = G.n_ids;
    if (n < 1 || !G.live || !G.Tcw || !G.parent || !G.loop_off || !G.cov_off || !G.lc_off) return false;
    auto id_ok = [&](int id) { return id >= 0 && id < n && G.live[id]; };
    if (!id_ok(G.loop_id) || !id_ok(G.cur_id)) return false;
    auto csr_ok = [&](const int32_t* off, const int32_t* ids) {
        if (off[0] != 0) return false;
        for (int i = 0; i < n; i++)
            if (off[i] > off[i + 1]) return false;
        if (off[n] > 0 && !ids) return false;
        for (int k = 0; k < off[n]; k++)
            if (!id_ok(ids[k])) return false;
        return true;
    };
    if (!csr_ok(G.loop_off, G.loop_ids) || !csr_ok(G.cov_off, G.cov_ids) || !csr_ok(G.lc_off, G.lc_ids)) return false;
    if (G.lc_off[n] > 0 && !G.lc_weight) return false;
    for (int i = 0; i < n; i++) {
        if (G.parent[i] >= n || (G.live[i] && G.parent[i] >= 0 && !G.live[G.parent[i]])) return false;
        if (!G.live[i] && (G.lc_off[i + 1] > G.lc_off[i])) return false;
    }
    if (G.n_corrected < 0 || G.n_noncorrected < 0) return false;
    if (G.n_corrected > 0 && (!G.corrected_ids || !G.corrected)) return false;
    if (G.n_noncorrected > 0 && (!G.noncorrected_ids || !G.noncorrected)) return false;
    for (int k = 0; k < G.n_corrected; k++)
        if (!id_ok(G.corrected_ids[k])) return false;
    for (int k = 0; k < G.n_noncorrected; k++)
        if (!id_ok(G.noncorrected_ids[k])) return false;
    return true;
}

// -> the edges and vScw (n_ids; the identity where no keyframe lives)
inline void eg_graph_edges(const EgGraphIn& G, std::vector<EgGraphEdge>* edges, std::vector<Sim3d>* vScw) {
    const int n = G.n_ids, minFeat = 100;
    std::vector<int> corr((size_t)n, -1), nonc((size_t)n, -1);
    for (int k = 0; k < G.n_corrected; k++) corr[G.corrected_ids[k]] = k;
    for (int k = 0; k < G.n_noncorrected; k++) nonc[G.noncorrected_ids[k]] = k;
    const Sim3d ident{{0, 0, 0, 1}, {0, 0, 0}, 1};
    vScw->assign((size_t)n, ident);
    for (int i = 0; i < n; i++) {  // :872-888
        if (!G.live[i]) continue;
        if (corr[i] >= 0) {
            (*vScw)[i] = G.corrected[corr[i]];
        } else {
            const float* T = G.Tcw + 16 * (size_t)i;
            const float R[9] = {T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10]}, t[3] = {T[3], T[7], T[11]};
            s3o_from_rts(R, t, 1.0f, &(*vScw)[i]);
        }
    }
    auto push = [&](int i, int j, const Sim3d& Sjw, const Sim3d& Swi) {
        EgGraphEdge e;
        e.v0 = i;
        e.v1 = j;
        s3o_mul(Sjw, Swi, &e.S);
        edges->push_back(e);
    };
    edges->clear();
    std::set<std::pair<int, int>> inserted;
    for (int i = 0; i < n; i++) {  // :910-939
        if (G.lc_off[i] == G.lc_off[i + 1]) continue;
        Sim3d Swi;
        s3o_inverse((*vScw)[i], &Swi);
        std::vector<std::pair<int, int>> row;  // (id, weight), ascending id
        for (int k = G.lc_off[i]; k < G.lc_off[i + 1]; k++) row.push_back({G.lc_ids[k], G.lc_weight[k]});
        std::sort(row.begin(), row.end());
        row.erase(std::unique(row.begin(), row.end(), [](const std::pair<int, int>& a, const std::pair<int, int>& b) { return a.first == b.first; }),
                  row.end());
        for (const std::pair<int, int>& jw : row) {
            const int j = jw.first;
            if ((i != G.cur_id || j != G.loop_id) && jw.second < minFeat) continue;
            push(i, j, (*vScw)[j], Swi);
            inserted.insert({std::min(i, j), std::max(i, j)});
        }
    }
    auto Sw_of = [&](int j) { return nonc[j] >= 0 ? G.noncorrected[nonc[j]] : (*vScw)[j]; };
    for (int i = 0; i < n; i++) {  // :944-1053
        if (!G.live[i]) continue;
        Sim3d Swi;
        s3o_inverse(Sw_of(i), &Swi);
        const int parent = G.parent[i];
        if (parent >= 0) push(i, parent, Sw_of(parent), Swi);
        std::vector<int> loops(G.loop_ids + G.loop_off[i], G.loop_ids + G.loop_off[i + 1]);
        std::sort(loops.begin(), loops.end());
        loops.erase(std::unique(loops.begin(), loops.end()), loops.end());
        for (int l : loops)
            if (l < i) push(i, l, Sw_of(l), Swi);
        for (int k = G.cov_off[i]; k < G.cov_off[i + 1]; k++) {
            const int j = G.cov_ids[k];
            if (j == parent || G.parent[j] == i || std::binary_search(loops.begin(), loops.end(), j)) continue;
            if (!(j < i)) continue;
            if (inserted.count({j, i})) continue;
            push(i, j, Sw_of(j), Swi);
        }
    }
}

}  // namespace orbmi
