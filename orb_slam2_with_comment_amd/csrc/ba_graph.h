// The host plan of a bundle-adjustment graph (orbmi_ba_problem), shared by
// Optimizer::LocalBundleAdjustment (lba.hip) and Optimizer::BundleAdjustment (gba.hip): the edge
// validation, the index tables the kernels address the graph through, and the checks of those
// tables against the lengths of the arrays they index.  HIP-free (include/orbmi.h and the standard
// library only), so a plain C++ program builds it: tests/cpp/ba_graph_check.cpp.
//   pt_start  npt + 1   edges of point p: [pt_start[p], pt_start[p + 1]) (edges come grouped by point)
//   kf_start  nkf + 1   CSR by keyframe over edge indices, in edge order
//   kf_edges  ne        the edge at keyframe-CSR position j
//   kf_pos    ne        position of edge e in the keyframe CSR (kf_edges[kf_pos[e]] == e)
//   kf_pt     ne        the point of the edge at position j (LocalBA only)
//   order     nkf       keyframe indices sorted by id (SparseOptimizer's vertex order), stable
//   rank, free_kf       nkf: the keyframe's pose block, -1 = not in the system; nf: rank's inverse
#pragma once
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/orbmi.h"

namespace orbmi {

constexpr int kBaMaxPoses = 30;  // LocalBA's free keyframes: 6 * 30 = 180 unknowns

struct BaPair { int x, y; };  // (edge into pose block i, edge into pose block j) of one point: the device's int2

// The two CSRs of a graph, into the caller's arrays (kf_pt may be null), with the validation of its
// edges in the counting pass: indices in range, edges grouped by point in ascending order, one edge
// per (point, keyframe) -- as the reference builds the graph from a map point's observations (a
// std::map per point): the per-keyframe Schur blocks sum each edge's B D^-1 B^T with itself only, so
// a second edge of one pair would lose its cross terms.  Otherwise ORBMI_E_ARG.
// With rank given (LocalBA) the fill also sums *pair_cap, the capacity of the pair lists built on the
// device: over the points, (edges into pose blocks)^2.  The fill checks that every edge lands inside
// its keyframe's segment, so that on ORBMI_OK kf_pos and kf_edges are in range and inverse to each
// other (ORBMI_E_UNSUPPORTED: never, by construction).
inline int ba_graph_index(const orbmi_ba_problem& P, int* pt_start, int* kf_start, int* kf_edges, int* kf_pos, int* kf_pt,
                          const int* rank = nullptr, long long* pair_cap = nullptr) {
    const int nkf = P.nkf, npt = P.npt, ne = P.nedge;
    std::memset(pt_start, 0, sizeof(int) * ((size_t)npt + 1));
    std::memset(kf_start, 0, sizeof(int) * ((size_t)nkf + 1));
    std::vector<int> fill(std::max(nkf, 1), -1);  // first: the last point seen by each keyframe
    for (int i = 0; i < ne; i++) {
        const orbmi_ba_edge& e = P.edges[i];
        if (e.point < 0 || e.point >= npt || e.kf < 0 || e.kf >= nkf) return ORBMI_E_ARG;
        if (i && e.point < P.edges[i - 1].point) return ORBMI_E_ARG;  // grouped by point
        if (fill[e.kf] == e.point) return ORBMI_E_ARG;                 // one edge per (point, keyframe)
        fill[e.kf] = e.point;
        pt_start[e.point + 1]++;
        kf_start[e.kf + 1]++;
    }
    for (int p = 0; p < npt; p++) pt_start[p + 1] += pt_start[p];
    for (int k = 0; k < nkf; k++) kf_start[k + 1] += kf_start[k];
    if (pt_start[npt] != ne || kf_start[nkf] != ne) return ORBMI_E_UNSUPPORTED;
    std::copy(kf_start, kf_start + nkf, fill.begin());  // then: the next free position of each keyframe
    long long cap = 0, m = 0;
    for (int i = 0, p = -1; i < ne; i++) {
        const orbmi_ba_edge& e = P.edges[i];
        const int j = fill[e.kf]++;
        if (j >= kf_start[e.kf + 1]) return ORBMI_E_UNSUPPORTED;
        kf_pos[i] = j;
        kf_edges[j] = i;
        if (kf_pt) kf_pt[j] = e.point;
        if (rank) {
            if (e.point != p) { cap += m * m; m = 0; p = e.point; }
            m += rank[e.kf] >= 0;
        }
    }
    if (pair_cap) *pair_cap = cap + m * m;
    return ORBMI_OK;
}

// The pose blocks in vertex (id) order; returns nf.  A keyframe is in the system when it is not
// fixed and -- with kf_start given (global BA) -- an edge names it; with kf_start null (LocalBA) a
// free keyframe without an edge stays in.  order, rank: nkf; free_kf: room for nkf.
inline int ba_graph_rank(const orbmi_ba_problem& P, const int* kf_start, int* order, int* rank, int* free_kf) {
    const int nkf = P.nkf;
    for (int k = 0; k < nkf; k++) { order[k] = k; rank[k] = -1; }
    std::stable_sort(order, order + nkf, [&](int x, int y) { return P.kfs[x].id < P.kfs[y].id; });
    int nf = 0;
    for (int oi = 0; oi < nkf; oi++) {
        const int k = order[oi];
        if (!P.kfs[k].fixed && (!kf_start || kf_start[k + 1] > kf_start[k])) { rank[k] = nf; free_kf[nf++] = k; }
    }
    return nf;
}

// The pose-pair blocks' ids.  Pair l = (ra, rb >= ra) in row-major order (l = ra nf - ra (ra - 1)
// / 2 + rb - ra) runs as block blk_id[l] of k_ba_schur.  Placed by row: the blocks of row ra
// (which all read the Hpl blocks of keyframe ra's edges) go to ids of one residue mod 8 -- one XCD
// under the round-robin dispatch, so their re-reads of those blocks hit one L2 (speed only).
// Rows are dealt to the 8 residues largest first onto the least loaded; pairs beyond a residue's
// ids take the ids left over, in increasing order.
// Every block id in [0, nblk) must name exactly one pair: an id no pair took would leave its
// blk_kf entry to whatever the pinned staging buffer last held, and the pair kernels index
// pose_idx / kf_start with it (the round-4 r04x illegal address, from a work-in-progress form of
// this table, on the first call that reused a larger graph's staging buffer).  So the table is
// checked before it is used: false = not a permutation (never, by construction; tested for
// every nf by tests/test_capi_exports.py through orbmi_debug_ba_schur_blocks and by
// tests/test_ba_graph_cpu.py).
inline bool ba_block_table(int nf, std::vector<int>& blk_id) {
    const int nblk = nf * (nf + 1) / 2;
    blk_id.assign(std::max(nblk, 1), -1);
    const int R = 8;
    std::vector<int> load(R, 0), grp(std::max(nf, 1));
    for (int r = 0; r < nf; r++) {  // row r holds nf - r pairs: already largest first
        const int g = (int)(std::min_element(load.begin(), load.end()) - load.begin());
        grp[r] = g;
        load[g] += nf - r;
    }
    std::vector<int> next(R);
    for (int g = 0; g < R; g++) next[g] = g;
    std::vector<char> used(std::max(nblk, 1), 0);
    std::vector<int> spill;
    int l = 0;
    for (int ra = 0; ra < nf; ra++)
        for (int rb = ra; rb < nf; rb++, l++) {
            const int g = grp[ra];
            if (next[g] < nblk) { blk_id[l] = next[g]; used[next[g]] = 1; next[g] += R; }
            else spill.push_back(l);
        }
    int free_id = 0;
    for (int x : spill) {
        while (free_id < nblk && used[free_id]) free_id++;
        if (free_id >= nblk) return false;
        blk_id[x] = free_id;
        used[free_id] = 1;
    }
    std::vector<char> hit(std::max(nblk, 1), 0);
    for (int x = 0; x < nblk; x++) {
        const int id = blk_id[x];
        if (id < 0 || id >= nblk || hit[id]) return false;
        hit[id] = 1;
    }
    return true;
}

// blk_kf (nblk x 2): the keyframes (a, b), id(a) <= id(b), of the pair that runs as block id
inline void ba_block_kf(int nf, const std::vector<int>& blk_id, const int* free_kf, int* blk_kf) {
    int l = 0;
    for (int ra = 0; ra < nf; ra++)
        for (int rb = ra; rb < nf; rb++, l++) { blk_kf[2 * blk_id[l]] = free_kf[ra]; blk_kf[2 * blk_id[l] + 1] = free_kf[rb]; }
}

// Global BA: the pairs of the non-zero blocks of S (i >= j): over the points, m (m + 1) / 2
inline long long gba_pair_count(const orbmi_ba_problem& P, const int* pt_start, const int* rank) {
    long long n = 0;
    for (int p = 0; p < P.npt; p++) {
        long long m = 0;
        for (int e = pt_start[p]; e < pt_start[p + 1]; e++) m += rank[P.edges[e].kf] >= 0;
        n += m * (m + 1) / 2;
    }
    return n;
}

// Global BA's pair lists: the blocks in ascending key r1 (r1 + 1) / 2 + r2 (r1 >= r2), a block's
// pairs in point order (a stable sort of the pairs as the points give them)
inline void gba_pair_lists(const orbmi_ba_problem& P, const int* pt_start, const int* rank, long long npair,
                           std::vector<int>* blk_ij, std::vector<int>* blk_start, std::vector<BaPair>* pairs) {
    struct Keyed { long long key; int ea, eb; };
    std::vector<Keyed> pl;
    pl.reserve((size_t)npair);
    for (int p = 0; p < P.npt; p++)
        for (int e1 = pt_start[p]; e1 < pt_start[p + 1]; e1++) {
            const int r1 = rank[P.edges[e1].kf];
            if (r1 < 0) continue;
            for (int e2 = pt_start[p]; e2 < pt_start[p + 1]; e2++) {
                const int r2 = rank[P.edges[e2].kf];
                if (r2 < 0 || r2 > r1) continue;
                pl.push_back(Keyed{(long long)r1 * (r1 + 1) / 2 + r2, e1, e2});
            }
        }
    std::stable_sort(pl.begin(), pl.end(), [](const Keyed& x, const Keyed& y) { return x.key < y.key; });
    blk_ij->clear();
    blk_start->clear();
    pairs->resize(pl.size());
    for (size_t t = 0; t < pl.size(); t++) {
        if (t == 0 || pl[t].key != pl[t - 1].key) {
            blk_ij->push_back(rank[P.edges[pl[t].ea].kf]);
            blk_ij->push_back(rank[P.edges[pl[t].eb].kf]);
            blk_start->push_back((int)t);
        }
        (*pairs)[t] = BaPair{pl[t].ea, pl[t].eb};
    }
    blk_start->push_back((int)pl.size());
}

// ---- the built tables against the lengths of the arrays they address, before any launch --------

// What both entries build: CSRs monotone from 0 to ne, kf_edges / kf_pos (/ kf_pt) in range and
// inverse to each other inside the edge's keyframe segment, rank and free_kf inverse to each other;
// with blk_kf (LocalBA) every entry of it a keyframe index.  kf_pt, blk_kf: null = not built.
// per_edge = false: without the pass over the edges, for LocalBA, which has ba_graph_index's verdict.
inline bool ba_tables_ok(const orbmi_ba_problem& P, int nf, const int* pt_start, const int* kf_start, const int* kf_edges,
                         const int* kf_pos, const int* kf_pt, const int* rank, const int* free_kf, const int* blk_kf,
                         bool per_edge = true) {
    const int nkf = P.nkf, npt = P.npt, ne = P.nedge;
    if (pt_start[0] != 0 || kf_start[0] != 0 || pt_start[npt] != ne || kf_start[nkf] != ne) return false;
    for (int p = 0; p < npt; p++)
        if (pt_start[p] > pt_start[p + 1]) return false;
    for (int k = 0; k < nkf; k++)
        if (kf_start[k] > kf_start[k + 1]) return false;
    for (int e = 0; per_edge && e < ne; e++) {
        const int j = kf_pos[e], k = P.edges[e].kf;
        if (kf_edges[e] < 0 || kf_edges[e] >= ne || j < kf_start[k] || j >= kf_start[k + 1] || kf_edges[j] != e) return false;
        if (kf_pt && kf_pt[j] != P.edges[e].point) return false;
    }
    if (nf < 0 || nf > nkf) return false;
    int in_system = 0;
    for (int k = 0; k < nkf; k++) {
        if (rank[k] < -1 || rank[k] >= nf) return false;
        in_system += rank[k] >= 0;
    }
    if (in_system != nf) return false;
    for (int i = 0; i < nf; i++)
        if (free_kf[i] < 0 || free_kf[i] >= nkf || rank[free_kf[i]] != i) return false;
    for (int i = 0, n = blk_kf ? nf * (nf + 1) : 0; i < n; i++)
        if (blk_kf[i] < 0 || blk_kf[i] >= nkf) return false;
    return true;
}

// Global BA's tables: the above, and the block and pair lists
inline bool gba_plan_ok(const orbmi_ba_problem& P, int nf, const int* pt_start, const int* kf_start, const int* kf_edges,
                        const int* kf_pos, const int* rank, const int* free_kf, const std::vector<int>& blk_ij,
                        const std::vector<int>& blk_start, const std::vector<BaPair>& pairs) {
    if (!ba_tables_ok(P, nf, pt_start, kf_start, kf_edges, kf_pos, nullptr, rank, free_kf, nullptr)) return false;
    const int nblk = (int)blk_ij.size() / 2, ne = P.nedge;
    if ((int)blk_start.size() != nblk + 1 || blk_start[0] != 0 || blk_start[nblk] != (int)pairs.size()) return false;
    for (int b = 0; b < nblk; b++) {
        const int i = blk_ij[2 * b], j = blk_ij[2 * b + 1];
        if (i < 0 || i >= nf || j < 0 || j > i || blk_start[b] > blk_start[b + 1]) return false;
    }
    for (const BaPair& p : pairs)
        if (p.x < 0 || p.x >= ne || p.y < 0 || p.y >= ne) return false;
    return true;
}

}  // namespace orbmi
