// Host check of csrc/ba_graph.h (no HIP): reads small bundle-adjustment graphs from a text file,
// builds the plan of Optimizer::LocalBundleAdjustment and of Optimizer::BundleAdjustment for each,
// as lba.hip and gba.hip do, and writes every table.  tests/test_ba_graph_cpu.py restates the tables
// by brute force and compares every line.  After each plan the two checks run on it as built and
// on corruptions of it ("corrupt NAME verdict", "na" where the plan is too small to corrupt so); for
// LocalBA also the form of the check that lba.hip calls ("lba_entry": per_edge = false).
//
//   ba_graph_check IN OUT
//
// IN:  scene NAME NKF NPT NE | kf ID FIXED (x NKF) | e POINT KF (x NE) | end
#include <cstdio>
#include <fstream>
#include <string>

#include "ba_graph.h"

using namespace orbmi;

static void row(FILE* f, const char* plan, const char* name, const int* v, size_t n) {
    fprintf(f, "%s %s", plan, name);
    for (size_t i = 0; i < n; i++) fprintf(f, " %d", v[i]);
    fprintf(f, "\n");
}
static void verdict(FILE* f, const char* plan, const char* name, int v) {
    if (v < 0) fprintf(f, "%s corrupt %s na\n", plan, name);
    else fprintf(f, "%s corrupt %s %d\n", plan, name, v);
}

struct Tables {
    int nf = 0;
    std::vector<int> pt_start, kf_start, kf_edges, kf_pos, kf_pt, order, rank, free_kf, blk_kf, blk_ij, blk_start;
    std::vector<BaPair> pairs;
};

static bool lba_ok(const orbmi_ba_problem& P, const Tables& t) {
    return ba_tables_ok(P, t.nf, t.pt_start.data(), t.kf_start.data(), t.kf_edges.data(), t.kf_pos.data(), t.kf_pt.data(),
                       t.rank.data(), t.free_kf.data(), t.blk_kf.data());
}
// the call lba.hip itself makes: without the pass over the edges, whose part ran inside ba_graph_index's fill
static bool lba_entry_ok(const orbmi_ba_problem& P, const Tables& t) {
    return ba_tables_ok(P, t.nf, t.pt_start.data(), t.kf_start.data(), t.kf_edges.data(), t.kf_pos.data(), t.kf_pt.data(),
                        t.rank.data(), t.free_kf.data(), t.blk_kf.data(), false);
}
static bool gba_ok(const orbmi_ba_problem& P, const Tables& t) {
    return gba_plan_ok(P, t.nf, t.pt_start.data(), t.kf_start.data(), t.kf_edges.data(), t.kf_pos.data(), t.rank.data(),
                       t.free_kf.data(), t.blk_ij, t.blk_start, t.pairs);
}

// the corruptions both plans have tables for
template <class Ok>
static void corrupt_common(FILE* f, const char* plan, const orbmi_ba_problem& P, const Tables& t, Ok ok) {
    Tables c = t;
    if (P.nedge > 0) { c.kf_edges[P.nedge / 2] = P.nedge; verdict(f, plan, "kf_edges_ne", ok(P, c)); }
    else verdict(f, plan, "kf_edges_ne", -1);
    c = t;
    c.pt_start[P.npt] += 1;
    verdict(f, plan, "pt_start_end", ok(P, c));
    c = t;
    if (t.nf >= 2) { std::swap(c.free_kf[0], c.free_kf[t.nf - 1]); verdict(f, plan, "free_kf_swap", ok(P, c)); }
    else verdict(f, plan, "free_kf_swap", -1);
}

static void scene(FILE* f, const orbmi_ba_problem& P) {
    const int nkf = P.nkf, npt = P.npt, ne = P.nedge;
    {  // LocalBA (lba.hip): every non-fixed keyframe is a pose block
        Tables t;
        t.pt_start.resize(npt + 1); t.kf_start.resize(nkf + 1); t.kf_edges.resize(ne); t.kf_pos.resize(ne); t.kf_pt.resize(ne);
        t.order.resize(nkf); t.rank.resize(nkf); t.free_kf.resize(nkf);
        t.nf = ba_graph_rank(P, nullptr, t.order.data(), t.rank.data(), t.free_kf.data());
        t.free_kf.resize(t.nf);
        std::vector<int> blk_id;
        const bool perm = ba_block_table(t.nf, blk_id);
        long long npair_cap = -1;
        const int rc = ba_graph_index(P, t.pt_start.data(), t.kf_start.data(), t.kf_edges.data(), t.kf_pos.data(),
                                      t.kf_pt.data(), t.rank.data(), &npair_cap);
        fprintf(f, "validate %d\n", rc);  // the edges' validation is part of the counting pass
        if (rc) return;
        t.blk_kf.assign((size_t)t.nf * (t.nf + 1), -7);
        if (perm) ba_block_kf(t.nf, blk_id, t.free_kf.data(), t.blk_kf.data());
        fprintf(f, "lba nf %d\n", t.nf);
        row(f, "lba", "pt_start", t.pt_start.data(), t.pt_start.size());
        row(f, "lba", "kf_start", t.kf_start.data(), t.kf_start.size());
        row(f, "lba", "kf_edges", t.kf_edges.data(), t.kf_edges.size());
        row(f, "lba", "kf_pos", t.kf_pos.data(), t.kf_pos.size());
        row(f, "lba", "kf_pt", t.kf_pt.data(), t.kf_pt.size());
        row(f, "lba", "order", t.order.data(), t.order.size());
        row(f, "lba", "rank", t.rank.data(), t.rank.size());
        row(f, "lba", "free_kf", t.free_kf.data(), t.free_kf.size());
        row(f, "lba", "blk_kf", t.blk_kf.data(), t.blk_kf.size());
        fprintf(f, "lba npair_cap %lld\n", npair_cap);
        fprintf(f, "lba ok %d\n", (int)(perm && lba_ok(P, t)));
        corrupt_common(f, "lba", P, t, lba_ok);
        Tables c = t;
        if (t.nf > 0) { c.blk_kf[t.nf] = nkf; verdict(f, "lba", "blk_kf_nkf", lba_ok(P, c)); }
        else verdict(f, "lba", "blk_kf_nkf", -1);
        fprintf(f, "lba_entry ok %d\n", (int)lba_entry_ok(P, t));
        corrupt_common(f, "lba_entry", P, t, lba_entry_ok);
        if (t.nf > 0) verdict(f, "lba_entry", "blk_kf_nkf", lba_entry_ok(P, c));
        else verdict(f, "lba_entry", "blk_kf_nkf", -1);
    }
    {  // global BA (gba.hip): the non-fixed keyframes that an edge names
        Tables t;
        t.pt_start.resize(npt + 1); t.kf_start.resize(nkf + 1); t.kf_edges.resize(ne); t.kf_pos.resize(ne);
        t.order.resize(nkf); t.rank.resize(nkf); t.free_kf.resize(nkf);
        const bool filled = ba_graph_index(P, t.pt_start.data(), t.kf_start.data(), t.kf_edges.data(), t.kf_pos.data(), nullptr) == ORBMI_OK;
        t.nf = ba_graph_rank(P, t.kf_start.data(), t.order.data(), t.rank.data(), t.free_kf.data());
        t.free_kf.resize(t.nf);
        const long long npair = gba_pair_count(P, t.pt_start.data(), t.rank.data());
        gba_pair_lists(P, t.pt_start.data(), t.rank.data(), npair, &t.blk_ij, &t.blk_start, &t.pairs);
        fprintf(f, "gba nf %d\n", t.nf);
        row(f, "gba", "pt_start", t.pt_start.data(), t.pt_start.size());
        row(f, "gba", "kf_start", t.kf_start.data(), t.kf_start.size());
        row(f, "gba", "kf_edges", t.kf_edges.data(), t.kf_edges.size());
        row(f, "gba", "kf_pos", t.kf_pos.data(), t.kf_pos.size());
        row(f, "gba", "order", t.order.data(), t.order.size());
        row(f, "gba", "rank", t.rank.data(), t.rank.size());
        row(f, "gba", "free_kf", t.free_kf.data(), t.free_kf.size());
        row(f, "gba", "blk_ij", t.blk_ij.data(), t.blk_ij.size());
        row(f, "gba", "blk_start", t.blk_start.data(), t.blk_start.size());
        static_assert(sizeof(BaPair) == 2 * sizeof(int), "a pair is two ints");
        row(f, "gba", "pairs", t.pairs.empty() ? nullptr : &t.pairs[0].x, 2 * t.pairs.size());
        fprintf(f, "gba npair %lld\n", npair);
        fprintf(f, "gba ok %d\n", (int)(filled && gba_ok(P, t)));
        corrupt_common(f, "gba", P, t, gba_ok);
        const size_t nblk = t.blk_ij.size() / 2;
        Tables c = t;
        if (nblk >= 2) { c.blk_start[1] = c.blk_start[2] + 1; verdict(f, "gba", "blk_start_down", gba_ok(P, c)); }
        else verdict(f, "gba", "blk_start_down", -1);
        c = t;
        if (!t.pairs.empty()) { c.pairs[t.pairs.size() / 2].y = -1; verdict(f, "gba", "pair_minus1", gba_ok(P, c)); }
        else verdict(f, "gba", "pair_minus1", -1);
    }
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    std::ifstream in(argv[1]);
    FILE* f = fopen(argv[2], "w");
    if (!in || !f) return 2;
    std::string tok, name;
    while (in >> tok) {
        if (tok == "end") break;
        if (tok != "scene") return 3;
        orbmi_ba_problem P{};
        in >> name >> P.nkf >> P.npt >> P.nedge;
        std::vector<orbmi_ba_keyframe> kfs(P.nkf);
        std::vector<orbmi_ba_point> pts(P.npt);
        std::vector<orbmi_ba_edge> edges(P.nedge);
        for (auto& k : kfs) { k = orbmi_ba_keyframe{}; in >> tok >> k.id >> k.fixed; if (tok != "kf") return 3; }
        for (auto& e : edges) { e = orbmi_ba_edge{}; in >> tok >> e.point >> e.kf; if (tok != "e") return 3; }
        for (auto& p : pts) p = orbmi_ba_point{};
        P.kfs = kfs.data(); P.pts = pts.data(); P.edges = edges.data();
        fprintf(f, "scene %s\n", name.c_str());
        scene(f, P);
    }
    // the block table of every size LocalBA solves
    for (int nf = 0; nf <= kBaMaxPoses; nf++) {
        std::vector<int> blk_id;
        const bool ok = ba_block_table(nf, blk_id);
        fprintf(f, "blktab %d %d", nf, (int)ok);
        for (int l = 0; l < nf * (nf + 1) / 2; l++) fprintf(f, " %d", blk_id[l]);
        fprintf(f, "\n");
    }
    fclose(f);
    return 0;
}
