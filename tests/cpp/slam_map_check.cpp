// Host check of csrc/slam_map.h (no HIP): reads scenes -- a small map and a script of Map
// operations -- from a text file, applies each script to orbmi::slam::Map and writes the whole map
// state after it, floats as their bit patterns.  tests/test_slam_map_cpu.py applies the same
// scripts to system.KeyFrame / system.MapPoint / StereoSLAM's two cullings and compares every line.
// Before each operation the program classifies, from the state the operation is about to read,
// which of the listed branches it will take, and counts them (the census at the end of the output).
//
//   slam_map_check IN OUT
//
// IN:  scene NAME | sf N bits.. | th bits | kf ID tcw[16] N (octave ur depth)*N |
//      mp ID pos[3] ref_kf first_kf visible found | op NAME ints.. | end
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>

#include "slam_map.h"

using namespace orbmi::slam;

static std::map<std::string, long> census;
static void hit(const char* name) { census[name]++; }

static float from_bits(uint32_t b) {
    float f;
    std::memcpy(&f, &b, 4);
    return f;
}
static uint32_t bits(float f) {
    uint32_t b;
    std::memcpy(&b, &f, 4);
    return b;
}
static float read_float(std::istream& in) {
    std::string t;
    in >> t;
    return from_bits((uint32_t)std::stoul(t, nullptr, 16));
}

// ---- the census: which branches an operation is about to take ------------------------------------
static void census_update_connections(const Map& M, int k) {
    std::map<int, int> counter, by_weight;
    for (int m : M.kfs[k].mps) {
        if (m < 0) continue;
        if (M.mps[m].bad) { hit("c_badslot"); continue; }
        for (auto& o : M.mps[m].obs)
            if (o.first != k) counter[o.first]++;
    }
    if (counter.empty()) return;
    int nmax = 0;
    bool any = false;
    for (auto& c : counter) {
        nmax = std::max(nmax, c.second);
        by_weight[c.second]++;
        if (c.second == 15) hit("c_w15");
        if (c.second == 14) hit("c_w14");
        any |= c.second >= 15;
    }
    for (auto& b : by_weight)
        if (b.first >= 15 && b.second >= 2) hit("c_tie");
    if (!any) {
        hit("c_fallback");
        if (by_weight[nmax] >= 2) hit("c_fallback_tie");
    }
    if (M.kfs[k].id == 0) hit("c_kf0");
    else if (!M.kfs[k].first_connection) hit("c_second");
}

static void census_set_bad(const Map& M, int m) {
    for (auto& o : M.mps[m].obs) hit(M.kfs[o.first].mps[o.second] == m ? "o_setbad_slot_cleared" : "o_setbad_slot_kept");
}

static void census_erase_observation(const Map& M, int m, int k) {
    const MapPoint& mp = M.mps[m];
    auto it = mp.obs.find(k);
    if (it == mp.obs.end()) return;
    const int after = mp.nobs - (M.kfs[k].ur[it->second] >= 0 ? 2 : 1);
    if (mp.ref_kf == k && mp.obs.size() > 1) hit("o_erase_ref");
    if (after == 3) hit("o_erase_to3");
    if (after == 2) {
        hit("o_erase_to2");
        for (auto& o : mp.obs)
            if (o.first != k) hit(M.kfs[o.first].mps[o.second] == m ? "o_setbad_slot_cleared" : "o_setbad_slot_kept");
    }
}

static void census_replace(const Map& M, int m, int other) {
    if (m == other) { hit("r_same"); return; }
    for (auto& o : M.mps[m].obs) hit(M.mps[other].obs.count(o.first) ? "r_slot_emptied" : "r_slot_replaced");
    if (M.mps[m].found > 0 && M.mps[m].visible > 0) hit("r_sums");
}

static void census_set_bad_keyframe(const Map& M, int k) {
    const KeyFrame& kf = M.kfs[k];
    if (kf.id == 0) { hit("s_kf0"); return; }
    hit("s_tcp");
    std::set<int> family{kf.parent};
    for (int c : kf.children)
        if (!M.kfs[c].bad) family.insert(c);
    for (int c : kf.children) {
        if (M.kfs[c].bad) { hit("s_bad_child"); continue; }
        const auto& cov = M.kfs[c].covisible;
        const bool with_parent = std::find(cov.begin(), cov.end(), kf.parent) != cov.end();
        bool with_sibling = false;
        std::map<int, int> by_weight;  // weights towards the possible parents, k itself aside
        for (int v : cov)
            if (v != k && family.count(v)) {
                with_sibling |= v != kf.parent;
                by_weight[M.get_weight(c, v)]++;
            }
        if (with_parent) hit("s_child_of_parent");
        else if (with_sibling) hit("s_second_round");
        else hit("s_child_to_parent");
        for (auto& b : by_weight)
            if (b.second >= 2) hit("s_equal_weights");
    }
}

static void census_keyframe_culling(const Map& M, int k, float th_depth) {
    for (int kk : M.kfs[k].covisible) {
        const KeyFrame& kf = M.kfs[kk];
        if (kf.id == 0) continue;
        int n_mps = 0, n_red = 0;
        for (size_t i = 0; i < kf.mps.size(); i++) {
            const int m = kf.mps[i];
            if (m < 0 || M.mps[m].bad) continue;
            if (kf.depth[i] > th_depth) { hit("k_depth_far"); continue; }
            if (kf.depth[i] < 0) { hit("k_depth_neg"); continue; }
            n_mps++;
            if (M.mps[m].nobs == 3) hit("k_nobs3");
            if (M.mps[m].nobs <= 3) continue;
            if (M.mps[m].nobs == 4) hit("k_nobs4");
            const int level = kf.keys[i].octave;
            int n = 0, after_third = 0;
            for (auto& o : M.mps[m].obs) {
                if (o.first == kk) continue;
                if (n >= 3) { after_third++; continue; }
                const int oct = M.kfs[o.first].keys[o.second].octave;
                if (oct == level + 1) hit("k_oct1");
                if (oct == level + 2) hit("k_oct2");
                if (oct <= level + 1) n++;
            }
            if (n >= 3 && after_third) hit("k_third_breaks");
            if (n >= 3) n_red++;
        }
        if (n_mps > 0 && n_red == 0.9 * n_mps) hit("k_at");
        if (n_red > 0.9 * n_mps && n_red - 1 <= 0.9 * n_mps) hit("k_above");
    }
}

static void census_map_point_culling(const Map& M, int k) {
    for (int m : M.recent_mps) {
        const MapPoint& mp = M.mps[m];
        if (mp.bad) { hit("m_bad_skipped"); continue; }
        const int gap = k - mp.first_kf_id;
        if (gap == 1) hit("m_gap1");
        if (gap == 2) hit("m_gap2");
        if (gap == 3) hit("m_gap3");
        if (4 * mp.found == mp.visible) hit("m_ratio_at");
        if ((float)mp.found / (float)mp.visible < 0.25f) hit("m_ratio_low");
        else if (gap >= 2 && mp.nobs <= 3) hit("m_few");
        else if (gap >= 3) hit("m_old");
        else hit("m_keep");
    }
}

// ---- one operation -----------------------------------------------------------------------------
static int nargs(const std::string& op) {
    static const std::map<std::string, int> n{
        {"slot", 3}, {"kfbad", 1}, {"recent", 1},  // raw writes that set a scene up
        {"kf_ow", 1}, {"tracked_map_points", 2}, {"get_weight", 2}, {"keyframes_in_map", 0}, {"count_mappoints", 0},
        {"obs_rows", 2}, {"sort_covisible", 1}, {"add_connection", 3}, {"erase_connection", 2}, {"change_parent", 2},
        {"update_connections", 1}, {"add_observation", 3}, {"erase_observation", 2}, {"set_bad", 1}, {"replace", 2},
        {"update_normal_and_depth", 1}, {"set_bad_keyframe", 1}, {"keyframe_culling", 1}, {"map_point_culling", 1}};
    auto it = n.find(op);
    if (it == n.end()) throw std::runtime_error("unknown op " + op);
    return it->second;
}

static void apply(Map& M, float th_depth, const std::string& op, const int* a, FILE* out) {
    hit(("op_" + op).c_str());
    if (op == "slot") M.kfs[a[0]].mps[a[1]] = a[2];
    else if (op == "kfbad") M.kfs[a[0]].bad = true;
    else if (op == "recent") M.recent_mps.push_back(a[0]);
    else if (op == "kf_ow") {
        float ow[3];
        M.kf_ow(a[0], ow);
        std::fprintf(out, "q kf_ow %08x %08x %08x\n", bits(ow[0]), bits(ow[1]), bits(ow[2]));
    } else if (op == "tracked_map_points") std::fprintf(out, "q tracked_map_points %d\n", M.tracked_map_points(M.kfs[a[0]], a[1]));
    else if (op == "get_weight") std::fprintf(out, "q get_weight %d\n", M.get_weight(a[0], a[1]));
    else if (op == "keyframes_in_map") std::fprintf(out, "q keyframes_in_map %d\n", M.keyframes_in_map());
    else if (op == "count_mappoints") std::fprintf(out, "q count_mappoints %d\n", M.count_mappoints());
    else if (op == "obs_rows") {
        std::vector<uint8_t> rows;
        std::vector<int32_t> off;
        M.obs_rows({a[0], a[1]}, rows, off);
        std::fprintf(out, "q obs_rows");
        for (int32_t o : off) std::fprintf(out, " %d", o);
        std::fprintf(out, " |");
        for (size_t r = 0; r < rows.size(); r += 32) std::fprintf(out, " %d:%d", rows[r], rows[r + 31]);
        std::fprintf(out, "\n");
    } else if (op == "sort_covisible") M.sort_covisible(M.kfs[a[0]]);
    else if (op == "add_connection") M.add_connection(a[0], a[1], a[2]);
    else if (op == "erase_connection") M.erase_connection(a[0], a[1]);
    else if (op == "change_parent") M.change_parent(a[0], a[1]);
    else if (op == "update_connections") {
        census_update_connections(M, a[0]);
        M.update_connections(a[0]);
    } else if (op == "add_observation") {
        if (M.mps[a[0]].obs.count(a[1])) hit("o_add_twice");
        else hit(M.kfs[a[1]].ur[a[2]] >= 0 ? "o_stereo" : "o_mono");
        M.add_observation(a[0], a[1], a[2]);
    } else if (op == "erase_observation") {
        census_erase_observation(M, a[0], a[1]);
        M.erase_observation(a[0], a[1]);
    } else if (op == "set_bad") {
        census_set_bad(M, a[0]);
        M.set_bad(a[0]);
    } else if (op == "replace") {
        census_replace(M, a[0], a[1]);
        std::fprintf(out, "q replace %d\n", M.replace(a[0], a[1]) ? 1 : 0);
    } else if (op == "update_normal_and_depth") M.update_normal_and_depth(a[0]);
    else if (op == "set_bad_keyframe") {
        census_set_bad_keyframe(M, a[0]);
        M.set_bad_keyframe(a[0]);
    } else if (op == "keyframe_culling") {
        census_keyframe_culling(M, a[0], th_depth);
        M.keyframe_culling(a[0], th_depth);
    } else if (op == "map_point_culling") {
        census_map_point_culling(M, a[0]);
        M.map_point_culling(a[0]);
    }
}

static void dump(const Map& M, FILE* out) {
    for (const KeyFrame& kf : M.kfs) {
        std::fprintf(out, "kf %d bad %d first %d parent %d | slots", kf.id, kf.bad, kf.first_connection, kf.parent);
        for (int m : kf.mps) std::fprintf(out, " %d", m);
        std::fprintf(out, " | conn");
        for (auto& c : kf.conn) std::fprintf(out, " %d:%d", c.first, c.second);
        std::fprintf(out, " | cov");
        for (int c : kf.covisible) std::fprintf(out, " %d", c);
        std::vector<int> ch = kf.children;
        std::sort(ch.begin(), ch.end());
        std::fprintf(out, " | ch");
        for (int c : ch) std::fprintf(out, " %d", c);
        std::fprintf(out, " | tcp");
        for (float v : kf.tcp) std::fprintf(out, " %08x", bits(v));
        std::fprintf(out, "\n");
    }
    for (const MapPoint& mp : M.mps) {
        std::fprintf(out, "mp %d bad %d nobs %d ref %d replaced %d visible %d found %d | obs", mp.id, mp.bad, mp.nobs, mp.ref_kf,
                     mp.replaced, mp.visible, mp.found);
        for (auto& o : mp.obs) std::fprintf(out, " %d:%d", o.first, o.second);
        std::fprintf(out, " | normal %08x %08x %08x max %08x min %08x\n", bits(mp.normal[0]), bits(mp.normal[1]),
                     bits(mp.normal[2]), bits(mp.max_distance), bits(mp.min_distance));
    }
    std::fprintf(out, "recent");
    for (int m : M.recent_mps) std::fprintf(out, " %d", m);
    std::fprintf(out, "\n");
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    std::ifstream in(argv[1]);
    FILE* out = std::fopen(argv[2], "w");
    if (!in || !out) return 2;
    Map M;
    float th_depth = 0;
    std::string tok;
    while (in >> tok) {
        if (tok == "scene") {
            std::string name;
            in >> name;
            M = Map();
            std::fprintf(out, "scene %s\n", name.c_str());
        } else if (tok == "sf") {
            int n;
            in >> n;
            M.scale_factors.resize(n);
            for (float& v : M.scale_factors) v = read_float(in);
        } else if (tok == "th") {
            th_depth = read_float(in);
        } else if (tok == "kf") {
            KeyFrame kf;
            int n;
            in >> kf.id;
            if (kf.id != (int)M.kfs.size()) return 3;
            for (float& v : kf.tcw) v = read_float(in);
            in >> n;
            kf.keys.resize(n);
            kf.ur.resize(n);
            kf.depth.resize(n);
            kf.mps.assign(n, -1);
            kf.desc.resize((size_t)32 * n);
            for (int i = 0; i < n; i++) {
                kf.keys[i] = orbmi_keypoint{};
                in >> kf.keys[i].octave;
                kf.ur[i] = read_float(in);
                kf.depth[i] = read_float(in);
                for (int b = 0; b < 32; b++) kf.desc[32 * i + b] = (uint8_t)(kf.id * 7 + i * 3 + b);
            }
            M.kfs.push_back(std::move(kf));
        } else if (tok == "mp") {
            MapPoint mp;
            in >> mp.id;
            if (mp.id != (int)M.mps.size()) return 3;
            for (float& v : mp.pos) v = read_float(in);
            in >> mp.ref_kf >> mp.first_kf_id >> mp.visible >> mp.found;
            M.mps.push_back(mp);
        } else if (tok == "op") {
            std::string op;
            in >> op;
            int a[3] = {0, 0, 0};
            for (int i = 0; i < nargs(op); i++) in >> a[i];
            apply(M, th_depth, op, a, out);
        } else if (tok == "end") {
            dump(M, out);
        } else {
            return 3;
        }
    }
    for (auto& c : census) std::fprintf(out, "census %s %ld\n", c.first.c_str(), c.second);
    std::fclose(out);
    return 0;
}
