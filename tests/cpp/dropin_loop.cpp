// orbmi::KeyFrameDatabase and orbmi::ORBmatcher::SearchByBoW(KF1, KF2, ...) of include/orbmi.hpp with
// the call shapes of LoopClosing::DetectLoop and ComputeSim3 (src/LoopClosing.cc:126-143, :299-330),
// for tests/test_loop_gpu.py to compare with the Python path.
//
//   dropin_loop detect <dir>
// in_db_head = scoring nkf ; in_db_ids, in_db_len (per stored keyframe), in_db_word, in_db_value
// (concatenated), in_ops = (op, id) pairs with op 1 add / 0 erase, in_q_word, in_q_value, in_connected,
// in_covisible (ids to take minScore over), in_covis_off, in_covis_ids; writes out_scores (doubles),
// out_min_score (float) and out_candidates.
//
//   dropin_loop bow <dir>
// in_cam, in_scale_factors, in_kf1_* / in_kf2_* = keys, desc, ok, fv_node, fv_off, fv_feat, in_param =
// nnratio check_ori; writes out_match12 and out_nmatches.
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "orbmi.hpp"

static std::string g_dir;

template <class T>
static std::vector<T> load(const std::string& name) {
    std::ifstream f(g_dir + "/in_" + name + ".bin", std::ios::binary | std::ios::ate);
    if (!f) throw std::runtime_error("missing input " + name);
    const std::streamsize bytes = f.tellg();
    std::vector<T> v((size_t)bytes / sizeof(T));
    f.seekg(0);
    if (bytes && !f.read(reinterpret_cast<char*>(v.data()), bytes)) throw std::runtime_error("short read");
    return v;
}

template <class T>
static void save(const std::string& name, const std::vector<T>& v) {
    std::ofstream f(g_dir + "/out_" + name + ".bin", std::ios::binary);
    f.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
}

static int run_detect() {
    const auto head = load<int32_t>("db_head"), ids = load<int32_t>("db_ids"), len = load<int32_t>("db_len");
    const auto word = load<uint32_t>("db_word");
    const auto value = load<double>("db_value");
    const auto ops = load<int32_t>("ops");
    size_t total = 0;
    for (int32_t l : len) total += (size_t)l;
    if (head.size() != 2 || ids.size() != len.size() || word.size() != total || value.size() != total)
        throw std::runtime_error("inconsistent database input");
    orbmi::KeyFrameDatabase db(head[0], (int)ids.size() + 1, (int)total + 1);
    size_t o = 0;
    for (size_t k = 0; k < ids.size(); k++) {
        orbmi::ORBVocabulary::BowVector v;
        v.word.assign(word.begin() + (long)o, word.begin() + (long)(o + (size_t)len[k]));
        v.value.assign(value.begin() + (long)o, value.begin() + (long)(o + (size_t)len[k]));
        db.store(ids[k], v);
        o += (size_t)len[k];
    }
    for (size_t k = 0; k + 1 < ops.size(); k += 2) {
        if (ops[k]) db.add(ops[k + 1]);
        else db.erase(ops[k + 1]);
    }
    orbmi::ORBVocabulary::BowVector q;
    q.word = load<uint32_t>("q_word");
    q.value = load<double>("q_value");
    // minScore over the covisibles (:126-140)
    const std::vector<double> scores = db.score(q, load<int32_t>("covisible"));
    float minScore = 1;
    for (double s : scores) {
        const float score = (float)s;
        if (score < minScore) minScore = score;
    }
    const std::vector<int32_t> cand =
        db.DetectLoopCandidates(q, minScore, load<int32_t>("connected"), load<int32_t>("covis_off"), load<int32_t>("covis_ids"));
    save("scores", scores);
    save("min_score", std::vector<float>{minScore});
    save("candidates", cand);
    return 0;
}

struct KF {
    std::vector<orbmi::KeyPoint> keys;
    std::vector<uint8_t> desc, ok;
    std::vector<uint32_t> node;
    std::vector<int32_t> off, feat;
    orbmi_frame_view view{};
    orbmi_feature_vector fv{};
};

static void load_kf(const std::string& p, const std::vector<float>& cam, const std::vector<float>& sf, KF& k) {
    k.keys = load<orbmi::KeyPoint>(p + "_keys");
    k.desc = load<uint8_t>(p + "_desc");
    k.ok = load<uint8_t>(p + "_ok");
    k.node = load<uint32_t>(p + "_fv_node");
    k.off = load<int32_t>(p + "_fv_off");
    k.feat = load<int32_t>(p + "_fv_feat");
    orbmi_frame_view& v = k.view;
    v.n = (int)k.keys.size();
    v.keys_un = k.keys.data();
    v.desc = k.desc.data();
    v.fx = cam[0]; v.fy = cam[1]; v.cx = cam[2]; v.cy = cam[3]; v.bf = cam[4]; v.mb = cam[5];
    v.min_x = 0; v.max_x = cam[6]; v.min_y = 0; v.max_y = cam[7];
    v.grid_w_inv = cam[8]; v.grid_h_inv = cam[9];
    v.nlevels = (int)sf.size();
    v.scale_factors = sf.data();
    v.log_scale_factor = cam[10];
    k.fv = orbmi_feature_vector{(int)k.node.size(), k.node.data(), k.off.data(), k.feat.data()};
}

static int run_bow() {
    const auto cam = load<float>("cam"), sf = load<float>("scale_factors"), param = load<float>("param");
    KF k1, k2;
    load_kf("kf1", cam, sf, k1);
    load_kf("kf2", cam, sf, k2);
    orbmi::ORBmatcher matcher(param[0], param[1] != 0);  // ORBmatcher matcher(0.75, true) (:299)
    std::vector<int32_t> match12;
    const int n = matcher.SearchByBoW(k1.view, k1.ok, k1.fv, k2.view, k2.ok, k2.fv, match12);
    save("match12", match12);
    save("nmatches", std::vector<int32_t>{n});
    return 0;
}

int main(int argc, char** argv) {
    try {
        if (argc == 3) {
            g_dir = argv[2];
            if (std::string(argv[1]) == "detect") return run_detect();
            if (std::string(argv[1]) == "bow") return run_bow();
        }
        fprintf(stderr, "usage: dropin_loop detect|bow <dir>\n");
        return 2;
    } catch (const std::exception& e) {
        fprintf(stderr, "dropin_loop: %s\n", e.what());
        return 1;
    }
}
