// The loop-closure adapters of include/orbmi.hpp with the call shapes of LoopClosing::ComputeSim3
// (src/LoopClosing.cc:317-398), for tests/test_sim3_gpu.py to compare with the Python path.
//
//   dropin_sim3 <in> <out> [minInliers]
// orbmi::Sim3Solver: SetRansacParameters(0.99, minInliers = 20, 300), then iterate(5) until a
// success or bNoMore.
// in : as tests/cpp/sim3_check.cpp (int32 n H fix_scale, float32 k1[4] k2[4], X1 X2 (n x 3)
//      float32, e1 e2 (n) int32, triples (H x 3) int32), then int32 N1 and mvnIndices1 (n) int32
// out: int32 iterations calls success bNoMore nInliers, float32 T12[16] scale t[3] R[9],
//      uint8 vbInliers[N1]
//
//   dropin_sim3 search <dir>
// orbmi::ORBmatcher::SearchBySim3 on the keyframe pair of <dir>: in_cam, in_scale_factors and
// in_kf1_* / in_kf2_* as tests/cpp/dropin_match_ba.cpp reads frames, in_mps1 / in_mps2, in_has1 /
// in_has2, in_match12, in_sim3 = s12 R12[9] t12[3] th; writes out_match12 and out_nfound.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "orbmi.hpp"

template <class T>
static bool rd(FILE* f, std::vector<T>& v) { return fread(v.data(), sizeof(T), v.size(), f) == v.size(); }

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

struct FrameData {
    std::vector<orbmi::KeyPoint> keys;
    std::vector<uint8_t> desc;
    std::vector<float> ur, tcw;
    explicit FrameData(const std::string& p)
        : keys(load<orbmi::KeyPoint>(p + "_keys")), desc(load<uint8_t>(p + "_desc")), ur(load<float>(p + "_ur")),
          tcw(load<float>(p + "_tcw")) {}
    orbmi_frame_view view(const std::vector<float>& cam, const std::vector<float>& sf) const {
        orbmi_frame_view v{};
        v.n = (int)keys.size();
        v.keys_un = keys.data();
        v.u_right = ur.data();
        v.desc = desc.data();
        v.tcw = tcw.data();
        v.fx = cam[0]; v.fy = cam[1]; v.cx = cam[2]; v.cy = cam[3]; v.bf = cam[4]; v.mb = cam[5];
        v.min_x = 0.f; v.max_x = cam[6]; v.min_y = 0.f; v.max_y = cam[7];
        v.grid_w_inv = cam[8]; v.grid_h_inv = cam[9];
        v.nlevels = (int)sf.size();
        v.scale_factors = sf.data();
        v.log_scale_factor = cam[10];
        return v;
    }
};

// ComputeSim3's guided search (src/LoopClosing.cc:379): matcher.SearchBySim3(mpCurrentKF, pKF,
// vpMapPointMatches, s, R, t, 7.5)
static int search(const char* dir) {
    g_dir = dir;
    try {
        const auto cam = load<float>("cam"), sf = load<float>("scale_factors"), sim3 = load<float>("sim3");
        const FrameData K1("kf1"), K2("kf2");
        const auto mps1 = load<orbmi_mappoint>("mps1"), mps2 = load<orbmi_mappoint>("mps2");
        const auto has1 = load<uint8_t>("has1"), has2 = load<uint8_t>("has2");
        auto match12 = load<int32_t>("match12");
        if (sim3.size() != 14) throw std::runtime_error("in_sim3: s12 R12[9] t12[3] th");
        orbmi::ORBmatcher matcher(0.75f, true);
        const int nFound = matcher.SearchBySim3(K1.view(cam, sf), mps1, has1, K2.view(cam, sf), mps2, has2, match12, sim3[0],
                                                &sim3[1], &sim3[10], sim3[13]);
        save("match12", match12);
        save("nfound", std::vector<int32_t>{nFound});
        printf("nFound %d\n", nFound);
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    if (std::string(argv[1]) == "search") return search(argv[2]);
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hd[3], N1 = 0;
    float k[8];
    if (fread(hd, sizeof(int32_t), 3, f) != 3 || fread(k, sizeof(float), 8, f) != 8 || hd[0] < 0 || hd[1] < 0) return 2;
    const int n = hd[0], H = hd[1];
    std::vector<float> X1(3 * (size_t)n), X2(3 * (size_t)n);
    std::vector<int32_t> e1(n), e2(n), tri(3 * (size_t)H), idx1(n);
    if (!rd(f, X1) || !rd(f, X2) || !rd(f, e1) || !rd(f, e2) || !rd(f, tri) || fread(&N1, sizeof(int32_t), 1, f) != 1 ||
        !rd(f, idx1))
        return 2;
    fclose(f);
    const int minInliers = argc > 3 ? atoi(argv[3]) : 20;
    try {
        orbmi::ORBmatcher matcher(0.75f, true);
        orbmi::Sim3Solver solver(X1, X2, e1, e2, idx1, N1, k, k + 4, hd[2] != 0);
        solver.SetRansacParameters(0.99, minInliers, 300);
        tri.resize(3 * (size_t)solver.GetIterations());
        solver.SetTriples(tri);
        bool bNoMore = false, ok = false;
        std::vector<bool> vbInliers;
        int nInliers = 0, calls = 0;
        float T12[16] = {0}, st[13] = {0};
        while (!ok && !bNoMore) {  // :349-398 for one candidate
            ok = solver.iterate(matcher, 5, bNoMore, vbInliers, nInliers, T12);
            calls++;
        }
        if (ok) {
            st[0] = solver.GetEstimatedScale();
            solver.GetEstimatedTranslation(st + 1);
            solver.GetEstimatedRotation(st + 4);
        }
        const int32_t head[5] = {solver.GetIterations(), calls, ok, bNoMore, nInliers};
        std::vector<uint8_t> vb(vbInliers.begin(), vbInliers.end());
        f = fopen(argv[2], "wb");
        if (!f || fwrite(head, sizeof(int32_t), 5, f) != 5 || fwrite(T12, sizeof(float), 16, f) != 16 ||
            fwrite(st, sizeof(float), 13, f) != 13 || fwrite(vb.data(), 1, vb.size(), f) != vb.size())
            return 2;
        fclose(f);
        printf("iterations %d calls %d success %d inliers %d\n", head[0], calls, (int)ok, nInliers);
    } catch (const orbmi::Error& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
