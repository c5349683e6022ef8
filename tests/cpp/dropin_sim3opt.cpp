// orbmi::OptimizeSim3 and orbmi::ORBmatcher::SearchByProjection(KF, Scw) of include/orbmi.hpp with
// the call shapes of LoopClosing::ComputeSim3 (src/LoopClosing.cc:399-471), for
// tests/test_sim3opt_gpu.py to compare with the Python path.
//
//   dropin_sim3opt <in> <out>
// in : one problem as tests/cpp/sim3opt_check.cpp reads it
// out: float64 q[4] t[3] s, float32 sR[9] t_f[3], int32 n_in n_bad iterations[2], uint8 inlier (n)
//
//   dropin_sim3opt search <dir>
// in_cam, in_scale_factors, in_kf_keys / _desc / _ur / _tcw as tests/cpp/dropin_match_ba.cpp reads
// frames, in_mps, in_matched, in_scw = Scw[12] th; writes out_matched and out_nmatches.
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

static int run_search(const char* dir) {
    g_dir = dir;
    const auto cam = load<float>("cam"), sf = load<float>("scale_factors");
    const auto keys = load<orbmi::KeyPoint>("kf_keys");
    const auto desc = load<uint8_t>("kf_desc");
    const auto ur = load<float>("kf_ur"), tcw = load<float>("kf_tcw");
    orbmi_frame_view v{};
    v.n = (int)keys.size();
    v.keys_un = keys.data();
    v.u_right = ur.data();
    v.desc = desc.data();
    v.tcw = tcw.data();
    v.fx = cam[0]; v.fy = cam[1]; v.cx = cam[2]; v.cy = cam[3]; v.bf = cam[4]; v.mb = cam[5];
    v.min_x = 0; v.max_x = cam[6]; v.min_y = 0; v.max_y = cam[7];
    v.grid_w_inv = cam[8]; v.grid_h_inv = cam[9];
    v.nlevels = (int)sf.size();
    v.scale_factors = sf.data();
    v.log_scale_factor = cam[10];
    const auto mps = load<orbmi_mappoint>("mps");
    auto matched = load<int32_t>("matched");
    const auto scw = load<float>("scw");
    orbmi::ORBmatcher matcher;
    const int n = matcher.SearchByProjection(v, scw.data(), mps, matched, (int)scw[12]);
    save("matched", matched);
    save("nmatches", std::vector<int32_t>{n});
    return 0;
}

int main(int argc, char** argv) {
    try {
        if (argc == 3 && std::string(argv[1]) == "search") return run_search(argv[2]);
        if (argc < 3) return 2;
        FILE* f = fopen(argv[1], "rb");
        if (!f) return 2;
        int32_t hd[2];
        float par[22];
        if (fread(hd, sizeof(int32_t), 2, f) != 2 || fread(par, sizeof(float), 22, f) != 22) return 2;
        const size_t n = (size_t)hd[0];
        orbmi::Sim3OptInput in;
        in.bFixScale = hd[1] != 0;
        in.th2 = par[0];
        for (int k = 0; k < 4; k++) { in.K1[k] = par[1 + k]; in.K2[k] = par[5 + k]; }
        for (int k = 0; k < 9; k++) in.R12[k] = par[9 + k];
        for (int k = 0; k < 3; k++) in.t12[k] = par[18 + k];
        in.s12 = par[21];
        in.x3Dc1.resize(3 * n); in.x3Dc2.resize(3 * n);
        in.obs1.resize(2 * n); in.obs2.resize(2 * n);
        in.invSigma2_1.resize(n); in.invSigma2_2.resize(n);
        for (std::vector<float>* v : {&in.x3Dc1, &in.x3Dc2, &in.obs1, &in.obs2, &in.invSigma2_1, &in.invSigma2_2})
            if (fread(v->data(), sizeof(float), v->size(), f) != v->size()) return 2;
        fclose(f);
        orbmi::ORBmatcher matcher;
        orbmi::Sim3OptOutput out;
        const int nIn = orbmi::OptimizeSim3(matcher, in, out);
        const double head[8] = {out.q[0], out.q[1], out.q[2], out.q[3], out.t[0], out.t[1], out.t[2], out.s};
        const int32_t cnt[4] = {nIn, out.nBad, out.iterations[0], out.iterations[1]};
        f = fopen(argv[2], "wb");
        if (!f) return 2;
        const bool ok = fwrite(head, sizeof(double), 8, f) == 8 && fwrite(out.sR, sizeof(float), 9, f) == 9 &&
                        fwrite(out.tf, sizeof(float), 3, f) == 3 && fwrite(cnt, sizeof(int32_t), 4, f) == 4 &&
                        fwrite(out.inlier.data(), 1, n, f) == n;
        fclose(f);
        return ok ? 0 : 2;
    } catch (const std::exception& e) {
        fprintf(stderr, "dropin_sim3opt: %s\n", e.what());
        return 1;
    }
}
