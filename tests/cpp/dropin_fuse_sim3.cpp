// orbmi::ORBmatcher::FuseSearch(KFs, Scw, ...) of include/orbmi.hpp with the call shape of
// LoopClosing::SearchAndFuse (src/LoopClosing.cc:725-754): one list of loop map points searched in
// several keyframes, each under its own Sim3, for tests/test_cpp_dropin_fuse_sim3.py to compare
// with the C call's arrays.
//
//   dropin_fuse_sim3 <in> <out>
// in : int32 nkf, n_mp, has_in_kf, nlevels; float32 th; float32 scale factors (nlevels); per keyframe
//      int32 n, float32 fx fy cx cy bf mb min_x max_x min_y max_y grid_w_inv grid_h_inv
//      log_scale_factor, keypoints (n x 28 B), descriptors (n x 32 B), float32 u_right (n); then
//      float32 Scw (nkf x 12), orbmi_mappoint (n_mp x 68 B), uint8 in_kf (nkf x n_mp, if has_in_kf)
// out: int32 best_idx (nkf x n_mp), int32 best_dist (nkf x n_mp), int32 nfused (nkf)
#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "orbmi.hpp"

namespace {

template <class T>
bool get(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

struct KeyFrameData {
    std::vector<orbmi_keypoint> keys;
    std::vector<uint8_t> desc;
    std::vector<float> ur;
};

}  // namespace

int main(int argc, char** argv) {
    try {
        if (argc < 3) return 2;
        FILE* f = fopen(argv[1], "rb");
        if (!f) return 2;
        int32_t hd[4];
        float th = 0;
        if (fread(hd, sizeof(int32_t), 4, f) != 4 || fread(&th, sizeof(float), 1, f) != 1) return 2;
        if (hd[0] < 0 || hd[1] < 0 || hd[3] < 1) return 2;
        const size_t nkf = (size_t)hd[0], n = (size_t)hd[1];
        std::vector<float> scale;
        if (!get(f, scale, (size_t)hd[3])) return 2;
        std::vector<KeyFrameData> data(nkf);
        std::vector<orbmi_frame_view> KFs(nkf);
        for (size_t k = 0; k < nkf; k++) {
            int32_t nk = 0;
            float c[13];
            if (fread(&nk, sizeof(int32_t), 1, f) != 1 || nk < 0 || fread(c, sizeof(float), 13, f) != 13) return 2;
            KeyFrameData& D = data[k];
            if (!get(f, D.keys, (size_t)nk) || !get(f, D.desc, 32 * (size_t)nk) || !get(f, D.ur, (size_t)nk)) return 2;
            orbmi_frame_view& v = KFs[k];
            v = orbmi_frame_view{};
            v.n = nk;
            v.keys_un = D.keys.data();
            v.u_right = D.ur.data();
            v.desc = D.desc.data();
            v.fx = c[0]; v.fy = c[1]; v.cx = c[2]; v.cy = c[3]; v.bf = c[4]; v.mb = c[5];
            v.min_x = c[6]; v.max_x = c[7]; v.min_y = c[8]; v.max_y = c[9];
            v.grid_w_inv = c[10]; v.grid_h_inv = c[11];
            v.nlevels = hd[3];
            v.scale_factors = scale.data();
            v.log_scale_factor = c[12];
        }
        std::vector<float> Scw;
        std::vector<orbmi_mappoint> mps;
        std::vector<uint8_t> in_kf;
        if (!get(f, Scw, 12 * nkf) || !get(f, mps, n) || !get(f, in_kf, hd[2] ? nkf * n : 0)) return 2;
        fclose(f);
        orbmi::ORBmatcher matcher;
        std::vector<int32_t> bestIdx, bestDist;
        std::vector<int> nFused;
        matcher.FuseSearch(KFs, Scw.data(), mps, in_kf, th, bestIdx, bestDist, nFused);
        f = fopen(argv[2], "wb");
        if (!f) return 2;
        const std::vector<int32_t> nf(nFused.begin(), nFused.end());
        const bool ok = fwrite(bestIdx.data(), sizeof(int32_t), bestIdx.size(), f) == bestIdx.size() &&
                        fwrite(bestDist.data(), sizeof(int32_t), bestDist.size(), f) == bestDist.size() &&
                        fwrite(nf.data(), sizeof(int32_t), nf.size(), f) == nf.size();
        fclose(f);
        return ok ? 0 : 2;
    } catch (const std::exception& e) {
        fprintf(stderr, "dropin_fuse_sim3: %s\n", e.what());
        return 1;
    }
}
