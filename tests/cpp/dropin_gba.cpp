// orbmi::Optimizer::GlobalBundleAdjustemnt of include/orbmi.hpp with the call shape of
// LoopClosing::RunGlobalBundleAdjustment (src/LoopClosing.cc:804), for tests/test_cpp_dropin_gba.py
// to compare with the Python path.
//
//   dropin_gba <in> <out>
// in : int32 nkf, npt, nedge, iterations, robust; then the orbmi_ba_keyframe, orbmi_ba_point and
//      orbmi_ba_edge records
// out: float32 Tcw (nkf x 16), float32 pos (npt x 3), uint8 included (npt), int32 iterations, status,
//      stop_check, checks, int32 trials (iterations of the input), float64 chi2 initial / final
#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "orbmi.hpp"

int main(int argc, char** argv) {
    try {
        if (argc < 3) return 2;
        FILE* f = fopen(argv[1], "rb");
        if (!f) return 2;
        int32_t hd[5];
        if (fread(hd, sizeof(int32_t), 5, f) != 5 || hd[0] < 0 || hd[1] < 0 || hd[2] < 0) return 2;
        std::vector<orbmi_ba_keyframe> kfs((size_t)hd[0]);
        std::vector<orbmi_ba_point> pts((size_t)hd[1]);
        std::vector<orbmi_ba_edge> edges((size_t)hd[2]);
        if (fread(kfs.data(), sizeof(orbmi_ba_keyframe), kfs.size(), f) != kfs.size() ||
            fread(pts.data(), sizeof(orbmi_ba_point), pts.size(), f) != pts.size() ||
            fread(edges.data(), sizeof(orbmi_ba_edge), edges.size(), f) != edges.size())
            return 2;
        fclose(f);
        orbmi::LocalBundleAdjuster ba;
        volatile int mbStopGBA = 0;
        const orbmi::BundleAdjustmentOutput out =
            orbmi::Optimizer::GlobalBundleAdjustemnt(ba, kfs, pts, edges, hd[3], &mbStopGBA, hd[4] != 0);
        const int32_t tail[4] = {out.iterations, out.status, out.stop_check, out.checks};
        const std::vector<int32_t> trials(out.trials.begin(), out.trials.end());
        const double chi[2] = {out.chi2Initial, out.chi2};
        f = fopen(argv[2], "wb");
        if (!f) return 2;
        const bool ok = fwrite(out.Tcw.data(), sizeof(float), out.Tcw.size(), f) == out.Tcw.size() &&
                        fwrite(out.pos.data(), sizeof(float), out.pos.size(), f) == out.pos.size() &&
                        fwrite(out.included.data(), 1, out.included.size(), f) == out.included.size() &&
                        fwrite(tail, sizeof(int32_t), 4, f) == 4 &&
                        fwrite(trials.data(), sizeof(int32_t), trials.size(), f) == trials.size() &&
                        fwrite(chi, sizeof(double), 2, f) == 2;
        fclose(f);
        return ok ? 0 : 2;
    } catch (const std::exception& e) {
        fprintf(stderr, "dropin_gba: %s\n", e.what());
        return 1;
    }
}
