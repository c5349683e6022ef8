// orbmi::Optimizer::OptimizeEssentialGraph and CorrectPoints of include/orbmi.hpp with the call shape
// of LoopClosing::CorrectLoop (src/LoopClosing.cc:662-664), for tests/test_cpp_dropin_essgraph.py
// to compare with the Python path.
//
//   dropin_essgraph <in> <out>
// in : one problem as tests/cpp/essgraph_check.cpp reads it, then int32 npoints, float32 points
//      (npoints x 3), int32 ref (npoints)
// out: float64 vertices (nv x 8), float32 Tcw (nv x 16), float64 chi2 before / after, int32 iterations
//      status, float32 points (npoints x 3): each corrected from its input vertex to the optimised one
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
        if (fread(hd, sizeof(int32_t), 5, f) != 5 || hd[0] < 1 || hd[2] < 0) return 2;
        const size_t nv = (size_t)hd[0], ne = (size_t)hd[2];
        orbmi::EssentialGraphInput in;
        in.fixed = hd[1];
        in.bFixScale = hd[3] != 0;
        in.iterations = hd[4];
        in.vertices.resize(8 * nv);
        in.v0.resize(ne);
        in.v1.resize(ne);
        in.measurements.resize(8 * ne);
        int32_t np = 0;
        if (fread(in.vertices.data(), sizeof(double), 8 * nv, f) != 8 * nv || fread(in.v0.data(), sizeof(int32_t), ne, f) != ne ||
            fread(in.v1.data(), sizeof(int32_t), ne, f) != ne || fread(in.measurements.data(), sizeof(double), 8 * ne, f) != 8 * ne ||
            fread(&np, sizeof(int32_t), 1, f) != 1 || np < 0)
            return 2;
        std::vector<float> points(3 * (size_t)np);
        std::vector<int32_t> ref((size_t)np);
        if (fread(points.data(), sizeof(float), points.size(), f) != points.size() ||
            fread(ref.data(), sizeof(int32_t), ref.size(), f) != ref.size())
            return 2;
        fclose(f);
        orbmi::ORBmatcher matcher;
        const orbmi::EssentialGraphOutput out = orbmi::Optimizer::OptimizeEssentialGraph(matcher, in);
        // vCorrectedSwc = the optimised estimates inverted, as the caller of CorrectPoints holds them:
        // (r.conjugate(), r.conjugate() * ((-1. / s) * t), 1. / s)
        std::vector<double> Swc(8 * nv);
        for (size_t i = 0; i < nv; i++) {
            const double* S = &out.vertices[8 * i];
            double* I = &Swc[8 * i];
            const double q[4] = {-S[0], -S[1], -S[2], S[3]}, m = -1. / S[7];
            const double v[3] = {m * S[4], m * S[5], m * S[6]};
            double ux = q[1] * v[2] - q[2] * v[1], uy = q[2] * v[0] - q[0] * v[2], uz = q[0] * v[1] - q[1] * v[0];
            ux = ux + ux; uy = uy + uy; uz = uz + uz;
            const double cx = q[1] * uz - q[2] * uy, cy = q[2] * ux - q[0] * uz, cz = q[0] * uy - q[1] * ux;
            I[0] = q[0]; I[1] = q[1]; I[2] = q[2]; I[3] = q[3];
            I[4] = (v[0] + q[3] * ux) + cx;
            I[5] = (v[1] + q[3] * uy) + cy;
            I[6] = (v[2] + q[3] * uz) + cz;
            I[7] = 1. / S[7];
        }
        const std::vector<float> moved = orbmi::Optimizer::CorrectPoints(matcher, points, ref, in.vertices, Swc);
        const double chi[2] = {out.chi2Before, out.chi2After};
        const int32_t tail[2] = {out.iterations, out.status};
        f = fopen(argv[2], "wb");
        if (!f) return 2;
        const bool ok = fwrite(out.vertices.data(), sizeof(double), 8 * nv, f) == 8 * nv &&
                        fwrite(out.Tcw.data(), sizeof(float), 16 * nv, f) == 16 * nv && fwrite(chi, sizeof(double), 2, f) == 2 &&
                        fwrite(tail, sizeof(int32_t), 2, f) == 2 &&
                        fwrite(moved.data(), sizeof(float), moved.size(), f) == moved.size();
        fclose(f);
        return ok ? 0 : 2;
    } catch (const std::exception& e) {
        fprintf(stderr, "dropin_essgraph: %s\n", e.what());
        return 1;
    }
}
