// Launch interface of the essential-graph kernels (essgraph.hip), used by capi_loop.cpp.
#pragma once
#include "matcher.h"
#include "essgraph.h"

namespace orbmi {

// One call's device arrays.  The plan's tables are eg_plan()'s, checked by eg_plan_ok() before
// anything is launched.
struct EgDev {
    int nv, ne, nf, nl, fix_scale;
    const EgEdge* edges;  // ne
    const int *vert_of, *col_ptr, *row_of, *upd_ptr, *upd, *asm_ptr, *asm_ent;
    double* recs;      // ne x kEgRec
    double *Hd, *Ho;   // nf x 49, nl x 49: H in the factor's layout
    double* b;         // nf x 7
    double *Ld, *Lo;   // the factor
    double* x;         // nf x 7
    double* y;         // nf x 7: the right-hand side the forward substitution works on
    double* chi2;      // ne: the trial's chi2 per edge
    double* out;       // kEgOut doubles
};
constexpr int kEgOutChi = 0;    // sum of chi2
constexpr int kEgOutScale = 1;  // computeScale's sum x (lambda x + b)
constexpr int kEgOutFail = 2;   // != 0: the solve met a bad pivot (x = 0)
constexpr int kEgOut = 4;

// e, chi2 and the three products of every edge at est -> recs; their chi2 summed -> out[kEgOutChi]
int launch_eg_linearize(Matcher& m, const EgDev& D, const Sim3d* est);
// recs -> Hd, Ho, b
int launch_eg_assemble(Matcher& m, const EgDev& D);
// (H + lambda I) x = b -> x, out[kEgOutScale], out[kEgOutFail]
int launch_eg_factor_solve(Matcher& m, const EgDev& D, double lambda);
// trial[v] = oplus(est[v], x) for every free vertex; the edges' chi2 at trial -> out[kEgOutChi]
int launch_eg_update(Matcher& m, const EgDev& D, const Sim3d* est, Sim3d* trial);
// CorrectLoop's arithmetic: out_points[i] = Swr[ref[i]].map(Srw[ref[i]].map(points[i])),
// out_tcw[k] = [R | t / s] of poses[k]
int launch_eg_correct(Matcher& m, int npoints, const float* points, const int32_t* ref, const Sim3d* Srw, const Sim3d* Swr,
                      float* out_points, int nposes, const Sim3d* poses, float* out_tcw);

}  // namespace orbmi
