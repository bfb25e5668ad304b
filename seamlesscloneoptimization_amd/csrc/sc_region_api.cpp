// sc_region_api.cpp -- the region solve on float32 images (sc_hip_region_check, sc_hip_region_device, sc_hip_region): the WLS problem on a
// domain of any shape.  One more array per job, state, says of every pixel the border kind calls an unknown whether it is solved for
// (SC_REGION_UNKNOWN), fixed at data's value (SC_REGION_KNOWN) or not part of the domain (SC_REGION_OUTSIDE: its links do not exist).
// The call is the WLS call with another folding of the caller's arrays into the coefficient planes E, S, Dg (sc_region.hip: why the
// unchanged operator launch is exact): the same entry code (sc_pcg.h; the front end with FLOAT_STATE), the same iteration, and
// RegionOperator (sc_pcg.h), a WlsOperator with its own
//   statistics  k_region_stats; a job with a state that is not 0, 1 or 2, an invalid weight or link where one is read, or -- without any
//               Dirichlet line -- a channel with UNKNOWN pixels that no KNOWN neighbour and no weight pins gets SC_ERR_BAD_ARG and leaves.
//   constants   s-bar = precond_smooth, or the mean of the links live in the region over the chunk's remaining jobs (1 without link
//               arrays); w-bar = precond_lambda, or (sum of w + sum of the UNKNOWN - KNOWN links) / (UNKNOWN pixels) over them: a KNOWN
//               neighbour holds its pixel as a data weight of the link's size would.  M = s-bar (A - w-bar / s-bar) on the whole rectangle.
//   set-up      k_region_setup;   operator   the WLS one (launch_wls_op);   output   k_region_out in place of the shared launch.
// state travels as every side array does: SideArrays::st, in PcgOperator::ds beside the job.
#include "sc_pcg.h"
#include <algorithm>
#include <cassert>
#include <cmath>
#include <vector>

using namespace sc;

namespace {

int region_validate(const sc_region_params *p, const sc_poisson_layout *l, const char **why)
{
    const char *own = !p ? nullptr : !std::isfinite(p->tol) ? "tol must be finite"
                    : !std::isfinite(p->precond_lambda) ? "precond_lambda must be finite"
                    : !std::isfinite(p->precond_smooth) ? "precond_smooth must be finite" : nullptr;
    return family_validate(p ? &p->kind : nullptr, l, own,
                           "a region solve is preconditioned by a direct solve: at most 8192 unknowns (pixels - 2) per side", why);
}

constexpr const char *METHOD_WHY = "a region solve is solved by SC_METHOD_AUTO and SC_METHOD_FFT only (conjugate gradients preconditioned by the direct solve)";
constexpr const char *FP64_WHY = "a region solve with SC_FLAG_FFT_FP64: at most 4096 unknowns per axis";

int carries_of(bool weight, bool links) { return FLOAT_DATA | FLOAT_STATE | (weight ? FLOAT_WEIGHT : 0) | (links ? FLOAT_SMOOTH : 0); }

PcgCall region_call(int kind, const sc_region_params *p) { return PcgCall{ kind, p->tol, p->max_iters, 400 }; }

} // namespace

extern "C" {

int sc_hip_region_check(const sc_region_params *p, const sc_poisson_layout *l)
{
    return region_validate(p, l, nullptr);
}

int sc_hip_region_device(void *inst, const sc_region_params *p, const sc_poisson_layout *l, sc_region_job *jobs, int n, bool bSync)
{
    Instance *I;
    int kind, rc = pcg_begin(inst, p, l, region_validate, METHOD_WHY, FP64_WHY, I, kind);
    if (rc) return rc;
    // the data term and the link arrays: all jobs or none, as the first job has them; a job that differs is refused (as one with exactly
    // one of the two link arrays)
    const bool weight = jobs && n > 0 && jobs[0].weight, links = jobs && n > 0 && (jobs[0].smooth_x || jobs[0].smooth_y);
    RegionOperator op(I, weight, links, p->precond_lambda, p->precond_smooth);
    return pcg_device_call(I, region_call(kind, p), l, carries_of(weight, links), jobs, n, [weight, links](const sc_region_job &j) {
        const bool stray = (!weight && j.weight) || (!links && (j.smooth_x || j.smooth_y));      // (refused through its data pointer)
        return FloatArrays{ j.gx, j.gy, j.lap, stray ? nullptr : j.data, j.weight, j.boundary, j.out, j.smooth_x, j.smooth_y, j.state }; }, op, bSync);
}

int sc_hip_region(void *inst, const sc_region_params *p, const sc_poisson_layout *l, const float *gx, const float *gy, const float *lap,
                  const float *data, const float *state, const float *weight, const float *smooth_x, const float *smooth_y,
                  const float *boundary, float *out)
{
    Instance *I;
    int kind, rc = pcg_begin(inst, p, l, region_validate, METHOD_WHY, FP64_WHY, I, kind);
    if (rc) return rc;
    if (!smooth_x != !smooth_y) { I->err = "smooth_x and smooth_y go together (both NULL: every link 1)"; return SC_ERR_BAD_ARG; }
    const bool has_w = weight != nullptr, links = smooth_x != nullptr;
    RegionOperator op(I, has_w, links, p->precond_lambda, p->precond_smooth);
    return pcg_host_call(I, region_call(kind, p), l, carries_of(has_w, links),
                         FloatArrays{ gx, gy, lap, data, weight, boundary, out, smooth_x, smooth_y, state }, op);
}

} // extern "C"
