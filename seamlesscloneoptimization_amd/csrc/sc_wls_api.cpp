// sc_wls_api.cpp -- the WLS solve on float32 images (sc_hip_wls_check, sc_hip_wls_device, sc_hip_wls): per-link smoothness weights on
// the gradient term,
//     minimise sum w (u - d)^2 + sum_x-links sx (u(x+1, y) - u(x, y) - gx)^2 + sum_y-links sy (u(x, y+1) - u(x, y) - gy)^2,
//     i.e.   L u = div(s g) - W d,     (L u)(p) = sum_q s(p, q) (u(q) - u(p)) - w(p) u(p),
// under every border kind of sc_hip_weighted.  The call is the weighted call with another operator: the same entry code (sc_pcg.h:
// pcg_begin, pcg_host_call, pcg_device_call; the front end with FLOAT_SMOOTH), the same iteration (pcg_run, sc_pcg.cpp), and WlsOperator
// (declared in sc_pcg.h, defined here; the robust call's RobustOperator, sc_robust_api.cpp, derives from it) in place of the weighted one:
//   statistics  per plane the sums of w and of the live links and how many of each are invalid (k_wls_stats); a job with an invalid
//               weight or link, or -- without any Dirichlet line -- with a channel of zero weight, gets SC_ERR_BAD_ARG and leaves.
//               Without link weights (a robust call without base links): the weighted call's statistics, the links not judged.
//   constants   s-bar = precond_smooth, or the mean live link of the chunk's remaining jobs (1 without link weights); w-bar =
//               precond_lambda, or their mean weight.  The preconditioner is M = s-bar (A - w-bar / s-bar): the direct solve with
//               lam = w-bar / s-bar, and the factor 1 / s-bar once, on u0.
//   set-up      b and the planes E, S, Dg (k_wls_setup; without link weights its constant-link form);   operator   k_pcg_op with WlsCoef.
// The jobs' arrays are the driver's (PcgOperator::dj, ds: it moves the jobs that stay to the front); the operator keeps the running sums.
#include "sc_pcg.h"
#include <algorithm>
#include <cmath>
#include <vector>

using namespace sc;

namespace {

int wls_validate(const sc_wls_params *p, const sc_poisson_layout *l, const char **why)
{
    const char *own = !p ? nullptr : !std::isfinite(p->tol) ? "tol must be finite"
                    : !std::isfinite(p->precond_lambda) ? "precond_lambda must be finite"
                    : !std::isfinite(p->precond_smooth) ? "precond_smooth must be finite" : nullptr;
    return family_validate(p ? &p->kind : nullptr, l, own,
                           "a WLS solve is preconditioned by a direct solve: at most 8192 unknowns (pixels - 2) per side", why);
}

constexpr int CARRIES = FLOAT_DATA | FLOAT_WEIGHT | FLOAT_SMOOTH;
constexpr const char *METHOD_WHY = "a WLS solve is solved by SC_METHOD_AUTO and SC_METHOD_FFT only (conjugate gradients preconditioned by the direct solve)";
constexpr const char *FP64_WHY = "a WLS solve with SC_FLAG_FFT_FP64: at most 4096 unknowns per axis";

} // namespace

namespace sc {

void WlsOperator::begin()
{
    wsum = ssum = 0.0;
    unit_links = !links;
}

void WlsOperator::stats(const PoissonGeo &g, const PcgGeo &wg, int m, double *d_stats, hipStream_t s)
{
    if (links) launch_wls_stats(g, wg, dj.data(), ds.data(), m, d_stats, s);
    else launch_weighted_stats(g, wg, dj.data(), ds.data(), m, d_stats, s);
}

const char *WlsOperator::judge(const PoissonGeo &g, int k, const double *st, int parts, bool no_dirichlet)
{
    double job_w, job_s = 0.0;
    bool bad_s = false;
    for (int c = 0; links && c < g.C; ++c) {
        const double *plane = st + (size_t)c * PCG_PARTS * WLS_STATS;
        bad_s = bad_s || stat_sum(plane, parts, 3) != 0.0;
        job_s += stat_sum(plane, parts, 2);
    }
    const char *why = judge_weights(g, st, parts, no_dirichlet,
                                    bad_s || !std::isfinite(job_s) ? "a live link weight is not finite or not > 0" : nullptr, job_w);
    if (why) return why;
    wsum += job_w;
    ssum += job_s;
    return nullptr;
}

float WlsOperator::precond_constant(const PoissonGeo &g, const PcgGeo &wg, int mv)
{
    const double planes = (double)(g.C * mv);
    const double wbar = plam > 0.f ? (double)plam : wsum / ((double)wg.nx * (double)wg.ny * planes);
    // (a plane of one unknown without a Dirichlet line has no link at all: its equation is -w u = b, any s-bar serves)
    const double live = wls_live_links(wg) * planes, sbar = psmooth > 0.f ? (double)psmooth : unit_links || !(live > 0.0) ? 1.0 : ssum / live;
    u0_scale = (float)(1.0 / sbar);
    return (float)(wbar / sbar);
}

void WlsOperator::scale_start(const PcgGeo &wg, int planes, float *U, hipStream_t s) { launch_pcg_scale(wg, planes, U, u0_scale, s); }

int WlsOperator::setup(const PoissonGeo &g, const PcgGeo &wg, bool lap, int mv, float *R, double *bb)
{
    PcgState &S = *I->pcg;
    for (DevBuf *b : { &S.e, &S.s, &S.dg }) {
        const int rc = ensure(I, *b, sizeof(float) * (size_t)wg.stride * g.C * mv, false);
        if (rc) return rc;
    }
    launch_wls_setup(g, wg, lap, dj.data(), ds.data(), mv, R, (float *)S.e.p, (float *)S.s.p, (float *)S.dg.p, bb, I->stream);
    return SC_OK;
}

void WlsOperator::apply(const PcgGeo &wg, int planes, bool residual, const float *P, float *Q, double *parts, hipStream_t s)
{
    const PcgState &S = *I->pcg;
    launch_wls_op(wg, planes, residual, P, (const float *)S.e.p, (const float *)S.s.p, (const float *)S.dg.p, Q, parts, s);
}

} // namespace sc

extern "C" {

int sc_hip_wls_check(const sc_wls_params *p, const sc_poisson_layout *l)
{
    return wls_validate(p, l, nullptr);
}

int sc_hip_wls_device(void *inst, const sc_wls_params *p, const sc_poisson_layout *l, sc_wls_job *jobs, int n, bool bSync)
{
    Instance *I;
    int kind, rc = pcg_begin(inst, p, l, wls_validate, METHOD_WHY, FP64_WHY, I, kind);
    if (rc) return rc;
    WlsOperator op(I, true, p->precond_lambda, p->precond_smooth);
    return pcg_device_call(I, PcgCall{ kind, p->tol, p->max_iters, 400 }, l, CARRIES, jobs, n, [](const sc_wls_job &j) {
        return FloatArrays{ j.gx, j.gy, j.lap, j.data, j.weight, j.boundary, j.out, j.smooth_x, j.smooth_y }; }, op, bSync);
}

int sc_hip_wls(void *inst, const sc_wls_params *p, const sc_poisson_layout *l, const float *gx, const float *gy, const float *lap,
               const float *data, const float *weight, const float *smooth_x, const float *smooth_y, const float *boundary, float *out)
{
    Instance *I;
    int kind, rc = pcg_begin(inst, p, l, wls_validate, METHOD_WHY, FP64_WHY, I, kind);
    if (rc) return rc;
    WlsOperator op(I, true, p->precond_lambda, p->precond_smooth);
    return pcg_host_call(I, PcgCall{ kind, p->tol, p->max_iters, 400 }, l, CARRIES,
                         FloatArrays{ gx, gy, lap, data, weight, boundary, out, smooth_x, smooth_y }, op);
}

} // extern "C"
