// sc_wls_api.cpp -- the WLS solve on float32 images (sc_hip_wls_check, sc_hip_wls_device, sc_hip_wls): per-link smoothness weights on
// the gradient term,
//     minimise sum w (u - d)^2 + sum_x-links sx (u(x+1, y) - u(x, y) - gx)^2 + sum_y-links sy (u(x, y+1) - u(x, y) - gy)^2,
//     i.e.   L u = div(s g) - W d,     (L u)(p) = sum_q s(p, q) (u(q) - u(p)) - w(p) u(p),
// under every border kind of sc_hip_weighted.  The call is the weighted call with another operator: the same front end (float_intake,
// float_stage with FLOAT_SMOOTH), the same iteration (pcg_run, sc_pcg.cpp), this file's WlsOperator in place of the weighted
// one:
//   statistics  per plane the sums of w and of the live links and how many of each are invalid (k_wls_stats); a job with an invalid
//               weight or link, or -- without any Dirichlet line -- with a channel of zero weight, gets SC_ERR_BAD_ARG and leaves.
//   constants   s-bar = precond_smooth, or the mean live link of the chunk's remaining jobs; w-bar = precond_lambda, or their mean
//               weight.  The preconditioner is M = s-bar (A - w-bar / s-bar): the direct solve with lam = w-bar / s-bar, and the
//               factor 1 / s-bar once, on u0.
//   set-up      b and the planes E, S, Dg (k_wls_setup);   operator   k_pcg_op with WlsCoef.
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

// what every entry starts with: the instance, the call's validation and the instance's word on it; kind: poisson_norm_kind's
int wls_begin(void *inst, const sc_wls_params *p, const sc_poisson_layout *l, Instance *&I, int &kind)
{
    int rc = begin_call(inst, I);
    if (rc) return rc;
    const char *why = "";
    if ((rc = wls_validate(p, l, &why))) { I->err = why; return rc; }
    kind = poisson_norm_kind(p->kind);
    return direct_instance_check(I, kind, l,
        "a WLS solve is solved by SC_METHOD_AUTO and SC_METHOD_FFT only (conjugate gradients preconditioned by the direct solve)",
        "a WLS solve with SC_FLAG_FFT_FP64: at most 4096 unknowns per axis");
}

constexpr int CARRIES = FLOAT_DATA | FLOAT_WEIGHT | FLOAT_SMOOTH;

struct WlsOperator final : PcgOperator {
    Instance *I;
    const float *const *all_w, *const *all_sx, *const *all_sy;
    float plam, psmooth;
    std::vector<const float *> dw, dsx, dsy;
    int kept = 0;
    double wsum = 0.0, ssum = 0.0;
    float u0_scale = 1.f;                  // 1 / s-bar of the current chunk
    WlsOperator(Instance *I_, const float *const *w, const float *const *sx, const float *const *sy, const sc_wls_params *p)
        : PcgOperator(WLS_STATS), I(I_), all_w(w), all_sx(sx), all_sy(sy), plam(p->precond_lambda), psmooth(p->precond_smooth) {}
    void begin(int i0, int m) override
    {
        dw.assign(all_w + i0, all_w + i0 + m);
        dsx.assign(all_sx + i0, all_sx + i0 + m);
        dsy.assign(all_sy + i0, all_sy + i0 + m);
        kept = 0;
        wsum = ssum = 0.0;
    }
    void stats(const PoissonGeo &g, const PcgGeo &wg, int m, double *d_stats, hipStream_t s) override
    {
        launch_wls_stats(g, wg, dj.data(), dw.data(), dsx.data(), dsy.data(), m, d_stats, s);
    }
    const char *judge(const PoissonGeo &g, int k, const double *st, int parts, bool no_dirichlet) override
    {
        double job_w = 0.0, job_s = 0.0;
        bool bad_w = false, bad_s = false, empty = false;
        for (int c = 0; c < g.C; ++c) {
            const double *plane = st + (size_t)c * PCG_PARTS * WLS_STATS;
            const double sum = stat_sum(plane, parts, 0);
            bad_w = bad_w || stat_sum(plane, parts, 1) != 0.0;
            bad_s = bad_s || stat_sum(plane, parts, 3) != 0.0;
            empty = empty || !(sum > 0.0);
            job_w += sum;
            job_s += stat_sum(plane, parts, 2);
        }
        if (bad_w || !std::isfinite(job_w)) return "a weight is negative or not finite";
        if (bad_s || !std::isfinite(job_s)) return "a live link weight is not finite or not > 0";
        if (no_dirichlet && empty) return "no data weight and no Dirichlet line";
        dw[kept] = dw[k];
        dsx[kept] = dsx[k];
        dsy[kept++] = dsy[k];
        wsum += job_w;
        ssum += job_s;
        return nullptr;
    }
    float precond_constant(const PoissonGeo &g, const PcgGeo &wg, int mv) override
    {
        const double planes = (double)(g.C * mv);
        const double wbar = plam > 0.f ? (double)plam : wsum / ((double)wg.nx * (double)wg.ny * planes);
        // (a plane of one unknown without a Dirichlet line has no link at all: its equation is -w u = b, any s-bar serves)
        const double links = wls_live_links(wg) * planes, sbar = psmooth > 0.f ? (double)psmooth : links > 0.0 ? ssum / links : 1.0;
        u0_scale = (float)(1.0 / sbar);
        return (float)(wbar / sbar);
    }
    void scale_start(const PcgGeo &wg, int planes, float *U, hipStream_t s) override { launch_pcg_scale(wg, planes, U, u0_scale, s); }
    int setup(const PoissonGeo &g, const PcgGeo &wg, bool lap, int mv, float *R, double *bb) override
    {
        PcgState &S = *I->pcg;
        for (DevBuf *b : { &S.e, &S.s, &S.dg }) {
            const int rc = ensure(I, *b, sizeof(float) * (size_t)wg.stride * g.C * mv, false);
            if (rc) return rc;
        }
        launch_wls_setup(g, wg, lap, dj.data(), dw.data(), dsx.data(), dsy.data(), mv, R, (float *)S.e.p, (float *)S.s.p, (float *)S.dg.p, bb,
                         I->stream);
        return SC_OK;
    }
    void apply(const PcgGeo &wg, int planes, bool residual, const float *P, float *Q, double *parts, hipStream_t s) override
    {
        const PcgState &S = *I->pcg;
        launch_wls_op(wg, planes, residual, P, (const float *)S.e.p, (const float *)S.s.p, (const float *)S.dg.p, Q, parts, s);
    }
};

} // namespace

extern "C" {

int sc_hip_wls_check(const sc_wls_params *p, const sc_poisson_layout *l)
{
    return wls_validate(p, l, nullptr);
}

int sc_hip_wls_device(void *inst, const sc_wls_params *p, const sc_poisson_layout *l, sc_wls_job *jobs, int n, bool bSync)
{
    Instance *I;
    int kind, rc = wls_begin(inst, p, l, I, kind);
    if (rc) return rc;
    FloatJobs v;
    const int worst = float_intake(I, kind, CARRIES, jobs, n, [](const sc_wls_job &j) {
        return FloatArrays{ j.gx, j.gy, j.lap, j.data, j.weight, j.boundary, j.out, j.smooth_x, j.smooth_y }; }, v, poisson_span(l));
    if (v.rcs.empty()) return worst;
    I->info.ms_h2d = I->info.ms_d2h = 0.f;
    WlsOperator op(I, v.w.data(), v.sx.data(), v.sy.data(), p);
    rc = pcg_run(I, PcgCall{ kind, p->tol, p->max_iters, 400 }, l, op, v.dj.data(), v.rcs.data(), (int)v.rcs.size(), bSync);
    return worse(worst, rc);
}

int sc_hip_wls(void *inst, const sc_wls_params *p, const sc_poisson_layout *l, const float *gx, const float *gy, const float *lap,
               const float *data, const float *weight, const float *smooth_x, const float *smooth_y, const float *boundary, float *out)
{
    Instance *I;
    int kind, rc = wls_begin(inst, p, l, I, kind);
    if (rc) return rc;
    const FloatArrays a{ gx, gy, lap, data, weight, boundary, out, smooth_x, smooth_y };
    const char *why = "";
    if ((rc = float_job_validate(kind, CARRIES, a, &why, poisson_span(l)))) { I->err = why; return rc; }
    FloatStaged s;
    if ((rc = float_stage(I, l, kind, CARRIES, a, s))) return rc;
    int job_rc = SC_ERR_HIP, *const job_rcs[1] = { &job_rc };
    WlsOperator op(I, &s.d_w, &s.d_sx, &s.d_sy, p);
    rc = pcg_run(I, PcgCall{ kind, p->tol, p->max_iters, 400 }, l, op, &s.job, job_rcs, 1, true);
    if (rc != SC_OK && rc != SC_ERR_NOT_CONVERGED) return rc;
    const float t[4] = { 0.f, I->info.ms_solve, 0.f, I->info.ms_call };     // (one solve stage: pcg_run times the call whole)
    return poisson_download(I, l, s.job.out, out, t, rc);
}

} // extern "C"
