// sc_weighted_api.cpp -- the weighted solve on float32 images (sc_hip_weighted_check, sc_hip_weighted_device, sc_hip_weighted):
//     minimise sum w (u - d)^2 + sum |grad u - g|^2,   i.e.   (A - W) u = div g - W d,   W = diag(w), w >= 0,
// A the 5-point operator of sc_hip_poisson under every border kind (a Dirichlet frame, SC_POISSON_NEUMANN, SC_POISSON_FREE_*,
// SC_POISSON_PERIODIC_*).  A call: the float32 families' front end (sc_poisson_api.cpp: validation, job intake or host staging) -> the
// shared conjugate gradients (pcg_run, sc_pcg.cpp) with this file's WeightedOperator:
//   statistics  per plane the sum of w and the number of weights that are negative or not finite (k_w_stats); a job with such a weight,
//               or -- without any Dirichlet line -- with a channel of zero weight, gets SC_ERR_BAD_ARG and leaves.
//   constant    lambda-bar = precond_lambda, or the mean of w over the unknowns that remain: the preconditioner is M = A - lambda-bar.
//   set-up      b = lap - w d less the neighbouring Dirichlet values, and w itself (k_w_setup);   operator   k_pcg_op with WeightedCoef.
#include "sc_pcg.h"
#include <algorithm>
#include <cmath>
#include <vector>

using namespace sc;

namespace {

int weighted_validate(const sc_weighted_params *p, const sc_poisson_layout *l, const char **why)
{
    const char *own = !p ? nullptr : !std::isfinite(p->tol) ? "tol must be finite"
                    : !std::isfinite(p->precond_lambda) ? "precond_lambda must be finite" : nullptr;
    return family_validate(p ? &p->kind : nullptr, l, own,
                           "a weighted solve is preconditioned by a direct solve: at most 8192 unknowns (pixels - 2) per side", why);
}

// what every entry starts with: the instance, the call's validation and the instance's word on it; kind: poisson_norm_kind's
int weighted_begin(void *inst, const sc_weighted_params *p, const sc_poisson_layout *l, Instance *&I, int &kind)
{
    int rc = begin_call(inst, I);
    if (rc) return rc;
    const char *why = "";
    if ((rc = weighted_validate(p, l, &why))) { I->err = why; return rc; }
    kind = poisson_norm_kind(p->kind);
    return direct_instance_check(I, kind, l,
        "a weighted solve is solved by SC_METHOD_AUTO and SC_METHOD_FFT only (conjugate gradients preconditioned by the direct solve)",
        "a weighted solve with SC_FLAG_FFT_FP64: at most 4096 unknowns per axis");
}

// This family's operator: A - W on the work planes, W = the weights copied onto S.w.
struct WeightedOperator final : PcgOperator {
    Instance *I;
    const float *const *all_w;
    float plam;
    std::vector<const float *> dw;
    int kept = 0;
    double wsum = 0.0;
    WeightedOperator(Instance *I_, const float *const *w, float plam_) : PcgOperator(2), I(I_), all_w(w), plam(plam_) {}
    void begin(int i0, int m) override { dw.assign(all_w + i0, all_w + i0 + m); kept = 0; wsum = 0.0; }
    void stats(const PoissonGeo &g, const PcgGeo &wg, int m, double *d_stats, hipStream_t s) override
    {
        launch_weighted_stats(g, wg, dj.data(), dw.data(), m, d_stats, s);
    }
    const char *judge(const PoissonGeo &g, int k, const double *st, int parts, bool no_dirichlet) override
    {
        double job_sum = 0.0;
        bool bad = false, empty = false;
        for (int c = 0; c < g.C; ++c) {
            const double *plane = st + (size_t)c * PCG_PARTS * 2;
            const double sum = stat_sum(plane, parts, 0);
            bad = bad || stat_sum(plane, parts, 1) != 0.0;
            empty = empty || !(sum > 0.0);
            job_sum += sum;
        }
        if (bad || !std::isfinite(job_sum)) return "a weight is negative or not finite";
        if (no_dirichlet && empty) return "no data weight and no Dirichlet line";
        dw[kept++] = dw[k];
        wsum += job_sum;
        return nullptr;
    }
    float precond_constant(const PoissonGeo &g, const PcgGeo &wg, int mv) override
    {
        const double n_unknowns = (double)wg.nx * (double)wg.ny * (double)(g.C * mv);
        return plam > 0.f ? plam : (float)(wsum / n_unknowns);      // (0: no weight anywhere, under Dirichlet lines -- the unscreened solve)
    }
    int setup(const PoissonGeo &g, const PcgGeo &wg, bool lap, int mv, float *R, double *bb) override
    {
        const int rc = ensure(I, I->pcg->w, sizeof(float) * (size_t)wg.stride * g.C * mv, false);
        if (rc) return rc;
        launch_weighted_setup(g, wg, lap, dj.data(), dw.data(), mv, R, (float *)I->pcg->w.p, bb, I->stream);
        return SC_OK;
    }
    void apply(const PcgGeo &wg, int planes, bool residual, const float *P, float *Q, double *parts, hipStream_t s) override
    {
        launch_weighted_op(wg, planes, residual, P, (const float *)I->pcg->w.p, Q, parts, s);
    }
};

} // namespace

extern "C" {

int sc_hip_weighted_check(const sc_weighted_params *p, const sc_poisson_layout *l)
{
    return weighted_validate(p, l, nullptr);
}

int sc_hip_weighted_device(void *inst, const sc_weighted_params *p, const sc_poisson_layout *l, sc_weighted_job *jobs, int n, bool bSync)
{
    Instance *I;
    int kind, rc = weighted_begin(inst, p, l, I, kind);
    if (rc) return rc;
    FloatJobs v;
    const int worst = float_intake(I, kind, FLOAT_DATA | FLOAT_WEIGHT, jobs, n, [](const sc_weighted_job &j) {
        return FloatArrays{ j.gx, j.gy, j.lap, j.data, j.weight, j.boundary, j.out }; }, v);
    if (v.rcs.empty()) return worst;
    I->info.ms_h2d = I->info.ms_d2h = 0.f;
    WeightedOperator op(I, v.w.data(), p->precond_lambda);
    rc = pcg_run(I, PcgCall{ kind, p->tol, p->max_iters, 200 }, l, op, v.dj.data(), v.rcs.data(), (int)v.rcs.size(), bSync);
    return worse(worst, rc);
}

int sc_hip_weighted(void *inst, const sc_weighted_params *p, const sc_poisson_layout *l, const float *gx, const float *gy,
                    const float *lap, const float *data, const float *weight, const float *boundary, float *out)
{
    Instance *I;
    int kind, rc = weighted_begin(inst, p, l, I, kind);
    if (rc) return rc;
    const FloatArrays a{ gx, gy, lap, data, weight, boundary, out };
    const char *why = "";
    if ((rc = float_job_validate(kind, FLOAT_DATA | FLOAT_WEIGHT, a, &why))) { I->err = why; return rc; }
    FloatStaged s;
    if ((rc = float_stage(I, l, kind, FLOAT_DATA | FLOAT_WEIGHT, a, s))) return rc;
    int job_rc = SC_ERR_HIP, *const job_rcs[1] = { &job_rc };
    WeightedOperator op(I, &s.d_w, p->precond_lambda);
    rc = pcg_run(I, PcgCall{ kind, p->tol, p->max_iters, 200 }, l, op, &s.job, job_rcs, 1, true);
    if (rc != SC_OK && rc != SC_ERR_NOT_CONVERGED) return rc;
    const float t[4] = { 0.f, I->info.ms_solve, 0.f, I->info.ms_call };     // (one solve stage: pcg_run times the call whole)
    return poisson_download(I, l, s.job.out, out, t, rc);
}

} // extern "C"
