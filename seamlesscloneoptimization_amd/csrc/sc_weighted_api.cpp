// sc_weighted_api.cpp -- the weighted solve on float32 images (sc_hip_weighted_check, sc_hip_weighted_device, sc_hip_weighted):
//     minimise sum w (u - d)^2 + sum |grad u - g|^2,   i.e.   (A - W) u = div g - W d,   W = diag(w), w >= 0,
// A the 5-point operator of sc_hip_poisson under every border kind (a Dirichlet frame, SC_POISSON_NEUMANN, SC_POISSON_FREE_*,
// SC_POISSON_PERIODIC_*).  A call: the conjugate-gradient families' entry code (sc_pcg.h: pcg_begin, then pcg_host_call or
// pcg_device_call around the float32 families' front end and pcg_run) with this file's validation and its WeightedOperator, which
// reads the chunk's jobs and their weights where the driver keeps them (PcgOperator::dj, ds):
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

constexpr int CARRIES = FLOAT_DATA | FLOAT_WEIGHT;
constexpr const char *METHOD_WHY = "a weighted solve is solved by SC_METHOD_AUTO and SC_METHOD_FFT only (conjugate gradients preconditioned by the direct solve)";
constexpr const char *FP64_WHY = "a weighted solve with SC_FLAG_FFT_FP64: at most 4096 unknowns per axis";

// This family's operator: A - W on the work planes, W = the weights copied onto S.w.
struct WeightedOperator final : PcgOperator {
    Instance *I;
    float plam;
    double wsum = 0.0;
    WeightedOperator(Instance *I_, float plam_) : PcgOperator(2), I(I_), plam(plam_) {}
    void begin() override { wsum = 0.0; }
    void stats(const PoissonGeo &g, const PcgGeo &wg, int m, double *d_stats, hipStream_t s) override
    {
        launch_weighted_stats(g, wg, dj.data(), ds.data(), m, d_stats, s);
    }
    const char *judge(const PoissonGeo &g, int k, const double *st, int parts, bool no_dirichlet) override
    {
        double job_sum;
        const char *why = judge_weights(g, st, parts, no_dirichlet, nullptr, job_sum);
        if (why) return why;
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
        launch_weighted_setup(g, wg, lap, dj.data(), ds.data(), mv, R, (float *)I->pcg->w.p, bb, I->stream);
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
    int kind, rc = pcg_begin(inst, p, l, weighted_validate, METHOD_WHY, FP64_WHY, I, kind);
    if (rc) return rc;
    WeightedOperator op(I, p->precond_lambda);
    return pcg_device_call(I, PcgCall{ kind, p->tol, p->max_iters, 200 }, l, CARRIES, jobs, n, [](const sc_weighted_job &j) {
        return FloatArrays{ j.gx, j.gy, j.lap, j.data, j.weight, j.boundary, j.out }; }, op, bSync);
}

int sc_hip_weighted(void *inst, const sc_weighted_params *p, const sc_poisson_layout *l, const float *gx, const float *gy,
                    const float *lap, const float *data, const float *weight, const float *boundary, float *out)
{
    Instance *I;
    int kind, rc = pcg_begin(inst, p, l, weighted_validate, METHOD_WHY, FP64_WHY, I, kind);
    if (rc) return rc;
    WeightedOperator op(I, p->precond_lambda);
    return pcg_host_call(I, PcgCall{ kind, p->tol, p->max_iters, 200 }, l, CARRIES, FloatArrays{ gx, gy, lap, data, weight, boundary, out }, op);
}

} // extern "C"
