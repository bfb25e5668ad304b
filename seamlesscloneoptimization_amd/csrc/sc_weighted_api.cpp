// sc_weighted_api.cpp -- the weighted solve on float32 images (sc_hip_weighted_check, sc_hip_weighted_device, sc_hip_weighted):
//     minimise sum w (u - d)^2 + sum |grad u - g|^2,   i.e.   (A - W) u = div g - W d,   W = diag(w), w >= 0,
// A the 5-point operator of sc_hip_poisson under every border kind (a Dirichlet frame, SC_POISSON_NEUMANN, SC_POISSON_FREE_*,
// SC_POISSON_PERIODIC_*).
//
// A call: the float32 families' front end (sc_poisson_api.cpp: validation, job intake or host staging, run_chunks) -> per chunk of at
// most SC_POISSON_MAX_PLANES planes
//   1. the weights' statistics (one launch, one host read -- the call's one mandatory wait): per plane the sum of w and the number of
//      weights that are negative or not finite.  A job with such a weight, or -- without any Dirichlet line -- with a channel of zero
//      weight, gets SC_ERR_BAD_ARG and leaves the chunk; lambda-bar = precond_lambda, or the mean of w over the unknowns that remain.
//   2. set-up: b = lap - w d less the neighbouring Dirichlet values, and w itself, onto compact work planes that hold the unknowns only
//      (from here on every vector is homogeneous on the Dirichlet lines).
//   3. u0 = M^-1 b, r = b - (A - W) u0, z = M^-1 r, p = z;  M = A - lambda-bar through direct_jobs_solve in its Laplacian form on the work
//      planes: jobs without data term and without boundary (both mean zero there), under a PoissonGeo that addresses the planes' rows by
//      pixel coordinates.  A frame on all four sides takes the same road, both axes of kind 0.
//   4. the iteration (sc_weighted.hip): q = (A - W) p | u += alpha p, r -= alpha q | z = M^-1 r | r . z | p = z + beta p -- four launches
//      of this file's and the preconditioner's three or five, nothing read by the host but the stop rule's norms, SC_WEIGHTED_POLL
//      iterations late.
//   5. u and the Dirichlet lines of boundary into the jobs' out.
// The iteration (pcg_chunk, pcg_run) is shared with the WLS call (sc_wls_api.cpp): a family describes its operator to it as a PcgOperator
// (sc_instance.h) -- statistics and what they refuse, the preconditioner's constant, set-up, a factor on the start, operator application; WeightedOperator below
// is this family's, and steps 1 to 5 are the launches it has always made, in the same order.
#include "sc_instance.h"
#include <algorithm>
#include <cmath>
#include <vector>

using namespace sc;

namespace {

constexpr int W_LAG = WeightedState::LAG, W_RING = WeightedState::RING;

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

struct ChunkResult { int iters = 0; bool converged = true; double rel = 0.0; };

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
    void stats(const PoissonGeo &g, const WeightedGeo &wg, int m, double *d_stats, hipStream_t s) override
    {
        launch_weighted_stats(g, wg, dj.data(), dw.data(), m, d_stats, s);
    }
    const char *judge(const PoissonGeo &g, int k, const double *st, int parts, bool no_dirichlet) override
    {
        double job_sum = 0.0;
        bool bad = false, empty = false;
        for (int c = 0; c < g.C; ++c) {
            const double *plane = st + (size_t)c * WEIGHTED_PARTS * 2;
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
    float precond_constant(const PoissonGeo &g, const WeightedGeo &wg, int mv) override
    {
        const double n_unknowns = (double)wg.nx * (double)wg.ny * (double)(g.C * mv);
        return plam > 0.f ? plam : (float)(wsum / n_unknowns);      // (0: no weight anywhere, under Dirichlet lines -- the unscreened solve)
    }
    int setup(const PoissonGeo &g, const WeightedGeo &wg, bool lap, int mv, float *R, double *bb) override
    {
        const int rc = ensure(I, I->wt.w, sizeof(float) * (size_t)wg.stride * g.C * mv, false);
        if (rc) return rc;
        launch_weighted_setup(g, wg, lap, dj.data(), dw.data(), mv, R, (float *)I->wt.w.p, bb, I->stream);
        return SC_OK;
    }
    void apply(const WeightedGeo &wg, int planes, bool residual, const float *P, float *Q, double *parts, hipStream_t s) override
    {
        launch_weighted_op(wg, planes, residual, P, (const float *)I->wt.w.p, Q, parts, s);
    }
};

} // namespace

namespace sc {

// One chunk of m same-size jobs.  Jobs that their family's statistics refuse get their code here and take no further part; the rest
// share one iteration and one code (the return value: SC_OK or SC_ERR_NOT_CONVERGED, or an error that ends the call).
static int pcg_chunk(Instance *I, const PcgCall &call, const PoissonGeo &g, PcgOperator &op, int *const *rcs, int m, ChunkResult &res, int &job_errors)
{
    const MixedGeo mg = poisson_mixed_geo(poisson_free_sides(call.kind), g.W, g.H, poisson_periodic(call.kind));
    const WeightedGeo wg = weighted_geo(mg);
    const bool lap = poisson_base(call.kind) == SC_POISSON_LAPLACIAN, no_dirichlet = poisson_no_dirichlet(call.kind);
    const bool fp64 = (I->opts.flags & SC_FLAG_FFT_FP64) != 0;
    const int nop = weighted_op_parts(wg), nstat = op.nstat;
    WeightedState &S = I->wt;
    hipStream_t s = I->stream;
    int rc;
    for (hipEvent_t &e : S.ev)
        if (!e) SC_HIP(I, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    // the partial sums: statistics (nstat per part) | bb | pq | rr | rz[0] | rz[1] | rr_tot
    const size_t all_planes = (size_t)g.C * m, per = all_planes * WEIGHTED_PARTS;
    if ((rc = ensure(I, S.red, sizeof(double) * (per * (nstat + 5) + all_planes), false))) return rc;
    if ((rc = ensure_pinned(I, S.h_red, sizeof(double) * (per * nstat + per + all_planes * W_RING)))) return rc;
    double *d_stats = (double *)S.red.p, *d_bb = d_stats + nstat * per, *d_pq = d_bb + per, *d_rr = d_pq + per;
    double *d_rz[2] = { d_rr + per, d_rr + 2 * per }, *d_tot = d_rr + 3 * per;
    double *h_stats = (double *)S.h_red.p, *h_bb = h_stats + nstat * per, *h_tot = h_bb + per;

    // 1. the statistics
    op.stats(g, wg, m, d_stats, s);
    SC_HIP(I, hipGetLastError());
    SC_HIP(I, hipMemcpyAsync(h_stats, d_stats, sizeof(double) * nstat * per, hipMemcpyDeviceToHost, s));
    SC_HIP(I, hipStreamSynchronize(s));
    std::vector<int *> live;       // the codes of the jobs that stay, their arrays moved to the front
    for (int k = 0; k < m; ++k) {
        const char *why = op.judge(g, k, h_stats + (size_t)k * g.C * WEIGHTED_PARTS * nstat, nop, no_dirichlet);
        if (why) {
            *rcs[k] = SC_ERR_BAD_ARG;
            if (!job_errors++) I->err = why;
        } else {
            op.dj[live.size()] = op.dj[k];
            live.push_back(rcs[k]);
        }
    }
    const int mv = (int)live.size(), planes = g.C * mv;
    res = ChunkResult();
    if (!mv) return SC_OK;
    const float lam = op.precond_constant(g, wg, mv);

    // 2. the work planes
    const size_t plane_bytes = sizeof(float) * (size_t)wg.stride * planes;
    for (DevBuf *b : { &S.u, &S.r, &S.p, &S.q })
        if ((rc = ensure(I, *b, plane_bytes, false))) return rc;
    float *U = (float *)S.u.p, *R = (float *)S.r.p, *P = (float *)S.p.p, *Q = (float *)S.q.p, *Z = Q;
    if ((rc = op.setup(g, wg, lap, mv, R, d_bb))) return rc;
    SC_HIP(I, hipGetLastError());
    SC_HIP(I, hipMemcpyAsync(h_bb, d_bb, sizeof(double) * (size_t)planes * WEIGHTED_PARTS, hipMemcpyDeviceToHost, s));
    // 3. the preconditioner: (A - lam) out = in on the work planes.  Pixel (x, y) of a plane is its unknown (x - x0, y - y0): the
    // pointers are moved back by the first unknown's offset, and only unknowns are ever addressed (no boundary: no Dirichlet line is
    // read or written)
    const PoissonGeo pg{ g.W, g.H, g.C, 1, (long long)wg.nx, wg.stride };
    const long long shift = (long long)wg.x0 + (long long)wg.y0 * wg.nx;
    std::vector<PoissonJobDev> pj(mv);
    auto precond = [&](const float *in, float *out) -> int {
        for (int k = 0; k < mv; ++k) {
            const long long o = (long long)k * g.C * wg.stride - shift;
            pj[k] = PoissonJobDev{ nullptr, nullptr, in + o, nullptr, out + o };
        }
        return direct_jobs_solve(I, pg, mg, true, pj.data(), mv, fp64, lam);
    };
    // the stop rule's mailbox: iteration k's norms into slot k % W_RING, event k % W_RING behind them
    auto post_norms = [&](int k) -> int {
        SC_HIP(I, hipMemcpyAsync(h_tot + (size_t)(k % W_RING) * planes, d_tot, sizeof(double) * planes, hipMemcpyDeviceToHost, s));
        SC_HIP(I, hipEventRecord(S.ev[k % W_RING], s));
        return SC_OK;
    };
    const double tol = call.tol > 0.f ? (double)call.tol : 1e-5;
    const int max_iters = call.max_iters > 0 ? call.max_iters : call.default_iters;
    std::vector<double> bb(planes, 0.0);
    bool have_bb = false;
    // the worst plane's ||r|| / ||b|| of iteration k (waits for its event)
    auto read_norms = [&](int k, double &worst) -> int {
        SC_HIP(I, hipEventSynchronize(S.ev[k % W_RING]));
        if (!have_bb) {          // (copied in front of every slot)
            for (int p = 0; p < planes; ++p)
                for (int i = 0; i < nop; ++i) bb[p] += h_bb[(size_t)p * WEIGHTED_PARTS + i];
            have_bb = true;
        }
        worst = 0.0;
        const double *t = h_tot + (size_t)(k % W_RING) * planes;
        for (int p = 0; p < planes; ++p) {
            const double rel = bb[p] > 0.0 ? std::sqrt(t[p] / bb[p]) : (t[p] > 0.0 ? INFINITY : 0.0);
            worst = rel > worst || rel != rel ? rel : worst;
        }
        return SC_OK;
    };
    if ((rc = precond(R, U))) return rc;                                           // u0 = M^-1 b
    op.scale_start(wg, planes, U, s);
    op.apply(wg, planes, true, U, R, d_rr, s);                                     // r = b - (A - W) u0
    if ((rc = precond(R, Z))) return rc;
    launch_weighted_dot(wg, planes, R, Z, d_rz[0], d_rr, nop, d_tot, s);
    if ((rc = post_norms(0))) return rc;
    launch_weighted_dir(wg, planes, P, Z, d_rz[0], nullptr, s);                    // p = z
    SC_HIP(I, hipGetLastError());

    // 4. the iteration
    int iters = 0;
    bool seen = false;
    double worst = 0.0;
    for (int k = 1; k <= max_iters; ++k) {
        if (k - W_LAG >= 0) {
            if ((rc = read_norms(k - W_LAG, worst))) return rc;
            if (worst <= tol) { seen = true; break; }
            if (worst != worst) break;                                             // NaN: nothing more to gain
        }
        op.apply(wg, planes, false, P, Q, d_pq, s);
        launch_weighted_update(wg, planes, U, R, P, Q, d_rz[(k - 1) & 1], d_pq, d_rr, s);
        if ((rc = precond(R, Z))) return rc;
        launch_weighted_dot(wg, planes, R, Z, d_rz[k & 1], d_rr, wg.eparts, d_tot, s);
        if ((rc = post_norms(k))) return rc;
        launch_weighted_dir(wg, planes, P, Z, d_rz[k & 1], d_rz[(k - 1) & 1], s);
        SC_HIP(I, hipGetLastError());
        iters = k;
    }
    // the norms not yet read: an iteration at or behind the one that was seen may have met tol as well; the last one is reported
    for (int k = std::max(0, iters - W_LAG + 1); k <= iters; ++k) {
        if ((rc = read_norms(k, worst))) return rc;
        if (worst <= tol) seen = true;
    }
    res.iters = iters;
    res.rel = worst;
    res.converged = seen;

    // 5. the output
    launch_weighted_out(g, wg, op.dj.data(), mv, U, s);
    SC_HIP(I, hipGetLastError());
    const int code = res.converged ? SC_OK : SC_ERR_NOT_CONVERGED;
    for (int k = 0; k < mv; ++k) *live[k] = code;
    return code;
}

int pcg_run(Instance *I, const PcgCall &call, const sc_poisson_layout *l, PcgOperator &op, const PoissonJobDev *jobs, int *const *rcs, int nv, bool timed)
{
    CallScope scope{ I };
    const PoissonGeo g{ l->cols, l->rows, l->channels, l->col_stride, l->row_stride, l->channel_stride };
    Geo geo{ 0, 0, g.W, g.H, 0, 0 };
    fill_info_geo(I, geo);
    I->stage_marks = false;          // (direct_jobs_solve's marks: a call of many solves records none)
    if (timed) SC_HIP(I, hipEventRecord(I->ev[0], I->stream));
    int job_errors = 0, sweeps = 0;
    bool converged = true;
    double rel = 0.0;
    int worst = run_chunks(I, g.C, rcs, nv, [&](int i0, int m) {
        ChunkResult res;
        op.dj.assign(jobs + i0, jobs + i0 + m);
        op.begin(i0, m);
        const int rc = pcg_chunk(I, call, g, op, rcs + i0, m, res, job_errors);
        sweeps = std::max(sweeps, res.iters);
        converged = converged && res.converged;
        rel = std::max(rel, res.rel);
        return rc;
    });
    if (worst != SC_OK && worst != SC_ERR_NOT_CONVERGED) return worst;
    if (job_errors) worst = worse(worst, SC_ERR_BAD_ARG);
    I->info.method = SC_METHOD_FFT;
    I->info.sweeps = sweeps;
    I->info.converged = converged ? 1 : 0;
    I->info.rel_residual = rel;
    I->info.sweep_launches = sweeps;
    I->info.ms_mask = I->info.ms_pre = I->info.ms_post = 0.f;
    I->info.ms_solve = I->info.ms_device_total = I->info.ms_call = 0.f;
    if (timed) {
        SC_HIP(I, hipEventRecord(I->ev[7], I->stream));
        SC_HIP(I, hipStreamSynchronize(I->stream));
        I->info.ms_solve = I->info.ms_device_total = I->info.ms_call = ev_ms(I->ev[0], I->ev[7]);
    }
    return worst;
}

} // namespace sc

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
