// sc_pcg.cpp -- the preconditioned conjugate gradients of the weighted, the WLS and the robust call (sc_pcg.h): a family's entry points
// run pcg_begin and then pcg_host_call or pcg_device_call, which hand pcg_run the validated jobs, their side arrays (SideArrays: one
// record per job) and the family's PcgOperator.  Per chunk of at most SC_POISSON_MAX_PLANES planes (run_chunks) the driver gives the
// operator the chunk's jobs and records (dj, ds) and keeps the two in step: when a job leaves, both move up in one statement.
//   1. the family's statistics (one launch, one host read -- the call's one mandatory wait); a job they refuse gets SC_ERR_BAD_ARG and
//      leaves the chunk, the rest give the preconditioner's constant lam.
//   2. set-up: b and the family's coefficients onto compact work planes that hold the unknowns only (from here on every vector is
//      homogeneous on the Dirichlet lines).
//   3. u0 = M^-1 b (times the family's factor), r = b - L u0, z = M^-1 r, p = z;  M = A - lam through direct_jobs_solve in its Laplacian
//      form on the work planes: jobs without data term and without boundary (both mean zero there), under a PoissonGeo that addresses
//      the planes' rows by pixel coordinates.  A frame on all four sides takes the same road, both axes of kind 0.  (PcgOperator::precond;
//      the volume family puts its own M^-1 there: a transform along the frames around the same direct solve.)
//   4. the iteration: q = L p | u += alpha p, r -= alpha q | z = M^-1 r | r . z | p = z + beta p -- four launches of sc_pcg.hip's and the
//      family's and the preconditioner's three or five, nothing read by the host but the stop rule's norms, SC_WEIGHTED_POLL iterations
//      late.
//   5. u and the Dirichlet lines of boundary into the jobs' out.
// Step 1 and the buffers are pcg_chunk_begin, steps 3 and 4 pcg_chunk_iterate -- which can also start from a U already on the work
// plane: no u0, r = b - L u at once -- and step 5 pcg_chunk_finish; the weighted and the WLS call run them once each around their set-up
// (pcg_chunk), the robust call (sc_robust_api.cpp) runs one iterate per reweighting round between one begin and one finish.
#include "sc_pcg.h"
#include <algorithm>
#include <cmath>
#include <vector>

namespace sc {

namespace {

constexpr int W_LAG = PcgState::LAG, W_RING = PcgState::RING;

} // namespace

// One chunk of m same-size jobs.  Jobs that their family's statistics refuse get their code here and take no further part; the rest
// share every solve and one code.
void PcgOperator::out(const PoissonGeo &g, const PcgGeo &wg, int mv, const float *U, hipStream_t s) { launch_pcg_out(g, wg, dj.data(), mv, U, s); }

// (A - lam) out = in on the work planes.  Pixel (x, y) of a plane is its unknown (x - x0, y - y0): the pointers are moved back by the
// first unknown's offset, and only unknowns are ever addressed (no boundary: no Dirichlet line is read or written)
int PcgOperator::precond(const PcgChunk &c, float lam, bool fp64, const float *in, float *out)
{
    const PoissonGeo &g = c.g;
    const PcgGeo &wg = c.wg;
    const PoissonGeo pg{ g.W, g.H, g.C, 1, (long long)wg.nx, wg.stride };
    const long long shift = (long long)wg.x0 + (long long)wg.y0 * wg.nx;
    std::vector<PoissonJobDev> pj(c.mv);
    for (int k = 0; k < c.mv; ++k) {
        const long long o = (long long)k * g.C * wg.stride - shift;
        pj[k] = PoissonJobDev{ nullptr, nullptr, in + o, nullptr, out + o };
    }
    return direct_jobs_solve(c.I, pg, c.mg, true, pj.data(), c.mv, fp64, lam);
}

int pcg_chunk_begin(Instance *I, const PcgCall &call, const PoissonGeo &g, PcgOperator &op, int *const *rcs, int m, int &job_errors, PcgChunk &c)
{
    c = PcgChunk();
    c.I = I;
    c.call = call;
    c.g = g;
    c.mg = poisson_mixed_geo(poisson_free_sides(call.kind), g.W, g.H, poisson_periodic(call.kind));
    c.wg = op.work_geo(c.mg);
    const PcgGeo &wg = c.wg;
    const bool no_dirichlet = poisson_no_dirichlet(call.kind);
    const int nop = c.nop = pcg_op_parts(wg), nstat = op.nstat, nround = op.nround;
    PcgState &S = *I->pcg;
    hipStream_t s = I->stream;
    int rc;
    for (hipEvent_t &e : S.ev)
        if (!e) SC_HIP(I, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    // the partial sums: statistics (nstat per part) | bb | pq | rr | rz[0] | rz[1] | rr_tot | the family's round sums (nround per part)
    const size_t all_planes = (size_t)g.C * m, per = all_planes * PCG_PARTS;
    if ((rc = ensure(I, S.red, sizeof(double) * (per * (nstat + 5) + all_planes + per * nround), false))) return rc;
    if ((rc = ensure_pinned(I, S.h_red, sizeof(double) * (per * nstat + per + all_planes * W_RING + per * nround)))) return rc;
    double *d_stats = (double *)S.red.p, *d_rr;
    c.d_bb = d_stats + nstat * per; c.d_pq = c.d_bb + per; c.d_rr = d_rr = c.d_pq + per;
    c.d_rz[0] = d_rr + per; c.d_rz[1] = d_rr + 2 * per; c.d_tot = d_rr + 3 * per; c.d_round = c.d_tot + all_planes;
    double *h_stats = (double *)S.h_red.p;
    c.h_bb = h_stats + nstat * per; c.h_tot = c.h_bb + per; c.h_round = c.h_tot + all_planes * W_RING;

    // the statistics
    op.stats(g, wg, m, d_stats, s);
    SC_HIP(I, hipGetLastError());
    SC_HIP(I, hipMemcpyAsync(h_stats, d_stats, sizeof(double) * nstat * per, hipMemcpyDeviceToHost, s));
    SC_HIP(I, hipStreamSynchronize(s));
    for (int k = 0; k < m; ++k) {          // the jobs that stay: they and their side arrays move to the front
        const char *why = op.judge(g, k, h_stats + (size_t)k * g.C * PCG_PARTS * nstat, nop, no_dirichlet);
        if (why) {
            *rcs[k] = SC_ERR_BAD_ARG;
            if (!job_errors++) I->err = why;
        } else {
            op.dj[c.live.size()] = op.dj[k], op.ds[c.live.size()] = op.ds[k];
            c.live.push_back(rcs[k]);
        }
    }
    c.mv = (int)c.live.size();
    c.planes = g.C * c.mv;
    if (!c.mv) return SC_OK;

    // the work planes
    const size_t plane_bytes = sizeof(float) * (size_t)wg.stride * c.planes;
    for (DevBuf *b : { &S.u, &S.r, &S.p, &S.q })
        if ((rc = ensure(I, *b, plane_bytes, false))) return rc;
    c.U = (float *)S.u.p; c.R = (float *)S.r.p; c.P = (float *)S.p.p; c.Q = (float *)S.q.p;
    return SC_OK;
}

int pcg_chunk_iterate(PcgChunk &c, PcgOperator &op, bool warm, PcgChunkResult &res)
{
    Instance *I = c.I;
    const PoissonGeo &g = c.g;
    const PcgGeo &wg = c.wg;
    const PcgCall &call = c.call;
    const bool fp64 = (I->opts.flags & SC_FLAG_FFT_FP64) != 0;
    const int nop = c.nop, mv = c.mv, planes = c.planes;
    PcgState &S = *I->pcg;
    hipStream_t s = I->stream;
    float *U = c.U, *R = c.R, *P = c.P, *Q = c.Q, *Z = Q;
    double *d_bb = c.d_bb, *d_pq = c.d_pq, *d_rr = c.d_rr, *const *d_rz = c.d_rz, *d_tot = c.d_tot, *h_bb = c.h_bb, *h_tot = c.h_tot;
    int rc;
    res = PcgChunkResult();
    const float lam = op.precond_constant(g, wg, mv);
    SC_HIP(I, hipMemcpyAsync(h_bb, d_bb, sizeof(double) * (size_t)planes * PCG_PARTS, hipMemcpyDeviceToHost, s));
    auto precond = [&](const float *in, float *out) -> int { return op.precond(c, lam, fp64, in, out); };      // the family's M^-1
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
                for (int i = 0; i < nop; ++i) bb[p] += h_bb[(size_t)p * PCG_PARTS + i];
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
    if (!warm) {
        if ((rc = precond(R, U))) return rc;                                       // u0 = M^-1 b
        op.scale_start(wg, planes, U, s);
    }
    op.apply(wg, planes, true, U, R, d_rr, s);                                     // r = b - L u0
    if ((rc = precond(R, Z))) return rc;
    launch_pcg_dot(wg, planes, R, Z, d_rz[0], d_rr, nop, d_tot, s);
    if ((rc = post_norms(0))) return rc;
    launch_pcg_dir(wg, planes, P, Z, d_rz[0], nullptr, s);                    // p = z
    SC_HIP(I, hipGetLastError());

    // the iteration
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
        launch_pcg_update(wg, planes, U, R, P, Q, d_rz[(k - 1) & 1], d_pq, d_rr, s);
        if ((rc = precond(R, Z))) return rc;
        launch_pcg_dot(wg, planes, R, Z, d_rz[k & 1], d_rr, wg.eparts, d_tot, s);
        if ((rc = post_norms(k))) return rc;
        launch_pcg_dir(wg, planes, P, Z, d_rz[k & 1], d_rz[(k - 1) & 1], s);
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
    return SC_OK;
}

int pcg_chunk_finish(PcgChunk &c, PcgOperator &op, int code)
{
    Instance *I = c.I;
    op.out(c.g, c.wg, c.mv, c.U, I->stream);
    SC_HIP(I, hipGetLastError());
    for (int k = 0; k < c.mv; ++k) *c.live[k] = code;
    return code;
}

namespace {

// the weighted and the WLS call's chunk: one cold solve (the return value: SC_OK or SC_ERR_NOT_CONVERGED, or an error that ends the call)
int pcg_chunk(Instance *I, const PcgCall &call, const PoissonGeo &g, PcgOperator &op, int *const *rcs, int m, PcgChunkResult &res, int &job_errors)
{
    PcgChunk c;
    int rc = pcg_chunk_begin(I, call, g, op, rcs, m, job_errors, c);
    res = PcgChunkResult();
    if (rc || !c.mv) return rc;
    if ((rc = op.setup(g, c.wg, poisson_base(call.kind) == SC_POISSON_LAPLACIAN, c.mv, c.R, c.d_bb))) return rc;
    SC_HIP(I, hipGetLastError());
    if ((rc = pcg_chunk_iterate(c, op, false, res))) return rc;
    return pcg_chunk_finish(c, op, res.converged ? SC_OK : SC_ERR_NOT_CONVERGED);
}

} // namespace

int pcg_run(Instance *I, const PcgCall &call, const sc_poisson_layout *l, PcgOperator &op, const PoissonJobDev *jobs, const SideArrays *sides,
            int *const *rcs, int nv, bool timed, PcgChunkFn chunk)
{
    if (!chunk) chunk = pcg_chunk;
    CallScope scope{ I };
    const PoissonGeo g{ l->cols, l->rows, l->channels, l->col_stride, l->row_stride, l->channel_stride };
    Geo geo{ 0, 0, g.W, g.H, 0, 0 };
    fill_info_geo(I, geo);
    I->stage_marks = false;          // (direct_jobs_solve's marks: a call of many solves records none)
    if (timed) SC_HIP(I, hipEventRecord(I->ev[0], I->stream));
    int job_errors = 0, sweeps = 0;
    bool converged = true;
    double rel = 0.0;
    int worst = run_chunks(I, op.chunk_planes(g.C), rcs, nv, [&](int i0, int m) {
        PcgChunkResult res;
        op.dj.assign(jobs + i0, jobs + i0 + m);
        op.ds.assign(sides + i0, sides + i0 + m);
        op.begin();
        const int rc = chunk(I, call, g, op, rcs + i0, m, res, job_errors);
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

int pcg_host_call(Instance *I, const PcgCall &call, const sc_poisson_layout *l, int carries, const FloatArrays &a, PcgOperator &op, PcgChunkFn chunk)
{
    const char *why = "";
    int rc;
    if ((rc = float_job_validate(call.kind, carries, a, &why, pcg_call_span(call, l), pcg_call_tspan(call, l), call.flow_floats))) { I->err = why; return rc; }
    FloatStaged s;
    if ((rc = float_stage(I, l, call.kind, carries, a, s, call.frames, call.frame_stride, call.tframes, call.flow_floats))) return rc;
    int job_rc = SC_ERR_HIP, *const job_rcs[1] = { &job_rc };
    rc = pcg_run(I, call, l, op, &s.job, &s.side, job_rcs, 1, true, chunk);
    if (rc != SC_OK && rc != SC_ERR_NOT_CONVERGED) return rc;
    const float t[4] = { 0.f, I->info.ms_solve, 0.f, I->info.ms_call };     // (one solve stage: pcg_run times the call whole)
    return poisson_download(I, l, s.job.out, a.out, t, rc, call.frames, call.frame_stride);
}

void pcg_release(Instance *I)
{
    if (!I->pcg) return;
    PcgState &S = *I->pcg;
    for (DevBuf *b : { &S.u, &S.r, &S.p, &S.q, &S.w, &S.e, &S.s, &S.dg, &S.f, &S.dct, &S.tab, &S.lnk, &S.rho, &S.act, &S.bad, &S.red }) dev_release(*b);
    if (S.h_red.p) (void)hipHostFree(S.h_red.p);
    if (S.h_bad.p) (void)hipHostFree(S.h_bad.p);
    for (hipEvent_t e : S.ev) if (e) (void)hipEventDestroy(e);
    delete I->pcg;
}

} // namespace sc
