// sc_bounded_api.cpp -- bounded solves on float32 images (sc_hip_bounded_check, sc_hip_bounded_device, sc_hip_bounded, sc_hip_bounded_trace):
// the region call's problem (sc_region_api.cpp) under the box constraint lower <= u <= upper at the UNKNOWN pixels, by the primal-dual
// active set method on the device.  The entry code is the region call's (sc_pcg.h: pcg_begin, pcg_host_call, pcg_device_call; the front
// end with FLOAT_STATE, and FLOAT_LOWER / FLOAT_UPPER when the jobs carry bound arrays), the iteration the shared conjugate gradients in
// their three steps (pcg_chunk_begin / pcg_chunk_iterate / pcg_chunk_finish), the operator the region call's with the set beside it
// (BoundedOperator).  Per chunk (bounded_chunk, a PcgChunkFn as robust_chunk is):
//   round 0     the region call's chunk: statistics, judgement (bound arrays are judged here as well: k_bounded_stats rides in front of
//               the statistics' one host read), set-up, a cold solve.  Without any finite bound that is all: the region call's output.
//   the mark    k_bounded_mark behind every solve: the next set and how many pixels changed -- one host read.  None: the end.
//   round k     k_bounded_setup under the new set (the iterate takes the bound where a pixel is or was active), its sums for w-bar -- a
//               second host read --, then a warm solve: r = b - L u, z = M^-1 r, p = z.
//   the end     no pixel changed (converged), or max_rounds solves have run; the output is taken under the set of the last solve.
#include "sc_pcg.h"
#include <algorithm>
#include <cmath>
#include <vector>

using namespace sc;

namespace {

int bounded_validate(const sc_bounded_params *p, const sc_poisson_layout *l, const char **why)
{
    const char *own = !p ? nullptr : !std::isfinite(p->tol) ? "tol must be finite"
                    : !std::isfinite(p->precond_lambda) ? "precond_lambda must be finite"
                    : !std::isfinite(p->precond_smooth) ? "precond_smooth must be finite"
                    : p->lower != p->lower || p->upper != p->upper ? "lower and upper must not be NaN"
                    : p->lower > p->upper ? "lower must not exceed upper" : nullptr;
    return family_validate(p ? &p->kind : nullptr, l, own,
                           "a bounded solve is preconditioned by a direct solve: at most 8192 unknowns (pixels - 2) per side", why);
}

constexpr const char *METHOD_WHY = "a bounded solve is solved by SC_METHOD_AUTO and SC_METHOD_FFT only (conjugate gradients preconditioned by the direct solve)";
constexpr const char *FP64_WHY = "a bounded solve with SC_FLAG_FFT_FP64: at most 4096 unknowns per axis";

int carries_of(bool weight, bool links, bool lower, bool upper)
{
    return FLOAT_DATA | FLOAT_STATE | (weight ? FLOAT_WEIGHT : 0) | (links ? FLOAT_SMOOTH : 0) | (lower ? FLOAT_LOWER : 0) | (upper ? FLOAT_UPPER : 0);
}

PcgCall bounded_call(int kind, const sc_bounded_params *p) { return PcgCall{ kind, p->tol, p->max_iters, 400 }; }

// The region operator with the set of the current round: round 0's system from the region call's launches, later rounds' from
// k_bounded_setup.  arrays: the jobs carry a bound array; bounded: the call has a finite bound anywhere.
struct BoundedOperator final : RegionOperator {
    const BoundScalars bs;
    const int max_rounds;
    const bool arrays, bounded;
    const float *set = nullptr;                // the set plane of the last solve (out)
    BoundedOperator(Instance *I_, bool weight, bool links_, bool lower, bool upper, const sc_bounded_params *p)
        : RegionOperator(I_, weight, links_, p->precond_lambda, p->precond_smooth, BOUNDED_SUMS), bs{ p->lower, p->upper },
          max_rounds(p->max_rounds > 0 ? p->max_rounds : 30), arrays(lower || upper),
          bounded(lower || upper || std::isfinite(p->lower) || std::isfinite(p->upper)) {}
    // the pinned block for the judgement of bound arrays, before the call runs (stats cannot fail)
    int prepare()
    {
        if (!arrays) return SC_OK;
        PcgState &S = *I->pcg;
        const size_t bytes = sizeof(double) * (size_t)SC_POISSON_MAX_PLANES * PCG_PARTS;
        const int rc = ensure(I, S.bad, bytes, false);
        return rc ? rc : ensure_pinned(I, S.h_bad, bytes);
    }
    void stats(const PoissonGeo &g, const PcgGeo &wg, int m, double *d_stats, hipStream_t s) override
    {
        RegionOperator::stats(g, wg, m, d_stats, s);
        if (!arrays) return;
        PcgState &S = *I->pcg;          // (the driver's wait for the statistics covers this copy: it follows on the same stream)
        launch_bounded_stats(g, wg, bs, dj.data(), ds.data(), m, (double *)S.bad.p, s);
        (void)hipMemcpyAsync(S.h_bad.p, S.bad.p, sizeof(double) * (size_t)g.C * m * PCG_PARTS, hipMemcpyDeviceToHost, s);
    }
    const char *judge(const PoissonGeo &g, int k, const double *st, int parts, bool no_dirichlet) override
    {
        // (the bounds first: a job the region call keeps adds to the chunk's sums)
        if (arrays) {
            const double *h = (const double *)I->pcg->h_bad.p + (size_t)k * g.C * PCG_PARTS;
            double n = 0.0;
            for (int c = 0; c < g.C; ++c)
                for (int i = 0; i < parts; ++i) n += h[(size_t)c * PCG_PARTS + i];
            if (n != 0.0) return "a bound is NaN or lower exceeds upper at an UNKNOWN pixel";
        }
        return RegionOperator::judge(g, k, st, parts, no_dirichlet);
    }
    void out(const PoissonGeo &g, const PcgGeo &wg, int mv, const float *U, hipStream_t s) override
    {
        if (set) launch_bounded_out(g, wg, bs, dj.data(), ds.data(), mv, U, set, s);
        else RegionOperator::out(g, wg, mv, U, s);
    }
};

// the chunk's round sums after one launch: one host read, the fields' totals over every plane's parts in one fixed order
int read_sums(PcgChunk &c, double (&totals)[BOUNDED_SUMS])
{
    Instance *I = c.I;
    const size_t parts = (size_t)c.planes * PCG_PARTS;
    SC_HIP(I, hipGetLastError());
    SC_HIP(I, hipMemcpyAsync(c.h_round, c.d_round, sizeof(double) * parts * BOUNDED_SUMS, hipMemcpyDeviceToHost, I->stream));
    SC_HIP(I, hipStreamSynchronize(I->stream));
    for (double &t : totals) t = 0.0;
    for (int p = 0; p < c.planes; ++p)
        for (int i = 0; i < c.nop; ++i)
            for (int f = 0; f < BOUNDED_SUMS; ++f) totals[f] += c.h_round[((size_t)p * PCG_PARTS + i) * BOUNDED_SUMS + f];
    return SC_OK;
}

// One chunk of a bounded call.  res: the total of the inner iterations, whether the set stopped changing, the last inner solve's
// residual.  The code: SC_ERR_NOT_CONVERGED when an inner solve ran out of max_iters (the rounds go on from its last iterate), else
// SC_OK -- running out of rounds included.
int bounded_chunk(Instance *I, const PcgCall &call, const PoissonGeo &g, PcgOperator &op_, int *const *rcs, int m, PcgChunkResult &res, int &job_errors)
{
    BoundedOperator &op = static_cast<BoundedOperator &>(op_);
    PcgState &S = *I->pcg;
    for (std::vector<int> *t : { &S.trace_changed, &S.trace_active, &S.trace_bounded_iters }) t->clear();
    op.set = nullptr;
    PcgChunk c;
    int rc = pcg_chunk_begin(I, call, g, op, rcs, m, job_errors, c);
    res = PcgChunkResult();
    if (rc || !c.mv) return rc;
    const bool lap = poisson_base(call.kind) == SC_POISSON_LAPLACIAN;
    if ((rc = op.setup(g, c.wg, lap, c.mv, c.R, c.d_bb))) return rc;
    SC_HIP(I, hipGetLastError());
    PcgChunkResult one;
    if ((rc = pcg_chunk_iterate(c, op, false, one))) return rc;
    int total = one.iters;
    bool inner = one.converged, met = !op.bounded;
    if (!op.bounded) {          // no finite bound anywhere: the region call's chunk
        S.trace_changed.push_back(0);
        S.trace_active.push_back(0);
        S.trace_bounded_iters.push_back(one.iters);
    } else {
        const size_t plane_floats = (size_t)c.wg.stride * c.planes;
        if ((rc = ensure(I, S.act, sizeof(float) * 2 * plane_floats, false))) return rc;
        float *cur = (float *)S.act.p, *next = cur + plane_floats;
        SC_HIP(I, hipMemsetAsync(cur, 0, sizeof(float) * plane_floats, I->stream));      // round 0's set: every pixel free
        for (int k = 0;; ++k) {
            double t[BOUNDED_SUMS];
            launch_bounded_mark(g, c.wg, lap, op.bs, op.dj.data(), op.ds.data(), c.mv, c.U, cur, next, c.d_round, I->stream);
            if ((rc = read_sums(c, t))) return rc;          // changed | active
            S.trace_changed.push_back((int)t[0]);
            S.trace_active.push_back((int)t[1]);
            S.trace_bounded_iters.push_back(one.iters);
            met = t[0] == 0.0;
            if (met || k + 1 >= op.max_rounds) break;
            launch_bounded_setup(g, c.wg, lap, op.bs, op.dj.data(), op.ds.data(), c.mv, next, cur, c.U, c.R, (float *)S.e.p, (float *)S.s.p,
                                 (float *)S.dg.p, c.d_bb, c.d_round, I->stream);
            if ((rc = read_sums(c, t))) return rc;          // w over the free pixels | free - held links | free pixels: w-bar's
            op.wsum = t[0]; op.uksum = t[1]; op.unknowns = t[2];
            std::swap(cur, next);
            if ((rc = pcg_chunk_iterate(c, op, true, one))) return rc;
            total += one.iters;
            inner = inner && one.converged;
        }
        op.set = cur;
    }
    res.iters = total;
    res.converged = met;
    res.rel = one.rel;
    return pcg_chunk_finish(c, op, inner ? SC_OK : SC_ERR_NOT_CONVERGED);
}

} // namespace

extern "C" {

int sc_hip_bounded_check(const sc_bounded_params *p, const sc_poisson_layout *l)
{
    return bounded_validate(p, l, nullptr);
}

int sc_hip_bounded_device(void *inst, const sc_bounded_params *p, const sc_poisson_layout *l, sc_bounded_job *jobs, int n, bool bSync)
{
    Instance *I;
    int kind, rc = pcg_begin(inst, p, l, bounded_validate, METHOD_WHY, FP64_WHY, I, kind);
    if (rc) return rc;
    // the data term, the link arrays and either bound array: all jobs or none, as the first job has them; a job that differs is refused
    const bool weight = jobs && n > 0 && jobs[0].weight, links = jobs && n > 0 && (jobs[0].smooth_x || jobs[0].smooth_y);
    const bool lower = jobs && n > 0 && jobs[0].lower, upper = jobs && n > 0 && jobs[0].upper;
    BoundedOperator op(I, weight, links, lower, upper, p);
    if ((rc = op.prepare())) return rc;
    return pcg_device_call(I, bounded_call(kind, p), l, carries_of(weight, links, lower, upper), jobs, n, [=](const sc_bounded_job &j) {
        const bool stray = (!weight && j.weight) || (!links && (j.smooth_x || j.smooth_y));      // (refused through its data pointer)
        FloatArrays a{ j.gx, j.gy, j.lap, stray ? nullptr : j.data, j.weight, j.boundary, j.out, j.smooth_x, j.smooth_y, j.state };
        a.lower = j.lower;
        a.upper = j.upper;
        if ((!lower && j.lower) || (!upper && j.upper)) a.refuse = "a bound array where the call's first job has none";
        return a; }, op, bSync, bounded_chunk);
}

int sc_hip_bounded(void *inst, const sc_bounded_params *p, const sc_poisson_layout *l, const float *gx, const float *gy, const float *lap,
                   const float *data, const float *state, const float *weight, const float *smooth_x, const float *smooth_y,
                   const float *boundary, const float *lower, const float *upper, float *out)
{
    Instance *I;
    int kind, rc = pcg_begin(inst, p, l, bounded_validate, METHOD_WHY, FP64_WHY, I, kind);
    if (rc) return rc;
    if (!smooth_x != !smooth_y) { I->err = "smooth_x and smooth_y go together (both NULL: every link 1)"; return SC_ERR_BAD_ARG; }
    const bool has_w = weight != nullptr, links = smooth_x != nullptr;
    BoundedOperator op(I, has_w, links, lower != nullptr, upper != nullptr, p);
    if ((rc = op.prepare())) return rc;
    FloatArrays a{ gx, gy, lap, data, weight, boundary, out, smooth_x, smooth_y, state };
    a.lower = lower;
    a.upper = upper;
    return pcg_host_call(I, bounded_call(kind, p), l, carries_of(has_w, links, lower != nullptr, upper != nullptr), a, op, bounded_chunk);
}

int sc_hip_bounded_trace(void *inst, int *changed, int *active, int *iters, int cap)
{
    Instance *I = get(inst);
    if (!I) return 0;
    const PcgState &S = *I->pcg;
    const int n = (int)S.trace_changed.size();
    for (int k = 0; k < std::min(n, cap); ++k) {
        if (changed) changed[k] = S.trace_changed[k];
        if (active) active[k] = S.trace_active[k];
        if (iters) iters[k] = S.trace_bounded_iters[k];
    }
    return n;
}

} // extern "C"
