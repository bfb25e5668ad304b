// sc_robust_api.cpp -- robust gradient solves on float32 images (sc_hip_robust_check, sc_hip_robust_device, sc_hip_robust,
// sc_hip_robust_trace): Lp penalties on the gradient and on the data term,
//     minimise sum w phi_q(u - d) + sum_x-links c_x phi_p(u(x+1,y) - u(x,y) - gx) + sum_y-links c_y phi_p(u(x,y+1) - u(x,y) - gy),
//     phi_r(t) = (2 / r) (t^2 + eps^2)^(r/2),      0 < p, q <= 2,
// by iteratively reweighted least squares on the device, under every border kind of sc_hip_wls -- and what the three robust families
// share on the host: the chunk (robust_chunk), the round (RobustRounds::reweigh) and the image and region calls' check and entry
// preamble (robust_validate, robust_begin).  The entry code is the WLS call's (sc_pcg.h: pcg_begin, pcg_host_call, pcg_device_call;
// FLOAT_SMOOTH when the jobs carry base links c), the iteration the shared conjugate gradients in their three steps (pcg_chunk_begin /
// pcg_chunk_iterate / pcg_chunk_finish), the operator the WLS call's (WlsOperator, sc_wls_api.cpp) with RobustRounds beside it.  Per chunk:
//   round 0     the quadratic problem: the base operator's chunk with the caller's links c and weights (default precond_*): statistics,
//               judgement (every per-job refusal of the family is made here), set-up, a cold solve from u0 = M^-1 b.
//   round k     reweigh() at the iterate of round k - 1 (below: the one description of a round), then a warm solve: r = b - L u, z =
//               M^-1 r, p = z.  Conjugate gradients started at u lower the round's quadratic surrogate at every iterate, so a round
//               lowers the robust energy even when its solve stops early.
//   the end     the round rule (no plane's -- joint forms: no job's -- energy fell by more than round_tol times its energy) or
//               max_rounds.  The energy of the last iterate comes from one more reweigh() rather than an energy-only kernel: one launch
//               of ~ the set-up's time per call against a second kernel to keep in step with the first; what it writes to b, E, S, Dg
//               is not used.
#include "sc_pcg.h"
#include <algorithm>
#include <cmath>
#include <vector>

using namespace sc;

namespace {

constexpr RobustFamily FAMILY = {
    "a robust solve is preconditioned by a direct solve: at most 8192 unknowns (pixels - 2) per side",
    "a robust solve is solved by SC_METHOD_AUTO and SC_METHOD_FFT only (conjugate gradients preconditioned by the direct solve)",
    "a robust solve with SC_FLAG_FFT_FP64: at most 4096 unknowns per axis" };

int carries_of(bool base_links) { return FLOAT_DATA | FLOAT_WEIGHT | (base_links ? FLOAT_SMOOTH : 0); }

// The WLS operator with the links of the current round: round 0 from the caller's arrays, later rounds from the iterate (k_robust_setup;
// the coupled forms: k_robust_rho, k_robust_setup_rho).  Sums: w' | links | energy.
struct RobustOperator final : WlsOperator, RobustRounds {
    RobustOperator(Instance *I_, bool base_links, const sc_robust_params *p)
        : WlsOperator(I_, base_links, 0.f, 0.f, ROBUST_SUMS + 1), RobustRounds(*p, ROBUST_SUMS) {}
    RobustRounds *rounds() override { return this; }
    int launch(PcgChunk &c, int cpl, double *esum) override
    {
        PcgState &S = *I->pcg;
        const int rc = cpl ? ensure(I, S.rho, sizeof(float) * robust_rho_floats(c.wg, c.g.C, c.mv, cpl), false) : SC_OK;
        if (rc) return rc;
        if (cpl)
            launch_robust_coupled(c.g, c.wg, dj.data(), ds.data(), c.mv, grad, data, cpl, c.U, (float *)S.rho.p, c.R, (float *)S.e.p,
                                  (float *)S.s.p, (float *)S.dg.p, c.d_bb, c.d_round, esum, I->stream);
        else
            launch_robust_setup(c.g, c.wg, dj.data(), ds.data(), c.mv, grad, data, c.U, c.R, (float *)S.e.p, (float *)S.s.p, (float *)S.dg.p, c.d_bb,
                                c.d_round, I->stream);
        return SC_OK;
    }
    void take(const double *t) override { wsum = t[0]; ssum = t[1]; unit_links = false; }
};

} // namespace

const char *sc::robust_penalties_why(std::initializer_list<RobustPenalty> terms, const char *p_why, const char *eps_why, float tol, float round_tol, int kind)
{
    for (const RobustPenalty &t : terms)
        if (robust_bad_exponent(t.p)) return p_why;
    for (const RobustPenalty &t : terms)
        if (robust_bad_eps(t.p, t.eps)) return eps_why;
    return !std::isfinite(tol) ? "tol must be finite"
         : !std::isfinite(round_tol) ? "round_tol must be finite"
         : poisson_base(kind) == SC_POISSON_LAPLACIAN ? "a robust solve needs the guidance itself: the base kind must be SC_POISSON_GUIDANCE" : nullptr;
}

int sc::robust_validate(const sc_robust_params *p, const sc_poisson_layout *l, const char *size_why, const char **why)
{
    const int kind = p ? p->kind & ~COUPLING_BITS : 0;
    const char *own = !p ? nullptr
                    : robust_penalties_why({ { p->p_grad, p->eps_grad }, { p->p_data, p->eps_data } }, "p_grad and p_data must lie in (0, 2]",
                                           "eps_grad and eps_data must be finite and > 0 where their exponent is not 2", p->tol, p->round_tol, kind);
    return family_validate(p ? &kind : nullptr, l, own, size_why, why);
}

int sc::robust_begin(void *inst, const sc_robust_params *p, const sc_poisson_layout *l, const RobustFamily &f, Instance *&I, PcgCall &call)
{
    int kind;
    const int rc = pcg_begin(inst, p, l, [&f](const sc_robust_params *q, const sc_poisson_layout *m, const char **why) {
        return robust_validate(q, m, f.size_why, why); }, f.method_why, f.fp64_why, I, kind);
    if (!rc) call = PcgCall{ kind & ~COUPLING_BITS, p->tol, p->max_iters, 400 };
    return rc;
}

// A later round of any robust call, at the chunk's iterate c.U:
//   1. the operator's launch puts the system at the iterate in place of its own -- b, E, S, Dg (the volume: F) with s = c rho_p(link
//      residual), w' = w rho_q(u - d) -- and leaves per part b . b and the round's sums: w', the live links by kind, the energy last;
//      under a coupling the rho launch's gradient energy parts follow them, under the joint forms a job's on its channel-0 plane;
//   2. one host read of all of it: the round's one mandatory wait;
//   3. the fold, in one fixed order -- planes, within a plane its parts, every field in that one pass, then the plane's gradient
//      parts: the totals go to the operator (take), whose precond_constant makes s-bar and w-bar of M from them, the energies to the
//      round rule per unit: a plane, or a job where the channels are coupled.
int RobustRounds::reweigh(PcgChunk &c, std::vector<double> &energy)
{
    Instance *I = c.I;
    const int cpl = coupling(c.g.C), per = (cpl & ROBUST_JOINT) ? c.g.C : 1, last = nsums - 1;
    const size_t parts = (size_t)c.planes * PCG_PARTS;
    const int rc = launch(c, cpl, c.d_round + parts * nsums);
    if (rc) return rc;
    SC_HIP(I, hipGetLastError());
    SC_HIP(I, hipMemcpyAsync(c.h_round, c.d_round, sizeof(double) * parts * (nsums + (cpl ? 1 : 0)), hipMemcpyDeviceToHost, I->stream));
    SC_HIP(I, hipStreamSynchronize(I->stream));
    energy.assign(c.planes / per, 0.0);
    double totals[VOLUME_ROBUST_SUMS] = {};
    for (int p = 0; p < c.planes; ++p) {
        for (int i = 0; i < c.nop; ++i) {
            const double *part = c.h_round + ((size_t)p * PCG_PARTS + i) * nsums;
            for (int f = 0; f < last; ++f) totals[f] += part[f];
            energy[p / per] += part[last];
        }
        const double *grad_parts = c.h_round + parts * nsums + (size_t)p * PCG_PARTS;
        for (int i = 0; cpl && p % per == 0 && i < c.nop; ++i) energy[p / per] += grad_parts[i];
    }
    take(totals);
    return SC_OK;
}

// One chunk of any robust call (the operator's rounds()): the
// quadratic round, the reweighting rounds, the output.  res: the total of the inner iterations, whether the round rule
// was met (always, when p = q = 2), the last inner solve's residual.  The code: SC_ERR_NOT_CONVERGED when an inner solve ran out of
// max_iters (the rounds go on from its last iterate), else SC_OK -- running out of rounds included.
int sc::robust_chunk(Instance *I, const PcgCall &call, const PoissonGeo &g, PcgOperator &op, int *const *rcs, int m, PcgChunkResult &res, int &job_errors)
{
    RobustRounds &rounds = *op.rounds();
    PcgState &S = *I->pcg;
    S.trace_energy.clear();
    S.trace_iters.clear();
    PcgChunk c;
    int rc = pcg_chunk_begin(I, call, g, op, rcs, m, job_errors, c);
    res = PcgChunkResult();
    if (rc || !c.mv) return rc;
    if ((rc = op.setup(g, c.wg, false, c.mv, c.R, c.d_bb))) return rc;
    SC_HIP(I, hipGetLastError());
    PcgChunkResult one;
    if ((rc = pcg_chunk_iterate(c, op, false, one))) return rc;
    int total = one.iters;
    bool inner = one.converged, met = rounds.quadratic();
    S.trace_iters.push_back(one.iters);
    const int max_rounds = rounds.quadratic() ? 0 : rounds.max_rounds > 0 ? rounds.max_rounds : 15;
    const double round_tol = rounds.round_tol == 0.f ? 1e-4 : (double)rounds.round_tol;
    std::vector<double> prev, cur;
    for (int k = 1;; ++k) {
        if ((rc = rounds.reweigh(c, cur))) return rc;          // the energy of round k - 1's iterate, and round k's system
        double sum = 0.0;
        for (double e : cur) sum += e;
        S.trace_energy.push_back(sum);
        if (k >= 2 && round_tol >= 0.0) {
            met = true;
            for (size_t p = 0; p < cur.size(); ++p)
                if (prev[p] - cur[p] > round_tol * prev[p]) met = false;
        }
        if (met || k > max_rounds) break;
        if ((rc = pcg_chunk_iterate(c, op, true, one))) return rc;
        total += one.iters;
        inner = inner && one.converged;
        S.trace_iters.push_back(one.iters);
        prev.swap(cur);
    }
    res.iters = total;
    res.converged = met;
    res.rel = one.rel;
    return pcg_chunk_finish(c, op, inner ? SC_OK : SC_ERR_NOT_CONVERGED);
}

extern "C" {

int sc_hip_robust_check(const sc_robust_params *p, const sc_poisson_layout *l)
{
    return robust_validate(p, l, FAMILY.size_why, nullptr);
}

int sc_hip_robust_device(void *inst, const sc_robust_params *p, const sc_poisson_layout *l, sc_robust_job *jobs, int n, bool bSync)
{
    Instance *I;
    PcgCall call;
    const int rc = robust_begin(inst, p, l, FAMILY, I, call);
    if (rc) return rc;
    // base links: all jobs or none, as the first job has them; a job that differs is refused (as one with exactly one of the two arrays)
    const bool base_links = jobs && n > 0 && (jobs[0].smooth_x || jobs[0].smooth_y);
    RobustOperator op(I, base_links, p);
    return pcg_device_call(I, call, l, carries_of(base_links), jobs, n, [base_links](const sc_robust_job &j) {
        const bool stray = !base_links && (j.smooth_x || j.smooth_y);          // (refused through its data pointer: "null data pointer")
        return FloatArrays{ j.gx, j.gy, nullptr, stray ? nullptr : j.data, j.weight, j.boundary, j.out, j.smooth_x, j.smooth_y }; }, op, bSync,
        robust_chunk);
}

int sc_hip_robust(void *inst, const sc_robust_params *p, const sc_poisson_layout *l, const float *gx, const float *gy, const float *data,
                  const float *weight, const float *smooth_x, const float *smooth_y, const float *boundary, float *out)
{
    Instance *I;
    PcgCall call;
    const int rc = robust_begin(inst, p, l, FAMILY, I, call);
    if (rc) return rc;
    if (!smooth_x != !smooth_y) { I->err = "smooth_x and smooth_y go together (both NULL: all base links 1)"; return SC_ERR_BAD_ARG; }
    const bool base_links = smooth_x != nullptr;
    RobustOperator op(I, base_links, p);
    return pcg_host_call(I, call, l, carries_of(base_links), FloatArrays{ gx, gy, nullptr, data, weight, boundary, out, smooth_x, smooth_y },
                         op, robust_chunk);
}

int sc_hip_robust_trace(void *inst, double *energy, int *iters, int cap)
{
    Instance *I = get(inst);
    if (!I) return 0;
    const PcgState &S = *I->pcg;
    const int n = (int)S.trace_energy.size();
    for (int k = 0; k < std::min(n, cap); ++k) {
        if (energy) energy[k] = S.trace_energy[k];
        if (iters) iters[k] = S.trace_iters[k];
    }
    return n;
}

} // extern "C"
