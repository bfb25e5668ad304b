// sc_region_robust_api.cpp -- robust region solves on float32 images (sc_hip_region_robust_check, sc_hip_region_robust_device,
// sc_hip_region_robust): the robust call's penalties (sc_robust_api.cpp) on the region call's domain of any shape (sc_region_api.cpp),
//     minimise over the UNKNOWN pixels  sum w phi_q(u - d) + sum_live x-links c_x phi_p(dx u - gx) + sum_live y-links c_y phi_p(dy u - gy),
// u = data at KNOWN pixels, boundary on the Dirichlet lines, no link to an OUTSIDE pixel, by iteratively reweighted least squares on the
// device.  The entry code is the region call's (sc_pcg.h: pcg_begin, pcg_host_call, pcg_device_call; the front end with FLOAT_STATE),
// the rounds are robust_chunk's (sc_robust_api.cpp), which drives this file's RegionRobustOperator through RobustRounds:
//   round 0     RegionOperator's chunk with default precond_*: statistics, judgement (every per-job refusal of the region call, "nothing
//               pins the channel" included, is made here), set-up, a cold solve.
//   round k     k_region_robust_setup at the iterate of round k - 1 (sc_region_robust.hip): b, E, S, Dg with s = c rho_p, w' = w rho_q
//               under the states, and per part b . b, the sums of w', of the live links and of the UNKNOWN - KNOWN links and the energy;
//               one host read of those gives s-bar = (sum of live s) / (live links) and w-bar = (sum of w' + sum of UNKNOWN - KNOWN s) /
//               (UNKNOWN pixels) -- the counts are round 0's: states do not change -- and the round rule's energies; then a warm solve.
//               With SC_ROBUST_ISOTROPIC / SC_ROBUST_JOINT_CHANNELS (and p_grad < 2; a joint form needs two channels) the system comes
//               from launch_region_robust_coupled's two launches; the gradient energy is the first one's, under the joint forms one
//               number per job on its channel-0 plane.
#include "sc_pcg.h"
#include <algorithm>
#include <cmath>
#include <vector>

using namespace sc;

namespace {

constexpr int COUPLING_BITS = SC_ROBUST_ISOTROPIC | SC_ROBUST_JOINT_CHANNELS;

int region_robust_validate(const sc_robust_params *p, const sc_poisson_layout *l, const char **why)
{
    const int kind = p ? p->kind & ~COUPLING_BITS : 0;          // the two bits are sc_robust_params' own: the family's kinds know nothing of them
    const char *own = !p ? nullptr
                    : robust_bad_exponent(p->p_grad) || robust_bad_exponent(p->p_data) ? "p_grad and p_data must lie in (0, 2]"
                    : robust_bad_eps(p->p_grad, p->eps_grad) || robust_bad_eps(p->p_data, p->eps_data) ? "eps_grad and eps_data must be finite and > 0 where their exponent is not 2"
                    : !std::isfinite(p->tol) ? "tol must be finite"
                    : !std::isfinite(p->round_tol) ? "round_tol must be finite"
                    : poisson_base(kind) == SC_POISSON_LAPLACIAN ? "a robust solve needs the guidance itself: the base kind must be SC_POISSON_GUIDANCE" : nullptr;
    return family_validate(p ? &kind : nullptr, l, own,
                           "a robust region solve is preconditioned by a direct solve: at most 8192 unknowns (pixels - 2) per side", why);
}

constexpr const char *METHOD_WHY = "a robust region solve is solved by SC_METHOD_AUTO and SC_METHOD_FFT only (conjugate gradients preconditioned by the direct solve)";
constexpr const char *FP64_WHY = "a robust region solve with SC_FLAG_FFT_FP64: at most 4096 unknowns per axis";

int carries_of(bool weight, bool links) { return FLOAT_DATA | FLOAT_STATE | (weight ? FLOAT_WEIGHT : 0) | (links ? FLOAT_SMOOTH : 0); }

// The region operator with the links of the current round: round 0 from the caller's arrays, later rounds from the iterate.
struct RegionRobustOperator final : RegionOperator, RobustRounds {
    const sc_robust_params prm;
    const RobustTerm grad, data;
    const int bits;          // ROBUST_ISO | ROBUST_JOINT as the caller set them
    RegionRobustOperator(Instance *I_, bool weight, bool base_links, const sc_robust_params *p)
        : RegionOperator(I_, weight, base_links, 0.f, 0.f, REGION_ROBUST_SUMS + 1), prm(*p), grad(robust_term(p->p_grad, p->eps_grad)),
          data(robust_term(p->p_data, p->eps_data)),
          bits(((p->kind & SC_ROBUST_ISOTROPIC) ? ROBUST_ISO : 0) | ((p->kind & SC_ROBUST_JOINT_CHANNELS) ? ROBUST_JOINT : 0)) {}
    RobustRounds *rounds() override { return this; }
    bool quadratic() const override { return grad.mode == 0 && data.mode == 0; }
    int max_rounds() const override { return prm.max_rounds; }
    float round_tol() const override { return prm.round_tol; }
    // the coupling that changes anything: none with p_grad = 2 (every form is sum c t^2), no joint form of one channel
    int coupling(int C) const { return grad.mode == 0 ? 0 : C == 1 ? bits & ~ROBUST_JOINT : bits; }
    // A later round: the system at the chunk's iterate in place of the operator's, the round's sums in place of the statistics' (the
    // counts of live links and of UNKNOWN pixels stay: the states do not change), and that iterate's energy (one wait) -- per plane,
    // or per job where the channels are coupled (the round rule's units)
    int reweigh(PcgChunk &c, std::vector<double> &energy) override
    {
        PcgState &S = *I->pcg;
        const int cpl = coupling(c.g.C), per = (cpl & ROBUST_JOINT) ? c.g.C : 1;
        const size_t parts = (size_t)c.planes * PCG_PARTS;
        if (cpl) {
            const int rc = ensure(I, S.rho, sizeof(float) * robust_rho_floats(c.wg, c.g.C, c.mv, cpl), false);
            if (rc) return rc;
            launch_region_robust_coupled(c.g, c.wg, dj.data(), ds.data(), c.mv, grad, data, cpl, c.U, (float *)S.rho.p, c.R, (float *)S.e.p,
                                         (float *)S.s.p, (float *)S.dg.p, c.d_bb, c.d_round, c.d_round + parts * REGION_ROBUST_SUMS, I->stream);
        } else
            launch_region_robust_setup(c.g, c.wg, dj.data(), ds.data(), c.mv, grad, data, c.U, c.R, (float *)S.e.p, (float *)S.s.p, (float *)S.dg.p,
                                       c.d_bb, c.d_round, I->stream);
        SC_HIP(I, hipGetLastError());
        SC_HIP(I, hipMemcpyAsync(c.h_round, c.d_round, sizeof(double) * parts * (REGION_ROBUST_SUMS + (cpl ? 1 : 0)), hipMemcpyDeviceToHost, I->stream));
        SC_HIP(I, hipStreamSynchronize(I->stream));
        energy.assign(c.planes / per, 0.0);
        wsum = ssum = uksum = 0.0;
        unit_links = false;
        for (int p = 0; p < c.planes; ++p) {
            const double *plane = c.h_round + (size_t)p * PCG_PARTS * REGION_ROBUST_SUMS;
            for (int i = 0; i < c.nop; ++i) {
                const double *part = plane + (size_t)i * REGION_ROBUST_SUMS;
                wsum += part[0];
                ssum += part[1];
                uksum += part[2];
                energy[p / per] += part[3];
            }
            // the coupled forms' gradient energy: the rho launch's parts, a job's on its channel-0 plane
            const double *grad_parts = c.h_round + parts * REGION_ROBUST_SUMS + (size_t)p * PCG_PARTS;
            for (int i = 0; cpl && p % per == 0 && i < c.nop; ++i) energy[p / per] += grad_parts[i];
        }
        return SC_OK;
    }
};

PcgCall region_robust_call(int kind, const sc_robust_params *p) { return PcgCall{ kind, p->tol, p->max_iters, 400 }; }

} // namespace

extern "C" {

int sc_hip_region_robust_check(const sc_robust_params *p, const sc_poisson_layout *l)
{
    return region_robust_validate(p, l, nullptr);
}

int sc_hip_region_robust_device(void *inst, const sc_robust_params *p, const sc_poisson_layout *l, sc_region_robust_job *jobs, int n, bool bSync)
{
    Instance *I;
    int kind, rc = pcg_begin(inst, p, l, region_robust_validate, METHOD_WHY, FP64_WHY, I, kind);
    if (rc) return rc;
    kind &= ~COUPLING_BITS;          // (poisson_norm_kind passes them through; RegionRobustOperator has them from p)
    // the data term and the base links: all jobs or none, as the first job has them; a job that differs is refused (as one with exactly
    // one of the two link arrays)
    const bool weight = jobs && n > 0 && jobs[0].weight, links = jobs && n > 0 && (jobs[0].smooth_x || jobs[0].smooth_y);
    RegionRobustOperator op(I, weight, links, p);
    return pcg_device_call(I, region_robust_call(kind, p), l, carries_of(weight, links), jobs, n, [weight, links](const sc_region_robust_job &j) {
        const bool stray = (!weight && j.weight) || (!links && (j.smooth_x || j.smooth_y));      // (refused through its data pointer)
        return FloatArrays{ j.gx, j.gy, nullptr, stray ? nullptr : j.data, j.weight, j.boundary, j.out, j.smooth_x, j.smooth_y, j.state }; }, op, bSync,
        robust_chunk);
}

int sc_hip_region_robust(void *inst, const sc_robust_params *p, const sc_poisson_layout *l, const float *gx, const float *gy, const float *data,
                         const float *state, const float *weight, const float *smooth_x, const float *smooth_y, const float *boundary, float *out)
{
    Instance *I;
    int kind, rc = pcg_begin(inst, p, l, region_robust_validate, METHOD_WHY, FP64_WHY, I, kind);
    if (rc) return rc;
    kind &= ~COUPLING_BITS;
    if (!smooth_x != !smooth_y) { I->err = "smooth_x and smooth_y go together (both NULL: every base link 1)"; return SC_ERR_BAD_ARG; }
    const bool has_w = weight != nullptr, links = smooth_x != nullptr;
    RegionRobustOperator op(I, has_w, links, p);
    return pcg_host_call(I, region_robust_call(kind, p), l, carries_of(has_w, links),
                         FloatArrays{ gx, gy, nullptr, data, weight, boundary, out, smooth_x, smooth_y, state }, op, robust_chunk);
}

} // extern "C"
