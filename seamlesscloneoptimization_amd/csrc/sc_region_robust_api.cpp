// sc_region_robust_api.cpp -- robust region solves on float32 images (sc_hip_region_robust_check, sc_hip_region_robust_device,
// sc_hip_region_robust): the robust call's penalties on the region call's domain of any shape (sc_region_api.cpp),
//     minimise over the UNKNOWN pixels  sum w phi_q(u - d) + sum_live x-links c_x phi_p(dx u - gx) + sum_live y-links c_y phi_p(dy u - gy),
// u = data at KNOWN pixels, boundary on the Dirichlet lines, no link to an OUTSIDE pixel, by iteratively reweighted least squares on the
// device.  The entry code is the region call's (sc_pcg.h: pcg_host_call, pcg_device_call; the front end with FLOAT_STATE) behind the
// robust calls' preamble; the chunk, its rounds and the round itself are sc_robust_api.cpp's (robust_chunk, RobustRounds::reweigh).
// This file says what differs from the image call: the base operator (round 0 is RegionOperator's chunk, "nothing pins the channel"
// among its refusals), the launches, and one more sum -- the UNKNOWN - KNOWN links' s, which joins the sum of w' in w-bar =
// (sum of w' + sum of UNKNOWN - KNOWN s) / (UNKNOWN pixels); s-bar = (sum of live s) / (live links).
#include "sc_pcg.h"

using namespace sc;

namespace {

constexpr RobustFamily FAMILY = {
    "a robust region solve is preconditioned by a direct solve: at most 8192 unknowns (pixels - 2) per side",
    "a robust region solve is solved by SC_METHOD_AUTO and SC_METHOD_FFT only (conjugate gradients preconditioned by the direct solve)",
    "a robust region solve with SC_FLAG_FFT_FP64: at most 4096 unknowns per axis" };

int carries_of(bool weight, bool links) { return FLOAT_DATA | FLOAT_STATE | (weight ? FLOAT_WEIGHT : 0) | (links ? FLOAT_SMOOTH : 0); }

// The region operator with the links of the current round: round 0 from the caller's arrays, later rounds from the iterate
// (k_region_robust_setup; the coupled forms: k_region_robust_rho, k_region_robust_setup_rho).  Sums: w' | links | UNKNOWN - KNOWN | energy.
struct RegionRobustOperator final : RegionOperator, RobustRounds {
    RegionRobustOperator(Instance *I_, bool weight, bool base_links, const sc_robust_params *p)
        : RegionOperator(I_, weight, base_links, 0.f, 0.f, REGION_ROBUST_SUMS + 1), RobustRounds(*p, REGION_ROBUST_SUMS) {}
    RobustRounds *rounds() override { return this; }
    int launch(PcgChunk &c, int cpl, double *esum) override
    {
        PcgState &S = *I->pcg;
        const int rc = cpl ? ensure(I, S.rho, sizeof(float) * robust_rho_floats(c.wg, c.g.C, c.mv, cpl), false) : SC_OK;
        if (rc) return rc;
        if (cpl)
            launch_region_robust_coupled(c.g, c.wg, dj.data(), ds.data(), c.mv, grad, data, cpl, c.U, (float *)S.rho.p, c.R, (float *)S.e.p,
                                         (float *)S.s.p, (float *)S.dg.p, c.d_bb, c.d_round, esum, I->stream);
        else
            launch_region_robust_setup(c.g, c.wg, dj.data(), ds.data(), c.mv, grad, data, c.U, c.R, (float *)S.e.p, (float *)S.s.p, (float *)S.dg.p,
                                       c.d_bb, c.d_round, I->stream);
        return SC_OK;
    }
    void take(const double *t) override { wsum = t[0]; ssum = t[1]; uksum = t[2]; unit_links = false; }
};

} // namespace

extern "C" {

int sc_hip_region_robust_check(const sc_robust_params *p, const sc_poisson_layout *l)
{
    return robust_validate(p, l, FAMILY.size_why, nullptr);
}

int sc_hip_region_robust_device(void *inst, const sc_robust_params *p, const sc_poisson_layout *l, sc_region_robust_job *jobs, int n, bool bSync)
{
    Instance *I;
    PcgCall call;
    const int rc = robust_begin(inst, p, l, FAMILY, I, call);
    if (rc) return rc;
    // the data term and the base links: all jobs or none, as the first job has them; a job that differs is refused (as one with exactly
    // one of the two link arrays)
    const bool weight = jobs && n > 0 && jobs[0].weight, links = jobs && n > 0 && (jobs[0].smooth_x || jobs[0].smooth_y);
    RegionRobustOperator op(I, weight, links, p);
    return pcg_device_call(I, call, l, carries_of(weight, links), jobs, n, [weight, links](const sc_region_robust_job &j) {
        const bool stray = (!weight && j.weight) || (!links && (j.smooth_x || j.smooth_y));      // (refused through its data pointer)
        return FloatArrays{ j.gx, j.gy, nullptr, stray ? nullptr : j.data, j.weight, j.boundary, j.out, j.smooth_x, j.smooth_y, j.state }; }, op, bSync,
        robust_chunk);
}

int sc_hip_region_robust(void *inst, const sc_robust_params *p, const sc_poisson_layout *l, const float *gx, const float *gy, const float *data,
                         const float *state, const float *weight, const float *smooth_x, const float *smooth_y, const float *boundary, float *out)
{
    Instance *I;
    PcgCall call;
    const int rc = robust_begin(inst, p, l, FAMILY, I, call);
    if (rc) return rc;
    if (!smooth_x != !smooth_y) { I->err = "smooth_x and smooth_y go together (both NULL: every base link 1)"; return SC_ERR_BAD_ARG; }
    const bool has_w = weight != nullptr, links = smooth_x != nullptr;
    RegionRobustOperator op(I, has_w, links, p);
    return pcg_host_call(I, call, l, carries_of(has_w, links), FloatArrays{ gx, gy, nullptr, data, weight, boundary, out, smooth_x, smooth_y, state }, op,
                         robust_chunk);
}

} // extern "C"
