// sc_screened_api.cpp -- the screened Poisson solve on float32 images (sc_hip_screened_check, sc_hip_screened_device, sc_hip_screened):
//     minimise lambda sum (u - d)^2 + sum |grad u - g|^2,   i.e.   (A - lambda) u = div g - lambda d,   lambda > 0,
// A the 5-point operator of sc_hip_poisson with a Dirichlet frame, a reflecting border (SC_POISSON_NEUMANN) or Dirichlet lines on
// some sides and free ones on the others (SC_POISSON_FREE_*), or with axes that wrap (SC_POISSON_PERIODIC_*).
//
// A call is a Poisson call (sc_poisson_api.cpp: poisson_run behind the families' shared front end; stage marks, codes) with
// PoissonCall::lam set: the jobs carry their data term, the launches that build the right-hand side read it (F = lap - lambda d:
// k_poisson_pre / k_poisson_pre_group; k_mix MODE 0 with any free side), and the direct solves divide by eigenvalue - lambda
// (k_fft_dst<1>'s exact branch, k_mix MODE 1).  Always the direct solve: SC_METHOD_AUTO resolves to SC_METHOD_FFT at any size.
#include "sc_instance.h"
#include <cmath>

using namespace sc;

namespace {

// host-only: the call's code for these parameters and this layout (SC_OK: it may run); `why` gets the reason
int screened_validate(const sc_screened_params *p, const sc_poisson_layout *l, const char **why)
{
    const char *own = p && !(std::isfinite(p->lambda) && p->lambda > 0.f) ? "lambda must be finite and > 0" : nullptr;
    return family_validate(p ? &p->kind : nullptr, l, own,
                           "a screened solve is a direct solve: at most 8192 unknowns (pixels - 2) per side", why);
}

// the call's code on this instance: the methods that serve it, the side limit of its transforms' precision
int screened_instance_check(Instance *I, int kind, const sc_poisson_layout *l)
{
    const int free = poisson_free_sides(kind), per = poisson_periodic(kind);
    return direct_instance_check(I, kind, l,
        "a screened solve is solved by SC_METHOD_AUTO and SC_METHOD_FFT only (the multigrid and the relaxation solvers know the unscreened operator)",
        per ? "a screened solve with periodic axes and SC_FLAG_FFT_FP64: at most 4096 unknowns per axis"
      : !free ? "a screened solve with SC_FLAG_FFT_FP64: at most 4096 unknowns (pixels - 2) per side"
      : free == 15 ? "a screened SC_POISSON_NEUMANN solve with SC_FLAG_FFT_FP64: the image must be at most 4096 x 4096"
                   : "a screened solve with free sides and SC_FLAG_FFT_FP64: at most 4096 unknowns per axis");
}

// what every entry starts with: the instance, both checks; kind: poisson_norm_kind's
int screened_begin(void *inst, const sc_screened_params *p, const sc_poisson_layout *l, Instance *&I, int &kind)
{
    int rc = begin_call(inst, I);
    if (rc) return rc;
    const char *why = "";
    if ((rc = screened_validate(p, l, &why))) { I->err = why; return rc; }
    kind = poisson_norm_kind(p->kind);
    return screened_instance_check(I, kind, l);
}

} // namespace

extern "C" {

int sc_hip_screened_check(const sc_screened_params *p, const sc_poisson_layout *l)
{
    return screened_validate(p, l, nullptr);
}

int sc_hip_screened_device(void *inst, const sc_screened_params *p, const sc_poisson_layout *l, sc_screened_job *jobs, int n, bool bSync)
{
    Instance *I;
    int kind, rc = screened_begin(inst, p, l, I, kind);
    if (rc) return rc;
    FloatJobs v;
    const int worst = float_intake(I, kind, FLOAT_DATA, jobs, n, [](const sc_screened_job &j) {
        return FloatArrays{ j.gx, j.gy, j.lap, j.data, nullptr, j.boundary, j.out }; }, v);
    if (v.rcs.empty()) return worst;
    float t[4] = { 0.f, 0.f, 0.f, 0.f };
    I->info.ms_h2d = I->info.ms_d2h = 0.f;
    rc = poisson_run(I, PoissonCall{ kind, 0.f, p->lambda }, l, v.dj.data(), v.rcs.data(), (int)v.rcs.size(), bSync, t);
    if (rc != SC_OK) return rc;     // (a direct solve: SC_ERR_NOT_CONVERGED would be an error like any other)
    poisson_set_timing(I, t);       // (zeros without bSync)
    return worst;
}

int sc_hip_screened(void *inst, const sc_screened_params *p, const sc_poisson_layout *l, const float *gx, const float *gy,
                    const float *lap, const float *data, const float *boundary, float *out)
{
    Instance *I;
    int kind, rc = screened_begin(inst, p, l, I, kind);
    if (rc) return rc;
    const FloatArrays a{ gx, gy, lap, data, nullptr, boundary, out };
    const char *why = "";
    if ((rc = float_job_validate(kind, FLOAT_DATA, a, &why))) { I->err = why; return rc; }
    FloatStaged s;
    if ((rc = float_stage(I, l, kind, FLOAT_DATA, a, s))) return rc;
    int job_rc = SC_OK, *const job_rcs[1] = { &job_rc };
    float t[4] = { 0.f, 0.f, 0.f, 0.f };
    rc = poisson_run(I, PoissonCall{ kind, 0.f, p->lambda }, l, &s.job, job_rcs, 1, true, t);
    if (rc != SC_OK) return rc;
    return poisson_download(I, l, s.job.out, out, t, rc);
}

} // extern "C"
