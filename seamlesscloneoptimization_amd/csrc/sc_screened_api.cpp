// sc_screened_api.cpp -- the screened Poisson solve on float32 images (sc_hip_screened_check, sc_hip_screened_device, sc_hip_screened):
//     minimise lambda sum (u - d)^2 + sum |grad u - g|^2,   i.e.   (A - lambda) u = div g - lambda d,   lambda > 0,
// A the 5-point operator of sc_hip_poisson with a Dirichlet frame, a reflecting border (SC_POISSON_NEUMANN) or Dirichlet lines on
// some sides and free ones on the others (SC_POISSON_FREE_*), or with axes that wrap (SC_POISSON_PERIODIC_*).
//
// A call is a Poisson call (sc_poisson_api.cpp: validation, chunks of at most SC_POISSON_MAX_PLANES planes, stage marks, codes) with
// PoissonCall::lam set: the jobs carry their data term, the launches that build the right-hand side read it (F = lap - lambda d:
// k_poisson_pre / k_poisson_pre_group; k_mix MODE 0 with any free side), and the direct solves divide by eigenvalue - lambda
// (k_fft_dst<1>'s exact branch, k_mix MODE 1).  Always the direct solve: SC_METHOD_AUTO resolves to SC_METHOD_FFT at any size.
#include "sc_instance.h"
#include <cmath>
#include <vector>

using namespace sc;

namespace {

// host-only: the call's code for these parameters and this layout (SC_OK: it may run); `why` gets the reason
int screened_validate(const sc_screened_params *p, const sc_poisson_layout *l, const char **why)
{
    const char *dummy;
    if (!why) why = &dummy;
    *why = "";
    if (!p || !l) { *why = "null pointer"; return SC_ERR_BAD_ARG; }
    if (!std::isfinite(p->lambda) || !(p->lambda > 0.f)) { *why = "lambda must be finite and > 0"; return SC_ERR_BAD_ARG; }
    const sc_poisson_params pp{ p->kind, 0.f };
    const int rc = poisson_validate(&pp, l, why);       // kind, channels, strides; the Neumann side limit; at least 3 x 3 under a frame
    if (rc) return rc;
    if (!poisson_direct(p->kind) && !fft_supported(l->cols - 2, l->rows - 2, false)) {
        *why = "a screened solve is a direct solve: at most 8192 unknowns (pixels - 2) per side";
        return SC_ERR_BAD_SIZE;
    }
    return SC_OK;
}

// the call's code on this instance: the methods that serve it, the side limit of its transforms' precision
int screened_instance_check(Instance *I, const sc_screened_params *p, const sc_poisson_layout *l)
{
    const int method = I->opts.method;
    if (method != SC_METHOD_AUTO && method != SC_METHOD_FFT) {
        I->err = "a screened solve is solved by SC_METHOD_AUTO and SC_METHOD_FFT only (the multigrid and the relaxation solvers know the unscreened operator)";
        return SC_ERR_BAD_ARG;
    }
    const int free = poisson_free_sides(p->kind), per = poisson_periodic(p->kind);
    return direct_fp64_check(I, free, l, per ? "a screened solve with periodic axes and SC_FLAG_FFT_FP64: at most 4096 unknowns per axis"
                                     : !free ? "a screened solve with SC_FLAG_FFT_FP64: at most 4096 unknowns (pixels - 2) per side"
                                     : free == 15 ? "a screened SC_POISSON_NEUMANN solve with SC_FLAG_FFT_FP64: the image must be at most 4096 x 4096"
                                                  : "a screened solve with free sides and SC_FLAG_FFT_FP64: at most 4096 unknowns per axis", per);
}

// a job's own code: data always, boundary with a Dirichlet line on any side, the arrays of its kind (poisson_norm_kind's), out; each
// 4-byte aligned
int screened_job_validate(int kind, const float *gx, const float *gy, const float *lap, const float *data, const float *b, const float *out,
                          const char **why)
{
    if (!data) { *why = "null data pointer"; return SC_ERR_BAD_ARG; }
    if (!aligned4(data)) { *why = "array pointer not 4-byte aligned"; return SC_ERR_BAD_ARG; }
    // (without a Dirichlet line on any side boundary is not read: poisson_job_validate then checks out in its place)
    return poisson_job_validate(kind, gx, gy, lap, poisson_no_dirichlet(kind) ? nullptr : b, out, why);
}

PoissonJobDev dev_job(int kind, const float *gx, const float *gy, const float *lap, const float *data, const float *b, float *out)
{
    PoissonJobDev j{ gx, gy, lap, poisson_no_dirichlet(kind) ? nullptr : b, out };
    j.d = data;
    return j;
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
    int rc = begin_call(inst, I);
    if (rc) return rc;
    const char *why = "";
    if ((rc = screened_validate(p, l, &why))) { I->err = why; return rc; }
    if ((rc = screened_instance_check(I, p, l))) return rc;
    const int kind = poisson_norm_kind(p->kind);
    if (!jobs || n <= 0) { I->err = "no jobs"; return SC_ERR_BAD_ARG; }
    int worst = SC_OK;
    std::vector<PoissonJobDev> dj;
    std::vector<int *> rcs;
    for (int i = 0; i < n; ++i) {
        sc_screened_job &j = jobs[i];
        const int vrc = screened_job_validate(kind, j.gx, j.gy, j.lap, j.data, j.boundary, j.out, &why);
        if (vrc != SC_OK) {
            j.rc = vrc;
            if (worst == SC_OK) { worst = vrc; I->err = why; }
            continue;
        }
        j.rc = SC_ERR_HIP;          // until its chunk has run
        dj.push_back(dev_job(kind, j.gx, j.gy, j.lap, j.data, j.boundary, j.out));
        rcs.push_back(&j.rc);
    }
    if (dj.empty()) return worst;
    float t[4] = { 0.f, 0.f, 0.f, 0.f };
    I->info.ms_h2d = I->info.ms_d2h = 0.f;
    rc = poisson_run(I, PoissonCall{ kind, 0.f, p->lambda }, l, dj.data(), rcs.data(), (int)dj.size(), bSync, t);
    if (rc != SC_OK) return rc;
    poisson_set_timing(I, t);       // (zeros without bSync)
    return worst;
}

int sc_hip_screened(void *inst, const sc_screened_params *p, const sc_poisson_layout *l, const float *gx, const float *gy,
                    const float *lap, const float *data, const float *boundary, float *out)
{
    Instance *I;
    int rc = begin_call(inst, I);
    if (rc) return rc;
    const char *why = "";
    if ((rc = screened_validate(p, l, &why))) { I->err = why; return rc; }
    if ((rc = screened_instance_check(I, p, l))) return rc;
    const int kind = poisson_norm_kind(p->kind);
    if ((rc = screened_job_validate(kind, gx, gy, lap, data, boundary, out, &why))) { I->err = why; return rc; }
    // one device block: the spans of the inputs, of data, of boundary under a Dirichlet frame (data's when they are one array), and
    // of out unless out is data or boundary (in place); each at a 256-byte boundary
    const size_t span = poisson_span(l), bytes = span * sizeof(float), slot = (bytes + 255) / 256 * 256;
    const bool guidance = poisson_base(kind) == SC_POISSON_GUIDANCE;
    if (poisson_no_dirichlet(kind)) boundary = nullptr;
    const bool b_is_d = boundary == data, own_b = boundary && !b_is_d, in_place = out == data || (boundary && out == boundary);
    const int n_in = guidance ? 2 : 1, slots = n_in + 1 + (own_b ? 1 : 0) + (in_place ? 0 : 1);
    if ((rc = ensure(I, I->d_pois, slot * slots, false))) return rc;
    uint8_t *d = (uint8_t *)I->d_pois.p;
    float *d_in0 = (float *)d, *d_in1 = guidance ? (float *)(d + slot) : nullptr;
    float *d_d = (float *)(d + slot * n_in);
    float *d_b = own_b ? (float *)(d + slot * (n_in + 1)) : (boundary ? d_d : nullptr);
    float *d_out = !in_place ? (float *)(d + slot * (slots - 1)) : (out == data ? d_d : d_b);
    SC_HIP(I, hipEventRecord(I->ev_k0, I->stream));
    if ((rc = upload_rows(I, I->h_face, d_in0, bytes, (const uint8_t *)(guidance ? gx : lap), bytes, bytes, 1))) return rc;
    if (guidance && (rc = upload_rows(I, I->h_body, d_in1, bytes, (const uint8_t *)gy, bytes, bytes, 1))) return rc;
    if ((rc = upload_rows(I, I->h_in, d_d, bytes, (const uint8_t *)data, bytes, bytes, 1))) return rc;
    if (own_b && (rc = upload_rows(I, I->h_mask, d_b, bytes, (const uint8_t *)boundary, bytes, bytes, 1))) return rc;
    const PoissonJobDev job = dev_job(kind, guidance ? d_in0 : nullptr, d_in1, guidance ? nullptr : d_in0, d_d, d_b, d_out);
    int job_rc = SC_OK, *const job_rcs[1] = { &job_rc };
    float t[4] = { 0.f, 0.f, 0.f, 0.f };
    rc = poisson_run(I, PoissonCall{ kind, 0.f, p->lambda }, l, &job, job_rcs, 1, true, t);
    if (rc != SC_OK) return rc;
    return poisson_download(I, l, d_out, out, t, rc);
}

} // extern "C"
