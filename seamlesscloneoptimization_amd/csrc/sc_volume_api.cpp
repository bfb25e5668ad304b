// sc_volume_api.cpp -- the volume solve on float32 frame stacks (sc_hip_volume_check, sc_hip_volume_device, sc_hip_volume): the region
// call's problem with unit spatial links on every one of `frames` images that share a layout, coupled by temporal links of the constant
// weight tau (sc_volume.hip: the system and its work planes).  The entry code and the iteration are the shared ones (sc_pcg.h; the
// front end with FLOAT_STATE | FLOAT_GT and the call's frame stride); VolumeOperator tells them
//   chunks      frames * channels work planes count per volume against SC_POISSON_MAX_PLANES;
//   geometry    one work plane per (volume, channel), its frames stacked along y: alpha, beta and the stop rule's norm are one per
//               (volume, channel), summed over all its frames, with the shared launches unchanged;
//   statistics  k_volume_stats; a volume with a state that is not 0, 1 or 2, an invalid weight where one is read, or -- without any
//               Dirichlet line -- a channel with UNKNOWN pixels that no KNOWN neighbour in space or time and no weight pins anywhere in
//               the volume gets SC_ERR_BAD_ARG and leaves;
//   constants   w-bar = precond_lambda, or (sum of w + sum of the UNKNOWN - KNOWN links, spatial 1 and temporal tau) / (UNKNOWN pixels)
//               over the chunk's remaining volumes;
//   set-up      k_volume_setup;   operator   k_volume_op;   output   k_volume_out;
//   M^-1        k_volume_dct along the frames, one direct_jobs_solve over all frames * channels * volumes planes with the shift
//               w-bar + tau (2 - 2 cos(pi k / frames)) of mode k, k_volume_dct transposed: exact for constant coefficients.
#include "sc_pcg.h"
#include <algorithm>
#include <cassert>
#include <cmath>
#include <vector>

using namespace sc;

namespace {

int volume_validate(const sc_volume_params *p, const sc_poisson_layout *l, const char **why)
{
    const char *dummy;
    if (!why) why = &dummy;
    const char *own = !p ? nullptr : !std::isfinite(p->tol) ? "tol must be finite"
                    : !std::isfinite(p->precond_lambda) ? "precond_lambda must be finite"
                    : !(std::isfinite(p->tau) && p->tau > 0.f) ? "tau must be finite and > 0"
                    : p->frames < 2 ? "a volume has at least 2 frames" : nullptr;
    const int rc = family_validate(p ? &p->kind : nullptr, l, own,
                                   "a volume solve is preconditioned by a direct solve: at most 8192 unknowns (pixels - 2) per side", why);
    if (rc) return rc;
    if ((long long)p->frames * l->channels > SC_POISSON_MAX_PLANES) {
        *why = "frames * channels must be at most SC_POISSON_MAX_PLANES";
        return SC_ERR_BAD_SIZE;
    }
    if (p->frame_stride < (long long)poisson_span(l)) { *why = "frame_stride is less than the span of one frame: frames would overlap"; return SC_ERR_BAD_ARG; }
    if ((unsigned __int128)p->frame_stride * (unsigned)p->frames >= ((unsigned __int128)1 << 60)) { *why = "the volume spans more than 2^60 floats"; return SC_ERR_BAD_ARG; }
    return SC_OK;
}

constexpr const char *METHOD_WHY = "a volume solve is solved by SC_METHOD_AUTO and SC_METHOD_FFT only (conjugate gradients preconditioned by the direct solve)";
constexpr const char *FP64_WHY = "a volume solve with SC_FLAG_FFT_FP64: at most 4096 unknowns per axis";

int carries_of(bool weight) { return FLOAT_DATA | FLOAT_STATE | FLOAT_GT | (weight ? FLOAT_WEIGHT : 0); }

struct VolumeOperator : PcgOperator {
    Instance *const I;
    const int T;
    const long long fs;
    const float tau, plam;
    const float *const *all_w = nullptr, *const *all_st = nullptr, *const *all_gt = nullptr;
    std::vector<const float *> dw, dst, dgt;      // the chunk's; behind judge: of the volumes that stay, in front
    int kept = 0;
    double wsum = 0.0, unknowns = 0.0, uksum = 0.0;      // of the volumes that stay
    VolumeOperator(Instance *I_, const sc_volume_params *p)
        : PcgOperator(VOLUME_STATS), I(I_), T(p->frames), fs(p->frame_stride), tau(p->tau), plam(p->precond_lambda) {}
    VolumeGeo geo(const PcgGeo &wg) const { return VolumeGeo{ T, wg.ny / T, fs, tau }; }
    void bind(const float *const *w, const float *const *, const float *const *) override { all_w = w; }
    void bind_state(const float *const *st) override { all_st = st; }
    void bind_gt(const float *const *gt) override { all_gt = gt; }
    int chunk_planes(int C) const override { return C * T; }
    PcgGeo work_geo(const MixedGeo &mg) const override
    {
        MixedGeo tall = mg;
        tall.ny = mg.ny * T;
        return pcg_geo(tall);
    }
    void begin(int i0, int m) override
    {
        dw.assign(all_w + i0, all_w + i0 + m);
        dst.assign(all_st + i0, all_st + i0 + m);
        dgt.assign(all_gt + i0, all_gt + i0 + m);
        kept = 0;
        wsum = unknowns = uksum = 0.0;
    }
    void stats(const PoissonGeo &g, const PcgGeo &wg, int m, double *d_stats, hipStream_t s) override
    {
        launch_volume_stats(g, wg, geo(wg), dj.data(), dw.data(), dst.data(), m, d_stats, s);
    }
    const char *judge(const PoissonGeo &g, int k, const double *st, int parts, bool no_dirichlet) override
    {
        double job[VOLUME_STATS] = {};
        bool loose = false;
        for (int c = 0; c < g.C; ++c) {      // a plane is the channel's whole volume: the pin check is the volume's, not a frame's
            const double *plane = st + (size_t)c * PCG_PARTS * VOLUME_STATS;
            double f[VOLUME_STATS];
            for (int i = 0; i < VOLUME_STATS; ++i) job[i] += f[i] = stat_sum(plane, parts, i);
            loose = loose || (no_dirichlet && f[2] > 0.0 && !(f[3] > 0.0) && !(f[0] > 0.0));
        }
        if (job[4] != 0.0) return "a state element is not 0, 1 or 2";
        if (job[1] != 0.0 || !std::isfinite(job[0])) return "a weight is negative or not finite";
        if (loose) return "nothing pins the channel: no Dirichlet line, no UNKNOWN - KNOWN link in space or time and no data weight";
        dw[kept] = dw[k];
        dgt[kept] = dgt[k];
        dst[kept++] = dst[k];
        wsum += job[0];
        unknowns += job[2];
        uksum += job[3];
        return nullptr;
    }
    // w-bar; the DCT table and the modes' shifts of this chunk go to the device here
    float precond_constant(const PoissonGeo &g, const PcgGeo &wg, int mv) override
    {
        // (a chunk without any UNKNOWN pixel: b = 0 on every plane, any regular M serves)
        const double wbar = plam > 0.f ? (double)plam : unknowns > 0.0 ? (wsum + uksum) / unknowns : 1.0;
        // without a Dirichlet line the rectangle's A is singular: judge kept only volumes whose every channel is pinned
        assert(!(mixed_zero_eig(wg.ax) && mixed_zero_eig(wg.ay)) || wbar > 0.0);
        launch_volume_tables(T, g.C * mv, wbar, (double)tau, table(), shifts(), I->stream);
        return (float)wbar;
    }
    // PcgState::tab: the shifts (double, planes * T of them at most SC_POISSON_MAX_PLANES) | the T x T table (float)
    double *shifts() const { return (double *)I->pcg->tab.p; }
    float *table() const { return (float *)(shifts() + SC_POISSON_MAX_PLANES); }
    int setup(const PoissonGeo &g, const PcgGeo &wg, bool lap, int mv, float *R, double *bb) override
    {
        PcgState &S = *I->pcg;
        int rc;
        for (DevBuf *b : { &S.e, &S.s, &S.dg, &S.f, &S.dct })
            if ((rc = ensure(I, *b, sizeof(float) * (size_t)wg.stride * g.C * mv, false))) return rc;
        if ((rc = ensure(I, S.tab, sizeof(double) * SC_POISSON_MAX_PLANES + sizeof(float) * (size_t)T * T, false))) return rc;
        launch_volume_setup(g, wg, geo(wg), lap, dj.data(), dw.data(), dst.data(), dgt.data(), mv, R, (float *)S.e.p, (float *)S.s.p, (float *)S.f.p,
                            (float *)S.dg.p, bb, I->stream);
        return SC_OK;
    }
    void apply(const PcgGeo &wg, int planes, bool residual, const float *P, float *Q, double *parts, hipStream_t s) override
    {
        PcgState &S = *I->pcg;
        launch_volume_op(wg, geo(wg), planes, residual, P, (const float *)S.e.p, (const float *)S.s.p, (const float *)S.f.p, (const float *)S.dg.p, Q,
                         parts, s);
    }
    // out = M^-1 in: forward along the frames into PcgState::dct, every mode's screened solve there in place (the first transform launch
    // has read a plane before the last one writes it), back into out.  A work plane is one job of T channels, a frame apart.
    int precond(const PcgChunk &c, float, bool fp64, const float *in, float *out) override
    {
        const PcgGeo &wg = c.wg;
        const VolumeGeo vg = geo(wg);
        float *X = (float *)I->pcg->dct.p;
        launch_volume_dct(wg, vg, c.planes, false, table(), in, X, I->stream);
        const PoissonGeo pg{ c.g.W, c.g.H, T, 1, (long long)wg.nx, (long long)wg.nx * vg.ny };
        const long long shift = (long long)wg.x0 + (long long)wg.y0 * wg.nx;
        std::vector<PoissonJobDev> pj(c.planes);
        for (int k = 0; k < c.planes; ++k) {
            float *x = X + (long long)k * wg.stride - shift;
            pj[k] = PoissonJobDev{ nullptr, nullptr, x, nullptr, x };
        }
        const int rc = direct_jobs_solve(I, pg, c.mg, true, pj.data(), c.planes, fp64, 0.f, shifts());
        if (rc) return rc;
        launch_volume_dct(wg, vg, c.planes, true, table(), X, out, I->stream);
        return SC_OK;
    }
    void out(const PoissonGeo &g, const PcgGeo &wg, int mv, const float *U, hipStream_t s) override
    {
        launch_volume_out(g, wg, geo(wg), dj.data(), dst.data(), mv, U, s);
    }
};

PcgCall volume_call(int kind, const sc_volume_params *p) { return PcgCall{ kind, p->tol, p->max_iters, 400, p->frames, p->frame_stride }; }

} // namespace

extern "C" {

int sc_hip_volume_check(const sc_volume_params *p, const sc_poisson_layout *l)
{
    return volume_validate(p, l, nullptr);
}

int sc_hip_volume_device(void *inst, const sc_volume_params *p, const sc_poisson_layout *l, sc_volume_job *jobs, int n, bool bSync)
{
    Instance *I;
    int kind, rc = pcg_begin(inst, p, l, volume_validate, METHOD_WHY, FP64_WHY, I, kind);
    if (rc) return rc;
    // the data term: all volumes or none, as the first one has it; a volume that differs is refused
    const bool weight = jobs && n > 0 && jobs[0].weight;
    VolumeOperator op(I, p);
    return pcg_device_call(I, volume_call(kind, p), l, carries_of(weight), jobs, n, [weight](const sc_volume_job &j) {
        const bool stray = !weight && j.weight;      // (refused through its data pointer)
        FloatArrays a{ j.gx, j.gy, j.lap, stray ? nullptr : j.data, j.weight, j.boundary, j.out, nullptr, nullptr, j.state };
        a.gt = j.gt;
        return a; }, op, bSync);
}

int sc_hip_volume(void *inst, const sc_volume_params *p, const sc_poisson_layout *l, const float *gx, const float *gy, const float *gt,
                  const float *lap, const float *data, const float *state, const float *weight, const float *boundary, float *out)
{
    Instance *I;
    int kind, rc = pcg_begin(inst, p, l, volume_validate, METHOD_WHY, FP64_WHY, I, kind);
    if (rc) return rc;
    VolumeOperator op(I, p);
    FloatArrays a{ gx, gy, lap, data, weight, boundary, out, nullptr, nullptr, state };
    a.gt = gt;
    return pcg_host_call(I, volume_call(kind, p), l, carries_of(weight != nullptr), a, op);
}

} // extern "C"
