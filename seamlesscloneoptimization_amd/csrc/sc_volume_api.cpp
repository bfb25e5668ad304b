// sc_volume_api.cpp -- the volume solves on float32 frame stacks (sc_hip_volume_check, sc_hip_volume_device, sc_hip_volume, and the
// same three of sc_hip_volume_wls and of sc_hip_volume_robust): the region call's problem on every one of `frames` images that share a layout, coupled by temporal
// links (sc_volume.hip: the system and its work planes).  sc_hip_volume has unit spatial links, temporal links of the constant weight
// tau and free ends of time; sc_hip_volume_wls takes per-link weights smooth_x, smooth_y, smooth_t and, if asked, periodic time.  One
// operator serves both: sc_hip_volume is the call without link arrays under free time.  The entry code and the iteration are the
// shared ones (sc_pcg.h; the front end with FLOAT_STATE | FLOAT_GT, FLOAT_SMOOTH and FLOAT_SMOOTH_T where the call has the arrays, the
// call's frame stride and the frames its temporal arrays hold); VolumeOperator tells them
//   chunks      frames * channels work planes count per volume against SC_POISSON_MAX_PLANES;
//   geometry    one work plane per (volume, channel), its frames stacked along y: alpha, beta and the stop rule's norm are one per
//               (volume, channel), summed over all its frames, with the shared launches unchanged;
//   statistics  k_volume_stats; a volume with a state that is not 0, 1 or 2, an invalid weight or link where one is read, or -- without
//               any Dirichlet line -- a channel with UNKNOWN pixels that no KNOWN neighbour in space or time and no weight pins anywhere
//               in the volume gets SC_ERR_BAD_ARG and leaves;
//   constants   over the chunk's remaining volumes: s-bar = precond_smooth, or the mean of the spatial links live in the region (1
//               without link arrays); tau-bar = precond_tau, or the mean of the live temporal links (tau without smooth_t); w-bar =
//               precond_lambda, or (sum of w + sum of the UNKNOWN - KNOWN links' weights) / (UNKNOWN pixels);
//   set-up      k_volume_setup;   operator   k_volume_op;   output   k_volume_out;
//   M^-1        M = s-bar A - w-bar + tau-bar A_t: k_volume_dct along the frames (the DCT-II; periodic time: the Hartley table), one
//               direct_jobs_solve over all frames * channels * volumes planes with the shift (w-bar + tau-bar mu_k) / s-bar of mode k,
//               k_volume_dct transposed: exact for constant coefficients.  The factor 1 / s-bar goes once on u0 (scale_start).
// All six side arrays of a volume come in PcgOperator::ds beside the job (NULL where the call carries none: the front end's word).
// sc_hip_volume_robust (its own three entries, below): Lp penalties on the spatial links, the temporal links and the data term.  Round 0
// is sc_hip_volume_wls's chunk with default precond_*; the chunk, its rounds and the round itself are sc_robust_api.cpp's (robust_chunk,
// RobustRounds::reweigh), for which VolumeRobustOperator provides the launch (k_volume_robust_setup, sc_volume_robust.hip) and takes
// the round's sums in place of the statistics'.
// sc_hip_volume_coupled (its own three entries, last): the robust volume call with a coupling -- SC_VOLUME_COUPLE_SPACE, _TIME, _CHANNELS
// -- beside the parameters, which the operator takes as launch words (ROBUST_ISO, ROBUST_TIME, ROBUST_JOINT); a round under an effective
// coupling is two launches (k_volume_robust_rho, k_volume_robust_setup_rho, sc_volume_coupled.hip) with PcgState::rho between them.
// sc_hip_volume_flow (its own three entries, behind sc_hip_volume_wls's): sc_hip_volume_wls with every temporal link along a flow.
// VolumeFlowOperator is VolumeOperator with the volumes' link planes (PcgState::lnk; sc_volume_flow.hip: the matching) built in front
// of the statistics -- and again in front of the set-up where a volume has left, since the planes lie in the order of the volumes that
// stay --, the statistics and the set-up in their flow forms, k_volume_flow_op, and M^-1 untouched: straight time links.  The two flow
// arrays come through the front end like every side array (FLOAT_FLOW, PcgCall::flow_floats: dense, no channel axis, their own
// length) and the call through volume_device_call and pcg_host_call; a volume whose unknowns the link planes' 32 bits cannot index is
// refused before anything runs (SC_ERR_BAD_SIZE), by sc_hip_volume_flow_check and by a call that carries a flow.
// sc_hip_volume_subflow (its own three entries, behind sc_hip_volume_flow's): the flow call with a real-valued flow, every temporal link a
// bilinear stencil.  VolumeSubflowOperator is VolumeOperator with the volumes' transposed links (PcgState::lnk; sc_volume_subflow.hip: no
// matching, a stable sort by target) built where VolumeFlowOperator builds its planes, the statistics and the set-up in their sub-pixel
// forms and the operator in product form (k_subflow_rho, k_subflow_op; PcgState::rho: rho | LT); the same front end, check and size rule.
// sc_hip_volume_flow_robust (its own three entries, behind sc_hip_volume_robust's): the robust volume call with every temporal link --
// its base weight, its gt, its penalty -- on the flow call's matched link.  VolumeFlowRobustOperator is VolumeFlowOperator (the matching,
// the statistics and their judgement, round 0's set-up, k_volume_flow_op) with the robust volume operator's rounds, whose launch is
// k_volume_flow_robust_setup (sc_volume_flow_robust.hip) through the same link planes, re-matched where a volume has left.
// sc_hip_volume_subflow_robust (its own three entries, behind sc_hip_volume_flow_robust's): the robust volume call with every temporal
// link -- its base weight, its gt, its penalty -- on the sub-pixel call's bilinear link.  VolumeSubflowRobustOperator is
// VolumeSubflowOperator (the transposed links, the statistics, round 0's set-up, k_subflow_rho and k_subflow_op) with the robust volume
// operator's rounds, whose launch is sc_volume_subflow_robust.hip's two kernels: they rewrite LT and SG in PcgState::rho and the spatial
// planes, the operator's launches stay as they are.
#include "sc_pcg.h"
#include <algorithm>
#include <cassert>
#include <cmath>
#include <vector>

using namespace sc;

namespace {

int volume_wls_validate(const sc_volume_wls_params *p, const sc_poisson_layout *l, const char **why)
{
    const char *dummy;
    if (!why) why = &dummy;
    const char *own = !p ? nullptr : !std::isfinite(p->tol) ? "tol must be finite"
                    : !std::isfinite(p->precond_lambda) ? "precond_lambda must be finite"
                    : !std::isfinite(p->precond_smooth) ? "precond_smooth must be finite"
                    : !std::isfinite(p->precond_tau) ? "precond_tau must be finite"
                    : !(std::isfinite(p->tau) && p->tau > 0.f) ? "tau must be finite and > 0"
                    : (p->time_periodic != 0 && p->time_periodic != 1) ? "time_periodic must be 0 or 1"
                    : p->frames < 2 ? "a volume has at least 2 frames"
                    : (p->time_periodic && p->frames < 3) ? "periodic time needs at least 3 frames" : nullptr;
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

// sc_hip_volume's parameters as the general call's: no constants for link arrays, free time
sc_volume_wls_params wls_params_of(const sc_volume_params *p)
{
    return sc_volume_wls_params{ p->kind, p->frames, p->frame_stride, p->tau, 0, p->tol, p->max_iters, p->precond_lambda, 0.f, 0.f };
}

int volume_validate(const sc_volume_params *p, const sc_poisson_layout *l, const char **why)
{
    if (!p) return volume_wls_validate(nullptr, l, why);
    const sc_volume_wls_params q = wls_params_of(p);
    return volume_wls_validate(&q, l, why);
}

constexpr const char *METHOD_WHY = "a volume solve is solved by SC_METHOD_AUTO and SC_METHOD_FFT only (conjugate gradients preconditioned by the direct solve)";
constexpr const char *FLOW_PAIR_WHY = "flow_x and flow_y go together (both NULL: straight temporal links)";
constexpr const char *FLOW_SIZE_WHY = "a flow volume solve indexes a volume's unknowns with 32 bits: unknowns per frame * frames must be below 2^31 - 1";
constexpr const char *FP64_WHY = "a volume solve with SC_FLAG_FFT_FP64: at most 4096 unknowns per axis";

int carries_of(bool weight, bool links, bool tlinks)
{
    return FLOAT_DATA | FLOAT_STATE | FLOAT_GT | (weight ? FLOAT_WEIGHT : 0) | (links ? FLOAT_SMOOTH : 0) | (tlinks ? FLOAT_SMOOTH_T : 0);
}

} // namespace

namespace sc {

void VolumeOperator::begin() { wsum = unknowns = uksum = ssum = scount = tsum = tcount = 0.0; }

void VolumeOperator::stats(const PoissonGeo &g, const PcgGeo &wg, int m, double *d_stats, hipStream_t s)
{
    launch_volume_stats(g, wg, geo(wg), dj.data(), ds.data(), m, d_stats, s, nstat == VOLUME_STATS);
}

const char *VolumeOperator::judge(const PoissonGeo &g, int k, const double *st, int parts, bool no_dirichlet)
{
    double job[VOLUME_STATS] = {};
    const int nf = std::min(nstat, (int)VOLUME_STATS);      // (a call without link arrays under free time: the link fields do not exist)
    bool loose = false;
    for (int c = 0; c < g.C; ++c) {      // a plane is the channel's whole volume: the pin check is the volume's, not a frame's
        const double *plane = st + (size_t)c * PCG_PARTS * nstat;
        double f[VOLUME_STATS] = {};
        for (int i = 0; i < nf; ++i) job[i] += f[i] = stat_sum(plane, parts, i);
        loose = loose || (no_dirichlet && f[2] > 0.0 && !(f[3] > 0.0) && !(f[0] > 0.0));
    }
    if (job[4] != 0.0) return "a state element is not 0, 1 or 2";
    if (job[1] != 0.0 || !std::isfinite(job[0])) return "a weight is negative or not finite";
    if (job[7] != 0.0 || !std::isfinite(job[5])) return "a spatial link weight live in the region is not finite or not > 0";
    if (job[10] != 0.0 || !std::isfinite(job[8])) return "a live temporal link weight is not finite or not > 0";
    if (loose) return "nothing pins the channel: no Dirichlet line, no UNKNOWN - KNOWN link in space or time and no data weight";
    wsum += job[0];
    unknowns += job[2];
    uksum += job[3];
    ssum += job[5];
    scount += job[6];
    tsum += job[8];
    tcount += job[9];
    return nullptr;
}

float VolumeOperator::precond_constant(const PoissonGeo &g, const PcgGeo &wg, int mv)
{
    const double sbar = psmooth > 0.f ? (double)psmooth : !links || !(scount > 0.0) ? 1.0 : ssum / scount;
    const double tbar = ptau > 0.f ? (double)ptau : !tlinks || !(tcount > 0.0) ? (double)tau : tsum / tcount;
    // (a chunk without any UNKNOWN pixel: b = 0 on every plane, any regular M serves)
    const double wbar = plam > 0.f ? (double)plam : unknowns > 0.0 ? (wsum + uksum) / unknowns : 1.0;
    // without a Dirichlet line the rectangle's A is singular: judge kept only volumes whose every channel is pinned
    assert(!(mixed_zero_eig(wg.ax) && mixed_zero_eig(wg.ay)) || wbar > 0.0);
    u0_scale = (float)(1.0 / sbar);
    launch_volume_tables(T, g.C * mv, periodic, wbar, tbar, sbar, table(), shifts(), I->stream);
    return (float)wbar;
}

// the factor 1 / s-bar that the modes' solves leave out (1: no launch)
void VolumeOperator::scale_start(const PcgGeo &wg, int planes, float *U, hipStream_t s)
{
    if (u0_scale != 1.f) launch_pcg_scale(wg, planes, U, u0_scale, s);
}

int VolumeOperator::setup(const PoissonGeo &g, const PcgGeo &wg, bool lap, int mv, float *R, double *bb)
{
    PcgState &S = *I->pcg;
    int rc;
    for (DevBuf *b : { &S.e, &S.s, &S.dg, &S.f, &S.dct })
        if ((rc = ensure(I, *b, sizeof(float) * (size_t)wg.stride * g.C * mv, false))) return rc;
    if ((rc = ensure(I, S.tab, sizeof(double) * SC_POISSON_MAX_PLANES + sizeof(float) * (size_t)T * T, false))) return rc;
    launch_volume_setup(g, wg, geo(wg), lap, dj.data(), ds.data(), mv, R, (float *)S.e.p, (float *)S.s.p, (float *)S.f.p, (float *)S.dg.p, bb,
                        I->stream);
    return SC_OK;
}

void VolumeOperator::apply(const PcgGeo &wg, int planes, bool residual, const float *P, float *Q, double *parts, hipStream_t s)
{
    PcgState &S = *I->pcg;
    launch_volume_op(wg, geo(wg), planes, residual, P, (const float *)S.e.p, (const float *)S.s.p, (const float *)S.f.p, (const float *)S.dg.p, Q,
                     parts, s);
}

// out = M^-1 in: forward along the frames into PcgState::dct, every mode's screened solve there in place (the first transform launch
// has read a plane before the last one writes it), back into out.  A work plane is one job of T channels, a frame apart.
int VolumeOperator::precond(const PcgChunk &c, float, bool fp64, const float *in, float *out)
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

void VolumeOperator::out(const PoissonGeo &g, const PcgGeo &wg, int mv, const float *U, hipStream_t s)
{
    launch_volume_out(g, wg, geo(wg), dj.data(), ds.data(), mv, U, s);
}

} // namespace sc

namespace {

PcgCall volume_call(int kind, const sc_volume_wls_params *p)
{
    return PcgCall{ kind, p->tol, p->max_iters, 400, p->frames, p->frame_stride, p->time_periodic ? p->frames : p->frames - 1 };
}

// the device call of the three families, on any one's jobs (links_of(job): its three link arrays and lap, NULLs where its job has none;
// Op: the family's operator, made from the call's parameters and what its volumes carry); the data term and the link arrays: all
// volumes or none, as the first one has them -- smooth_x / smooth_y and smooth_t judged separately; a volume that differs is refused
// with a reason of its own (as one with exactly one of smooth_x / smooth_y is by the front end).  The flow call's two flow arrays
// likewise (call.flow_floats > 0: the first volume has them); exactly one of the two is refused whatever the first volume has.
struct VolumeLinks { const float *sx, *sy, *smt, *lap, *fx = nullptr, *fy = nullptr; };
template <class Op, class Params, class Job, class LinksOf>
int volume_device_call(Instance *I, const PcgCall &call, const Params *p, const sc_poisson_layout *l, Job *jobs, int n, bool bSync, LinksOf links_of,
                       PcgChunkFn chunk = nullptr)
{
    const VolumeLinks first = jobs && n > 0 ? links_of(jobs[0]) : VolumeLinks{ nullptr, nullptr, nullptr, nullptr };
    const bool weight = jobs && n > 0 && jobs[0].weight, links = first.sx || first.sy, tlinks = first.smt != nullptr;
    const bool flow = call.flow_floats > 0;
    Op op(I, p, links, tlinks);
    return pcg_device_call(I, call, l, carries_of(weight, links, tlinks) | (flow ? FLOAT_FLOW : 0), jobs, n, [=](const Job &j) {
        const VolumeLinks k = links_of(j);
        FloatArrays a{ j.gx, j.gy, k.lap, j.data, j.weight, j.boundary, j.out, k.sx, k.sy, j.state };
        a.gt = j.gt;
        a.smooth_t = k.smt;
        a.flow_x = k.fx;
        a.flow_y = k.fy;
        a.refuse = !weight && j.weight ? "a volume has a weight where the first volume of the call has none"
                 : !links && (k.sx || k.sy) ? "a volume has smooth_x / smooth_y where the first volume of the call has none"
                 : !tlinks && k.smt ? "a volume has smooth_t where the first volume of the call has none"
                 : !k.fx != !k.fy ? FLOW_PAIR_WHY
                 : !flow && k.fx ? "a volume has a flow where the first volume of the call has none"
                 : flow && !k.fx ? "a volume has no flow where the first volume of the call has one" : nullptr;
        return a; }, op, bSync, chunk);
}

// ---- the flow volume call (nround_: the sums of a round, for the robust flow call that stands on this operator)
struct VolumeFlowOperator : VolumeOperator {
    int built = -1;      // the volumes whose link planes stand, in dj's order
    VolumeFlowOperator(Instance *I_, const sc_volume_wls_params *p, bool links_, bool tlinks_, int nround_ = 0)
        : VolumeOperator(I_, p, links_, tlinks_, nround_, OwnStats{ VOLUME_FLOW_STATS }) {}
    // (the entries have made PcgState::lnk large enough for a chunk: flow_links_ensure)
    int *fwd() const { return (int *)I->pcg->lnk.p; }
    int *bwd(const PcgGeo &wg) const { return fwd() + flow_link_stride(wg) * std::max(1, SC_POISSON_MAX_PLANES / (chan * T)); }
    int chan = 1;        // the call's channels: the planes that share a volume's link planes
    void begin() override { VolumeOperator::begin(); built = -1; }
    void match(const PoissonGeo &g, const PcgGeo &wg, int m, hipStream_t s)
    {
        chan = g.C;
        launch_flow_links(g, wg, geo(wg), ds.data(), m, fwd(), bwd(wg), s);
        built = m;
    }
    void stats(const PoissonGeo &g, const PcgGeo &wg, int m, double *d_stats, hipStream_t s) override
    {
        match(g, wg, m, s);
        launch_volume_flow_stats(g, wg, geo(wg), dj.data(), ds.data(), m, fwd(), bwd(wg), d_stats, s);
    }
    const char *judge(const PoissonGeo &g, int k, const double *st, int parts, bool no_dirichlet) override
    {
        double frac = 0.0;
        for (int c = 0; c < g.C; ++c) frac += stat_sum(st + (size_t)c * PCG_PARTS * nstat, parts, VOLUME_STATS);
        if (frac != 0.0) return "a flow value is finite and not a whole number";
        return VolumeOperator::judge(g, k, st, parts, no_dirichlet);
    }
    int setup(const PoissonGeo &g, const PcgGeo &wg, bool lap, int mv, float *R, double *bb) override
    {
        PcgState &S = *I->pcg;
        int rc;
        for (DevBuf *b : { &S.e, &S.s, &S.dg, &S.f, &S.dct })
            if ((rc = ensure(I, *b, sizeof(float) * (size_t)wg.stride * g.C * mv, false))) return rc;
        if ((rc = ensure(I, S.tab, sizeof(double) * SC_POISSON_MAX_PLANES + sizeof(float) * (size_t)T * T, false))) return rc;
        if (mv != built) match(g, wg, mv, I->stream);      // a volume left: dj and ds moved up, the planes follow
        launch_volume_flow_setup(g, wg, geo(wg), lap, dj.data(), ds.data(), mv, fwd(), bwd(wg), R, (float *)S.e.p, (float *)S.s.p, (float *)S.f.p,
                                 (float *)S.dg.p, bb, I->stream);
        return SC_OK;
    }
    void apply(const PcgGeo &wg, int planes, bool residual, const float *P, float *Q, double *parts, hipStream_t s) override
    {
        PcgState &S = *I->pcg;
        launch_volume_flow_op(wg, geo(wg), planes, chan, residual, P, (const float *)S.e.p, (const float *)S.s.p, (const float *)S.f.p,
                              (const float *)S.dg.p, fwd(), bwd(wg), Q, parts, s);
    }
};

// the work planes of a flow call's volume, and the call's own refusal of a size (SC_ERR_BAD_SIZE; SC_OK: none)
PcgGeo flow_work_geo(const sc_volume_wls_params *p, const sc_poisson_layout *l, int kind)
{
    return volume_work_geo(poisson_mixed_geo(poisson_free_sides(kind), l->cols, l->rows, poisson_periodic(kind)), p->frames);
}
int volume_flow_validate(const sc_volume_wls_params *p, const sc_poisson_layout *l, const char **why)
{
    const char *dummy;
    if (!why) why = &dummy;
    const int rc = volume_wls_validate(p, l, why);
    if (rc) return rc;
    if (!flow_indexable(flow_work_geo(p, l, poisson_norm_kind(p->kind)))) { *why = FLOW_SIZE_WHY; return SC_ERR_BAD_SIZE; }
    return SC_OK;
}
// the link planes of one chunk: fwd | bwd, each of as many volumes as a chunk holds at most
int flow_links_ensure(Instance *I, const sc_volume_wls_params *p, const sc_poisson_layout *l, int kind)
{
    const int per = std::max(1, SC_POISSON_MAX_PLANES / (l->channels * p->frames));
    return ensure(I, I->pcg->lnk, sizeof(int) * 2 * (size_t)flow_link_stride(flow_work_geo(p, l, kind)) * per, false);
}
// the call of a volume with a flow: volume_call and the floats of one of its dense flow arrays
PcgCall volume_flow_call(int kind, const sc_volume_wls_params *p, const sc_poisson_layout *l)
{
    PcgCall call = volume_call(kind, p);
    call.flow_floats = (size_t)call.tframes * (size_t)l->rows * (size_t)l->cols;
    return call;
}

// ---- the sub-pixel flow volume call: VolumeOperator with the volumes' transposed bilinear links (PcgState::lnk; sc_volume_subflow.hip)
// built in front of the statistics -- and again in front of the set-up where a volume has left --, the statistics and the set-up in
// their sub-pixel forms and the operator in product form: PcgState::rho holds rho | LT per work plane, PcgState::f the mask of the
// UNKNOWN pixels.  M^-1 untouched: straight time links.
// the sub-pixel call's parameters: the WLS volume call's and the volumes the call holds (the link storage is sized by them)
struct VolumeSubflowParams { const sc_volume_wls_params *p; int volumes; };
// the volumes a chunk of the call holds at most: a chunk's share of SC_POISSON_MAX_PLANES, or the call's volumes where those are fewer
int subflow_chunk_volumes(int volumes, int channels, int frames)
{
    return std::max(1, std::min(volumes, SC_POISSON_MAX_PLANES / (channels * frames)));
}
// (nround_: the sums of a round, for the robust sub-pixel call that stands on this operator)
struct VolumeSubflowOperator : VolumeOperator {
    int built = -1;      // the volumes whose links stand, in dj's order
    int chan = 1;        // the call's channels: the planes that share a volume's links
    size_t lt_at = 0;    // where LT starts in PcgState::rho, in floats
    const int volumes;   // of the call
    VolumeSubflowOperator(Instance *I_, const VolumeSubflowParams *c, bool links_, bool tlinks_, int nround_ = 0)
        : VolumeOperator(I_, c->p, links_, tlinks_, nround_, OwnStats{ VOLUME_STATS }), volumes(c->volumes) {}
    // (the entries have made PcgState::lnk large enough for a chunk: subflow_links_ensure)
    SubflowStore st{};   // where they lie in PcgState::lnk (build)
    void begin() override { VolumeOperator::begin(); built = -1; }
    void build(const PoissonGeo &g, const PcgGeo &wg, int m, hipStream_t s)
    {
        chan = g.C;
        st = subflow_store(wg, subflow_chunk_volumes(volumes, chan, T));      // (subflow_links_ensure's count: ent and fw lie behind all its volumes' off)
        launch_subflow_links(g, wg, geo(wg), ds.data(), m, st, I->pcg->lnk.p, s);
        built = m;
    }
    void stats(const PoissonGeo &g, const PcgGeo &wg, int m, double *d_stats, hipStream_t s) override
    {
        build(g, wg, m, s);
        launch_volume_subflow_stats(g, wg, geo(wg), dj.data(), ds.data(), m, st, I->pcg->lnk.p, d_stats, s);
    }
    int setup(const PoissonGeo &g, const PcgGeo &wg, bool lap, int mv, float *R, double *bb) override
    {
        PcgState &S = *I->pcg;
        int rc;
        for (DevBuf *b : { &S.e, &S.s, &S.dg, &S.f, &S.dct })
            if ((rc = ensure(I, *b, sizeof(float) * (size_t)wg.stride * g.C * mv, false))) return rc;
        lt_at = (size_t)wg.stride * g.C * mv;
        // (a call with rounds: a round's temporal partials lie behind rho | LT)
        if ((rc = ensure(I, S.rho, sizeof(float) * 2 * lt_at + (nround ? sizeof(double) * subflow_robust_partials(g.C * mv) : 0), false))) return rc;
        if ((rc = ensure(I, S.tab, sizeof(double) * SC_POISSON_MAX_PLANES + sizeof(float) * (size_t)T * T, false))) return rc;
        if (mv != built) build(g, wg, mv, I->stream);      // a volume left: dj and ds moved up, the links follow
        float *rho = (float *)S.rho.p;
        launch_volume_subflow_setup(g, wg, geo(wg), lap, dj.data(), ds.data(), mv, st, S.lnk.p, rho + lt_at, rho, R, (float *)S.e.p, (float *)S.s.p,
                                    (float *)S.f.p, (float *)S.dg.p, bb, I->stream);
        return SC_OK;
    }
    void apply(const PcgGeo &wg, int planes, bool residual, const float *P, float *Q, double *parts, hipStream_t s) override
    {
        PcgState &S = *I->pcg;
        float *rho = (float *)S.rho.p;
        launch_volume_subflow_op(wg, geo(wg), planes, chan, residual, st, S.lnk.p, P, (const float *)S.e.p, (const float *)S.s.p, (const float *)S.f.p,
                                 (const float *)S.dg.p, rho + lt_at, rho, Q, parts, s);
    }
};

// the links of one chunk and the build's scratch
int subflow_links_ensure(Instance *I, const sc_volume_wls_params *p, const sc_poisson_layout *l, int kind, int volumes)
{
    return ensure(I, I->pcg->lnk, subflow_store(flow_work_geo(p, l, kind), subflow_chunk_volumes(volumes, l->channels, p->frames)).total, false);
}

// ---- the robust volume call: the volume operator with the links of the current round -- round 0 from the caller's arrays (the WLS
// volume call's system, default precond_*), later rounds from the iterate (k_volume_robust_setup).  Its statistics are always the full
// form: a round's means divide by the counts of live links.
sc_volume_wls_params wls_params_of(const sc_volume_robust_params *p)
{
    return sc_volume_wls_params{ p->kind, p->frames, p->frame_stride, p->tau, p->time_periodic, p->tol, p->max_iters, 0.f, 0.f, 0.f };
}

int volume_robust_validate(const sc_volume_robust_params *p, const sc_poisson_layout *l, const char **why)
{
    const char *dummy;
    if (!why) why = &dummy;
    if (!p) return volume_wls_validate(nullptr, l, why);
    const sc_volume_wls_params q = wls_params_of(p);          // (the coupling bits stay in kind: the family's kinds refuse them)
    const int rc = volume_wls_validate(&q, l, why);
    if (rc) return rc;
    const char *own = robust_penalties_why({ { p->p_grad, p->eps_grad }, { p->p_time, p->eps_time }, { p->p_data, p->eps_data } },
                                           "p_grad, p_time and p_data must lie in (0, 2]",
                                           "eps_grad, eps_time and eps_data must be finite and > 0 where their exponent is not 2", p->tol, p->round_tol,
                                           p->kind);
    if (!own && (p->kind & COUPLING_BITS)) own = "the coupled forms are not offered on volumes";
    if (own) { *why = own; return SC_ERR_BAD_ARG; }
    return SC_OK;
}

// the coupled volume call's parameters: the robust volume call's and the coupling as the launches' words
struct VolumeCoupledParams { const sc_volume_robust_params *p; int bits; };
int coupling_words(int coupling)
{
    return ((coupling & SC_VOLUME_COUPLE_SPACE) ? ROBUST_ISO : 0) | ((coupling & SC_VOLUME_COUPLE_TIME) ? ROBUST_TIME : 0) |
           ((coupling & SC_VOLUME_COUPLE_CHANNELS) ? ROBUST_JOINT : 0);
}

// Sums: w' | spatial links | temporal links | UNKNOWN - KNOWN | energy.  (kind carries no coupling bits: the check refuses them; the
// coupled call's come beside the parameters.)
struct VolumeRobustOperator final : VolumeOperator, RobustRounds {
    const bool base_links, base_tlinks;
    VolumeRobustOperator(Instance *I_, const sc_volume_robust_params *p, bool links_, bool tlinks_)
        : VolumeRobustOperator(I_, p, wls_params_of(p), links_, tlinks_, 0) {}
    VolumeRobustOperator(Instance *I_, const VolumeCoupledParams *c, bool links_, bool tlinks_)
        : VolumeRobustOperator(I_, c->p, wls_params_of(c->p), links_, tlinks_, c->bits) {}
    VolumeRobustOperator(Instance *I_, const sc_volume_robust_params *p, const sc_volume_wls_params &q, bool links_, bool tlinks_, int words)
        : VolumeOperator(I_, &q, links_, tlinks_, VOLUME_ROBUST_SUMS + (words ? 1 : 0), true),
          RobustRounds(robust_term(p->p_grad, p->eps_grad), robust_term(p->p_data, p->eps_data), robust_term(p->p_time, p->eps_time), p->max_rounds,
                       p->round_tol, p->kind, VOLUME_ROBUST_SUMS, words),
          base_links(links_), base_tlinks(tlinks_) {}
    RobustRounds *rounds() override { return this; }
    // the coupling that changes anything: SPACE and TIME not with p_grad = 2 (TIME: p_time = p_grad), CHANNELS not on one channel and
    // not with p_grad = p_time = 2
    int coupling(int C) const override
    {
        int b = bits;
        if (grad.mode == 0) b &= ~(ROBUST_ISO | ROBUST_TIME);
        if (C == 1 || (grad.mode == 0 && time.mode == 0)) b &= ~ROBUST_JOINT;
        return b;
    }
    void begin() override
    {
        VolumeOperator::begin();
        links = base_links;          // round 0 of a new chunk: the caller's arrays again
        tlinks = base_tlinks;
    }
    int launch(PcgChunk &c, int cpl, double *esum) override
    {
        PcgState &S = *I->pcg;
        if (cpl) {
            const VolumeGeo vg = geo(c.wg);
            const int rc = ensure(I, S.rho, sizeof(float) * volume_rho_floats(volume_rho_geo(c.wg, vg, grad, time, cpl), c.g.C, c.mv, cpl), false);
            if (rc) return rc;
            launch_volume_robust_coupled(c.g, c.wg, vg, dj.data(), ds.data(), c.mv, grad, time, data, cpl, c.U, (float *)S.rho.p, c.R, (float *)S.e.p,
                                         (float *)S.s.p, (float *)S.f.p, (float *)S.dg.p, c.d_bb, c.d_round, esum, I->stream);
            return SC_OK;
        }
        launch_volume_robust_setup(c.g, c.wg, geo(c.wg), dj.data(), ds.data(), c.mv, grad, time, data, c.U, c.R, (float *)S.e.p, (float *)S.s.p,
                                   (float *)S.f.p, (float *)S.dg.p, c.d_bb, c.d_round, I->stream);
        return SC_OK;
    }
    void take(const double *t) override { wsum = t[0]; ssum = t[1]; tsum = t[2]; uksum = t[3]; links = tlinks = true; }
};

// ---- the robust flow volume call: the flow operator -- its matching, statistics, judgement, round 0's set-up and k_volume_flow_op --
// with the robust volume operator's rounds: a later round's system from the iterate through the link planes
// (k_volume_flow_robust_setup, sc_volume_flow_robust.hip).  The robust flow call has no coupling: its check refuses the bits; the
// coupled flow call's words come beside the parameters as the coupled call's do (VolumeCoupledParams), and a round under an effective
// coupling is the two launches of sc_volume_flow_coupled.hip.
struct VolumeFlowRobustOperator final : VolumeFlowOperator, RobustRounds {
    const bool base_links, base_tlinks;
    VolumeFlowRobustOperator(Instance *I_, const sc_volume_robust_params *p, bool links_, bool tlinks_)
        : VolumeFlowRobustOperator(I_, p, wls_params_of(p), links_, tlinks_, 0) {}
    VolumeFlowRobustOperator(Instance *I_, const VolumeCoupledParams *c, bool links_, bool tlinks_)
        : VolumeFlowRobustOperator(I_, c->p, wls_params_of(c->p), links_, tlinks_, c->bits) {}
    VolumeFlowRobustOperator(Instance *I_, const sc_volume_robust_params *p, const sc_volume_wls_params &q, bool links_, bool tlinks_, int words)
        : VolumeFlowOperator(I_, &q, links_, tlinks_, VOLUME_ROBUST_SUMS + (words ? 1 : 0)),
          RobustRounds(robust_term(p->p_grad, p->eps_grad), robust_term(p->p_data, p->eps_data), robust_term(p->p_time, p->eps_time), p->max_rounds,
                       p->round_tol, p->kind, VOLUME_ROBUST_SUMS, words),
          base_links(links_), base_tlinks(tlinks_) {}
    RobustRounds *rounds() override { return this; }
    // VolumeRobustOperator::coupling's rule
    int coupling(int C) const override
    {
        int b = bits;
        if (grad.mode == 0) b &= ~(ROBUST_ISO | ROBUST_TIME);
        if (C == 1 || (grad.mode == 0 && time.mode == 0)) b &= ~ROBUST_JOINT;
        return b;
    }
    void begin() override
    {
        VolumeFlowOperator::begin();
        links = base_links;          // round 0 of a new chunk: the caller's arrays again
        tlinks = base_tlinks;
    }
    int launch(PcgChunk &c, int cpl, double *esum) override
    {
        PcgState &S = *I->pcg;
        if (c.mv != built) match(c.g, c.wg, c.mv, I->stream);      // the planes lie in the order of the volumes that stay
        if (cpl) {
            const VolumeGeo vg = geo(c.wg);
            const int rc = ensure(I, S.rho, sizeof(float) * volume_rho_floats(volume_rho_geo(c.wg, vg, grad, time, cpl), c.g.C, c.mv, cpl), false);
            if (rc) return rc;
            launch_volume_flow_robust_coupled(c.g, c.wg, vg, dj.data(), ds.data(), c.mv, grad, time, data, cpl, fwd(), bwd(c.wg), c.U, (float *)S.rho.p,
                                              c.R, (float *)S.e.p, (float *)S.s.p, (float *)S.f.p, (float *)S.dg.p, c.d_bb, c.d_round, esum, I->stream);
            return SC_OK;
        }
        launch_volume_flow_robust_setup(c.g, c.wg, geo(c.wg), dj.data(), ds.data(), c.mv, grad, time, data, fwd(), bwd(c.wg), c.U, c.R, (float *)S.e.p,
                                        (float *)S.s.p, (float *)S.f.p, (float *)S.dg.p, c.d_bb, c.d_round, I->stream);
        return SC_OK;
    }
    void take(const double *t) override { wsum = t[0]; ssum = t[1]; tsum = t[2]; uksum = t[3]; links = tlinks = true; }
};

// ---- the robust sub-pixel flow volume call: the sub-pixel operator -- its transposed links, statistics, round 0's set-up, k_subflow_rho
// and k_subflow_op -- with the robust volume operator's rounds: a later round's LT, SG and spatial planes from the iterate
// (sc_volume_subflow_robust.hip).  The call has no coupling: its check refuses the bits.
struct VolumeSubflowRobustParams { const sc_volume_robust_params *p; int volumes; };
struct VolumeSubflowRobustOperator final : VolumeSubflowOperator, RobustRounds {
    const bool base_links, base_tlinks;
    VolumeSubflowRobustOperator(Instance *I_, const VolumeSubflowRobustParams *c, bool links_, bool tlinks_)
        : VolumeSubflowRobustOperator(I_, c->p, wls_params_of(c->p), c->volumes, links_, tlinks_) {}
    VolumeSubflowRobustOperator(Instance *I_, const sc_volume_robust_params *p, const sc_volume_wls_params &q, int volumes_, bool links_, bool tlinks_)
        : VolumeSubflowRobustOperator(I_, p, VolumeSubflowParams{ &q, volumes_ }, links_, tlinks_) {}
    VolumeSubflowRobustOperator(Instance *I_, const sc_volume_robust_params *p, const VolumeSubflowParams &sp, bool links_, bool tlinks_)
        : VolumeSubflowOperator(I_, &sp, links_, tlinks_, VOLUME_ROBUST_SUMS),
          RobustRounds(robust_term(p->p_grad, p->eps_grad), robust_term(p->p_data, p->eps_data), robust_term(p->p_time, p->eps_time), p->max_rounds,
                       p->round_tol, p->kind, VOLUME_ROBUST_SUMS),
          base_links(links_), base_tlinks(tlinks_) {}
    RobustRounds *rounds() override { return this; }
    int coupling(int) const override { return 0; }
    void begin() override
    {
        VolumeSubflowOperator::begin();
        links = base_links;          // round 0 of a new chunk: the caller's arrays again
        tlinks = base_tlinks;
    }
    int launch(PcgChunk &c, int, double *) override
    {
        PcgState &S = *I->pcg;
        if (c.mv != built) build(c.g, c.wg, c.mv, I->stream);      // the links lie in the order of the volumes that stay
        float *rho = (float *)S.rho.p;
        launch_volume_subflow_robust_setup(c.g, c.wg, geo(c.wg), dj.data(), ds.data(), c.mv, grad, time, data, st, S.lnk.p, c.U, rho + lt_at, rho,
                                           (double *)(rho + 2 * lt_at), c.R, (float *)S.e.p, (float *)S.s.p, (float *)S.f.p, (float *)S.dg.p, c.d_bb,
                                           c.d_round, I->stream);
        return SC_OK;
    }
    void take(const double *t) override { wsum = t[0]; ssum = t[1]; tsum = t[2]; uksum = t[3]; links = tlinks = true; }
};

PcgCall volume_robust_call(int kind, const sc_volume_robust_params *p)
{
    return PcgCall{ kind, p->tol, p->max_iters, 400, p->frames, p->frame_stride, p->time_periodic ? p->frames : p->frames - 1 };
}

constexpr const char *ROBUST_METHOD_WHY = "a robust volume solve is solved by SC_METHOD_AUTO and SC_METHOD_FFT only (conjugate gradients preconditioned by the direct solve)";

// the robust flow call's check: the robust volume call's, then the flow call's refusal of a size
int volume_flow_robust_validate(const sc_volume_robust_params *p, const sc_poisson_layout *l, const char **why)
{
    const char *dummy;
    if (!why) why = &dummy;
    const int rc = volume_robust_validate(p, l, why);
    if (rc) return rc;
    const sc_volume_wls_params q = wls_params_of(p);
    if (!flow_indexable(flow_work_geo(&q, l, poisson_norm_kind(p->kind)))) { *why = FLOW_SIZE_WHY; return SC_ERR_BAD_SIZE; }
    return SC_OK;
}
// the call of a robust volume with a flow: volume_robust_call and the floats of one of its dense flow arrays
PcgCall volume_flow_robust_call(int kind, const sc_volume_robust_params *p, const sc_poisson_layout *l)
{
    PcgCall call = volume_robust_call(kind, p);
    call.flow_floats = (size_t)call.tframes * (size_t)l->rows * (size_t)l->cols;
    return call;
}

// the coupled call's check: the robust volume call's (coupling bits in kind included), then the coupling's own two refusals
int volume_coupled_validate(const sc_volume_robust_params *p, int coupling, const sc_poisson_layout *l, const char **why)
{
    const char *dummy;
    if (!why) why = &dummy;
    const int rc = volume_robust_validate(p, l, why);
    if (rc) return rc;
    const char *own = (coupling & ~(SC_VOLUME_COUPLE_SPACE | SC_VOLUME_COUPLE_TIME | SC_VOLUME_COUPLE_CHANNELS)) ? "coupling has bits that are not SC_VOLUME_COUPLE_*"
                    : ((coupling & SC_VOLUME_COUPLE_TIME) && !(coupling & SC_VOLUME_COUPLE_SPACE)) ? "SC_VOLUME_COUPLE_TIME comes with SC_VOLUME_COUPLE_SPACE"
                    : ((coupling & SC_VOLUME_COUPLE_TIME) && (p->p_time != p->p_grad || p->eps_time != p->eps_grad))
                        ? "SC_VOLUME_COUPLE_TIME is one penalty: p_time must equal p_grad and eps_time eps_grad" : nullptr;
    if (own) { *why = own; return SC_ERR_BAD_ARG; }
    return SC_OK;
}

// the coupled flow call's check: the coupled call's, then the flow call's refusal of a size
int volume_flow_coupled_validate(const sc_volume_robust_params *p, int coupling, const sc_poisson_layout *l, const char **why)
{
    const char *dummy;
    if (!why) why = &dummy;
    const int rc = volume_coupled_validate(p, coupling, l, why);
    if (rc) return rc;
    const sc_volume_wls_params q = wls_params_of(p);
    if (!flow_indexable(flow_work_geo(&q, l, poisson_norm_kind(p->kind)))) { *why = FLOW_SIZE_WHY; return SC_ERR_BAD_SIZE; }
    return SC_OK;
}

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
    const sc_volume_wls_params q = wls_params_of(p);
    return volume_device_call<VolumeOperator>(I, volume_call(kind, &q), &q, l, jobs, n, bSync,
                                              [](const sc_volume_job &j) { return VolumeLinks{ nullptr, nullptr, nullptr, j.lap }; });
}

int sc_hip_volume(void *inst, const sc_volume_params *p, const sc_poisson_layout *l, const float *gx, const float *gy, const float *gt,
                  const float *lap, const float *data, const float *state, const float *weight, const float *boundary, float *out)
{
    Instance *I;
    int kind, rc = pcg_begin(inst, p, l, volume_validate, METHOD_WHY, FP64_WHY, I, kind);
    if (rc) return rc;
    const sc_volume_wls_params q = wls_params_of(p);
    VolumeOperator op(I, &q, false, false);
    FloatArrays a{ gx, gy, lap, data, weight, boundary, out, nullptr, nullptr, state };
    a.gt = gt;
    return pcg_host_call(I, volume_call(kind, &q), l, carries_of(weight != nullptr, false, false), a, op);
}

int sc_hip_volume_wls_check(const sc_volume_wls_params *p, const sc_poisson_layout *l)
{
    return volume_wls_validate(p, l, nullptr);
}

int sc_hip_volume_wls_device(void *inst, const sc_volume_wls_params *p, const sc_poisson_layout *l, sc_volume_wls_job *jobs, int n, bool bSync)
{
    Instance *I;
    int kind, rc = pcg_begin(inst, p, l, volume_wls_validate, METHOD_WHY, FP64_WHY, I, kind);
    if (rc) return rc;
    return volume_device_call<VolumeOperator>(I, volume_call(kind, p), p, l, jobs, n, bSync,
                                              [](const sc_volume_wls_job &j) { return VolumeLinks{ j.smooth_x, j.smooth_y, j.smooth_t, j.lap }; });
}

int sc_hip_volume_wls(void *inst, const sc_volume_wls_params *p, const sc_poisson_layout *l, const float *gx, const float *gy, const float *gt,
                      const float *lap, const float *data, const float *state, const float *weight, const float *smooth_x, const float *smooth_y,
                      const float *smooth_t, const float *boundary, float *out)
{
    Instance *I;
    int kind, rc = pcg_begin(inst, p, l, volume_wls_validate, METHOD_WHY, FP64_WHY, I, kind);
    if (rc) return rc;
    if (!smooth_x != !smooth_y) { I->err = "smooth_x and smooth_y go together (both NULL: every spatial link 1)"; return SC_ERR_BAD_ARG; }
    const bool links = smooth_x != nullptr, tlinks = smooth_t != nullptr;
    VolumeOperator op(I, p, links, tlinks);
    FloatArrays a{ gx, gy, lap, data, weight, boundary, out, smooth_x, smooth_y, state };
    a.gt = gt;
    a.smooth_t = smooth_t;
    return pcg_host_call(I, volume_call(kind, p), l, carries_of(weight != nullptr, links, tlinks), a, op);
}

int sc_hip_volume_flow_check(const sc_volume_wls_params *p, const sc_poisson_layout *l)
{
    return volume_flow_validate(p, l, nullptr);
}

// (without flow arrays the call is sc_hip_volume_wls: its validation, its operator, its launches)
int sc_hip_volume_flow_device(void *inst, const sc_volume_wls_params *p, const sc_poisson_layout *l, sc_volume_flow_job *jobs, int n, bool bSync)
{
    const bool flow = jobs && n > 0 && (jobs[0].flow_x || jobs[0].flow_y);
    Instance *I;
    int kind, rc = flow ? pcg_begin(inst, p, l, volume_flow_validate, METHOD_WHY, FP64_WHY, I, kind)
                        : pcg_begin(inst, p, l, volume_wls_validate, METHOD_WHY, FP64_WHY, I, kind);
    if (rc) return rc;
    auto links_of = [](const sc_volume_flow_job &j) { return VolumeLinks{ j.smooth_x, j.smooth_y, j.smooth_t, j.lap, j.flow_x, j.flow_y }; };
    if (!flow) return volume_device_call<VolumeOperator>(I, volume_call(kind, p), p, l, jobs, n, bSync, links_of);
    if ((rc = flow_links_ensure(I, p, l, kind))) return rc;
    return volume_device_call<VolumeFlowOperator>(I, volume_flow_call(kind, p, l), p, l, jobs, n, bSync, links_of);
}

int sc_hip_volume_flow(void *inst, const sc_volume_wls_params *p, const sc_poisson_layout *l, const float *gx, const float *gy, const float *gt,
                       const float *lap, const float *data, const float *state, const float *weight, const float *smooth_x, const float *smooth_y,
                       const float *smooth_t, const float *flow_x, const float *flow_y, const float *boundary, float *out)
{
    if (!flow_x && !flow_y)
        return sc_hip_volume_wls(inst, p, l, gx, gy, gt, lap, data, state, weight, smooth_x, smooth_y, smooth_t, boundary, out);
    Instance *I;
    int kind, rc = pcg_begin(inst, p, l, volume_flow_validate, METHOD_WHY, FP64_WHY, I, kind);
    if (rc) return rc;
    if (!smooth_x != !smooth_y) { I->err = "smooth_x and smooth_y go together (both NULL: every spatial link 1)"; return SC_ERR_BAD_ARG; }
    if (!flow_x != !flow_y) { I->err = FLOW_PAIR_WHY; return SC_ERR_BAD_ARG; }
    if ((rc = flow_links_ensure(I, p, l, kind))) return rc;
    const bool links = smooth_x != nullptr, tlinks = smooth_t != nullptr;
    VolumeFlowOperator op(I, p, links, tlinks);
    FloatArrays a{ gx, gy, lap, data, weight, boundary, out, smooth_x, smooth_y, state };
    a.gt = gt;
    a.smooth_t = smooth_t;
    a.flow_x = flow_x;
    a.flow_y = flow_y;
    return pcg_host_call(I, volume_flow_call(kind, p, l), l, carries_of(weight != nullptr, links, tlinks) | FLOAT_FLOW, a, op);
}

int sc_hip_volume_subflow_check(const sc_volume_wls_params *p, const sc_poisson_layout *l)
{
    return volume_flow_validate(p, l, nullptr);
}

// (without flow arrays the call is sc_hip_volume_wls: its validation, its operator, its launches)
int sc_hip_volume_subflow_device(void *inst, const sc_volume_wls_params *p, const sc_poisson_layout *l, sc_volume_flow_job *jobs, int n, bool bSync)
{
    const bool flow = jobs && n > 0 && (jobs[0].flow_x || jobs[0].flow_y);
    Instance *I;
    int kind, rc = flow ? pcg_begin(inst, p, l, volume_flow_validate, METHOD_WHY, FP64_WHY, I, kind)
                        : pcg_begin(inst, p, l, volume_wls_validate, METHOD_WHY, FP64_WHY, I, kind);
    if (rc) return rc;
    auto links_of = [](const sc_volume_flow_job &j) { return VolumeLinks{ j.smooth_x, j.smooth_y, j.smooth_t, j.lap, j.flow_x, j.flow_y }; };
    if (!flow) return volume_device_call<VolumeOperator>(I, volume_call(kind, p), p, l, jobs, n, bSync, links_of);
    if ((rc = subflow_links_ensure(I, p, l, kind, n))) return rc;
    const VolumeSubflowParams sp{ p, n };
    return volume_device_call<VolumeSubflowOperator>(I, volume_flow_call(kind, p, l), &sp, l, jobs, n, bSync, links_of);
}

int sc_hip_volume_subflow(void *inst, const sc_volume_wls_params *p, const sc_poisson_layout *l, const float *gx, const float *gy, const float *gt,
                          const float *lap, const float *data, const float *state, const float *weight, const float *smooth_x, const float *smooth_y,
                          const float *smooth_t, const float *flow_x, const float *flow_y, const float *boundary, float *out)
{
    if (!flow_x && !flow_y)
        return sc_hip_volume_wls(inst, p, l, gx, gy, gt, lap, data, state, weight, smooth_x, smooth_y, smooth_t, boundary, out);
    Instance *I;
    int kind, rc = pcg_begin(inst, p, l, volume_flow_validate, METHOD_WHY, FP64_WHY, I, kind);
    if (rc) return rc;
    if (!smooth_x != !smooth_y) { I->err = "smooth_x and smooth_y go together (both NULL: every spatial link 1)"; return SC_ERR_BAD_ARG; }
    if (!flow_x != !flow_y) { I->err = FLOW_PAIR_WHY; return SC_ERR_BAD_ARG; }
    if ((rc = subflow_links_ensure(I, p, l, kind, 1))) return rc;
    const bool links = smooth_x != nullptr, tlinks = smooth_t != nullptr;
    const VolumeSubflowParams sp{ p, 1 };
    VolumeSubflowOperator op(I, &sp, links, tlinks);
    FloatArrays a{ gx, gy, lap, data, weight, boundary, out, smooth_x, smooth_y, state };
    a.gt = gt;
    a.smooth_t = smooth_t;
    a.flow_x = flow_x;
    a.flow_y = flow_y;
    return pcg_host_call(I, volume_flow_call(kind, p, l), l, carries_of(weight != nullptr, links, tlinks) | FLOAT_FLOW, a, op);
}

int sc_hip_volume_robust_check(const sc_volume_robust_params *p, const sc_poisson_layout *l)
{
    return volume_robust_validate(p, l, nullptr);
}

int sc_hip_volume_robust_device(void *inst, const sc_volume_robust_params *p, const sc_poisson_layout *l, sc_volume_robust_job *jobs, int n, bool bSync)
{
    Instance *I;
    int kind, rc = pcg_begin(inst, p, l, volume_robust_validate, ROBUST_METHOD_WHY, FP64_WHY, I, kind);
    if (rc) return rc;
    return volume_device_call<VolumeRobustOperator>(I, volume_robust_call(kind, p), p, l, jobs, n, bSync, [](const sc_volume_robust_job &j) {
        return VolumeLinks{ j.smooth_x, j.smooth_y, j.smooth_t, nullptr }; }, robust_chunk);
}

int sc_hip_volume_robust(void *inst, const sc_volume_robust_params *p, const sc_poisson_layout *l, const float *gx, const float *gy, const float *gt,
                         const float *data, const float *state, const float *weight, const float *smooth_x, const float *smooth_y,
                         const float *smooth_t, const float *boundary, float *out)
{
    Instance *I;
    int kind, rc = pcg_begin(inst, p, l, volume_robust_validate, ROBUST_METHOD_WHY, FP64_WHY, I, kind);
    if (rc) return rc;
    if (!smooth_x != !smooth_y) { I->err = "smooth_x and smooth_y go together (both NULL: every spatial base link 1)"; return SC_ERR_BAD_ARG; }
    const bool links = smooth_x != nullptr, tlinks = smooth_t != nullptr;
    VolumeRobustOperator op(I, p, links, tlinks);
    FloatArrays a{ gx, gy, nullptr, data, weight, boundary, out, smooth_x, smooth_y, state };
    a.gt = gt;
    a.smooth_t = smooth_t;
    return pcg_host_call(I, volume_robust_call(kind, p), l, carries_of(weight != nullptr, links, tlinks), a, op, robust_chunk);
}

int sc_hip_volume_flow_robust_check(const sc_volume_robust_params *p, const sc_poisson_layout *l)
{
    return volume_flow_robust_validate(p, l, nullptr);
}

// (without flow arrays the call is sc_hip_volume_robust: its validation, its operator, its launches)
int sc_hip_volume_flow_robust_device(void *inst, const sc_volume_robust_params *p, const sc_poisson_layout *l, sc_volume_flow_robust_job *jobs, int n,
                                     bool bSync)
{
    const bool flow = jobs && n > 0 && (jobs[0].flow_x || jobs[0].flow_y);
    Instance *I;
    int kind, rc = flow ? pcg_begin(inst, p, l, volume_flow_robust_validate, ROBUST_METHOD_WHY, FP64_WHY, I, kind)
                        : pcg_begin(inst, p, l, volume_robust_validate, ROBUST_METHOD_WHY, FP64_WHY, I, kind);
    if (rc) return rc;
    auto links_of = [](const sc_volume_flow_robust_job &j) { return VolumeLinks{ j.smooth_x, j.smooth_y, j.smooth_t, nullptr, j.flow_x, j.flow_y }; };
    if (!flow) return volume_device_call<VolumeRobustOperator>(I, volume_robust_call(kind, p), p, l, jobs, n, bSync, links_of, robust_chunk);
    const sc_volume_wls_params q = wls_params_of(p);
    if ((rc = flow_links_ensure(I, &q, l, kind))) return rc;
    return volume_device_call<VolumeFlowRobustOperator>(I, volume_flow_robust_call(kind, p, l), p, l, jobs, n, bSync, links_of, robust_chunk);
}

int sc_hip_volume_flow_robust(void *inst, const sc_volume_robust_params *p, const sc_poisson_layout *l, const float *gx, const float *gy, const float *gt,
                              const float *data, const float *state, const float *weight, const float *smooth_x, const float *smooth_y,
                              const float *smooth_t, const float *flow_x, const float *flow_y, const float *boundary, float *out)
{
    if (!flow_x && !flow_y) return sc_hip_volume_robust(inst, p, l, gx, gy, gt, data, state, weight, smooth_x, smooth_y, smooth_t, boundary, out);
    Instance *I;
    int kind, rc = pcg_begin(inst, p, l, volume_flow_robust_validate, ROBUST_METHOD_WHY, FP64_WHY, I, kind);
    if (rc) return rc;
    if (!smooth_x != !smooth_y) { I->err = "smooth_x and smooth_y go together (both NULL: every spatial base link 1)"; return SC_ERR_BAD_ARG; }
    if (!flow_x != !flow_y) { I->err = FLOW_PAIR_WHY; return SC_ERR_BAD_ARG; }
    const sc_volume_wls_params q = wls_params_of(p);
    if ((rc = flow_links_ensure(I, &q, l, kind))) return rc;
    const bool links = smooth_x != nullptr, tlinks = smooth_t != nullptr;
    VolumeFlowRobustOperator op(I, p, links, tlinks);
    FloatArrays a{ gx, gy, nullptr, data, weight, boundary, out, smooth_x, smooth_y, state };
    a.gt = gt;
    a.smooth_t = smooth_t;
    a.flow_x = flow_x;
    a.flow_y = flow_y;
    return pcg_host_call(I, volume_flow_robust_call(kind, p, l), l, carries_of(weight != nullptr, links, tlinks) | FLOAT_FLOW, a, op, robust_chunk);
}

int sc_hip_volume_subflow_robust_check(const sc_volume_robust_params *p, const sc_poisson_layout *l)
{
    return volume_flow_robust_validate(p, l, nullptr);
}

// (without flow arrays the call is sc_hip_volume_robust: its validation, its operator, its launches)
int sc_hip_volume_subflow_robust_device(void *inst, const sc_volume_robust_params *p, const sc_poisson_layout *l, sc_volume_flow_robust_job *jobs, int n,
                                        bool bSync)
{
    const bool flow = jobs && n > 0 && (jobs[0].flow_x || jobs[0].flow_y);
    Instance *I;
    int kind, rc = flow ? pcg_begin(inst, p, l, volume_flow_robust_validate, ROBUST_METHOD_WHY, FP64_WHY, I, kind)
                        : pcg_begin(inst, p, l, volume_robust_validate, ROBUST_METHOD_WHY, FP64_WHY, I, kind);
    if (rc) return rc;
    auto links_of = [](const sc_volume_flow_robust_job &j) { return VolumeLinks{ j.smooth_x, j.smooth_y, j.smooth_t, nullptr, j.flow_x, j.flow_y }; };
    if (!flow) return volume_device_call<VolumeRobustOperator>(I, volume_robust_call(kind, p), p, l, jobs, n, bSync, links_of, robust_chunk);
    const sc_volume_wls_params q = wls_params_of(p);
    if ((rc = subflow_links_ensure(I, &q, l, kind, n))) return rc;
    const VolumeSubflowRobustParams sp{ p, n };
    return volume_device_call<VolumeSubflowRobustOperator>(I, volume_flow_robust_call(kind, p, l), &sp, l, jobs, n, bSync, links_of, robust_chunk);
}

int sc_hip_volume_subflow_robust(void *inst, const sc_volume_robust_params *p, const sc_poisson_layout *l, const float *gx, const float *gy,
                                 const float *gt, const float *data, const float *state, const float *weight, const float *smooth_x,
                                 const float *smooth_y, const float *smooth_t, const float *flow_x, const float *flow_y, const float *boundary, float *out)
{
    if (!flow_x && !flow_y) return sc_hip_volume_robust(inst, p, l, gx, gy, gt, data, state, weight, smooth_x, smooth_y, smooth_t, boundary, out);
    Instance *I;
    int kind, rc = pcg_begin(inst, p, l, volume_flow_robust_validate, ROBUST_METHOD_WHY, FP64_WHY, I, kind);
    if (rc) return rc;
    if (!smooth_x != !smooth_y) { I->err = "smooth_x and smooth_y go together (both NULL: every spatial base link 1)"; return SC_ERR_BAD_ARG; }
    if (!flow_x != !flow_y) { I->err = FLOW_PAIR_WHY; return SC_ERR_BAD_ARG; }
    const sc_volume_wls_params q = wls_params_of(p);
    if ((rc = subflow_links_ensure(I, &q, l, kind, 1))) return rc;
    const bool links = smooth_x != nullptr, tlinks = smooth_t != nullptr;
    const VolumeSubflowRobustParams sp{ p, 1 };
    VolumeSubflowRobustOperator op(I, &sp, links, tlinks);
    FloatArrays a{ gx, gy, nullptr, data, weight, boundary, out, smooth_x, smooth_y, state };
    a.gt = gt;
    a.smooth_t = smooth_t;
    a.flow_x = flow_x;
    a.flow_y = flow_y;
    return pcg_host_call(I, volume_flow_robust_call(kind, p, l), l, carries_of(weight != nullptr, links, tlinks) | FLOAT_FLOW, a, op, robust_chunk);
}

int sc_hip_volume_coupled_check(const sc_volume_robust_params *p, int coupling, const sc_poisson_layout *l)
{
    return volume_coupled_validate(p, coupling, l, nullptr);
}

int sc_hip_volume_coupled_device(void *inst, const sc_volume_robust_params *p, int coupling, const sc_poisson_layout *l, sc_volume_robust_job *jobs, int n,
                                 bool bSync)
{
    Instance *I;
    int kind, rc = pcg_begin(inst, p, l, [coupling](const sc_volume_robust_params *q, const sc_poisson_layout *m, const char **why) {
        return volume_coupled_validate(q, coupling, m, why); }, ROBUST_METHOD_WHY, FP64_WHY, I, kind);
    if (rc) return rc;
    const VolumeCoupledParams cp{ p, coupling_words(coupling) };
    return volume_device_call<VolumeRobustOperator>(I, volume_robust_call(kind, p), &cp, l, jobs, n, bSync, [](const sc_volume_robust_job &j) {
        return VolumeLinks{ j.smooth_x, j.smooth_y, j.smooth_t, nullptr }; }, robust_chunk);
}

int sc_hip_volume_coupled(void *inst, const sc_volume_robust_params *p, int coupling, const sc_poisson_layout *l, const float *gx, const float *gy,
                          const float *gt, const float *data, const float *state, const float *weight, const float *smooth_x, const float *smooth_y,
                          const float *smooth_t, const float *boundary, float *out)
{
    Instance *I;
    int kind, rc = pcg_begin(inst, p, l, [coupling](const sc_volume_robust_params *q, const sc_poisson_layout *m, const char **why) {
        return volume_coupled_validate(q, coupling, m, why); }, ROBUST_METHOD_WHY, FP64_WHY, I, kind);
    if (rc) return rc;
    if (!smooth_x != !smooth_y) { I->err = "smooth_x and smooth_y go together (both NULL: every spatial base link 1)"; return SC_ERR_BAD_ARG; }
    const bool links = smooth_x != nullptr, tlinks = smooth_t != nullptr;
    const VolumeCoupledParams cp{ p, coupling_words(coupling) };
    VolumeRobustOperator op(I, &cp, links, tlinks);
    FloatArrays a{ gx, gy, nullptr, data, weight, boundary, out, smooth_x, smooth_y, state };
    a.gt = gt;
    a.smooth_t = smooth_t;
    return pcg_host_call(I, volume_robust_call(kind, p), l, carries_of(weight != nullptr, links, tlinks), a, op, robust_chunk);
}

int sc_hip_volume_flow_coupled_check(const sc_volume_robust_params *p, int coupling, const sc_poisson_layout *l)
{
    return volume_flow_coupled_validate(p, coupling, l, nullptr);
}

// (without flow arrays the call is sc_hip_volume_coupled: its validation, its operator, its launches)
int sc_hip_volume_flow_coupled_device(void *inst, const sc_volume_robust_params *p, int coupling, const sc_poisson_layout *l,
                                      sc_volume_flow_robust_job *jobs, int n, bool bSync)
{
    const bool flow = jobs && n > 0 && (jobs[0].flow_x || jobs[0].flow_y);
    Instance *I;
    int kind, rc = pcg_begin(inst, p, l, [coupling, flow](const sc_volume_robust_params *q, const sc_poisson_layout *m, const char **why) {
        return flow ? volume_flow_coupled_validate(q, coupling, m, why) : volume_coupled_validate(q, coupling, m, why); }, ROBUST_METHOD_WHY, FP64_WHY, I, kind);
    if (rc) return rc;
    const VolumeCoupledParams cp{ p, coupling_words(coupling) };
    auto links_of = [](const sc_volume_flow_robust_job &j) { return VolumeLinks{ j.smooth_x, j.smooth_y, j.smooth_t, nullptr, j.flow_x, j.flow_y }; };
    if (!flow) return volume_device_call<VolumeRobustOperator>(I, volume_robust_call(kind, p), &cp, l, jobs, n, bSync, links_of, robust_chunk);
    const sc_volume_wls_params q = wls_params_of(p);
    if ((rc = flow_links_ensure(I, &q, l, kind))) return rc;
    return volume_device_call<VolumeFlowRobustOperator>(I, volume_flow_robust_call(kind, p, l), &cp, l, jobs, n, bSync, links_of, robust_chunk);
}

int sc_hip_volume_flow_coupled(void *inst, const sc_volume_robust_params *p, int coupling, const sc_poisson_layout *l, const float *gx, const float *gy,
                               const float *gt, const float *data, const float *state, const float *weight, const float *smooth_x,
                               const float *smooth_y, const float *smooth_t, const float *flow_x, const float *flow_y, const float *boundary, float *out)
{
    if (!flow_x && !flow_y)
        return sc_hip_volume_coupled(inst, p, coupling, l, gx, gy, gt, data, state, weight, smooth_x, smooth_y, smooth_t, boundary, out);
    Instance *I;
    int kind, rc = pcg_begin(inst, p, l, [coupling](const sc_volume_robust_params *q, const sc_poisson_layout *m, const char **why) {
        return volume_flow_coupled_validate(q, coupling, m, why); }, ROBUST_METHOD_WHY, FP64_WHY, I, kind);
    if (rc) return rc;
    if (!smooth_x != !smooth_y) { I->err = "smooth_x and smooth_y go together (both NULL: every spatial base link 1)"; return SC_ERR_BAD_ARG; }
    if (!flow_x != !flow_y) { I->err = FLOW_PAIR_WHY; return SC_ERR_BAD_ARG; }
    const sc_volume_wls_params q = wls_params_of(p);
    if ((rc = flow_links_ensure(I, &q, l, kind))) return rc;
    const bool links = smooth_x != nullptr, tlinks = smooth_t != nullptr;
    const VolumeCoupledParams cp{ p, coupling_words(coupling) };
    VolumeFlowRobustOperator op(I, &cp, links, tlinks);
    FloatArrays a{ gx, gy, nullptr, data, weight, boundary, out, smooth_x, smooth_y, state };
    a.gt = gt;
    a.smooth_t = smooth_t;
    a.flow_x = flow_x;
    a.flow_y = flow_y;
    return pcg_host_call(I, volume_flow_robust_call(kind, p, l), l, carries_of(weight != nullptr, links, tlinks) | FLOAT_FLOW, a, op, robust_chunk);
}

} // extern "C"
