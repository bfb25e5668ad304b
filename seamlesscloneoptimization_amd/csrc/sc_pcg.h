// sc_pcg.h -- the preconditioned conjugate gradients that the weighted, the WLS and the robust call share: the work planes' geometry and
// tiling, the instance's state, what a family tells the iteration about its operator (PcgOperator), the driver and the entry code around
// it (pcg_run, pcg_begin, pcg_host_call, pcg_device_call; sc_pcg.cpp), the launches (sc_pcg.hip: the shared ones; sc_weighted.hip,
// sc_wls.hip, sc_robust.hip, sc_region.hip, sc_region_robust.hip, sc_bounded.hip, sc_volume.hip, sc_volume_flow.hip, sc_volume_subflow.hip, sc_volume_robust.hip, sc_volume_coupled.hip: a family's statistics, set-up and operator), the link operator
// of the WLS and the robust call (WlsOperator, sc_wls_api.cpp), the volume families' (VolumeOperator, sc_volume_api.cpp) and what the three
// robust calls share: their rounds, their check and their entry preamble (RobustRounds, robust_chunk, robust_begin; sc_robust_api.cpp).
//     L u = b,  L negative definite,  preconditioned by direct_jobs_solve with a constant: M = A - lam.
// Work planes are compact float32: only the nx x ny unknowns of MixedGeo, row after row, planes `stride` floats apart (a multiple of 4:
// float4 access); plane p = member C + channel.  Tiling of the launches that walk a plane in 2-D (statistics, set-up, operator): column
// group x of 256 columns, band y of `rows` rows, one partial sum per workgroup, cg * bands <= PCG_PARTS of them per plane; of the
// element-wise launches (update, dot, direction, scale): `eparts` segments of whole float4 groups.  Partial sums are doubles at
// parts[plane * PCG_PARTS + i]; whoever needs a total adds the parts of its plane itself, in one fixed order (first wave, then
// shuffles): no atomics, no host round trip.
#pragma once
#include "sc_instance.h"
#include <cassert>
#include <climits>
#include <cmath>
#include <initializer_list>

namespace sc {

constexpr int PCG_PARTS = 256;
struct PcgGeo { int nx, ny, ax, ay, x0, y0, cg, bands, rows, eparts, egroups; long long stride; };
PcgGeo pcg_geo(const MixedGeo &mg);
inline int pcg_op_parts(const PcgGeo &wg) { return wg.cg * wg.bands; }

// The instance's state (Instance::pcg, made with the instance): work planes [planes][PcgGeo::stride] of float32 (q holds L p, then the
// preconditioned residual z), the double partial sums, and the stop rule's mailbox: the per-plane ||r||^2 of iteration k goes to slot
// k % RING of the pinned block with event k % RING behind it, and the host reads iteration k - LAG before it enqueues iteration k
struct PcgState {
    enum { LAG = SC_WEIGHTED_POLL, RING = SC_WEIGHTED_POLL + 1 };
    DevBuf u, r, p, q;
    DevBuf w;                              // the weighted solve's coefficient plane (sc_weighted.hip): the weights
    DevBuf e, s, dg;                       // the WLS solve's (sc_wls.hip): links east, links south, the diagonal
    DevBuf f, dct, tab;                    // the volume solve's (sc_volume.hip): links to the next frame (the sub-pixel flow call: 1 at UNKNOWN pixels, else 0); the transformed planes; the DCT table (float) and the modes' shifts (double)
    DevBuf lnk;                            // the flow volume solve's (sc_volume_flow.hip): the int32 link planes fwd | bwd per volume; the sub-pixel flow call's (sc_volume_subflow.hip): off | ent | fw of a chunk's volumes and the build's scratch (SubflowStore)
    DevBuf rho;                            // the robust solve's coupled forms (sc_robust.hip): rho of every owner's magnitude; the sub-pixel flow call's: rho | LT, a work plane each per (volume, channel)
    DevBuf act;                            // the bounded solve's two set planes (sc_bounded.hip): 0 free, +1 upper-active, -1 lower-active
    DevBuf bad, h_bad;                     // ... and its judgement of bound arrays: per part the UNKNOWN pixels with an invalid bound (double; device, pinned)
    DevBuf red;                            // double: the family's statistics | b.b | p.q | r.r | r.z of even / odd iterations (PCG_PARTS per plane each) | ||r||^2 per plane | a family's round sums
    DevBuf h_red;                          // pinned: the statistics' copy | b.b parts | RING slots of ||r||^2 per plane | a family's round sums
    hipEvent_t ev[RING]{};
    std::vector<double> trace_energy;      // the last robust call's last chunk (sc_hip_robust_trace): per round the energy of its iterate
    std::vector<int> trace_iters;          // ... and its inner iterations
    // the last bounded call's last chunk (sc_hip_bounded_trace), its own three: per round the pixels that changed set, the active ones, the inner iterations
    std::vector<int> trace_changed, trace_active, trace_bounded_iters;
};
void pcg_release(Instance *I);             // frees Instance::pcg and all it holds

// What a family tells the iteration about its operator.  Per chunk, in this order: begin -> stats (one launch per 16 jobs, `nstat`
// doubles per part; the driver reads them back: the chunk's one mandatory wait) -> judge for every job, in order (a reason: the job gets
// SC_ERR_BAD_ARG and leaves; NULL: it stays, its sums count, and the driver moves its dj and ds to the front) -> setup -> precond_constant ->
// scale_start on u0 (a cold start only) -> apply, once in its residual form and then once per iteration, precond wherever M^-1 is
// applied.  Everything else -- the update, dot and direction launches, the stop rule's mailbox -- is the driver's own, and so are the
// defaults of precond (direct_jobs_solve with precond_constant's lam), out, work_geo and chunk_planes, which only the volume family
// replaces.
struct PcgChunk;
struct RobustRounds;
struct PcgOperator {
    const int nstat;                       // doubles per part of the statistics launch
    const int nround;                      // doubles per part a family's own later launches sum (PcgChunk::d_round; the robust call's rounds)
    std::vector<PoissonJobDev> dj;         // the chunk's jobs; behind judge: the ones that stay, in front
    std::vector<SideArrays> ds;            // ... and their side arrays, record k beside job k: the driver assigns and moves the two together
    explicit PcgOperator(int nstat_, int nround_ = 0) : nstat(nstat_), nround(nround_) {}
    virtual ~PcgOperator() = default;
    // work planes per job and channel that run_chunks counts against SC_POISSON_MAX_PLANES (the volume call: its frames), and the work
    // planes' geometry: by default one plane of mg's unknowns per (job, channel) (the volume call: its frames stacked along y)
    virtual int chunk_planes(int C) const { return C; }
    virtual PcgGeo work_geo(const MixedGeo &mg) const { return pcg_geo(mg); }
    virtual void begin() = 0;                                                       // a new chunk (dj, ds are set): the running sums start over
    virtual void stats(const PoissonGeo &g, const PcgGeo &wg, int m, double *d_stats, hipStream_t s) = 0;
    // st: job k's statistics, its C planes' PCG_PARTS * nstat doubles each, of which the first `parts` parts are set
    virtual const char *judge(const PoissonGeo &g, int k, const double *st, int parts, bool no_dirichlet) = 0;
    virtual float precond_constant(const PoissonGeo &g, const PcgGeo &wg, int mv) = 0;      // lam: the driver's preconditioner is A - lam
    virtual int setup(const PoissonGeo &g, const PcgGeo &wg, bool lap, int mv, float *R, double *bb) = 0;      // R = b, the coefficient planes, bb = the parts of b . b
    // the start u0 = (A - lam)^-1 b where the family's preconditioner is a multiple of A - lam: its one-off factor (a constant factor
    // on the preconditioner changes no later iterate, so the loop never applies it).  The default: none.
    virtual void scale_start(const PcgGeo &wg, int planes, float *U, hipStream_t s) {}
    virtual void apply(const PcgGeo &wg, int planes, bool residual, const float *P, float *Q, double *parts, hipStream_t s) = 0;
    // the output launch of the mv jobs that stayed (dj): by default U at the unknowns and boundary's values on the Dirichlet lines
    virtual void out(const PoissonGeo &g, const PcgGeo &wg, int mv, const float *U, hipStream_t s);
    // the preconditioner: out = M^-1 in on the chunk's work planes.  The default: (A - lam) out = in through direct_jobs_solve, plane
    // by plane (lam: precond_constant's)
    virtual int precond(const PcgChunk &c, float lam, bool fp64, const float *in, float *out);
    // the reweighting rounds of an operator that robust_chunk may drive (the robust call's, the robust volume call's); NULL: it has none
    virtual RobustRounds *rounds() { return nullptr; }
    // the sum of field f of one plane's statistics over its first `parts` parts
    double stat_sum(const double *plane, int parts, int f) const
    {
        double sum = 0.0;
        for (int i = 0; i < parts; ++i) sum += plane[(size_t)nstat * i + f];
        return sum;
    }
    // A job's weights, fields 0 (the sum) and 1 (how many are invalid) of its statistics: the reason they refuse it, or `own` (the
    // family's own reason against the job, which ranks behind an invalid weight), or a channel without weight where nothing else
    // pins it; NULL: none.  job_w: the job's sum.
    const char *judge_weights(const PoissonGeo &g, const double *st, int parts, bool no_dirichlet, const char *own, double &job_w) const
    {
        bool bad = false, empty = false;
        job_w = 0.0;
        for (int c = 0; c < g.C; ++c) {
            const double *plane = st + (size_t)c * PCG_PARTS * nstat;
            const double sum = stat_sum(plane, parts, 0);
            bad = bad || stat_sum(plane, parts, 1) != 0.0;
            empty = empty || !(sum > 0.0);
            job_w += sum;
        }
        if (bad || !std::isfinite(job_w)) return "a weight is negative or not finite";
        if (own) return own;
        return no_dirichlet && empty ? "no data weight and no Dirichlet line" : nullptr;
    }
};
// kind: poisson_norm_kind's; frames, frame_stride: the volume call's -- a job's arrays are `frames` images under the layout, frame_stride
// floats apart; tframes: how many of them the temporal arrays hold (gt, smooth_t: frames - 1 with free time, frames with periodic time)
// flow_floats: the floats of one of the flow volume call's dense flow arrays (0: the call has none)
struct PcgCall { int kind; float tol; int max_iters; int default_iters; int frames = 1; long long frame_stride = 0; int tframes = 0; size_t flow_floats = 0; };
// the floats from an array's pointer to one past its last element, all frames of the call (pcg_call_tspan: of a temporal array)
inline size_t pcg_call_span(const PcgCall &call, const sc_poisson_layout *l) { return poisson_span(l) + (size_t)(call.frames - 1) * (size_t)call.frame_stride; }
inline size_t pcg_call_tspan(const PcgCall &call, const sc_poisson_layout *l)
{
    return call.tframes > 0 ? poisson_span(l) + (size_t)(call.tframes - 1) * (size_t)call.frame_stride : 0;
}
struct PcgChunkResult { int iters = 0; bool converged = true; double rel = 0.0; };
// One chunk of m same-size jobs between its prologue and its output, in three steps a family's driver may put its own between:
//   pcg_chunk_begin    the statistics, the judgement of every job (a refused one gets SC_ERR_BAD_ARG and leaves), the buffers; mv = the
//                      jobs that stay (0: nothing more to do)
//   pcg_chunk_iterate  one solve of L u = b: R holds b, d_bb the parts of b . b, the operator's coefficient planes are set.  Cold: u0 =
//                      M^-1 b times scale_start's factor.  Warm: U holds the start.  Either way r = b - L u through apply's residual
//                      form, z = M^-1 r, p = z, then the iteration; M = A - precond_constant().  res: this solve's figures
//   pcg_chunk_finish   U and the Dirichlet lines into the jobs' out, `code` to every job that stayed
struct PcgChunk {
    Instance *I = nullptr;
    PcgCall call{};
    PoissonGeo g{};
    MixedGeo mg{};
    PcgGeo wg{};
    int mv = 0, planes = 0, nop = 0;
    float *U = nullptr, *R = nullptr, *P = nullptr, *Q = nullptr;
    double *d_bb = nullptr, *d_pq = nullptr, *d_rr = nullptr, *d_rz[2] = { nullptr, nullptr }, *d_tot = nullptr, *h_bb = nullptr, *h_tot = nullptr;
    double *d_round = nullptr, *h_round = nullptr;      // PcgOperator::nround doubles per part, PCG_PARTS parts per plane
    std::vector<int *> live;                            // the codes of the jobs that stay
};
int pcg_chunk_begin(Instance *I, const PcgCall &call, const PoissonGeo &g, PcgOperator &op, int *const *rcs, int m, int &job_errors, PcgChunk &c);
int pcg_chunk_iterate(PcgChunk &c, PcgOperator &op, bool warm, PcgChunkResult &res);
int pcg_chunk_finish(PcgChunk &c, PcgOperator &op, int code);
// one chunk of a call: jobs i0 .. of the call's and their side arrays are op.dj and op.ds already; sets res and the jobs' codes, returns the chunk's code (run_chunks')
using PcgChunkFn = int (*)(Instance *I, const PcgCall &call, const PoissonGeo &g, PcgOperator &op, int *const *rcs, int m, PcgChunkResult &res,
                           int &job_errors);
// The validated jobs of a call and their side arrays (sides[k]: job k's) through chunks (run_chunks) and sc_run_info.  Returns the worst
// code, the jobs' own refusals included.
// chunk: NULL: begin, setup, one cold solve, finish (the weighted and the WLS call).  sc_run_info's sweeps, converged and rel_residual
// are the chunks' res: the most iterations, all converged, the worst residual.
int pcg_run(Instance *I, const PcgCall &call, const sc_poisson_layout *l, PcgOperator &op, const PoissonJobDev *jobs, const SideArrays *sides, int *const *rcs,
            int nv, bool timed, PcgChunkFn chunk = nullptr);
// What every entry of the three families starts with: the instance, the family's validation of the call (its sc_hip_*_check) and the
// instance's word on a direct solve, with the family's two reasons; kind: poisson_norm_kind's
template <class Params, class Validate> int pcg_begin(void *inst, const Params *p, const sc_poisson_layout *l, Validate validate,
                                                      const char *method_why, const char *fp64_why, Instance *&I, int &kind)
{
    int rc = begin_call(inst, I);
    if (rc) return rc;
    const char *why = "";
    if ((rc = validate(p, l, &why))) { I->err = why; return rc; }
    kind = poisson_norm_kind(p->kind);
    return direct_instance_check(I, kind, l, method_why, fp64_why);
}
// ... and ends with.  A host entry: the job's validation, float_stage, pcg_run on the staged job and its side arrays, the download into out
int pcg_host_call(Instance *I, const PcgCall &call, const sc_poisson_layout *l, int carries, const FloatArrays &a, PcgOperator &op,
                  PcgChunkFn chunk = nullptr);
// A device entry: float_intake (the jobs it refuses get their codes), pcg_run on the others and their side arrays; the worst code
template <class Job, class ArraysOf> int pcg_device_call(Instance *I, const PcgCall &call, const sc_poisson_layout *l, int carries, Job *jobs, int n,
                                                         ArraysOf arrays_of, PcgOperator &op, bool timed, PcgChunkFn chunk = nullptr)
{
    FloatJobs v;
    const int worst = float_intake(I, call.kind, carries, jobs, n, arrays_of, v, pcg_call_span(call, l), pcg_call_tspan(call, l), call.flow_floats);
    if (v.rcs.empty()) return worst;
    I->info.ms_h2d = I->info.ms_d2h = 0.f;
    return worse(worst, pcg_run(I, call, l, op, v.dj.data(), v.side.data(), v.rcs.data(), (int)v.rcs.size(), timed, chunk));
}

// ---- the shared launches (sc_pcg.hip)
// alpha = sum(rz) / sum(pq) per plane (0 when that is not finite);  U += alpha P,  R -= alpha Q,  rr = the parts of R . R
void launch_pcg_update(const PcgGeo &wg, int planes, float *U, float *R, const float *P, const float *Q, const double *rz, const double *pq, double *rr, hipStream_t s);
// rz = the parts of R . Z;  rr_tot[plane] = the sum of the nrr parts of rr (for the stop rule)
void launch_pcg_dot(const PcgGeo &wg, int planes, const float *R, const float *Z, double *rz, const double *rr, int nrr, double *rr_tot, hipStream_t s);
// P = Z + beta P, beta = sum(rz) / sum(rz_old) per plane (rz_old == nullptr: P = Z)
void launch_pcg_dir(const PcgGeo &wg, int planes, float *P, const float *Z, const double *rz, const double *rz_old, hipStream_t s);
void launch_pcg_scale(const PcgGeo &wg, int planes, float *U, float f, hipStream_t s);      // U *= f
// the jobs' out: U at the unknowns, boundary's values on the Dirichlet lines
void launch_pcg_out(const PoissonGeo &g, const PcgGeo &wg, const PoissonJobDev *jobs, int m, const float *U, hipStream_t s);

// ---- the families' launches.  Those that read the jobs' arrays take m jobs and their side arrays (sides[k]: job k's) and go through the
// family's table, a kernel parameter: Table::set(i, job, side) copies into slot i the members that table has (host side only; the
// layout is the kernels').  fn(table, i0, cnt) launches jobs i0 .. i0 + cnt - 1 (for_job_tables); what a launch decides by "the call
// has this array" it reads off the table's first record.
template <class Table, class Fn> void for_side_tables(const PoissonJobDev *jobs, const SideArrays *sides, int m, Fn fn)
{
    for_job_tables<Table>(m, [&](Table &t, int i, int k) { t.set(i, jobs[k], sides[k]); }, fn);
}

// ---- the weighted family (sc_weighted.hip): L = A - W, W = diag(w) >= 0
struct WeightedJobs {
    enum { MAX = 16 }; PoissonJobDev j[MAX]; const float *w[MAX];
    void set(int i, const PoissonJobDev &job, const SideArrays &a) { j[i] = job; w[i] = a.w; }
};
// stats[(plane * PCG_PARTS + i) * 2] = the part's sum of w over the unknowns, [.. + 1] = how many of them are negative or not finite
void launch_weighted_stats(const PoissonGeo &g, const PcgGeo &wg, const PoissonJobDev *jobs, const SideArrays *sides, int m, double *stats, hipStream_t s);
// R = b = lap - w d (screened_rhs's order) less the neighbouring Dirichlet lines' values, Wc = w, bb = the parts of b . b
void launch_weighted_setup(const PoissonGeo &g, const PcgGeo &wg, bool lap, const PoissonJobDev *jobs, const SideArrays *sides, int m, float *R, float *Wc,
                           double *bb, hipStream_t s);
// residual = false: Q = (A - W) P, parts of P . Q;  true: Q = Q - (A - W) P in place, parts of Q . Q
void launch_weighted_op(const PcgGeo &wg, int planes, bool residual, const float *P, const float *Wc, float *Q, double *parts, hipStream_t s);

// ---- the WLS family (sc_wls.hip): (L u)(p) = sum_q s(p, q) (u(q) - u(p)) - w(p) u(p), per-link weights sx, sy > 0 under the call's layout
struct WlsJobs {
    enum { MAX = 16 }; PoissonJobDev j[MAX]; const float *w[MAX], *sx[MAX], *sy[MAX];
    void set(int i, const PoissonJobDev &job, const SideArrays &a) { j[i] = job; w[i] = a.w; sx[i] = a.sx; sy[i] = a.sy; }
};
constexpr int WLS_STATS = 4;
// the live links of one plane: those with at least one end among the unknowns
double wls_live_links(const PcgGeo &wg);
// stats[(plane * PCG_PARTS + i) * WLS_STATS + ..] = the part's sum of w | how many w are negative or not finite | the sum of its
// live links, each counted once | how many of them are not finite or not > 0
void launch_wls_stats(const PoissonGeo &g, const PcgGeo &wg, const PoissonJobDev *jobs, const SideArrays *sides, int m, double *stats, hipStream_t s);
// R = b (the order: seamlessclone_hip.h, the WLS section), E / S = the link to the next unknown column / row (0: none), Dg = the sum of
// the four incident links, Dirichlet ones included, plus w; bb = the parts of b . b.  sx NULL (for every job of the call; guidance form
// only): every link that exists is 1 and neither array is read -- the bytes of a call given arrays of 1.0f
void launch_wls_setup(const PoissonGeo &g, const PcgGeo &wg, bool lap, const PoissonJobDev *jobs, const SideArrays *sides, int m, float *R, float *E,
                      float *S, float *Dg, double *bb, hipStream_t s);
// residual = false: Q = L P, parts of P . Q;  true: Q = Q - L P in place, parts of Q . Q
void launch_wls_op(const PcgGeo &wg, int planes, bool residual, const float *P, const float *E, const float *S, const float *Dg, float *Q,
                   double *parts, hipStream_t s);
// The operator of the system "data weights + per-link weights" (sc_wls_api.cpp): the WLS call's, and through RobustOperator
// (sc_robust_api.cpp) every round's of the robust call.  links: the jobs carry link weights; without them every link that exists is 1 --
// the weighted call's statistics (two fields, the links not judged), s-bar = 1, launch_wls_setup's constant-link form.  plam, psmooth:
// precond_lambda and precond_smooth (0: the means).
struct WlsOperator : PcgOperator {
    Instance *const I;
    const bool links;
    const float plam, psmooth;
    double wsum = 0.0, ssum = 0.0;                 // the sums of the weights and of the live links of the jobs that stay
    bool unit_links = false;                       // every live link is 1: s-bar is
    float u0_scale = 1.f;                          // 1 / s-bar
    WlsOperator(Instance *I_, bool links_, float plam_, float psmooth_, int nround_ = 0, int nstat_ = 0)      // nstat_: a subclass's own statistics
        : PcgOperator(nstat_ ? nstat_ : links_ ? WLS_STATS : 2, nround_), I(I_), links(links_), plam(plam_), psmooth(psmooth_) {}
    void begin() override;
    void stats(const PoissonGeo &g, const PcgGeo &wg, int m, double *d_stats, hipStream_t s) override;
    const char *judge(const PoissonGeo &g, int k, const double *st, int parts, bool no_dirichlet) override;
    float precond_constant(const PoissonGeo &g, const PcgGeo &wg, int mv) override;
    int setup(const PoissonGeo &g, const PcgGeo &wg, bool lap, int mv, float *R, double *bb) override;
    void scale_start(const PcgGeo &wg, int planes, float *U, hipStream_t s) override;
    void apply(const PcgGeo &wg, int planes, bool residual, const float *P, float *Q, double *parts, hipStream_t s) override;
};

// ---- the region family (sc_region.hip): the WLS system on a domain of any shape -- per job one more array, state, under the call's
// layout: 0 an unknown, 1 known (u = data), 2 outside the domain (its links do not exist); w NULL: no data term, sx NULL: every link 1
struct RegionJobs {
    enum { MAX = 16 }; PoissonJobDev j[MAX]; const float *w[MAX], *sx[MAX], *sy[MAX], *st[MAX];
    void set(int i, const PoissonJobDev &job, const SideArrays &a) { j[i] = job; w[i] = a.w; sx[i] = a.sx; sy[i] = a.sy; st[i] = a.st; }
};
constexpr int REGION_STATS = 8;
// stats[(plane * PCG_PARTS + i) * REGION_STATS + ..] = the part's sum of w over the UNKNOWN pixels | how many of those w are invalid |
// the sum of its links live in the region, each counted once | how many of them are invalid | its UNKNOWN pixels | the sum of its
// UNKNOWN - KNOWN links | its state elements that are not 0, 1 or 2 | its links live in the region
void launch_region_stats(const PoissonGeo &g, const PcgGeo &wg, const PoissonJobDev *jobs, const SideArrays *sides, int m, double *stats, hipStream_t s);
// R = b (the order: seamlessclone_hip.h, the region section); E / S = the link to the next column / row where both ends are UNKNOWN; Dg =
// the sum of the incident links live in the region plus w; all four 0 at every pixel that is not UNKNOWN; bb = the parts of b . b
void launch_region_setup(const PoissonGeo &g, const PcgGeo &wg, bool lap, const PoissonJobDev *jobs, const SideArrays *sides, int m, float *R, float *E,
                         float *S, float *Dg, double *bb, hipStream_t s);
// the jobs' out: U at UNKNOWN pixels, data's bits at KNOWN and OUTSIDE pixels, boundary's bits on the Dirichlet lines
void launch_region_out(const PoissonGeo &g, const PcgGeo &wg, const PoissonJobDev *jobs, const SideArrays *sides, int m, const float *U, hipStream_t s);
// The operator of the region families (sc_region_api.cpp: its head comment says what it tells the iteration): sc_hip_region's, and through
// RegionRobustOperator (sc_region_robust_api.cpp) every round's of the robust region call.
struct RegionOperator : WlsOperator {
    const bool has_w;
    double unknowns = 0.0, uksum = 0.0, lcount = 0.0;      // of the jobs that stay: UNKNOWN pixels, the sum of UNKNOWN - KNOWN links, links live in the region
    RegionOperator(Instance *I_, bool weight, bool links_, float plam_, float psmooth_, int nround_ = 0)      // nround_: a subclass's round sums
        : WlsOperator(I_, links_, plam_, psmooth_, nround_, REGION_STATS), has_w(weight) {}
    void begin() override
    {
        WlsOperator::begin();
        unknowns = uksum = lcount = 0.0;
    }
    void stats(const PoissonGeo &g, const PcgGeo &wg, int m, double *d_stats, hipStream_t s) override
    {
        launch_region_stats(g, wg, dj.data(), ds.data(), m, d_stats, s);
    }
    const char *judge(const PoissonGeo &g, int k, const double *st, int parts, bool no_dirichlet) override
    {
        double job[REGION_STATS] = {};
        bool loose = false;
        for (int c = 0; c < g.C; ++c) {
            const double *plane = st + (size_t)c * PCG_PARTS * REGION_STATS;
            double f[REGION_STATS];
            for (int i = 0; i < REGION_STATS; ++i) job[i] += f[i] = stat_sum(plane, parts, i);
            // (a plane without an UNKNOWN pixel has nothing to pin: b = 0, data and boundary are copied)
            loose = loose || (no_dirichlet && f[4] > 0.0 && !(f[5] > 0.0) && !(f[0] > 0.0));
        }
        if (job[6] != 0.0) return "a state element is not 0, 1 or 2";
        if (job[1] != 0.0 || !std::isfinite(job[0])) return "a weight is negative or not finite";
        if (job[3] != 0.0 || !std::isfinite(job[2])) return "a link weight live in the region is not finite or not > 0";
        if (loose) return "nothing pins the channel: no Dirichlet line, no UNKNOWN - KNOWN link and no data weight";
        wsum += job[0];
        ssum += job[2];
        unknowns += job[4];
        uksum += job[5];
        lcount += job[7];
        return nullptr;
    }
    float precond_constant(const PoissonGeo &g, const PcgGeo &wg, int mv) override
    {
        const double sbar = psmooth > 0.f ? (double)psmooth : unit_links || !(lcount > 0.0) ? 1.0 : ssum / lcount;
        // (a chunk without any UNKNOWN pixel: b = 0 on every plane, any regular M serves)
        const double wbar = plam > 0.f ? (double)plam : unknowns > 0.0 ? (wsum + uksum) / unknowns : sbar;
        // without a Dirichlet line the rectangle's A is singular: judge kept only jobs whose every channel has a KNOWN neighbour or weight
        assert(!(mixed_zero_eig(wg.ax) && mixed_zero_eig(wg.ay)) || wbar > 0.0);
        u0_scale = (float)(1.0 / sbar);
        return (float)(wbar / sbar);
    }
    int setup(const PoissonGeo &g, const PcgGeo &wg, bool lap, int mv, float *R, double *bb) override
    {
        PcgState &S = *I->pcg;
        for (DevBuf *b : { &S.e, &S.s, &S.dg }) {
            const int rc = ensure(I, *b, sizeof(float) * (size_t)wg.stride * g.C * mv, false);
            if (rc) return rc;
        }
        launch_region_setup(g, wg, lap, dj.data(), ds.data(), mv, R, (float *)S.e.p, (float *)S.s.p, (float *)S.dg.p, bb, I->stream);
        return SC_OK;
    }
    void out(const PoissonGeo &g, const PcgGeo &wg, int mv, const float *U, hipStream_t s) override
    {
        launch_region_out(g, wg, dj.data(), ds.data(), mv, U, s);
    }
};

// ---- the volume family (sc_volume.hip): the region system on a stack of T frames, plus temporal links between (q, t) and (q, t + 1)
// -- and, under periodic time, between (q, T - 1) and (q, 0).  A spatial link weighs sx / sy (NULL: 1), a temporal one lt = tau * smt
// rounded to float32 (smt NULL: tau).  A job's arrays hold T frames fs floats apart (gt, smt: T - 1, with periodic time T; element
// (q, t) belongs to the link from frame t to the next).  Work planes: one per (volume, channel), the frames stacked along y: wg.ny =
// T * (a frame's rows of unknowns), wg from VolumeOperator::work_geo.
struct VolumeJobs {
    enum { MAX = 16 }; PoissonJobDev j[MAX]; const float *w[MAX], *st[MAX], *gt[MAX], *sx[MAX], *sy[MAX], *smt[MAX];
    void set(int i, const PoissonJobDev &job, const SideArrays &a)
    {
        j[i] = job; w[i] = a.w; st[i] = a.st; gt[i] = a.gt; sx[i] = a.sx; sy[i] = a.sy; smt[i] = a.smt;
    }
};
struct VolumeGeo { int T, ny; long long fs; float tau; int periodic; };      // ny: a frame's rows of unknowns; periodic: time wraps
// the work planes' geometry of a volume of T frames of mg's unknowns (VolumeOperator::work_geo; sc_hip_pcg_plan)
inline PcgGeo volume_work_geo(const MixedGeo &mg, int T)
{
    MixedGeo tall = mg;
    tall.ny = mg.ny * T;
    return pcg_geo(tall);
}
constexpr int VOLUME_STATS = 11, VOLUME_STATS_PLAIN = 5;
// stats[(plane * PCG_PARTS + i) * VOLUME_STATS + ..] = the part's sum of w over the UNKNOWN pixels | how many of those w are invalid |
// its UNKNOWN pixels | the sum of its UNKNOWN - KNOWN links' weights, spatial and temporal | its state elements that are not 0, 1 or 2 |
// the sum of its spatial links live in the region (k_region_stats' owner rule) | how many there are | how many are invalid | the sum of
// its live temporal links lt (the earlier frame owns a link, frame T - 1 the wrapping one) | how many there are | how many are invalid.
// A call without any link array under free time (the first record's sx and smt NULL, vg.periodic 0) has parts of the first VOLUME_STATS_PLAIN
// fields alone, as sc_hip_volume always had: stats[(plane * PCG_PARTS + i) * VOLUME_STATS_PLAIN + ..].
// full: VOLUME_STATS fields per part whatever the call carries (the robust volume call: its rounds need the links' counts).
void launch_volume_stats(const PoissonGeo &g, const PcgGeo &wg, const VolumeGeo &vg, const PoissonJobDev *jobs, const SideArrays *sides, int m,
                         double *stats, hipStream_t s, bool full = false);
// R = b (the order: seamlessclone_hip.h, the volume sections); E / S / F = the link to the next column / row / frame where both ends are
// UNKNOWN (F in the last frame's rows: the wrapping link, 0 with free time); Dg = the sum of the incident live links plus w; all five 0
// at every pixel that is not UNKNOWN; bb = the parts of b . b
void launch_volume_setup(const PoissonGeo &g, const PcgGeo &wg, const VolumeGeo &vg, bool lap, const PoissonJobDev *jobs, const SideArrays *sides, int m,
                         float *R, float *E, float *S, float *F, float *Dg, double *bb, hipStream_t s);
// residual = false: Q = L P, parts of P . Q;  true: Q = Q - L P in place, parts of Q . Q
void launch_volume_op(const PcgGeo &wg, const VolumeGeo &vg, int planes, bool residual, const float *P, const float *E, const float *S, const float *F,
                      const float *Dg, float *Q, double *parts, hipStream_t s);
// D[k * T + t] = the orthonormal transform along the frames that diagonalises A_t (free time: the DCT-II; periodic time: the Hartley
// table, symmetric and its own inverse), computed in double, rounded to float32; lam[p * T + k] = the shift of mode k of every one of
// the `planes` work planes: (float)((wbar + tau mu_k) / sbar) as a double, mu_k = 2 - 2 cos(pi k / T), periodic: 2 - 2 cos(2 pi k / T)
void launch_volume_tables(int T, int planes, bool periodic, double wbar, double tau, double sbar, float *D, double *lam, hipStream_t s);
// out[p][k] = sum_t D[k][t] in[p][t] (transposed: sum_t D[t][k] in[p][t]) for every pixel of the frames of `planes` work planes
void launch_volume_dct(const PcgGeo &wg, const VolumeGeo &vg, int planes, bool transposed, const float *D, const float *in, float *out, hipStream_t s);
// the jobs' out, frame by frame: U at UNKNOWN pixels, data's bits at KNOWN and OUTSIDE pixels, boundary's bits on the Dirichlet lines
void launch_volume_out(const PoissonGeo &g, const PcgGeo &wg, const VolumeGeo &vg, const PoissonJobDev *jobs, const SideArrays *sides, int m,
                       const float *U, hipStream_t s);
// The operator of the volume families (sc_volume_api.cpp; its head comment says what it tells the iteration): sc_hip_volume's and
// sc_hip_volume_wls's, and through VolumeRobustOperator every round's of the robust volume call.  links, tlinks: the call's volumes
// carry smooth_x / smooth_y, smooth_t (a robust round: its own links, always); full_stats: the statistics in their VOLUME_STATS form
// whatever the call carries.
struct VolumeOperator : PcgOperator {
    Instance *const I;
    const int T;
    const long long fs;
    const float tau, plam, psmooth, ptau;
    const bool periodic;
    bool links, tlinks;
    // of the volumes that stay: the sums of w and of the UNKNOWN - KNOWN links, the UNKNOWN pixels, the sum and the number of the spatial
    // links live in the region and of the live temporal links
    double wsum = 0.0, unknowns = 0.0, uksum = 0.0, ssum = 0.0, scount = 0.0, tsum = 0.0, tcount = 0.0;
    float u0_scale = 1.f;                                          // 1 / s-bar
    VolumeOperator(Instance *I_, const sc_volume_wls_params *p, bool links_, bool tlinks_, int nround_ = 0, bool full_stats = false)
        : PcgOperator(full_stats || links_ || tlinks_ || p->time_periodic ? VOLUME_STATS : VOLUME_STATS_PLAIN, nround_), I(I_), T(p->frames),
          fs(p->frame_stride), tau(p->tau), plam(p->precond_lambda), psmooth(p->precond_smooth), ptau(p->precond_tau),
          periodic(p->time_periodic != 0), links(links_), tlinks(tlinks_) {}
    VolumeGeo geo(const PcgGeo &wg) const { return VolumeGeo{ T, wg.ny / T, fs, tau, periodic ? 1 : 0 }; }
    int chunk_planes(int C) const override { return C * T; }
    PcgGeo work_geo(const MixedGeo &mg) const override { return volume_work_geo(mg, T); }
    void begin() override;
    void stats(const PoissonGeo &g, const PcgGeo &wg, int m, double *d_stats, hipStream_t s) override;
    const char *judge(const PoissonGeo &g, int k, const double *st, int parts, bool no_dirichlet) override;
    float precond_constant(const PoissonGeo &g, const PcgGeo &wg, int mv) override;      // w-bar; the table along the frames and the modes' shifts go to the device here
    void scale_start(const PcgGeo &wg, int planes, float *U, hipStream_t s) override;
    // PcgState::tab: the shifts (double, planes * T of them at most SC_POISSON_MAX_PLANES) | the T x T table (float)
    double *shifts() const { return (double *)I->pcg->tab.p; }
    float *table() const { return (float *)(shifts() + SC_POISSON_MAX_PLANES); }
    int setup(const PoissonGeo &g, const PcgGeo &wg, bool lap, int mv, float *R, double *bb) override;
    void apply(const PcgGeo &wg, int planes, bool residual, const float *P, float *Q, double *parts, hipStream_t s) override;
    int precond(const PcgChunk &c, float, bool fp64, const float *in, float *out) override;
    void out(const PoissonGeo &g, const PcgGeo &wg, int mv, const float *U, hipStream_t s) override;
protected:
    // a subclass with statistics of its own length (the flow call's: VOLUME_FLOW_STATS)
    struct OwnStats { int nstat; };
    VolumeOperator(Instance *I_, const sc_volume_wls_params *p, bool links_, bool tlinks_, int nround_, OwnStats own)
        : PcgOperator(own.nstat, nround_), I(I_), T(p->frames), fs(p->frame_stride), tau(p->tau), plam(p->precond_lambda), psmooth(p->precond_smooth),
          ptau(p->precond_tau), periodic(p->time_periodic != 0), links(links_), tlinks(tlinks_) {}
};

// ---- the flow volume call (sc_volume_flow.hip, and the flow forms of sc_volume.hip's statistics and set-up): sc_hip_volume_wls's system
// with every temporal link along a whole-numbered flow.  Per volume two dense float32 arrays fx, fy without channel axis -- element
// (X, Y, t) at (t H + Y) W + X, T - 1 frames, with periodic time T -- say that pixel (X, Y) of frame t is pixel (X + fx, Y + fy) of the
// next frame.  The link planes: per volume (shared by its channels) two int32 planes of nx * T ny work-plane indices (t ny + y) nx + x,
// `stride` ints apart: fwd[i] = the element that i's link leads to, bwd[i] = the element whose link arrives at i, -1: none.  Matching
// (seamlessclone_hip.h, the flow section): a pixel is a candidate when both components are finite, whole, at most 1e6 in magnitude and
// its target lies in the work rectangle (a periodic axis wraps); of the candidates of one target the smallest index holds the link.
struct FlowLinks { const int *fwd, *bwd; long long stride; };      // of the launch's first volume
struct FlowArrays {                                                 // the flow arrays of a launch's volumes (the matching; the statistics count their fractional elements)
    enum { MAX = 16 }; const float *fx[MAX], *fy[MAX];
    void set(int i, const SideArrays &a) { fx[i] = a.fx; fy[i] = a.fy; }
};
// what the link planes index: a volume's work-plane elements nx * T ny.  A flow call needs them below INT_MAX (the planes' empty mark)
inline bool flow_indexable(const PcgGeo &wg) { return (long long)wg.nx * wg.ny < (long long)INT_MAX; }
constexpr int VOLUME_FLOW_STATS = VOLUME_STATS + 1;      // VOLUME_STATS' fields | the flow elements of the work rectangle that are finite and not whole
inline long long flow_link_stride(const PcgGeo &wg) { return ((long long)wg.nx * wg.ny + 3) / 4 * 4; }
// fwd and bwd of m volumes from their flow arrays (sides[k].fx, .fy): bwd = INT_MAX, every candidate's integer atomicMin(bwd[target],
// own index) -- the one atomic, its outcome independent of order --, then fwd[p] = target where bwd[target] == p and INT_MAX -> -1
void launch_flow_links(const PoissonGeo &g, const PcgGeo &wg, const VolumeGeo &vg, const SideArrays *sides, int m, int *fwd, int *bwd, hipStream_t s);
// launch_volume_stats in its VOLUME_FLOW_STATS form and launch_volume_setup with the temporal neighbours read through the link planes
void launch_volume_flow_stats(const PoissonGeo &g, const PcgGeo &wg, const VolumeGeo &vg, const PoissonJobDev *jobs, const SideArrays *sides, int m,
                              const int *fwd, const int *bwd, double *stats, hipStream_t s);
void launch_volume_flow_setup(const PoissonGeo &g, const PcgGeo &wg, const VolumeGeo &vg, bool lap, const PoissonJobDev *jobs, const SideArrays *sides,
                              int m, const int *fwd, const int *bwd, float *R, float *E, float *S, float *F, float *Dg, double *bb, hipStream_t s);
// launch_volume_op with tb = F[bwd[i]] P[bwd[i]] and tf = F[i] P[fwd[i]] (0 where there is none); C: the planes per volume
void launch_volume_flow_op(const PcgGeo &wg, const VolumeGeo &vg, int planes, int C, bool residual, const float *P, const float *E, const float *S,
                           const float *F, const float *Dg, const int *fwd, const int *bwd, float *Q, double *parts, hipStream_t s);

// ---- the sub-pixel flow volume call (sc_volume_subflow.hip): sc_hip_volume_wls's system with every temporal link a bilinear stencil
// along a real-valued flow -- the flow call's two arrays, their values taken as they are.  The link p holds has up to four taps in the
// next frame (seamlessclone_hip.h, the sub-pixel section: floorf, the float32 fractions and products, a tap of weight 0 left out); no
// matching: every candidate holds its link.  Per volume (shared by its channels) PcgState::lnk holds, in the order of the volumes that
// stay: off, n + 1 int64 row starts (n = nx * T ny work-plane elements; n + 2 apart), and ent, the rows' entries -- bits 0..31 the
// source's work-plane index, bits 32..63 the tap's float32 weight --, for every target the taps that arrive at it in ascending (source,
// tap) order (4 n apart; off[n] of them are set); fw, the flow cropped to the work rectangle, dx | dy (n floats each, 2 n apart), NaN
// where a pixel holds no link.  Behind them the build's scratch for one volume: keys in and out, values in, a pass's counts.
struct SubflowLinks { const long long *off; const unsigned long long *ent; const float *fw; long long n; };      // of the launch's first volume
struct SubflowStore { long long n; int per; size_t off_b, ent_b, fw_b, kin_b, kout_b, vin_b, tmp_b, tmp_bytes, total; };      // byte offsets into lnk
// the storage of a chunk of at most `per` volumes (the entries pass the call's own volumes where those are fewer than a chunk holds)
SubflowStore subflow_store(const PcgGeo &wg, int per);
// off, ent and fw of m volumes from their flow arrays (sides[k].fx, .fy), volume by volume: every tap slot's (target, (source, weight)),
// a stable radix sort by target (one stable split per key bit), every row's start by bisection.  Linear in the volume whatever the
// longest row; no atomics.
void launch_subflow_links(const PoissonGeo &g, const PcgGeo &wg, const VolumeGeo &vg, const SideArrays *sides, int m, const SubflowStore &st, void *lnk,
                                hipStream_t s);
// launch_volume_stats in its full form with the temporal fields of the bilinear links (a link counted once, at its source; in the
// UNKNOWN - KNOWN sum lt * (1 where the source is KNOWN, else the sum of b over its KNOWN taps))
void launch_volume_subflow_stats(const PoissonGeo &g, const PcgGeo &wg, const VolumeGeo &vg, const PoissonJobDev *jobs, const SideArrays *sides, int m,
                                 const SubflowStore &st, void *lnk, double *stats, hipStream_t s);
// two launches: LT = the weight of the link every element holds where it is live (else 0) and SG = lt * (gt less the KNOWN taps' b * data,
// plus data at a KNOWN source); then launch_volume_setup's planes with b's temporal part SG(i) - sum over the arrivals of b SG(source),
// F = 1 at UNKNOWN pixels (else 0) and Dg = the spatial links and w alone.  SG may be the plane launch_volume_subflow_op overwrites.
void launch_volume_subflow_setup(const PoissonGeo &g, const PcgGeo &wg, const VolumeGeo &vg, bool lap, const PoissonJobDev *jobs, const SideArrays *sides,
                                 int m, const SubflowStore &st, void *lnk, float *LT, float *SG, float *R, float *E, float *S, float *F, float *Dg,
                                 double *bb, hipStream_t s);
// two launches: RHO(p) = LT(p) (sum_k b_k F P at the taps - F(p) P(p)); then launch_volume_op with the temporal part F(i) (RHO(i) - sum
// over the arrivals of b RHO(source)); C: the planes per volume
void launch_volume_subflow_op(const PcgGeo &wg, const VolumeGeo &vg, int planes, int C, bool residual, const SubflowStore &st, const void *lnk, const float *P,
                              const float *E, const float *S, const float *F, const float *Dg, const float *LT, float *RHO, float *Q, double *parts,
                              hipStream_t s);

// ---- the robust family (sc_robust.hip): the WLS system of one reweighting round, its links and weights taken at an iterate
// one penalty phi_r(t) = (2 / r) (t^2 + eps^2)^(r/2) as the kernel takes it: mode 0: r = 2 (rho = 1), 1: r = 1 (rho = 1 / sqrt), 2: powf;
// eps2 = eps * eps rounded to float32, half_exp = (r - 2) / 2, scale = 2 / r
struct RobustTerm { int mode; float eps2, half_exp, scale; };
inline RobustTerm robust_term(float r, float eps)
{
    RobustTerm t;
    t.mode = r == 2.f ? 0 : r == 1.f ? 1 : 2;
    t.eps2 = t.mode ? eps * eps : 0.f;
    t.half_exp = (r - 2.f) * 0.5f;
    t.scale = 2.f / r;
    return t;
}
// what the robust calls' checks refuse of an exponent and of its eps
inline bool robust_bad_exponent(float r) { return !(r > 0.f && r <= 2.f); }
inline bool robust_bad_eps(float r, float eps) { return r != 2.f && !(std::isfinite(eps) && eps > 0.f); }
// the two bits of sc_robust_params::kind that are the robust calls' own (the families' kinds know nothing of them), and the launches' word for them
constexpr int COUPLING_BITS = SC_ROBUST_ISOTROPIC | SC_ROBUST_JOINT_CHANNELS;
// (ROBUST_TIME: the coupled volume call's third word -- the forward temporal link shares the pixel's magnitude; it comes with ROBUST_ISO)
constexpr int ROBUST_ISO = 1, ROBUST_JOINT = 2, ROBUST_TIME = 4;
// The reweighting rounds of a robust call: what robust_chunk (sc_robust_api.cpp) asks of an operator beyond PcgOperator
// (PcgOperator::rounds).  The penalties (time: the volume call's; elsewhere exponent 2), max_rounds and round_tol as the caller gave
// them, the caller's coupling bits as ROBUST_ISO | ROBUST_JOINT (from kind; the coupled volume call's come as launch words of their
// own, `launch_bits`, ROBUST_TIME among them).  A later round is reweigh() -- the one place that says what a round
// does --, of which an operator provides three things:
//   nsums   the doubles per part its round launch sums, the energy last (ROBUST_SUMS, REGION_ROBUST_SUMS, VOLUME_ROBUST_SUMS);
//   launch  the set-up at the iterate c.U in place of the operator's system: b into c.R, the coefficient planes, the parts of b . b into
//           c.d_bb, the sums into c.d_round; under a coupling (coupling(C), not 0) the two launches of the coupled forms, PcgState::rho
//           ensured, the gradient energy's parts behind the sums at `esum`;
//   take    the folded sums (nsums - 1 totals, in the launch's order) in place of the statistics' sums, and the operator's flag that
//           later rounds' links are the iterate's (the counts of links and of UNKNOWN pixels stay round 0's: states do not change).
struct RobustRounds {
    const RobustTerm grad, data, time;
    const int max_rounds;
    const float round_tol;
    const int bits, nsums;
    RobustRounds(const RobustTerm &grad_, const RobustTerm &data_, const RobustTerm &time_, int max_rounds_, float round_tol_, int kind, int nsums_,
                 int launch_bits = 0)
        : grad(grad_), data(data_), time(time_), max_rounds(max_rounds_), round_tol(round_tol_),
          bits(((kind & SC_ROBUST_ISOTROPIC) ? ROBUST_ISO : 0) | ((kind & SC_ROBUST_JOINT_CHANNELS) ? ROBUST_JOINT : 0) | launch_bits), nsums(nsums_) {}
    RobustRounds(const sc_robust_params &p, int nsums_)
        : RobustRounds(robust_term(p.p_grad, p.eps_grad), robust_term(p.p_data, p.eps_data), robust_term(2.f, 0.f), p.max_rounds, p.round_tol, p.kind,
                       nsums_) {}
    virtual ~RobustRounds() = default;
    bool quadratic() const { return grad.mode == 0 && data.mode == 0 && time.mode == 0; }      // every exponent is 2: no round runs
    // the coupling that changes anything: none with p_grad = 2 (every form is sum c t^2), no joint form of one channel (the volume
    // call has a rule of its own: its temporal penalty counts too)
    virtual int coupling(int C) const { return grad.mode == 0 ? 0 : C == 1 ? bits & ~ROBUST_JOINT : bits; }
    virtual int launch(PcgChunk &c, int coupling, double *esum) = 0;
    virtual void take(const double *totals) = 0;
    // One round's system, its means and the energy of the chunk's iterate per unit of the round rule -- a plane, or a job where the
    // channels are coupled (one host wait)
    int reweigh(PcgChunk &c, std::vector<double> &energy);
};
// One chunk of a robust call (sc_robust_api.cpp; a PcgChunkFn): the quadratic round, the reweighting rounds of op.rounds(), the output,
// PcgState's trace
int robust_chunk(Instance *I, const PcgCall &call, const PoissonGeo &g, PcgOperator &op, int *const *rcs, int m, PcgChunkResult &res, int &job_errors);
// What the image and the region call's entries share (sc_robust_api.cpp).  robust_validate: the check of either, `size_why` the family's
// reason against more than 8192 unknowns per side.  robust_penalties_why: the penalties' own reason against a call, NULL: none -- the
// exponents (p_why), their eps (eps_why), tol, round_tol, the base kind; the volume call's check has it too.  robust_begin: pcg_begin
// with robust_validate, and the call without the coupling bits (poisson_norm_kind passes them through; RobustRounds has them from p).
struct RobustPenalty { float p, eps; };
struct RobustFamily { const char *size_why, *method_why, *fp64_why; };
const char *robust_penalties_why(std::initializer_list<RobustPenalty> terms, const char *p_why, const char *eps_why, float tol, float round_tol, int kind);
int robust_validate(const sc_robust_params *p, const sc_poisson_layout *l, const char *size_why, const char **why);
int robust_begin(void *inst, const sc_robust_params *p, const sc_poisson_layout *l, const RobustFamily &f, Instance *&I, PcgCall &call);
constexpr int ROBUST_SUMS = 3;
// the robust volume call's launch (sc_volume_robust.hip): launch_volume_setup in its guidance form with s = c rho(link residual of U)
// on every live link -- c: sx, sy (NULL: 1) with `grad`, lt = tau * smt (NULL: tau) with `time` -- and w' = w rho(U - d) with `data`;
// the value of u across a link is data's at a KNOWN pixel, boundary's on a Dirichlet line, U's at an UNKNOWN one.  sums[(plane *
// PCG_PARTS + i) * VOLUME_ROBUST_SUMS + ..] = the part's sum of w' | of its live spatial links s | of its live temporal links | of its
// UNKNOWN - KNOWN links | the energy of U; every live link once, by launch_volume_stats' owner rule
constexpr int VOLUME_ROBUST_SUMS = 5;
void launch_volume_robust_setup(const PoissonGeo &g, const PcgGeo &wg, const VolumeGeo &vg, const PoissonJobDev *jobs, const SideArrays *sides, int m,
                                const RobustTerm &grad, const RobustTerm &time, const RobustTerm &data, const float *U, float *R, float *E, float *S,
                                float *F, float *Dg, double *bb, double *sums, hipStream_t s);
// the robust flow volume call's launch (sc_volume_flow_robust.hip): launch_volume_robust_setup with the two temporal neighbours of an
// element read through the volumes' link planes (fwd, bwd as launch_flow_links left them, in the jobs' order) -- the held link's lt and
// gt at the element itself, the arriving link's at its source, the neighbour's value U[fwd[i]] / U[bwd[i]] where it is UNKNOWN; the
// same sums, a temporal link counted once at its source
void launch_volume_flow_robust_setup(const PoissonGeo &g, const PcgGeo &wg, const VolumeGeo &vg, const PoissonJobDev *jobs, const SideArrays *sides, int m,
                                     const RobustTerm &grad, const RobustTerm &time, const RobustTerm &data, const int *fwd, const int *bwd,
                                     const float *U, float *R, float *E, float *S, float *F, float *Dg, double *bb, double *sums, hipStream_t s);
// the robust sub-pixel flow volume call's launch (sc_volume_subflow_robust.hip), two kernels on one grid: k_subflow_robust_sigma writes
// LT = robust_link(time, lt, sum_k b_k u~(q_k), u~(p), gt).s of every live bilinear link at its source and SG = LT * g' where
// launch_volume_subflow_setup writes them (u~: U at an UNKNOWN pixel, data at a KNOWN one) and its block's temporal sums into tp
// (subflow_robust_partials(planes) doubles); k_subflow_robust_setup is launch_volume_robust_setup's spatial walk with
// launch_volume_subflow_setup's temporal part of b, F and Dg, and adds its block's tp into the sums: launch_volume_robust_setup's five
// fields, a temporal link counted once, at its source, with launch_volume_subflow_stats' UNKNOWN - KNOWN share
size_t subflow_robust_partials(int planes);
void launch_volume_subflow_robust_setup(const PoissonGeo &g, const PcgGeo &wg, const VolumeGeo &vg, const PoissonJobDev *jobs, const SideArrays *sides, int m,
                                        const RobustTerm &grad, const RobustTerm &time, const RobustTerm &data, const SubflowStore &st, void *lnk,
                                        const float *U, float *LT, float *SG, double *tp, float *R, float *E, float *S, float *F, float *Dg, double *bb,
                                        double *sums, hipStream_t s);
// the coupled volume call's two launches (sc_volume_coupled.hip; coupling: ROBUST_ISO | ROBUST_TIME | ROBUST_JOINT, not 0 and effective):
// k_volume_robust_rho writes rho of every owner's magnitudes to the rho planes and esum as launch_robust_coupled (the gradient-and-time
// energy's parts; under ROBUST_JOINT on the volume's channel-0 plane only), k_volume_robust_setup_rho is launch_volume_robust_setup with
// s read from them, field 4 of its sums the data term's energy alone.  The rho planes: per unit (a volume under ROBUST_JOINT, else a
// work plane) `unit` floats, its components at ox, oy, ot -- one under ROBUST_ISO | ROBUST_TIME, xy | t under ROBUST_ISO, else x | y |
// t; a component whose penalty has exponent 2 is not stored -- of T frames `fstride` floats apart, rows of rw = x0 + nx floats.
struct VolumeRhoGeo { int rw; long long fstride, ox, oy, ot, unit; };
inline VolumeRhoGeo volume_rho_geo(const PcgGeo &wg, const VolumeGeo &vg, const RobustTerm &grad, const RobustTerm &time, int coupling)
{
    VolumeRhoGeo r{ wg.x0 + wg.nx, ((long long)(wg.x0 + wg.nx) * (wg.y0 + vg.ny) + 63) / 64 * 64, 0, 0, 0, 0 };
    const long long comp = r.fstride * vg.T;
    long long n = 0;
    if (grad.mode != 0) {
        r.ox = n; n += comp;
        r.oy = (coupling & ROBUST_ISO) ? r.ox : n;
        if (!(coupling & ROBUST_ISO)) n += comp;
    }
    if (coupling & ROBUST_TIME) r.ot = r.ox;
    else if (time.mode != 0) { r.ot = n; n += comp; }
    r.unit = n;
    return r;
}
inline size_t volume_rho_floats(const VolumeRhoGeo &rg, int C, int m, int coupling) { return (size_t)rg.unit * ((coupling & ROBUST_JOINT) ? m : C * m); }
void launch_volume_robust_coupled(const PoissonGeo &g, const PcgGeo &wg, const VolumeGeo &vg, const PoissonJobDev *jobs, const SideArrays *sides, int m,
                                  const RobustTerm &grad, const RobustTerm &time, const RobustTerm &data, int coupling, const float *U, float *Rho,
                                  float *R, float *E, float *S, float *F, float *Dg, double *bb, double *sums, double *esum, hipStream_t s);
// the coupled flow volume call's two launches (sc_volume_flow_coupled.hip): launch_volume_robust_coupled with the temporal neighbours of
// an element read through the volumes' link planes (fwd, bwd as launch_flow_links left them, in the jobs' order).  The owner of a
// temporal link is its source: its rho is written at the source's own [frame][Y][X] element of the t-component (under ROBUST_TIME: of
// the one component, with the source's spatial links in the magnitude) and read there by the pixel it arrives at, through bwd.  The
// same rho planes, sums and esum; a temporal link is counted once, at its source.
void launch_volume_flow_robust_coupled(const PoissonGeo &g, const PcgGeo &wg, const VolumeGeo &vg, const PoissonJobDev *jobs, const SideArrays *sides,
                                       int m, const RobustTerm &grad, const RobustTerm &time, const RobustTerm &data, int coupling, const int *fwd,
                                       const int *bwd, const float *U, float *Rho, float *R, float *E, float *S, float *F, float *Dg, double *bb,
                                       double *sums, double *esum, hipStream_t s);
// k_wls_setup with s = c rho_p(link residual of U), w' = w rho_q(U - d) (c = sx, sy; NULL for every job: 1): R = b, E, S, Dg as
// launch_wls_setup in its guidance form, bb = the parts of b . b, sums[(plane * PCG_PARTS + i) * ROBUST_SUMS + ..] = the part's sum of
// w' | the sum of its live links s, each counted once as launch_wls_stats counts them | the energy of U
void launch_robust_setup(const PoissonGeo &g, const PcgGeo &wg, const PoissonJobDev *jobs, const SideArrays *sides, int m, const RobustTerm &grad, const RobustTerm &data, const float *U, float *R, float *E, float *S,
                         float *Dg, double *bb, double *sums, hipStream_t s);
// The coupled forms (SC_ROBUST_ISOTROPIC, SC_ROBUST_JOINT_CHANNELS; p_grad < 2 only): one magnitude M over the links that share a
// penalty, s = c rho_p(M) on each of them.  Two launches: k_robust_rho writes rho of every owner (a link's low end) to the rho planes
// -- addressed by pixel, rows of x0 + nx floats, robust_rho_stride apart; per unit (a job under ROBUST_JOINT, else a plane) one plane
// (ROBUST_ISO) or two (x-links, y-links) -- and esum[plane * PCG_PARTS + i] = the part's gradient energy, under ROBUST_JOINT on the
// job's channel-0 plane only (the others' are not written); k_robust_setup_rho is launch_robust_setup with s read from those planes,
// field 2 of its sums the data term's energy alone.
inline long long robust_rho_stride(const PcgGeo &wg) { return ((long long)(wg.x0 + wg.nx) * (wg.y0 + wg.ny) + 63) / 64 * 64; }
inline size_t robust_rho_floats(const PcgGeo &wg, int C, int m, int coupling)
{
    return (size_t)robust_rho_stride(wg) * ((coupling & ROBUST_ISO) ? 1 : 2) * ((coupling & ROBUST_JOINT) ? m : C * m);
}
void launch_robust_coupled(const PoissonGeo &g, const PcgGeo &wg, const PoissonJobDev *jobs, const SideArrays *sides, int m, const RobustTerm &grad, const RobustTerm &data, int coupling, const float *U, float *Rho,
                           float *R, float *E, float *S, float *Dg, double *bb, double *sums, double *esum, hipStream_t s);
// the robust region call's launches (sc_region_robust.hip): launch_region_setup in its guidance form with s = c rho_p(link residual of U)
// on every link live in the region (c = sx, sy; NULL: 1) and w' = w rho_q(U - d) (w NULL: no data term); the value of u across a link is
// data's at a KNOWN pixel, boundary's on a Dirichlet line, U's at an UNKNOWN one.  sums[(plane * PCG_PARTS + i) * REGION_ROBUST_SUMS + ..]
// = the part's sum of w' | of its live links s | of its UNKNOWN - KNOWN links s | the energy of U; every live link once, by
// launch_region_stats' owner rule.  No allocation, no synchronise.
constexpr int REGION_ROBUST_SUMS = 4;
void launch_region_robust_setup(const PoissonGeo &g, const PcgGeo &wg, const PoissonJobDev *jobs, const SideArrays *sides, int m,
                                const RobustTerm &grad, const RobustTerm &data, const float *U, float *R, float *E, float *S, float *Dg,
                                double *bb, double *sums, hipStream_t s);
// its coupled forms (coupling: ROBUST_ISO | ROBUST_JOINT, not 0; p_grad < 2): launch_robust_coupled's two launches restricted to the
// links live in the region -- k_region_robust_rho writes rho of every owner with a live link to the rho planes (robust_rho_stride,
// robust_rho_floats) and esum as launch_robust_coupled, k_region_robust_setup_rho is launch_region_robust_setup with s read from them,
// field 3 of its sums the data term's energy alone
void launch_region_robust_coupled(const PoissonGeo &g, const PcgGeo &wg, const PoissonJobDev *jobs, const SideArrays *sides, int m,
                                  const RobustTerm &grad, const RobustTerm &data, int coupling, const float *U, float *Rho, float *R, float *E,
                                  float *S, float *Dg, double *bb, double *sums, double *esum, hipStream_t s);

// ---- the bounded family (sc_bounded.hip): the region system under lower <= u <= upper at the UNKNOWN pixels, by the primal-dual active
// set method -- every round the region system with the active pixels held at their bound (seamlessclone_hip.h, the bounded section).  A
// set plane lies beside the work planes (PcgGeo::stride apart): 0 free, +1 upper-active, -1 lower-active, 0 at a pixel that is not UNKNOWN.
struct BoundedJobs {
    enum { MAX = 16 }; PoissonJobDev j[MAX]; const float *w[MAX], *sx[MAX], *sy[MAX], *st[MAX], *lo[MAX], *hi[MAX];
    void set(int i, const PoissonJobDev &job, const SideArrays &a)
    {
        j[i] = job; w[i] = a.w; sx[i] = a.sx; sy[i] = a.sy; st[i] = a.st; lo[i] = a.lo; hi[i] = a.hi;
    }
};
struct BoundScalars { float lo, hi; };      // the bounds of a job without the array
constexpr int BOUNDED_SUMS = 3;
// bad[plane * PCG_PARTS + i] = the part's UNKNOWN pixels whose bound is NaN or whose lower > upper
void launch_bounded_stats(const PoissonGeo &g, const PcgGeo &wg, const BoundScalars &bs, const PoissonJobDev *jobs, const SideArrays *sides, int m,
                          double *bad, hipStream_t s);
// r = L u - b of the original system at every pixel active in `cur` (the rule asks for it nowhere else), u read through that set (an
// active pixel: its bound), and the set rule: the next set into `next`; sums[(plane * PCG_PARTS + i) * BOUNDED_SUMS + ..] = the part's pixels whose set changed | its active pixels
void launch_bounded_mark(const PoissonGeo &g, const PcgGeo &wg, bool lap, const BoundScalars &bs, const PoissonJobDev *jobs, const SideArrays *sides,
                         int m, const float *U, const float *cur, float *next, double *sums, hipStream_t s);
// launch_region_setup with the pixels active in `set` treated as KNOWN at their bound; U = the bound wherever `set` or `prev` (the set
// of the solve before) is active; sums[..] = the part's sum of w over the free pixels | of its links from a free pixel to a KNOWN or
// active one | its free pixels
void launch_bounded_setup(const PoissonGeo &g, const PcgGeo &wg, bool lap, const BoundScalars &bs, const PoissonJobDev *jobs, const SideArrays *sides,
                          int m, const float *set, const float *prev, float *U, float *R, float *E, float *S, float *Dg, double *bb, double *sums,
                          hipStream_t s);
// the jobs' out: the bound's bits at the pixels active in `set`, U clamped into its bounds at the free ones, data's bits at KNOWN and
// OUTSIDE pixels, boundary's bits on the Dirichlet lines
void launch_bounded_out(const PoissonGeo &g, const PcgGeo &wg, const BoundScalars &bs, const PoissonJobDev *jobs, const SideArrays *sides, int m,
                        const float *U, const float *set, hipStream_t s);

} // namespace sc
