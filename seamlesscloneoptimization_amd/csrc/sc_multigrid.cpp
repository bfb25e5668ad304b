// sc_multigrid.cpp -- geometric multigrid V-cycle for the ROI Poisson system (SURVEY.md
// section 8 row f1): red-black GS smoothing, residual in double, normalised-transpose
// restriction, bilinear prolongation, on the hierarchy sc_mg_levels.cpp builds.
// Level 0 runs the exact 5-point kernels of the sweep solvers; coarser levels the general
// ones.  Converges ~20x per V(2,2) cycle at every size tried (tools/mg_proto2.py).
// In this file: the cycle (vcycle, the bottom and tail launches), the predicates that choose the
// field formats, the stop rule, the schedule of a fused solve's level-0 launches and the two drivers.
#include "sc_instance.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <cstdlib>

namespace sc {

static int run_bottom(Instance *I, size_t l0, int pre, int post)
{
    MGBottomArgs a;
    a.nlevels = (int)(I->mg.size() - l0);
    a.pre = pre; a.post = post;
    const MGLevel &last = I->mg.back();
    a.coarse_sweeps = std::max(8, std::min(64, 2 * std::max(last.g.x.n, last.g.y.n)));
    int off = 0;
    for (int i = 0; i < a.nlevels; ++i) {
        const MGLevel &L = I->mg[l0 + i];
        a.lv[i].g = L.g; a.lv[i].omega = L.omega;
        a.lv[i].pitch = bottom_pitch(L);
        const int plane = a.lv[i].pitch * (L.g.y.n + 2);
        a.lv[i].offU = off; a.lv[i].offF = off + plane;
        off += 2 * plane;
    }
    a.fd_level = I->fd_level; a.fd_nxp = I->fd_nxp; a.fd_nyp = I->fd_nyp;
    a.fd_mats = (const float *)I->mg_fd.p;
    a.fd_off = 0;
    if (a.fd_level >= 0) {
        // levels below the directly solved one are not visited: the FD region takes their place in LDS
        a.fd_off = (a.lv[a.fd_level].offF + a.lv[a.fd_level].pitch * (I->mg[l0 + a.fd_level].g.y.n + 2) + 3) & ~3;
        off = a.fd_off + (int)fd_lds_floats(a.fd_nxp, a.fd_nyp);
    }
    a.lds_floats = off;
    a.Ftop = I->mg[l0].F;
    a.Utop = I->mg[l0].U;
    int rc;
    if ((rc = fd_wait(I))) return rc;          // the matrices of a new hierarchy are being built on the second stream (build_fd)
    if (I->fd_mm && I->fd_level == 0) {      // the usual case: this level solved directly on the matrix cores, nothing below it is visited
        MGBottomMM m;
        m.mm = (const unsigned char *)((const float *)I->mg_fd.p + I->fd_mm_off);
        m.Ftop = I->mg[l0].F; m.Utop = I->mg[l0].U;
        m.nx = I->mg[l0].g.x.n; m.ny = I->mg[l0].g.y.n;
        if (launch_mg_bottom_mm(m, I->fd_npx, I->fd_npy, I->F.C, I->stream)) return SC_OK;
    }
    launch_mg_bottom(a, I->F.C, I->stream);
    return SC_OK;
}

// The level above the bottom and the bottom in one launch (k_mg_tail): level l is that level, the bottom's first level is the one
// solved directly on the matrix cores with at most 64 padded unknowns per side, and l itself is a plain float level (>= 2: level 1
// has its own composed / float16 forms).
bool tail_serves(const Instance *I, size_t l)
{
    if (l < 2 || l + 1 != I->mg_bottom || legacy_path(I->opts, SC_LEGACY_SEPARATE_TAIL) || I->opts.sweeps_per_launch == 1) return false;
    if (!I->fd_mm || I->fd_level != 0 || I->fd_npx > 64 || I->fd_npy > 64) return false;
    if (mg_params(I->opts).pre < 1) return false;          // the launch takes the residual of the colour swept last as zero
    const MGGeom &g = I->mg[l].g;
    return g.x.n <= 127 && g.y.n <= 127 && g.x.nc <= 63 && g.y.nc <= 63;
}

int run_tail(Instance *I, size_t l, int pre, int post, bool &done, unsigned long long *stamps)
{
    done = false;
    MGTail t;
    t.stamps = stamps;
    t.mm = (const unsigned char *)((const float *)I->mg_fd.p + I->fd_mm_off);
    t.F = I->mg[l].F; t.U = I->mg[l].U; t.g = I->mg[l].g; t.pre = pre; t.post = post;
    t.rag = I->rag.dev; t.lev = (int)l; t.rag_uniform = I->rag.pad_uniform;
    int rc;
    if ((rc = fd_wait(I))) return rc;
    done = launch_mg_tail(t, I->fd_npx, I->fd_npy, I->F.C, I->stream);
    return SC_OK;
}

// Smoothing of a coarse level (l >= 1) with the fused general kernel; U <-> T ping-pong, both
// carry zero rings.  mode (first launch only): TBM_ZEROIN = the current correction is all zero
// (nothing is read), TBM_PROLONG = add the interpolated correction of level l+1 while loading.
static int smooth_gen(Instance *I, size_t l, int n, int mode, Field E)
{
    MGLevel &L = I->mg[l];
    int left = n;
    while (left > 0) {
        const int T = std::min(2, left);
        if (!launch_rb_tb_gen(L.U, L.T, L.F, T, L.g, mode, E, I->stream, I->rag.dev, (int)l, !legacy_path(I->opts, SC_LEGACY_UNPACKED_TILES))) {
            if (I->rag.dev) { I->err = "size class: coarse-level form not instantiated"; return SC_ERR_BAD_ARG; }
            break;
        }
        std::swap(L.U, L.T);
        mode = TBM_PLAIN;
        left -= T;
    }
    if (left > 0 && mode != TBM_PLAIN) return SC_ERR_BAD_ARG; // cannot happen: depths 1 and 2 always exist
    for (int s = 0; s < left; ++s) {
        launch_rb_half_gen(L.U, L.F, 0, 1.0f, L.g, I->stream);
        launch_rb_half_gen(L.U, L.F, 1, 1.0f, L.g, I->stream);
    }
    return SC_OK;
}

// no_post: bit l set = level l gets no post-smoothing and no prolongation launch of its own -- the level above interpolates
// from "its correction + the interpolated correction of the level below" directly (sc_mg_device.h, ComposeArgs).  Used for
// level 1 (composed by the level-0 launch); doing the same for level 3 inside level 2's post launch was measured neutral
// (481 vs 494 us for a single 2048^2 clone, no change in throughput) and is not kept.
int vcycle(Instance *I, size_t l, int pre, int post, unsigned no_post)
{
    const bool skip_post = l > 0 && l < 32 && ((no_post >> l) & 1u);
    MGLevel &L = I->mg[l];
    int rc;
    if (l > 0 && l == I->mg_bottom) return run_bottom(I, l, pre, post);
    if (!skip_post && tail_serves(I, l)) {
        bool done = false;
        if ((rc = run_tail(I, l, pre, post, done)) || done) return rc;
        if (I->rag.dev) { I->err = "size class: the bottom launch does not serve this shape"; return SC_ERR_BAD_ARG; }
    }
    if (l + 1 == I->mg.size()) { // coarsest level outside the bottom kernel: SOR with its optimal factor
        const int n = std::max(8, std::min(64, 2 * std::max(L.g.x.n, L.g.y.n)));
        if (l == 0) return run_sweeps(I, SC_METHOD_SOR, n, L.omega, 1);
        launch_fill_zero(L.U, I->stream);
        for (int s = 0; s < n; ++s) {
            launch_rb_half_gen(L.U, L.F, 0, L.omega, L.g, I->stream);
            launch_rb_half_gen(L.U, L.F, 1, L.omega, L.g, I->stream);
        }
        return SC_OK;
    }
    MGLevel &Lc = I->mg[l + 1];
    // a level without post-smoothing does all its sweeps before the restriction
    int pre_here = pre;
    if (skip_post) {
        const int want = I->opts.mg_level1_sweeps > 0 ? I->opts.mg_level1_sweeps : 4;   // measured (tests/tools/level1_sweeps.py): 3 sweeps are 5 % faster per cycle but full-range noise then needs a 4th cycle
        pre_here = std::max(pre, std::min(want, pre + post));
    }
    // ---- pre-smoothing (levels >= 1 start from a zero correction), residual + restriction
    bool restricted = false;
    if (l == 0) {
        if ((rc = run_sweeps(I, SC_METHOD_RBGS, pre_here, 1.0f, I->opts.sweeps_per_launch))) return rc;
    } else if (pre_here > 0 && I->opts.sweeps_per_launch != 1 &&
               launch_cycle_coarse(L.T, L.F, Lc.F, L.g, pre_here, I->stream, l == 1 && skip_post && mg_level1_half(I), I->rag.dev, (int)l,
                                   !legacy_path(I->opts, SC_LEGACY_UNPACKED_TILES))) {
        std::swap(L.U, L.T);      // one launch did all three
        restricted = true;
    } else if (I->rag.dev) {
        I->err = "size class: coarse-level form not instantiated"; return SC_ERR_BAD_ARG;
    } else if (pre_here > 0) {
        if ((rc = smooth_gen(I, l, pre_here, TBM_ZEROIN, Field{}))) return rc;
    } else {
        launch_fill_zero(L.U, I->stream);
    }
    if (!restricted) launch_residual_restrict(l == 0 ? result(I) : L.U, L.F, Lc.F, L.g, I->stream);
    if ((rc = vcycle(I, l + 1, pre, post, no_post))) return rc;
    if (skip_post) return SC_OK;
    // ---- prolongation fused into the first post-smoothing launch
    if (l == 0) {
        const int T = std::min(2, post);
        int nb = 0;
        if (T > 0 && I->opts.sweeps_per_launch != 1) {
            Field &in = result(I);
            Field &out = I->result_in_U1 ? I->U0 : I->U1;
            nb = launch_rb_tb_prolong0(in, out, I->F, T, L.g, Lc.U, (float *)I->mg_partial.p, I->stream);
        }
        if (nb > 0) {
            I->result_in_U1 = !I->result_in_U1;
            I->info.sweep_launches += 1;
            launch_max_final((const float *)I->mg_partial.p, nb, I->d_maxcorr, I->stream);
            if ((rc = run_sweeps(I, SC_METHOD_RBGS, post - T, 1.0f, I->opts.sweeps_per_launch))) return rc;
        } else {
            launch_prolong_add(Lc.U, result(I), L.g, (float *)I->mg_partial.p, I->d_maxcorr, I->stream);
            if ((rc = run_sweeps(I, SC_METHOD_RBGS, post, 1.0f, I->opts.sweeps_per_launch))) return rc;
        }
    } else if (post > 0) {
        if ((rc = smooth_gen(I, l, post, TBM_PROLONG, Lc.U))) return rc;
    } else {
        launch_prolong_add(Lc.U, L.U, L.g, nullptr, nullptr, I->stream);
    }
    return SC_OK;
}

// The fused level-0 cycle kernel is the only reader of the right-hand side that understands float16; every other
// path (sweep solvers, unfused cycle, residual-based stop rule, stage hooks) needs the float field.
static bool fused_level0(const sc_solver_opts &o)
{
    const int pre = mg_params(o).pre, post = mg_params(o).post;
    return o.sweeps_per_launch != 1 && pre >= 1 && pre <= 2 && post >= 1 && post <= 2;   // the forms sc_cycle0.hip instantiates
}

// Fused solve on the current hierarchy: does level 1 run pre-smoothing only, with the level-0 launch composing its
// prolongation source from levels 1 and 2 (sc_cycle0.hip, ComposeArgs)?  Needs a launched level 1 with a level 2 below
// it and the standard 2 + 2 cycle.  The contraction per cycle is within a few percent of the full V(2,2)
// (oracle/mg_np.py runs the same schedule); one launch per cycle less is worth ~10 % of the clone throughput.
bool mg_composes_level1(const Instance *I)
{
    const sc_solver_opts &o = I->opts;
    const int pre = mg_params(o).pre, post = mg_params(o).post;
    return !(o.flags & SC_FLAG_NO_COMPOSE_L1) && mg_ladder_composes(I->mg.size(), I->mg_bottom) && pre == 2 && post == 2;
}

// Level 1 with float16 fields (sc_cycle0.hip, TAG bit 7): the composed schedule on the float16 right-hand side -- the default
// fast path -- with level 1's standard four sweeps (the only depth the float16 level-1 launch is instantiated for).
bool mg_level1_half(const Instance *I)
{
    const sc_solver_opts &o = I->opts;
    return !(o.flags & SC_FLAG_FLOAT_L1) && mg_composes_level1(I) && I->f_half && fused_level0(o) && o.tol <= 0.f &&
           (o.mg_level1_sweeps == 0 || o.mg_level1_sweeps == 4);
}

// The field between the FIRST level-0 launches of a solve as 16-bit fixed point (sc_cycle0.hip, TAG bits 8, 9): the fast path
// with float16 level-1 fields whose last cycle leaves output bytes (`out_wanted` in mg_solve).  The launch before the judged
// cycle reads the 16-bit field and writes float: the judged cycle, and a solve that goes on after it, run on float fields, and
// two cycles lie between the last rounding (<= 1/128) and the output.
static bool mg_field_q16(const Instance *I, bool out_wanted)
{
    return out_wanted && I->u_half && !(I->opts.flags & SC_FLAG_FLOAT_FIELD) && !I->force_float_field && mg_level1_half(I);
}

bool mg_reads_half_rhs(const Instance *I)
{
    const sc_solver_opts &o = I->opts;
    // at least two levels: min(W, H) - 2 > 3 (build_levels)
    return !(o.flags & (SC_FLAG_FLOAT_RHS | SC_FLAG_OPENCV_GREY_MASK)) && !I->edit_call && effective_method(I) == SC_METHOD_MULTIGRID && o.tol <= 0.f && fused_level0(o) && std::min(I->F.W, I->F.H) - 2 > 3;
}

// What every level-0 launch of the fused solve says alike (sc_cycle0.hip): the solution and its partner, the right-hand sides, level 1's correction
// (E: read by a launch that prolongs; composed: on the composed schedule, mg_composes_level1), formats, geometry, size class, stream.  A site adds the rest.
Cycle0Launch level0_launch(Instance *I, bool composed)
{
    Cycle0Launch d;
    d.Uin = result(I); d.Uout = I->result_in_U1 ? I->U0 : I->U1;
    d.F = I->F; d.Fc = I->mg[1].F; d.E = I->mg[1].U;
    d.g = I->mg[0].g;
    d.f_half = I->f_half; d.l1_half = I->mg_l1_half;
    d.rag = I->rag.dev;
    d.s = I->stream;
    if ((d.composed = composed)) { d.comp.E2 = I->mg[2].U; d.comp.g1 = I->mg[1].g; }
    return d;
}

// Stop rule.  The error left after a cycle is about rho / (1 - rho) times the correction it applied, rho being the
// contraction per cycle (measured: the prediction matches the next correction to ~10 %).  With two successive
// corrections known the bound is applied to that prediction: error <= 0.1 x update_tol (0.025 grey levels at the
// default 0.25, i.e. the error the plain threshold "correction <= update_tol" leaves at rho = 0.09).  A solve that
// contracts faster stops on a larger last correction, a slower one on a smaller.  Without a previous correction
// (max_sweeps = 1) the plain threshold decides.
static bool stop_rule(float utol, float m, float m_prev)
{
    if (m_prev > 0.f) {
        const float rho = std::min(0.5f, std::max(0.02f, m / m_prev));
        return m * rho / (1.0f - rho) <= 0.1f * utol;
    }
    return m <= utol;
}

// the per-workgroup maxima of one fused solve: two cycles' worth of nb_cap each at part_base (pinned, folded by the host: host_fold; or device), `sat` behind them
struct Level0Maxima { bool host_fold; int nb_cap; float *part_base; AbortFlag sat; };

// max |correction| of the cycle just launched = max over its per-workgroup maxima (at part_now; `cyc` already counts the
// cycle), and of the cycle before when its maxima are at hand.  A few thousand maxima are folded here on the host, out of
// the pinned buffer the launches wrote them to (host_fold); large grids (groups of clones) reduce both lists on the device
// first (one launch) and copy three words.  m_prev < 0: unknown.  `output` (the splice or post-process of the result, or nothing) is enqueued between the launch
// and the read-back: it then starts without a gap while the host waits.  saturated: a 16-bit store of this solve left its range.
template <class Output>
static int correction_maxima(Instance *I, const Level0Maxima &x, int cyc, int nb, int nb_prev, float *part_now, Output output, float &m, float &m_prev,
                             bool &saturated)
{
    m = 0.f; m_prev = -1.f;
    int orc;
    if (x.host_fold) {
        const bool have_prev = nb_prev > 0;                       // the launch of the previous cycle wrote the other half
        if ((orc = output())) return orc;
        SC_HIP(I, hipStreamSynchronize(I->stream));               // the maxima are in the pinned buffer when the launch has ended
        if (x.sat.p) { unsigned w; memcpy(&w, (const float *)I->h_partial.p + 2 * (size_t)x.nb_cap, sizeof(w)); saturated = w == x.sat.gen; }
        const float *hp = (const float *)I->h_partial.p + (size_t)(cyc & 1) * x.nb_cap;            // this cycle's half
        const float *hq = (const float *)I->h_partial.p + (size_t)((cyc + 1) & 1) * x.nb_cap;      // the previous cycle's
        for (int i = 0; i < nb; ++i) m = hp[i] > m ? hp[i] : m;
        if (have_prev) {
            m_prev = 0.f;
            for (int i = 0; i < nb_prev; ++i) m_prev = hq[i] > m_prev ? hq[i] : m_prev;
        }
    } else {
        const float *part_prev = x.part_base + (size_t)((cyc + 1) & 1) * x.nb_cap;
        launch_max_final2(part_now, nb, part_prev, nb_prev > 0 ? nb_prev : 0, I->d_maxcorr, I->stream, x.sat.p);
        if ((orc = output())) return orc;
        SC_HIP(I, hipMemcpyAsync(I->h_maxcorr, I->d_maxcorr, 3 * sizeof(unsigned), hipMemcpyDeviceToHost, I->stream));
        SC_HIP(I, hipStreamSynchronize(I->stream));
        memcpy(&m, &I->h_maxcorr[0], sizeof(float));
        memcpy(&m_prev, &I->h_maxcorr[1], sizeof(float));
        saturated = x.sat.p && I->h_maxcorr[2] == x.sat.gen;
    }
    return SC_OK;
}

// ---- the schedule of a fused solve ------------------------------------------------------------------------------------------------
// Fused level-0 form: one launch per cycle does [prolongation +] post-smoothing of this cycle,
// pre-smoothing of the next, residual and restriction (sc_cycle0.hip).  The first launch has no
// correction to add.  A cycle whose result the stop rule is about to judge is launched in its
// "final" form instead (prolongation + post-smoothing only): when the rule accepts it -- the normal
// case for the third cycle -- nothing was computed for a cycle that never runs, and the field is
// exactly the textbook V-cycle's; when it does not, one pre-smoothing + residual + restriction launch
// (the form of the very first launch) catches up and the cycles continue.
//
// Output straight from the last cycle.  When the caller armed the splice (out_wanted) the judged cycle does not write its field: it
// adds the float-table node correction, clamps, truncates and leaves output BYTES (planar, in the memory of the partner field; a small
// kernel interleaves them into the destination) -- 3 bytes less written and 9 less read per pixel and channel than field +
// post-process.  The node correction it adds is the one of the iterate BEFORE that cycle, whose cell shares the previous launch leaves
// behind (lowmode_early_kind: the two differ by 0.001-0.003 grey levels, 0.05 in the worst case the stop rule admits).  If the rule
// rejects the cycle, the same cycle is launched again in the form that writes the field (its input is untouched) and the solve
// continues as without this.

// Is the cycle behind `cyc` completed ones judged?  The first two corrections of a solve are never below the stop threshold unless the
// initial guess was already the answer, and every check costs a host round trip (~25 us), so checking starts with the third cycle.
static bool fused_judged(const FusedFacts &f, int cyc) { return !(cyc + 1 < 3 && cyc + 1 < f.budget && !f.tol); }

// the launch that opens the cycle behind S.cyc completed ones -- or, behind that cycle's refused bytes form, its field form
static FusedStep fused_cycle(FusedSchedule &S, bool bytes_refused)
{
    const FusedFacts &f = S.f;
    const bool judged = fused_judged(f, S.cyc), next_judged = !judged && fused_judged(f, S.cyc + 1);
    FusedStep s;
    s.prolong = true; s.composed = f.composed; s.coarse_first = !bytes_refused;
    s.judged = s.final_cycle = judged;      // the judged cycle runs in its final form and leaves the node correction's cell shares (sc_lowmode.hip)
    s.sweeps = judged ? f.post : f.post + f.pre;
    const int bands = judged && !f.separate_restrict ? f.post : 0;
    s.bands_sweeps = bytes_refused ? 0 : bands;      // (asked for when the cycle opened)
    if (judged && S.early_ready) {
        s.kind = FUSED_JUDGED_BYTES; s.out_bytes = s.lm = true;
        S.early_ready = false;
        return s;
    }
    s.kind = judged ? FUSED_JUDGED_FIELD : next_judged ? FUSED_BEFORE_JUDGED : FUSED_FULL;
    s.bands = bands; s.sat = true;
    s.q16_in = S.u_q16; s.q16_out = S.u_q16 && !next_judged;      // the launch before the judged cycle writes float again
    s.ask_early = f.out_wanted && next_judged;
    return s;
}

// The step before the judged cycle of a solve that wants bytes, once lowmode_early_kind has answered: 1 the bytes may carry the node
// correction of this step's result, which leaves its cell shares; 3 the a-priori bound does not cover this size (the float tables' low
// modes are off by more than 4 %) -- the same, but the bytes stand only IF the judged cycle's measured update keeps the difference
// below the same 0.049 grey levels (early_cond, decided with the stop rule); 0 there is no correction to add; 2 the field-keeping path.
void fused_early(FusedSchedule &S, FusedStep &s, int early_kind)
{
    const FusedFacts &f = S.f;
    S.early_cond = early_kind == 3;
    if (early_kind == 2) return;
    if (early_kind == 0) s.nodes = NODES_NOTHING;
    else {
        if (!f.separate_restrict) s.bands = s.bands_sweeps = f.post + f.pre;
        // a group of clones: its coarse levels fill the chip, nothing to overlap (measured: -2 %); a small clone: the two
        // cross-stream waits cost more than the 15-us chain they hide (154x100 ... 300x194 patches: +20 us; neutral at 730^2 ... 800^2,
        // -2..3 % from 900^2 on: the threshold is 0.79 Mpix, 1 Mpix until late in round 4); one large clone: on the second stream,
        // beside the coarse levels of the next cycle (-15 us of 500 at 2048^2)
        s.nodes = f.small ? NODES_MAIN : NODES_SECOND;
    }
    S.early_ready = true;
}

// The next level-0 launch of the solve; `verdict`: what the stop rule made of the step handed out last, where that one was judged.
FusedStep fused_next(FusedSchedule &S, int verdict)
{
    const FusedFacts &f = S.f;
    const bool was_cycle = S.last == FUSED_FULL || S.last == FUSED_BEFORE_JUDGED || S.last == FUSED_JUDGED_BYTES || S.last == FUSED_JUDGED_FIELD;
    const bool was_judged = S.last == FUSED_JUDGED_BYTES || S.last == FUSED_JUDGED_FIELD;
    FusedStep s;
    if (S.last < 0) {
        // on the float16 path the pre-process stored the initial field as float16 as well (this launch only)
        s.kind = FUSED_FIRST; s.sweeps = f.pre; s.u_half = f.u_half; s.q16_out = f.q16; s.sat = true;
    } else if (S.last == FUSED_JUDGED_BYTES && verdict != VERDICT_ACCEPT && verdict != VERDICT_SATURATED) {
        s = fused_cycle(S, true);          // refused: the same cycle again in the form that keeps the field, then on as usual
    } else {
        if (S.last == FUSED_JUDGED_BYTES) S.sweep_launches += 1;
        if (was_cycle) S.cyc += 1;
        if (was_judged && verdict == VERDICT_ACCEPT) S.result = SC_OK;
        else if (was_judged && verdict == VERDICT_SATURATED) S.result = SC_RETRY_FLOAT_FIELD;      // nothing was written (AbortFlag)
        else if (S.cyc >= f.budget) S.result = SC_ERR_NOT_CONVERGED;
        else if (S.last == FUSED_JUDGED_FIELD) { s.kind = FUSED_CATCH_UP; s.sweeps = f.pre; }      // pre-smoothing + residual + restriction for the next cycle
        else s = fused_cycle(S, false);
    }
    if (s.kind != FUSED_DONE && s.kind != FUSED_JUDGED_BYTES) S.sweep_launches += 1;
    S.u_q16 = s.q16_out;
    S.last = s.kind;
    return s;
}

Cycle0Launch step_launch(Cycle0Launch d, const FusedStep &s)
{
    d.sweeps = s.sweeps; d.prolong = s.prolong; d.final_cycle = s.final_cycle; d.out_bytes = s.out_bytes;
    d.u_half = s.u_half; d.q16_in = s.q16_in; d.q16_out = s.q16_out;
    return d;
}

// the optional residual-based stop (tol > 0): the relative residual into the run's info; stop: it meets the tolerance
static int residual_stop(Instance *I, bool &stop)
{
    double r[2];
    int rc = eval_residual(I, r);
    if (rc) return rc;
    const double rel = (r[1] > 0.0) ? std::sqrt(r[0] / r[1]) : std::sqrt(r[0]);
    I->info.rel_residual = rel;
    stop = rel <= (double)I->opts.tol;
    return SC_OK;
}

// The fused solve: asks the schedule for the next level-0 launch, runs the coarse levels in front of a launch that opens a cycle,
// launches it, and where the step is judged hands the stop rule's verdict back.
static int mg_solve_fused(Instance *I, int pre, int post, float utol, int budget)
{
    const sc_solver_opts &o = I->opts;
    int rc;
    const bool out_wanted = I->spec_post.armed && o.tol <= 0.f && !(o.flags & SC_FLAG_KEEP_FIELD) && pre == 2 && post == 2;
    const bool q16 = I->mg_l1_half && mg_field_q16(I, out_wanted) && budget > 1;      // (max_sweeps = 1: the first cycle is the judged one)
    const int nb_cap = cycle0_blocks(I->F.W, I->F.H, I->F.C, 4);   // deepest form = largest halo = most workgroups
    // The 16-bit stores check their range (sc_cycle0.hip, c0_q16_checked): one that saturates writes this solve's generation
    // word behind the partial maxima; the output launches then write nothing, the read-back of the maxima brings the word
    // along, and the clone is repeated on float fields (SC_RETRY_FLOAT_FIELD).  A NaN pattern: no maximum ever has these bits.
    // Up to 16384 workgroups (single clones, small groups) the host folds the per-workgroup maxima itself -- and the launches
    // store them (and the saturation word) STRAIGHT INTO PINNED HOST MEMORY: no read-back copy behind the judged cycle (a
    // command of its own on the critical path, ~4 us + its gap).  Larger grids fold on the device first.
    const bool host_fold = nb_cap <= 16384;
    if (host_fold && (rc = ensure_pinned(I, I->h_partial, sizeof(float) * (2 * (size_t)nb_cap + 64)))) return rc;
    float *const part_base = host_fold ? (float *)I->h_partial.p : (float *)I->mg_partial.p;
    AbortFlag sat;
    if (q16) {      // the device word sits behind the device list of maxima (the output launches test it there), its host copy behind the pinned one
        sat.p = (unsigned *)((float *)I->mg_partial.p + 2 * (size_t)nb_cap);
        sat.host = host_fold ? (unsigned *)((float *)I->h_partial.p + 2 * (size_t)nb_cap) : nullptr;
        sat.gen = 0x7fc00000u | (++I->sat_counter & 0x3fffffu);
    }
    I->sat = sat;
    const Level0Maxima maxima{ host_fold, nb_cap, part_base, sat };
    FusedSchedule S{ FusedFacts{ pre, post, budget, o.tol > 0.f, out_wanted, q16, I->u_half, mg_composes_level1(I), legacy_path(o, SC_LEGACY_SEPARATE_RESTRICT),
                                 I->F.C > 3 || (size_t)I->F.W * I->F.H < (size_t)3 << 18 } };
    const int launches_before = I->info.sweep_launches;
    int nb_last = 0;                   // workgroups (= partial maxima) of the previous cycle's level-0 launch
    float4 *bands = nullptr;           // the current cycle's buffer for the node correction's cell shares
    LmNodes early_lm;                  // the node correction for the judged cycle's bytes (CN == nullptr: none to add)
    int verdict = VERDICT_NONE;
    for (;;) {
        FusedStep s = fused_next(S, verdict);
        I->info.sweep_launches = launches_before + S.sweep_launches;
        if (s.kind == FUSED_DONE) break;
        verdict = VERDICT_NONE;
        if (s.coarse_first && (rc = vcycle(I, 1, pre, post, s.composed ? (1u << 1) : 0u))) return rc;
        if (s.ask_early) fused_early(S, s, lowmode_early_kind(I, utol));
        if (s.coarse_first) bands = s.bands_sweeps ? lowmode_bands_buffer(I, s.bands_sweeps) : nullptr;
        if (s.lm && I->aux_pending) {          // the node correction is ready when the launch that adds it starts
            SC_HIP(I, hipStreamWaitEvent(I->stream, I->ev_join, 0));
            I->aux_pending = false;
        }
        float *const part_now = part_base + (size_t)((S.cyc + 1) & 1) * nb_cap;    // this cycle's maxima; the previous cycle's sit in the other half
        Cycle0Launch d = step_launch(level0_launch(I, s.composed), s);
        if (s.prolong) d.partial = part_now;
        if (s.bands) d.bands = bands;
        if (s.lm) d.lm = early_lm;
        if (s.sat) d.sat = sat;
        // The judged bytes of a same-size group (no size class, one table of jobs): the launch writes the members' destinations itself where
        // that form exists and the grid is large enough to pay for workgroups of three-fold length; it is given the members' jobs (their
        // guards) and the saturation word, the splice's two tests, and no splice launch follows.
        bool interleaved = false;
        if (s.out_bytes) {
            const SolveTarget &to = I->spec_post.to;
            if (to.group && !d.rag && to.group->size() <= (size_t)ImageJobs::MAX && to.group->size() * 3 == (size_t)I->F.C && (*to.group)[0].W == 0 &&
                !legacy_path(o, SC_LEGACY_SPLICE_LAUNCH)) {
                const long tiles = (long)cycle0_blocks(I->F.W, I->F.H, (int)to.group->size(), s.sweeps);
                Cycle0Launch d3 = d;
                d3.out_interleaved = true; d3.jobs = to.group->data(); d3.njobs = (int)to.group->size(); d3.sat = sat;
                int T3, TAG3;
                bool PRO3;
                if ((tiles >= SC_OUT3_MIN_TILES || legacy_path(o, SC_FORCE_INTERLEAVED_OUT)) && cycle0_form(d3, T3, PRO3, TAG3)) { d = d3; interleaved = true; }
            }
        }
        // The first launch of a same-size group whose pre-process stored no initial field (Instance::u0_bytes): it reads the members' destination
        // bytes where that form exists for the step's facts; where it does not (nothing composed, level 1 in float, one pre-sweep), a
        // small launch stores the float16 planes after all and the planes' form runs -- never on planes nobody wrote.
        if (s.kind == FUSED_FIRST && s.u_half) {
            int reader = 1;
            if (I->u0_bytes) {
                const SolveTarget &to = I->spec_post.to;
                Cycle0Launch d3 = d;
                d3.u_half = false; d3.in_bytes = true; d3.jobs = to.group ? to.group->data() : nullptr; d3.njobs = to.group ? (int)to.group->size() : 0;
                int T3, TAG3;
                bool PRO3;
                if (d3.jobs && cycle0_form(d3, T3, PRO3, TAG3)) { d = d3; reader = 2; }
                else if (!to.group) { I->err = "internal: no initial field stored for a solve without members"; return SC_ERR_BAD_ARG; }
                else { launch_u0_half_group(to.group->data(), (int)to.group->size(), I->U0, I->stream); reader = 4; }
            }
            I->u0_reader |= reader;
        }
        const int nb = launch_cycle0(d);
        if (s.out_bytes && nb <= 0) { verdict = VERDICT_NO_FORM; continue; }
        if (s.prolong ? nb <= 0 : nb < 0) { I->err = "cycle0: unsupported depth"; return SC_ERR_BAD_ARG; }
        const Field Q = I->result_in_U1 ? I->U0 : I->U1;      // (where a bytes form left its bytes)
        if (s.out_bytes) I->bytes_writer |= interleaved ? 2 : 1;
        if (!s.out_bytes) I->result_in_U1 = !I->result_in_U1;
        if (s.kind == FUSED_FIRST) {
            if (I->rag.dev && I->rag.ready_pending) {      // a size class: its zeroed coarse planes and tables were made on the second stream beside everything up to here
                SC_HIP(I, hipStreamWaitEvent(I->stream, I->rag.ev_ready, 0));      // (the matrices: run_tail waits for them)
                I->rag.ready_pending = false;
            }
            I->u_half = I->u0_bytes = false;             // consumed: both U buffers hold float (or 16-bit fixed point: u_q16) from here on
            I->mg_q16_last = q16;
        } else if (!s.out_bytes) {
            lowmode_bands_written(I, d.bands ? result(I).p : nullptr);
        }
        I->u_q16 = s.q16_out;
        if (s.nodes != NODES_NONE) {       // the node correction the next cycle's output will carry, from this launch's field
            early_lm = LmNodes();
            if (s.nodes == NODES_MAIN) {
                if ((rc = lowmode_nodes(I, result(I), early_lm))) return rc;
            } else if (s.nodes == NODES_SECOND) {
                SC_HIP(I, hipEventRecord(I->ev_fork, I->stream));
                SC_HIP(I, hipStreamWaitEvent(I->aux, I->ev_fork, 0));
                if ((rc = lowmode_nodes(I, result(I), early_lm, I->aux))) return rc;
                SC_HIP(I, hipEventRecord(I->ev_join, I->aux));
                I->aux_pending = true;
            }
        }
        if (!s.prolong) continue;
        SC_HIP(I, hipGetLastError());
        const int nb_prev = nb_last;
        if (!s.out_bytes) nb_last = nb;
        if (!s.judged) continue;
        // the output goes in FIRST (see Instance::spec_post), the read-back of the maxima follows it
        float m, m_prev;
        bool saturated = false;
        if (s.out_bytes)
            rc = correction_maxima(I, maxima, S.cyc + 1, nb, nb_prev, part_now, [&]() -> int {
                    const SolveTarget &to = I->spec_post.to;
                    if (interleaved) return SC_OK;      // the judged launch wrote the destinations itself
                    if (!to.group) launch_splice_planar(Q, to.org, to.step, I->stream, I->guard, sat);
                    else launch_splice_planar_group(Q, to.group->data(), (int)to.group->size(), I->stream, sat);
                    return SC_OK;
                }, m, m_prev, saturated);
        else
            rc = correction_maxima(I, maxima, S.cyc + 1, nb, nb_prev, part_now, [&]() -> int {
                    if (!(I->spec_post.armed && o.tol <= 0.f)) return SC_OK;
                    const int lrc = write_output(I, I->spec_post.to, sat);
                    if (lrc) return lrc;
                    I->spec_post.done = true;
                    return SC_OK;
                }, m, m_prev, saturated);
        if (rc) return rc;
        I->info.last_update = m;
        bool stop = false;
        if (saturated) {
            if (!s.out_bytes) I->spec_post.done = false;
            verdict = VERDICT_SATURATED;
        } else if (s.out_bytes) {
            const bool early_ok = !(S.early_cond && I->lm.max_ratio * (double)m > 0.049);
            if (stop_rule(utol, m, m_prev) && early_ok) { I->spec_post.done = true; I->out_direct = true; verdict = VERDICT_ACCEPT; }
            else verdict = early_ok ? VERDICT_REJECT : VERDICT_REJECT_EARLY;
        } else {
            if (o.tol > 0.f && (rc = residual_stop(I, stop))) return rc;
            if (stop || stop_rule(utol, m, m_prev)) verdict = VERDICT_ACCEPT;
            else { I->spec_post.done = false; verdict = VERDICT_REJECT; }     // not converged: the field moves on, the output is written again later
        }
    }
    I->info.sweeps = S.cyc;
    if (S.result == SC_RETRY_FLOAT_FIELD) return S.result;
    I->info.converged = S.result == SC_OK ? 1 : 0;
    return S.result;
}

int mg_solve(Instance *I)
{
    const sc_solver_opts &o = I->opts;
    int rc = build_levels(I);
    if (rc) return rc;
    {
        const int nb = std::max(std::max(prolong_blocks(I->F.W - 2, I->F.H - 2, I->F.C), tb_blocks_level0(I->F.W, I->F.H, I->F.C, 2)),
                                cycle0_blocks(I->F.W, I->F.H, I->F.C, 4));      // the deepest forms have the most workgroups
        if ((rc = ensure(I, I->mg_partial, sizeof(float) * (2 * (size_t)nb + 64)))) return rc;   // two cycles' worth (see the stop rule) + the saturation word behind them
    }
    const MGParams mp = mg_params(o);
    const int pre = mp.pre, post = mp.post, budget = mp.budget;
    const float utol = mp.utol;
    // level 1 in float16 or float: the two formats put a plane's ring and pads at different bytes, so a switch re-zeroes the planes
    const bool l1h = I->mg.size() >= 2 && mg_level1_half(I);
    if (I->mg.size() >= 2 && l1h != I->mg_l1_half) {
        MGLevel &L1 = I->mg[1];
        SC_HIP(I, hipMemsetAsync(L1.U.p, 0, L1.U.bytes(), I->stream));
        SC_HIP(I, hipMemsetAsync(L1.F.p, 0, L1.F.bytes(), I->stream));
        SC_HIP(I, hipMemsetAsync(L1.T.p, 0, L1.T.bytes(), I->stream));
        I->mg_l1_half = l1h;
    }
    // the level-0 scratch is the ping-pong partner of the solution; the residual field only
    // writes its interior, and both buffers carry the same ring, so it stays a valid partner
    int cyc = 0;
    bool ok = false;
    const bool fused0 = fused_level0(o) && I->mg.size() >= 2;
    if (I->f_half && !(fused0 && o.tol <= 0.f)) { I->err = "internal: float16 right-hand side on a path that needs float"; return SC_ERR_BAD_ARG; }
    if (fused0) return mg_solve_fused(I, pre, post, utol, budget);      // one launch per cycle on level 0 (sc_cycle0.hip)
    while (cyc < budget) {
        if ((rc = vcycle(I, 0, pre, post))) return rc;
        ++cyc;
        SC_HIP(I, hipGetLastError());
        if (I->mg.size() == 1) { ok = true; break; } // single level: solved by SOR above
        SC_HIP(I, hipMemcpyAsync(I->h_maxcorr, I->d_maxcorr, sizeof(unsigned), hipMemcpyDeviceToHost, I->stream));
        SC_HIP(I, hipStreamSynchronize(I->stream));
        float m;
        unsigned bits = *I->h_maxcorr;
        memcpy(&m, &bits, sizeof(float));
        I->info.last_update = m;
        bool stop = false;
        if (o.tol > 0.f && (rc = residual_stop(I, stop))) return rc;
        if (stop) { ok = true; break; }
        if (m <= utol) { ok = true; break; }
    }
    I->info.sweeps = cyc;
    I->info.converged = ok ? 1 : 0;
    return ok ? SC_OK : SC_ERR_NOT_CONVERGED;
}

} // namespace sc
