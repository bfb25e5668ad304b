// sc_volume_flow_coupled.hip -- the coupled flow volume call's two kernels (sc_hip_volume_flow_coupled*, sc_volume_api.cpp:
// VolumeFlowRobustOperator's launches in a reweighting round under a coupling): k_volume_flow_robust_rho and
// k_volume_flow_robust_setup_rho, k_volume_robust_rho and k_volume_robust_setup_rho (sc_volume_coupled.hip: the forms, the magnitudes,
// the float32 order, the rho planes) with the temporal neighbours of an element taken from the volume's link planes (sc_pcg.h: what they
// hold; sc_volume_flow.hip: the matching) as k_volume_flow_robust_setup takes them (sc_volume_flow_robust.hip).
// The owner of a temporal link is its source, the element i that holds it: lt = tau * smooth_t, gt and -- new here -- the link's rho are
// stored at i; under SPACE | TIME the pixel's magnitude is (a_x + a_y) + a_t with a_t of the held link, nothing where it holds none; a
// link that arrives at a pixel plays no part in that pixel's magnitude.  The matching is per volume, liveness per channel: under JOINT a
// magnitude sums the channels in which the link is live.  The wrap of periodic time is in the indices, so there is no periodic form.
// The t-component of rho is written at the owner's own [frame][Y][X] element only -- no atomics; the pixel a link arrives at reads it at
// the source jb = bwd[i], whose frame, row and column come from the work-plane index: the source may lie in another band, another column
// group or (periodic time) a frame other than t - 1.  The rho launch and the set-up launch are ordered by the stream.
// Per element beyond the straight pair: one int32 load per channel in the rho kernel (under JOINT the same word again: looked up once
// per pixel the forms need up to 24 VGPRs more), two in the set-up, and in place of the neighbours one frame away a gather of state, of
// U or data, and in the set-up of rho, smooth_t and gt at the back link's source -- as coalesced as the flow is smooth.
#include "sc_region_device.h"
#include <cmath>
#include <type_traits>

namespace sc {

namespace {

// grid: cg x bands x units; esum[(the unit's first plane * PCG_PARTS + part)] = the part's gradient-and-time energy
template <bool LNK, bool SPACE, bool TIME, bool JOINT>
__global__ __launch_bounds__(WL) void k_volume_flow_robust_rho(PoissonGeo g, PcgGeo wg, VolumeGeo vg, VolumeJobs t, RobustTerm tg, RobustTerm tt,
                                                                VolumeRhoGeo rg, FlowLinks fl, const float *__restrict__ U, float *__restrict__ Rho,
                                                                double *__restrict__ esum)
{
    __shared__ double ws[4];
    lane_term(tg); lane_term(tt);
    const int unit = (int)blockIdx.z, member = JOINT ? unit : unit / g.C;
    const int k0 = JOINT ? 0 : unit - member * g.C, k1 = JOINT ? g.C : k0 + 1;
    const PoissonJobDev &j = t.j[member];
    const float *__restrict__ st = t.st[member], *__restrict__ gt = t.gt[member];
    const float *__restrict__ sx = LNK ? t.sx[member] : nullptr, *__restrict__ sy = LNK ? t.sy[member] : nullptr;
    const float *__restrict__ smt = LNK ? t.smt[member] : nullptr;
    const bool px = wg.ax == MIXED_PERIODIC, py = wg.ay == MIXED_PERIODIC;
    const bool rho_g = tg.mode != 0, rho_t = TIME || tt.mode != 0;      // the penalty has a rho to store (exponent 2: none)
    const int nx = wg.nx, fny = vg.ny, x = (int)blockIdx.x * WL + (int)threadIdx.x;
    const int y0 = (int)blockIdx.y * wg.rows, y1 = min(y0 + wg.rows, wg.ny);
    const float tau = vg.tau;
    float *__restrict__ ru = Rho + (size_t)unit * rg.unit;
    float *__restrict__ rx = ru + rg.ox, *__restrict__ ry = ru + rg.oy, *__restrict__ rt = ru + rg.ot;
    double s_e = 0.0;
    if (x < nx) {
        const int X = wg.x0 + x, xe = x < nx - 1 ? x + 1 : 0;
        for (int y = y0; y < y1; ++y) {
            const FrameRow fr(vg, y);
            const int Y = wg.y0 + fr.yy;
            const size_t ro = (size_t)y * nx, li = ro + x;
            // the magnitudes, has_*, e2: k_volume_robust_rho's; mt and the t-share of mx: the held link's
            float mx = 0.f, my = 0.f, mt = 0.f, mw = 0.f, mn = 0.f;
            bool has_x = false, has_y = false, has_t = false, has_w = false, has_n = false;
            double e2 = 0.0;
            for (int k = k0; k < k1; ++k) {
                const long long o = (long long)X * g.cs + (long long)Y * g.rs + (long long)k * g.chs + (long long)fr.t * vg.fs;
                const int kp = state_kind(st[o]);
                if (kp == NB_NONE) continue;
                const bool unk = kp == NB_UNKNOWN;
                const Around a(g, wg, st, X, Y, o, px, py);
                // the link this element holds: the volume's, its target's offset in this channel
                const TimeAround ta(g, wg, vg, fl, member, k, y, x);
                const int jf = ta.jf;
                const long long of = ta.of;
                const int kf = time_kind(st, of, ta.hf);
                const float *__restrict__ ul = U + (size_t)(member * g.C + k) * wg.stride;
                auto value = [&](int kq, long long off, size_t i) { return kq == NB_UNKNOWN ? ul[i] : kq == NB_KNOWN ? j.d[off] : j.b[off]; };
                auto live = [&](int kq) { return kq != NB_NONE && (unk || kq == NB_UNKNOWN); };
                const float uc = value(kp, o, li);
                float ax = 0.f, ay = 0.f, at = 0.f;
                if (live(a.ke)) {
                    const float tr = (value(a.ke, a.oe, ro + xe) - uc) - j.gx[o];
                    if (rho_g) { ax = coupled_sq(sx, o, tr); has_x = true; }
                    else e2 += (double)(sx ? sx[o] : 1.f) * (double)rounded_product(tr, tr);
                }
                if (live(a.ks)) {
                    const float tr = (value(a.ks, a.os, fr.yy < fny - 1 ? li + nx : li - (size_t)(fny - 1) * nx) - uc) - j.gy[o];
                    if (rho_g) { ay = coupled_sq(sy, o, tr); has_y = true; }
                    else e2 += (double)(sy ? sy[o] : 1.f) * (double)rounded_product(tr, tr);
                }
                if (live(kf)) {          // (kf is NB_NONE without a held link: jf >= 0 here)
                    const float tr = (value(kf, of, (size_t)jf) - uc) - (gt ? gt[o] : 0.f), lt = time_link(smt, o, tau);
                    if (TIME || (JOINT && rho_t)) {
                        at = rounded_product(lt, rounded_product(tr, tr));
                        has_t = true;
                    } else {          // the uncoupled penalty: robust_link's rho and energy
                        float q;
                        const float rho = robust_rho(tt, tr, q);
                        if (rho_t) { rt[(size_t)fr.t * rg.fstride + (size_t)Y * rg.rw + X] = rho; }
                        e2 += robust_phi(tt, lt, q, rho);
                    }
                }
                if (SPACE) mx += TIME ? (ax + ay) + at : ax + ay;
                else { mx += ax; my += ay; }
                if (!TIME) mt += at;
                if (unk && a.kw == NB_DIRICHLET) {
                    const float tr = (uc - j.b[a.ow]) - j.gx[a.ow];
                    if (rho_g) { mw += coupled_sq(sx, a.ow, tr); has_w = true; }
                    else e2 += (double)(sx ? sx[a.ow] : 1.f) * (double)rounded_product(tr, tr);
                }
                if (unk && a.kn == NB_DIRICHLET) {
                    const float tr = (uc - j.b[a.on]) - j.gy[a.on];
                    if (rho_g) { mn += coupled_sq(sy, a.on, tr); has_n = true; }
                    else e2 += (double)(sy ? sy[a.on] : 1.f) * (double)rounded_product(tr, tr);
                }
            }
            const size_t i = (size_t)fr.t * rg.fstride + (size_t)Y * rg.rw + X;
            double e_x = 0.0, e_y = 0.0, e_t = 0.0, e_w = 0.0, e_n = 0.0;
            if (SPACE ? (has_x || has_y || (TIME && has_t)) : has_x) rx[i] = coupled_rho(tg, mx, e_x);
            if (!SPACE && has_y) ry[i] = coupled_rho(tg, my, e_y);
            if (!TIME && has_t) rt[i] = coupled_rho(tt, mt, e_t);
            if (has_w) rx[i - 1] = coupled_rho(tg, mw, e_w);              // (a low Dirichlet line: X == 1)
            if (has_n) ry[i - rg.rw] = coupled_rho(tg, mn, e_n);          // (Y == 1)
            s_e += ((e_x + e_y) + e_t) + ((e_w + e_n) + e2);
        }
    }
    s_e = block_sum(s_e, ws);
    if (threadIdx.x == 0) esum[(size_t)(JOINT ? unit * g.C : unit) * PCG_PARTS + blockIdx.y * wg.cg + blockIdx.x] = s_e;
}

// k_volume_robust_setup_rho (its walk, its order, its five sums) with the temporal neighbours through the link planes: the held link's
// rho, lt and gt at the pixel's own element, the arriving link's at its source jb = bwd[i] -- the rho element [jb's frame][row][column]
// of the work-plane index; the values across a link as k_volume_flow_robust_setup takes them.  Field 4 of the sums: the data term's
// energy alone.  gmode, tmode: the modes of the spatial and of the temporal penalty (0: no rho, the base link itself).
template <bool NOW, bool LNK, bool SPACE, bool TIME, bool JOINT>
__global__ __launch_bounds__(WL) void k_volume_flow_robust_setup_rho(PoissonGeo g, PcgGeo wg, VolumeGeo vg, VolumeJobs t, int gmode, int tmode,
                                                                      RobustTerm td, VolumeRhoGeo rg, FlowLinks fl, const float *__restrict__ Rho,
                                                                      const float *__restrict__ U, float *__restrict__ R, float *__restrict__ E,
                                                                      float *__restrict__ S, float *__restrict__ F, float *__restrict__ Dg,
                                                                      double *__restrict__ bb, double *__restrict__ sums)
{
    __shared__ double ws[VOLUME_ROBUST_SUMS + 1][4];
    lane_term(td);
    const PcgBand bd(g, wg);
    const PoissonJobDev &j = t.j[bd.member];
    const float *__restrict__ w = t.w[bd.member], *__restrict__ st = t.st[bd.member], *__restrict__ gt = t.gt[bd.member];
    const float *__restrict__ sx = LNK ? t.sx[bd.member] : nullptr, *__restrict__ sy = LNK ? t.sy[bd.member] : nullptr;
    const float *__restrict__ smt = LNK ? t.smt[bd.member] : nullptr;
    const bool px = wg.ax == MIXED_PERIODIC, py = wg.ay == MIXED_PERIODIC;
    const bool rho_g = gmode != 0, rho_t = TIME || tmode != 0;
    const int nx = wg.nx, x = bd.x, n2 = wg.nx * vg.ny;
    const float *__restrict__ ul = U + (size_t)bd.p * wg.stride;
    const float tau = vg.tau;
    const float *__restrict__ ru = Rho + (size_t)(JOINT ? bd.member : bd.p) * rg.unit;
    const float *__restrict__ rx = ru + rg.ox, *__restrict__ ry = ru + rg.oy, *__restrict__ rt = ru + rg.ot;
    const size_t col = (size_t)bd.p * wg.stride + (size_t)(x < nx ? x : 0);
    float *__restrict__ rc = R + col, *__restrict__ ec = E + col, *__restrict__ sco = S + col, *__restrict__ fc = F + col, *__restrict__ dc = Dg + col;
    double s_bb = 0.0, s_w = 0.0, s_l = 0.0, s_t = 0.0, s_uk = 0.0, s_e = 0.0;
    if (x < nx) {
        const int X = wg.x0 + x;
        const int Xw = X > 0 ? X - 1 : g.W - 1;                                     // the owner of the west link
        // s = c rho, one rounded product (no base array: rho itself; exponent 2: the base link itself); a temporal link: c = lt, always
        auto space_link = [&](const float *__restrict__ c, long long off, const float *__restrict__ plane, size_t i) {
            return !rho_g ? (c ? c[off] : 1.f) : c ? rounded_product(c[off], plane[i]) : plane[i];
        };
        auto time_s = [&](long long off, size_t i) {
            const float lt = time_link(smt, off, tau);
            return rho_t ? rounded_product(lt, rt[i]) : lt;
        };
        for (int y = bd.y0; y < bd.y1; ++y) {
            const FrameRow fr(vg, y);
            const int Y = wg.y0 + fr.yy;
            const long long o = bd.pixel(g, X, Y) + (long long)fr.t * vg.fs;
            const size_t ro = (size_t)y * nx, li = ro + x;
            const size_t rf = (size_t)fr.t * rg.fstride, rr = rf + (size_t)Y * rg.rw;
            const int kp = state_kind(st[o]);
            float v = 0.f, e = 0.f, so = 0.f, f = 0.f, dg = 0.f;
            if (kp != NB_NONE) {
                const bool unk = kp == NB_UNKNOWN;
                const Around a(g, wg, st, X, Y, o, px, py);
                const TimeAround ta(g, wg, vg, fl, bd.member, bd.c, y, x);
                const int jb = ta.jb;
                const int kb = time_kind(st, ta.ob, ta.hb), kf = time_kind(st, ta.of, ta.hf);
                auto live = [&](int kq) { return kq != NB_NONE && (unk || kq == NB_UNKNOWN); };
                float le = 0.f, ls = 0.f, lf = 0.f, lw = 0.f, ln = 0.f, lb = 0.f;
                if (live(a.ke)) {
                    le = space_link(sx, o, rx, rr + X);
                    if (kp + a.ke == NB_KNOWN) s_uk += (double)le;
                }
                if (live(a.ks)) {
                    ls = space_link(sy, o, ry, rr + X);
                    if (kp + a.ks == NB_KNOWN) s_uk += (double)ls;
                }
                if (live(kf)) {
                    lf = time_s(o, rr + X);
                    if (kp + kf == NB_KNOWN) s_uk += (double)lf;
                }
                s_l += (double)le + (double)ls;
                s_t += (double)lf;
                if (unk) {
                    const float uc = ul[li];
                    if (a.kw != NB_NONE) lw = space_link(sx, a.ow, rx, rr + Xw);
                    if (a.kn != NB_NONE) ln = space_link(sy, a.on, ry, rf + (size_t)(Y > 0 ? Y - 1 : g.H - 1) * rg.rw + X);
                    if (kb != NB_NONE) {     // (an arriving link: jb >= 0; its rho where its source wrote it)
                        const int tb = jb / n2, rb = jb - tb * n2, yb = rb / nx, xb = rb - yb * nx;
                        lb = time_s(ta.ob, (size_t)tb * rg.fstride + (size_t)(wg.y0 + yb) * rg.rw + (size_t)(wg.x0 + xb));
                    }
                    // the links to a low Dirichlet line have no other owner
                    if (a.kw == NB_DIRICHLET) s_l += (double)lw;
                    if (a.kn == NB_DIRICHLET) s_l += (double)ln;
                    const float pa = a.ke == NB_NONE ? 0.f : rounded_product(le, j.gx[o]);
                    const float pb = a.kw == NB_NONE ? 0.f : rounded_product(lw, j.gx[a.ow]);
                    const float pc = a.ks == NB_NONE ? 0.f : rounded_product(ls, j.gy[o]);
                    const float pd = a.kn == NB_NONE ? 0.f : rounded_product(ln, j.gy[a.on]);
                    const float pe = (kf == NB_NONE || !gt) ? 0.f : rounded_product(lf, gt[o]);
                    const float pf = (kb == NB_NONE || !gt) ? 0.f : rounded_product(lb, gt[ta.ob]);
                    v = ((pa - pb) + (pc - pd)) + (pe - pf);
                    float wr = 0.f;
                    if (!NOW) {
                        double e_d;
                        wr = robust_data(td, w[o], j.d[o], uc, v, e_d);
                        s_w += (double)wr;
                        s_e += e_d;
                    }
                    if (a.kw == NB_DIRICHLET) v -= rounded_product(lw, j.b[a.ow]);
                    if (a.kn == NB_DIRICHLET) v -= rounded_product(ln, j.b[a.on]);
                    if (a.ke == NB_DIRICHLET) v -= rounded_product(le, j.b[a.oe]);
                    if (a.ks == NB_DIRICHLET) v -= rounded_product(ls, j.b[a.os]);
                    if (a.kw == NB_KNOWN) v -= rounded_product(lw, j.d[a.ow]);
                    if (a.kn == NB_KNOWN) v -= rounded_product(ln, j.d[a.on]);
                    if (a.ke == NB_KNOWN) v -= rounded_product(le, j.d[a.oe]);
                    if (a.ks == NB_KNOWN) v -= rounded_product(ls, j.d[a.os]);
                    if (kb == NB_KNOWN) v -= rounded_product(lb, j.d[ta.ob]);
                    if (kf == NB_KNOWN) v -= rounded_product(lf, j.d[ta.of]);
                    e = a.ke == NB_UNKNOWN ? le : 0.f;
                    so = a.ks == NB_UNKNOWN ? ls : 0.f;
                    f = kf == NB_UNKNOWN ? lf : 0.f;
                    dg = (((lw + le) + (ln + ls)) + (lb + lf)) + wr;
                }
            }
            rc[ro] = v;
            ec[ro] = e;
            sco[ro] = so;
            fc[ro] = f;
            dc[ro] = dg;
            s_bb += (double)v * (double)v;
        }
    }
    part_store(s_bb, ws[0], wg, bb);
    part_store(s_w, ws[1], wg, sums, VOLUME_ROBUST_SUMS, 0);
    part_store(s_l, ws[2], wg, sums, VOLUME_ROBUST_SUMS, 1);
    part_store(s_t, ws[3], wg, sums, VOLUME_ROBUST_SUMS, 2);
    part_store(s_uk, ws[4], wg, sums, VOLUME_ROBUST_SUMS, 3);
    part_store(s_e, ws[5], wg, sums, VOLUME_ROBUST_SUMS, 4);
}

struct FlowCoupledArgs {
    const RobustTerm &grad, &time, &data;
    FlowLinks fl;
    const float *U;
    float *Rho, *R, *E, *S, *F, *Dg;
    double *bb, *sums, *esum;
    hipStream_t s;
};

template <bool NOW, bool LNK, bool SPACE, bool TIME, bool JOINT>
void flow_coupled_launches(const PoissonGeo &g, const PcgGeo &wg, const VolumeGeo &vg, const VolumeJobs &t, int cnt, const VolumeRhoGeo &rg,
                           const FlowCoupledArgs &a)
{
    const unsigned planes = (unsigned)(g.C * cnt);
    hipLaunchKernelGGL((k_volume_flow_robust_rho<LNK, SPACE, TIME, JOINT>), dim3((unsigned)wg.cg, (unsigned)wg.bands, JOINT ? (unsigned)cnt : planes),
                       dim3(WL), 0, a.s, g, wg, vg, t, a.grad, a.time, rg, a.fl, a.U, a.Rho, a.esum);
    hipLaunchKernelGGL((k_volume_flow_robust_setup_rho<NOW, LNK, SPACE, TIME, JOINT>), dim3((unsigned)wg.cg, (unsigned)wg.bands, planes), dim3(WL), 0,
                       a.s, g, wg, vg, t, a.grad.mode, a.time.mode, a.data, rg, a.fl, a.Rho, a.U, a.R, a.E, a.S, a.F, a.Dg, a.bb, a.sums);
}

template <bool SPACE, bool TIME, bool JOINT>
void flow_coupled_form(bool now, bool lnk, const PoissonGeo &g, const PcgGeo &wg, const VolumeGeo &vg, const VolumeJobs &t, int cnt,
                       const VolumeRhoGeo &rg, const FlowCoupledArgs &a)
{
    auto go = now ? (lnk ? flow_coupled_launches<true, true, SPACE, TIME, JOINT> : flow_coupled_launches<true, false, SPACE, TIME, JOINT>)
                  : (lnk ? flow_coupled_launches<false, true, SPACE, TIME, JOINT> : flow_coupled_launches<false, false, SPACE, TIME, JOINT>);
    go(g, wg, vg, t, cnt, rg, a);
}

} // namespace

void launch_volume_flow_robust_coupled(const PoissonGeo &g, const PcgGeo &wg, const VolumeGeo &vg, const PoissonJobDev *jobs, const SideArrays *sides,
                                       int m, const RobustTerm &grad, const RobustTerm &time, const RobustTerm &data, int coupling, const int *fwd,
                                       const int *bwd, const float *U, float *Rho, float *R, float *E, float *S, float *F, float *Dg, double *bb,
                                       double *sums, double *esum, hipStream_t s)
{
    const VolumeRhoGeo rg = volume_rho_geo(wg, vg, grad, time, coupling);
    const long long ls = flow_link_stride(wg);
    const bool space = (coupling & ROBUST_ISO) != 0, tm = (coupling & ROBUST_TIME) != 0, joint = (coupling & ROBUST_JOINT) != 0;
    for_side_tables<VolumeJobs>(jobs, sides, m, [&](const VolumeJobs &t, int i0, int cnt) {
        const size_t o = (size_t)g.C * i0 * wg.stride, po = (size_t)g.C * i0 * PCG_PARTS;
        const size_t ro = (size_t)(joint ? i0 : g.C * i0) * rg.unit;
        const bool now = !t.w[0], lnk = t.sx[0] || t.smt[0];
        const FlowCoupledArgs a{ grad, time, data, FlowLinks{ fwd + ls * i0, bwd + ls * i0, ls }, U + o, Rho + ro, R + o, E + o, S + o, F + o, Dg + o,
                                 bb + po, sums + po * VOLUME_ROBUST_SUMS, esum + po, s };
        // the five legal forms, as for_volume_coupled_tables (sc_volume_coupled.hip) deals them
        if (space && tm && joint) flow_coupled_form<true, true, true>(now, lnk, g, wg, vg, t, cnt, rg, a);
        else if (space && tm) flow_coupled_form<true, true, false>(now, lnk, g, wg, vg, t, cnt, rg, a);
        else if (space && joint) flow_coupled_form<true, false, true>(now, lnk, g, wg, vg, t, cnt, rg, a);
        else if (space) flow_coupled_form<true, false, false>(now, lnk, g, wg, vg, t, cnt, rg, a);
        else flow_coupled_form<false, false, true>(now, lnk, g, wg, vg, t, cnt, rg, a);
    });
}

} // namespace sc
