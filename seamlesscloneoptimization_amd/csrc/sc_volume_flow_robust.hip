// sc_volume_flow_robust.hip -- the robust flow volume call's one kernel of its own (sc_hip_volume_flow_robust*, sc_volume_api.cpp:
// VolumeFlowRobustOperator's launch in a reweighting round): k_volume_flow_robust_setup, k_volume_robust_setup (sc_volume_robust.hip:
// the round's system, the value of u across a link, the sums and their owner rule, the zero condition) with the two temporal
// neighbours of an element taken from the volume's link planes (sc_pcg.h: what they hold; sc_volume_flow.hip: the matching) as
// k_volume_setup's flow form takes them.  The round's system of
//     minimise  sum w phi_q(u - d) + sum c_x phi_p(dx u - gx) + sum c_y phi_p(dy u - gy)
//                                  + sum_(matched live links i -> fwd[i]) c_t(i) phi_r(u[fwd[i]] - u[i] - gt(i))
// is the flow volume system with s = c rho(link residual) on every live link and w' = w rho_q(u - d) at the iterate U.
// A temporal link lives at its source: the link element i holds leads to jf = fwd[i], its base weight lt = tau * smooth_t and its gt
// are stored at i's own offset o; the link that arrives at i comes from jb = bwd[i] and its lt and gt are stored at jb's offset.  A
// neighbour's kind is state's at the offset TimeAround's flow constructor gives; its value is U[j] where it is UNKNOWN -- a link
// plane's index IS the work-plane index -- and data's where it is KNOWN.  Both ends compute the link's weight as robust_link(time,
// base, u_target, u_source, gt_source) on the same operands: F at the source and the target's share of Dg carry the same bits.  The
// wrap of periodic time is in the indices, so there is no periodic form.
// Per element beyond k_volume_robust_setup: two int32 loads (the link planes), and in place of the two neighbours one frame away a
// gather of state, and of U or data, smooth_t and gt, at the two ends -- as coalesced as the flow is smooth.  No atomics, no LDS but
// the block sums'.
#include "sc_region_device.h"
#include <cmath>

namespace sc {

namespace {

// NOW, LNK: k_volume_robust_setup's.  sums: VOLUME_ROBUST_SUMS' fields under its owner rule -- a temporal link is counted once, at
// its source, whether that end is UNKNOWN or KNOWN.
template <bool NOW, bool LNK>
__global__ __launch_bounds__(WL) void k_volume_flow_robust_setup(PoissonGeo g, PcgGeo wg, VolumeGeo vg, VolumeJobs t, RobustTerm tg, RobustTerm tt,
                                                                  RobustTerm td, FlowLinks fl, const float *__restrict__ U, float *__restrict__ R,
                                                                  float *__restrict__ E, float *__restrict__ S, float *__restrict__ F,
                                                                  float *__restrict__ Dg, double *__restrict__ bb, double *__restrict__ sums)
{
    __shared__ double ws[VOLUME_ROBUST_SUMS + 1][4];
    lane_term(tg); lane_term(tt); lane_term(td);
    const PcgBand bd(g, wg);
    const PoissonJobDev &j = t.j[bd.member];
    const float *__restrict__ w = t.w[bd.member], *__restrict__ st = t.st[bd.member], *__restrict__ gt = t.gt[bd.member];
    const float *__restrict__ sx = LNK ? t.sx[bd.member] : nullptr, *__restrict__ sy = LNK ? t.sy[bd.member] : nullptr;
    const float *__restrict__ smt = LNK ? t.smt[bd.member] : nullptr;
    const bool px = wg.ax == MIXED_PERIODIC, py = wg.ay == MIXED_PERIODIC;
    const int nx = wg.nx, fny = vg.ny, x = bd.x;
    const float *__restrict__ ul = U + (size_t)bd.p * wg.stride;
    const float tau = vg.tau;
    // this lane's column of the five planes it writes: per-lane pointers, so that the planes' bases need no scalar registers inside the walk
    const size_t col = (size_t)bd.p * wg.stride + (size_t)(x < nx ? x : 0);
    float *__restrict__ rc = R + col, *__restrict__ ec = E + col, *__restrict__ sco = S + col, *__restrict__ fc = F + col, *__restrict__ dc = Dg + col;
    double s_bb = 0.0, s_w = 0.0, s_l = 0.0, s_t = 0.0, s_uk = 0.0, s_e = 0.0;
    if (x < nx) {
        const int xw = x > 0 ? x - 1 : nx - 1, xe = x < nx - 1 ? x + 1 : 0;      // (read only where the neighbour is UNKNOWN: then a column of the plane)
        for (int y = bd.y0; y < bd.y1; ++y) {
            const FrameRow fr(vg, y);
            const int X = wg.x0 + x, Y = wg.y0 + fr.yy;
            const long long o = bd.pixel(g, X, Y) + (long long)fr.t * vg.fs;
            const size_t ro = (size_t)y * nx, li = ro + x;
            const int kp = state_kind(st[o]);
            float v = 0.f, e = 0.f, so = 0.f, f = 0.f, dg = 0.f;
            if (kp != NB_NONE) {
                const bool unk = kp == NB_UNKNOWN;
                const Around a(g, wg, st, X, Y, o, px, py);
                // the ends of the two links of element li: their offsets under the layout, and their work-plane indices (>= 0 where the link exists)
                const TimeAround ta(g, wg, vg, fl, bd.member, bd.c, y, x);
                const int jb = ta.jb, jf = ta.jf;
                const int kb = time_kind(st, ta.ob, ta.hb), kf = time_kind(st, ta.of, ta.hf);
                // u at this pixel and across a link: U at an UNKNOWN pixel (i: its element of the plane), data at a KNOWN one, boundary on a Dirichlet line
                auto value = [&](int k, long long off, size_t i) { return k == NB_UNKNOWN ? ul[i] : k == NB_KNOWN ? j.d[off] : j.b[off]; };
                auto live = [&](int kq) { return kq != NB_NONE && (unk || kq == NB_UNKNOWN); };
                const float uc = value(kp, o, li);
                // the links this pixel owns: east, south, the held one -- evaluated at a KNOWN low end or source as well, for the sums
                RobustLink east{ 0.f, 0.0 }, south{ 0.f, 0.0 }, fwd{ 0.f, 0.0 }, west{ 0.f, 0.0 }, north{ 0.f, 0.0 }, back{ 0.f, 0.0 };
                float g_e = 0.f, g_s = 0.f, g_f = 0.f, g_w = 0.f, g_n = 0.f, g_b = 0.f, u_e = 0.f, u_s = 0.f, u_f = 0.f, u_w = 0.f, u_n = 0.f, u_b = 0.f;
                if (live(a.ke)) {
                    u_e = value(a.ke, a.oe, ro + xe);
                    g_e = j.gx[o];
                    east = robust_link(tg, sx ? sx[o] : 1.f, u_e, uc, g_e);
                    if (kp + a.ke == NB_KNOWN) s_uk += (double)east.s;
                }
                if (live(a.ks)) {
                    u_s = value(a.ks, a.os, fr.yy < fny - 1 ? li + nx : li - (size_t)(fny - 1) * nx);
                    g_s = j.gy[o];
                    south = robust_link(tg, sy ? sy[o] : 1.f, u_s, uc, g_s);
                    if (kp + a.ks == NB_KNOWN) s_uk += (double)south.s;
                }
                if (live(kf)) {          // (kf is NB_NONE without a held link: jf >= 0 here)
                    u_f = value(kf, ta.of, (size_t)jf);
                    g_f = gt ? gt[o] : 0.f;
                    fwd = robust_link(tt, time_link(smt, o, tau), u_f, uc, g_f);
                    if (kp + kf == NB_KNOWN) s_uk += (double)fwd.s;
                }
                s_l += (double)east.s + (double)south.s;
                s_t += (double)fwd.s;
                s_e += (east.e + south.e) + fwd.e;
                if (unk) {
                    if (a.kw != NB_NONE) {
                        u_w = value(a.kw, a.ow, ro + xw);
                        g_w = j.gx[a.ow];
                        west = robust_link(tg, sx ? sx[a.ow] : 1.f, uc, u_w, g_w);
                    }
                    if (a.kn != NB_NONE) {
                        u_n = value(a.kn, a.on, fr.yy > 0 ? li - nx : li + (size_t)(fny - 1) * nx);
                        g_n = j.gy[a.on];
                        north = robust_link(tg, sy ? sy[a.on] : 1.f, uc, u_n, g_n);
                    }
                    if (kb != NB_NONE) {     // (an arriving link: jb >= 0; its base weight and gt at its source)
                        u_b = value(kb, ta.ob, (size_t)jb);
                        g_b = gt ? gt[ta.ob] : 0.f;
                        back = robust_link(tt, time_link(smt, ta.ob, tau), uc, u_b, g_b);
                    }
                    // the links to a low Dirichlet line have no other owner
                    if (a.kw == NB_DIRICHLET) { s_l += (double)west.s; s_e += west.e; }
                    if (a.kn == NB_DIRICHLET) { s_l += (double)north.s; s_e += north.e; }
                    const float lw = west.s, le = east.s, ln = north.s, ls = south.s, lb = back.s, lf = fwd.s;
                    const float pa = a.ke == NB_NONE ? 0.f : rounded_product(le, g_e);
                    const float pb = a.kw == NB_NONE ? 0.f : rounded_product(lw, g_w);
                    const float pc = a.ks == NB_NONE ? 0.f : rounded_product(ls, g_s);
                    const float pd = a.kn == NB_NONE ? 0.f : rounded_product(ln, g_n);
                    const float pe = (kf == NB_NONE || !gt) ? 0.f : rounded_product(lf, g_f);
                    const float pf = (kb == NB_NONE || !gt) ? 0.f : rounded_product(lb, g_b);
                    v = ((pa - pb) + (pc - pd)) + (pe - pf);
                    float wr = 0.f;
                    if (!NOW) {
                        double e_d;
                        wr = robust_data(td, w[o], j.d[o], uc, v, e_d);
                        s_w += (double)wr;
                        s_e += e_d;
                    }
                    if (a.kw == NB_DIRICHLET) v -= rounded_product(lw, u_w);
                    if (a.kn == NB_DIRICHLET) v -= rounded_product(ln, u_n);
                    if (a.ke == NB_DIRICHLET) v -= rounded_product(le, u_e);
                    if (a.ks == NB_DIRICHLET) v -= rounded_product(ls, u_s);
                    if (a.kw == NB_KNOWN) v -= rounded_product(lw, u_w);
                    if (a.kn == NB_KNOWN) v -= rounded_product(ln, u_n);
                    if (a.ke == NB_KNOWN) v -= rounded_product(le, u_e);
                    if (a.ks == NB_KNOWN) v -= rounded_product(ls, u_s);
                    if (kb == NB_KNOWN) v -= rounded_product(lb, u_b);
                    if (kf == NB_KNOWN) v -= rounded_product(lf, u_f);
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

} // namespace

void launch_volume_flow_robust_setup(const PoissonGeo &g, const PcgGeo &wg, const VolumeGeo &vg, const PoissonJobDev *jobs, const SideArrays *sides, int m,
                                     const RobustTerm &grad, const RobustTerm &time, const RobustTerm &data, const int *fwd, const int *bwd,
                                     const float *U, float *R, float *E, float *S, float *F, float *Dg, double *bb, double *sums, hipStream_t s)
{
    const long long ls = flow_link_stride(wg);
    for_side_tables<VolumeJobs>(jobs, sides, m, [&](const VolumeJobs &t, int i0, int cnt) {
        const dim3 grid((unsigned)wg.cg, (unsigned)wg.bands, (unsigned)(g.C * cnt));
        const size_t o = (size_t)g.C * i0 * wg.stride, po = (size_t)g.C * i0 * PCG_PARTS;
        const bool now = !t.w[0], lnk = t.sx[0] || t.smt[0];
        const FlowLinks fl{ fwd + ls * i0, bwd + ls * i0, ls };
        double *b = bb + po, *sm = sums + po * VOLUME_ROBUST_SUMS;
        auto form = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, dim3(WL), 0, s, g, wg, vg, t, grad, time, data, fl, U + o, R + o, E + o, S + o, F + o, Dg + o, b, sm);
        };
        if (now && lnk) form(k_volume_flow_robust_setup<true, true>);
        else if (now) form(k_volume_flow_robust_setup<true, false>);
        else if (lnk) form(k_volume_flow_robust_setup<false, true>);
        else form(k_volume_flow_robust_setup<false, false>);
    });
}

} // namespace sc
