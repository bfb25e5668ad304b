// sc_volume_robust.hip -- the robust volume call's one kernel of its own (sc_hip_volume_robust*, sc_volume_api.cpp: VolumeRobustOperator's
// launch in a reweighting round, which RobustRounds::reweigh in sc_robust_api.cpp describes): k_volume_robust_setup, k_volume_setup
// (sc_volume.hip) with every link computed from the current iterate as k_robust_setup (sc_robust.hip) computes them.  The system of a
// round of
//     minimise  sum w phi_q(u - d) + sum c_x phi_p(dx u - gx) + sum c_y phi_p(dy u - gy) + sum c_t phi_r(u_(t+1) - u_t - gt)
// over the UNKNOWN pixels of a stack of frames is the WLS volume system with s = c rho(link residual) on every live link and w' = w
// rho_q(u - d), all at the iterate U on the work plane of stacked frames (sc_volume.hip: its layout).  c_x, c_y: smooth_x, smooth_y
// (NULL: 1); c_t = lt = tau * smooth_t, one rounded product (NULL: tau).
// The value of u across a link is NOT the work plane's wherever the neighbour is not UNKNOWN -- u0 = M^-1 b and z = M^-1 r fill the
// whole rectangle (sc_region.hip) --: it is data's at a KNOWN pixel, boundary's on a Dirichlet line and U's only at an UNKNOWN one.
// Both ends of a link compute its weight by one expression on the same operands -- t = (u_hi - u_lo) - g, hi / lo by the link's
// direction, then robust_link -- whichever end evaluates it: the same bits, so E / S / F of one end and the other end's share of Dg
// agree and L stays symmetric.  Nothing is carried from row to row: every link is computed where it is used (a launch per round
// against tens of operator launches), so a band may start anywhere inside a frame.
// The zero condition of the region family holds after every round: R = E = S = F = Dg = 0 at every pixel that is not UNKNOWN, and E,
// S, F are 0 on a link whose other end is not UNKNOWN.
// What is read: the header's elements of the WLS volume call -- a link weight and its g only where the link is live, data at UNKNOWN
// pixels only with a weight -- and U at UNKNOWN pixels.
#include "sc_region_device.h"
#include <cmath>

namespace sc {

namespace {

// NOW: no weight (w and data at UNKNOWN pixels are not read);  LNK: the call has a base link array (each array then is a uniform
// pointer test; false: every spatial base link is 1, every temporal one tau, no array is looked at);  PER: periodic time.
// sums[(plane * PCG_PARTS + part) * VOLUME_ROBUST_SUMS + ..] = the sum of w' | of the live spatial links s | of the live temporal
// links | of the UNKNOWN - KNOWN links of either kind | the energy of U, in double from the float32 values as robust_phi gives it.
// Every live link is counted once, under k_volume_stats' owner rule: by its low end (the last pixel of a periodic axis owns the
// wrapping link, the earlier frame a temporal link, frame T - 1 the wrapping one) whether that end is UNKNOWN or KNOWN, and by its
// UNKNOWN end where the other lies on a low Dirichlet line.
template <bool NOW, bool LNK, bool PER>
__global__ __launch_bounds__(WL) void k_volume_robust_setup(PoissonGeo g, PcgGeo wg, VolumeGeo vg, VolumeJobs t, RobustTerm tg, RobustTerm tt, RobustTerm td,
                                                             const float *__restrict__ U, float *__restrict__ R, float *__restrict__ E,
                                                             float *__restrict__ S, float *__restrict__ F, float *__restrict__ Dg,
                                                             double *__restrict__ bb, double *__restrict__ sums)
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
    const size_t n2 = (size_t)nx * fny;
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
                const TimeAround ta(vg, fr.t, o, PER);
                const int kb = time_kind(st, ta.ob, ta.hb), kf = time_kind(st, ta.of, ta.hf);
                // u at this pixel and across a link: U at an UNKNOWN pixel (li: its element of the plane), data at a KNOWN one, boundary on a Dirichlet line
                auto value = [&](int k, long long off, size_t i) { return k == NB_UNKNOWN ? ul[i] : k == NB_KNOWN ? j.d[off] : j.b[off]; };
                auto live = [&](int kq) { return kq != NB_NONE && (unk || kq == NB_UNKNOWN); };
                const float uc = value(kp, o, li);
                // the links this pixel owns: east, south, forward -- evaluated at a KNOWN low end as well, for the sums
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
                if (live(kf)) {
                    const size_t i_f = !PER || fr.t < vg.T - 1 ? li + n2 : li - (size_t)(vg.T - 1) * n2;
                    u_f = value(kf, ta.of, i_f);
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
                    if (kb != NB_NONE) {
                        const size_t i_b = !PER || fr.t > 0 ? li - n2 : li + (size_t)(vg.T - 1) * n2;
                        u_b = value(kb, ta.ob, i_b);
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

template <bool NOW, bool LNK> void robust_form(bool per, dim3 grid, hipStream_t s, const PoissonGeo &g, const PcgGeo &wg, const VolumeGeo &vg, const VolumeJobs &t,
                                               const RobustTerm &tg, const RobustTerm &tt, const RobustTerm &td, const float *U, float *R, float *E, float *S,
                                               float *F, float *Dg, double *bb, double *sums)
{
    if (per) hipLaunchKernelGGL((k_volume_robust_setup<NOW, LNK, true>), grid, dim3(WL), 0, s, g, wg, vg, t, tg, tt, td, U, R, E, S, F, Dg, bb, sums);
    else hipLaunchKernelGGL((k_volume_robust_setup<NOW, LNK, false>), grid, dim3(WL), 0, s, g, wg, vg, t, tg, tt, td, U, R, E, S, F, Dg, bb, sums);
}

} // namespace

void launch_volume_robust_setup(const PoissonGeo &g, const PcgGeo &wg, const VolumeGeo &vg, const PoissonJobDev *jobs, const SideArrays *sides, int m,
                                const RobustTerm &grad, const RobustTerm &time, const RobustTerm &data, const float *U, float *R, float *E, float *S,
                                float *F, float *Dg, double *bb, double *sums, hipStream_t s)
{
    for_side_tables<VolumeJobs>(jobs, sides, m, [&](const VolumeJobs &t, int i0, int cnt) {
        const dim3 grid((unsigned)wg.cg, (unsigned)wg.bands, (unsigned)(g.C * cnt));
        const size_t o = (size_t)g.C * i0 * wg.stride, po = (size_t)g.C * i0 * PCG_PARTS;
        const bool now = !t.w[0], lnk = t.sx[0] || t.smt[0], per = vg.periodic != 0;
        double *b = bb + po, *sm = sums + po * VOLUME_ROBUST_SUMS;
        if (now && lnk) robust_form<true, true>(per, grid, s, g, wg, vg, t, grad, time, data, U + o, R + o, E + o, S + o, F + o, Dg + o, b, sm);
        else if (now) robust_form<true, false>(per, grid, s, g, wg, vg, t, grad, time, data, U + o, R + o, E + o, S + o, F + o, Dg + o, b, sm);
        else if (lnk) robust_form<false, true>(per, grid, s, g, wg, vg, t, grad, time, data, U + o, R + o, E + o, S + o, F + o, Dg + o, b, sm);
        else robust_form<false, false>(per, grid, s, g, wg, vg, t, grad, time, data, U + o, R + o, E + o, S + o, F + o, Dg + o, b, sm);
    });
}

} // namespace sc
