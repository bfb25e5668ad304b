// sc_volume_subflow_robust.hip -- the robust sub-pixel flow volume call's two kernels of its own (sc_hip_volume_subflow_robust*,
// sc_volume_api.cpp: VolumeSubflowRobustOperator's launch in a reweighting round, which RobustRounds::reweigh in sc_robust_api.cpp
// describes).  A round of
//     minimise  sum w phi_q(u - d) + sum c_x phi_p(dx u - gx) + sum c_y phi_p(dy u - gy)
//               + sum over the live links p of c_t(p) phi_r(sum_k b_k(p) u~(q_k(p)) - u~(p) - gt(p))
// is the sub-pixel system (sc_volume_subflow.hip: -B^T S B in product form) with S taken at the iterate: a link's weight lives only at
// its source, in the LT plane that k_subflow_rho and k_subflow_op read, so a round rewrites LT, SG and the spatial planes and the
// operator's launches stay as they are; "both ends see the same bits" holds by construction.
//   k_subflow_robust_sigma   per work-plane element the link it holds, LT = robust_link(time, c_t, hi, u~(p), gt).s with hi = sum_k b_k
//                            u~(q_k) in float32 in tap order, SG = LT * g' (k_subflow_sigma's g'); its block's three temporal partials;
//   k_subflow_robust_setup   k_volume_robust_setup's spatial walk (sc_volume_robust.hip) with k_subflow_setup's temporal part of b, F = 1
//                            at UNKNOWN pixels and Dg the spatial links and w' alone; the five VOLUME_ROBUST_SUMS fields.
// u~ is U at an UNKNOWN pixel and data at a KNOWN one.  Both launches have one grid and one block numbering: the sigma launch leaves
// its block's sums of LT, of the UNKNOWN - KNOWN share and of the temporal energy in a small double array (three per part, part_store's
// addressing), the same block of the set-up launch adds them into fields 2, 3 and 4 of its own sums.  No atomics; two runs, the same
// bytes; one host read per round (reweigh's).
#include "sc_subflow_device.h"
#include <cmath>

namespace sc {

namespace {

constexpr int SUBFLOW_ROBUST_PARTIALS = 3;      // sum of LT | UNKNOWN - KNOWN share | temporal energy

// tp[(plane * PCG_PARTS + part) * 3 + ..]: the block's temporal sums, every link counted once, at its source -- k_subflow_stats' rule
// for the UNKNOWN - KNOWN share: LT * (1 where the source is KNOWN, else the sum of b over the KNOWN taps).  gt and smooth_t are read at
// the source of a live link only.
__global__ __launch_bounds__(WL) void k_subflow_robust_sigma(PoissonGeo g, PcgGeo wg, VolumeGeo vg, VolumeJobs t, SubflowLinks L, RobustTerm tt,
                                                              const float *__restrict__ U, float *__restrict__ LT, float *__restrict__ SG,
                                                              double *__restrict__ tp)
{
    __shared__ double ws[SUBFLOW_ROBUST_PARTIALS][4];
    lane_term(tt);
    const PcgBand bd(g, wg);
    const PoissonJobDev &j = t.j[bd.member];
    const float *__restrict__ st = t.st[bd.member], *__restrict__ gt = t.gt[bd.member], *__restrict__ smt = t.smt[bd.member];
    const float *__restrict__ fw = L.fw + (long long)bd.member * 2 * L.n;
    const float *__restrict__ ul = U + (size_t)bd.p * wg.stride;
    double s_t = 0.0, s_uk = 0.0, s_e = 0.0;
    if (bd.x < wg.nx)
        for (int y = bd.y0; y < bd.y1; ++y) {
            const FrameRow fr(vg, y);
            const long long o = bd.pixel(g, wg.x0 + bd.x, wg.y0 + fr.yy) + (long long)fr.t * vg.fs;
            const size_t ip = (size_t)y * wg.nx + bd.x;
            int q[4];
            float b[4];
            float lt = 0.f, sg = 0.f;
            if (subflow_taps(wg, vg, fw[ip], fw[L.n + ip], bd.x, fr.yy, fr.t, q, b)) {
                const int kp = state_kind(st[o]);
                bool dead = kp == NB_NONE, unk = kp == NB_UNKNOWN;
                float hi = 0.f, kb = 0.f, kd = 0.f;
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (q[k] >= 0) {
                        const long long oq = subflow_offset(g, wg, vg, bd.c, q[k]);
                        const int kq = state_kind(st[oq]);
                        dead = dead || kq == NB_NONE;
                        unk = unk || kq == NB_UNKNOWN;
                        float uq = 0.f;
                        if (kq == NB_UNKNOWN) uq = ul[q[k]];
                        else if (kq == NB_KNOWN) {
                            uq = j.d[oq];
                            kb += b[k];
                            kd += b[k] * uq;
                        }
                        hi += b[k] * uq;
                    }
                if (!dead && unk) {
                    const float up = kp == NB_UNKNOWN ? ul[ip] : j.d[o], gv = gt ? gt[o] : 0.f;
                    const RobustLink lk = robust_link(tt, time_link(smt, o, vg.tau), hi, up, gv);
                    lt = lk.s;
                    float gp = gv - kd;
                    if (kp == NB_KNOWN) gp += up;
                    sg = lt * gp;
                    s_t += (double)lt;
                    s_uk += (double)lt * (double)(kp == NB_KNOWN ? 1.f : kb);
                    s_e += lk.e;
                }
            }
            const size_t i = (size_t)bd.p * wg.stride + ip;
            LT[i] = lt;
            SG[i] = sg;
        }
    part_store(s_t, ws[0], wg, tp, SUBFLOW_ROBUST_PARTIALS, 0);
    part_store(s_uk, ws[1], wg, tp, SUBFLOW_ROBUST_PARTIALS, 1);
    part_store(s_e, ws[2], wg, tp, SUBFLOW_ROBUST_PARTIALS, 2);
}

// NOW: no weight (w and data at UNKNOWN pixels are not read);  LNK: the call has a spatial base link array (false: every spatial base
// link is 1, no array is looked at).  The spatial links, w', the Dirichlet and KNOWN folds and the sums' owner rule are
// k_volume_robust_setup's; the temporal part of b at an UNKNOWN pixel i is SG(i) less the sum over the arrivals (s, b) of b * SG(s) in the
// rows' fixed order, as in k_subflow_setup.  sums: launch_volume_robust_setup's five fields, the temporal shares from the sigma launch's
// partials of this block.
template <bool NOW, bool LNK>
__global__ __launch_bounds__(WL) void k_subflow_robust_setup(PoissonGeo g, PcgGeo wg, VolumeGeo vg, VolumeJobs t, SubflowLinks L, RobustTerm tg, RobustTerm td,
                                                              const float *__restrict__ U, const float *__restrict__ SG, const double *__restrict__ tp,
                                                              float *__restrict__ R, float *__restrict__ E, float *__restrict__ S, float *__restrict__ F,
                                                              float *__restrict__ Dg, double *__restrict__ bb, double *__restrict__ sums)
{
    __shared__ double ws[VOLUME_ROBUST_SUMS + 1][4];
    lane_term(tg); lane_term(td);
    const PcgBand bd(g, wg);
    const PoissonJobDev &j = t.j[bd.member];
    const float *__restrict__ w = t.w[bd.member], *__restrict__ st = t.st[bd.member];
    const float *__restrict__ sx = LNK ? t.sx[bd.member] : nullptr, *__restrict__ sy = LNK ? t.sy[bd.member] : nullptr;
    const long long *__restrict__ off = L.off + (long long)bd.member * (L.n + 2);
    const unsigned long long *__restrict__ ent = L.ent + (long long)bd.member * 4 * L.n;
    const bool px = wg.ax == MIXED_PERIODIC, py = wg.ay == MIXED_PERIODIC;
    const int nx = wg.nx, fny = vg.ny, x = bd.x;
    const float *__restrict__ ul = U + (size_t)bd.p * wg.stride, *__restrict__ sg = SG + (size_t)bd.p * wg.stride;
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
                // u at this pixel and across a link: U at an UNKNOWN pixel (li: its element of the plane), data at a KNOWN one, boundary on a Dirichlet line
                auto value = [&](int k, long long at, size_t i) { return k == NB_UNKNOWN ? ul[i] : k == NB_KNOWN ? j.d[at] : j.b[at]; };
                auto live = [&](int kq) { return kq != NB_NONE && (unk || kq == NB_UNKNOWN); };
                const float uc = value(kp, o, li);
                // the spatial links this pixel owns: east, south -- evaluated at a KNOWN low end as well, for the sums
                RobustLink east{ 0.f, 0.0 }, south{ 0.f, 0.0 }, west{ 0.f, 0.0 }, north{ 0.f, 0.0 };
                float g_e = 0.f, g_s = 0.f, g_w = 0.f, g_n = 0.f, u_e = 0.f, u_s = 0.f, u_w = 0.f, u_n = 0.f;
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
                s_l += (double)east.s + (double)south.s;
                s_e += east.e + south.e;
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
                    // the links to a low Dirichlet line have no other owner
                    if (a.kw == NB_DIRICHLET) { s_l += (double)west.s; s_e += west.e; }
                    if (a.kn == NB_DIRICHLET) { s_l += (double)north.s; s_e += north.e; }
                    const float lw = west.s, le = east.s, ln = north.s, ls = south.s;
                    float arr = 0.f;
                    for (long long k = off[li], k1 = off[li + 1]; k < k1; ++k) {
                        const unsigned long long en = ent[k];
                        arr += __uint_as_float((unsigned int)(en >> 32)) * sg[(unsigned int)en];
                    }
                    const float tm = sg[li] - arr;
                    const float pa = a.ke == NB_NONE ? 0.f : rounded_product(le, g_e);
                    const float pb = a.kw == NB_NONE ? 0.f : rounded_product(lw, g_w);
                    const float pc = a.ks == NB_NONE ? 0.f : rounded_product(ls, g_s);
                    const float pd = a.kn == NB_NONE ? 0.f : rounded_product(ln, g_n);
                    v = ((pa - pb) + (pc - pd)) + tm;
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
                    e = a.ke == NB_UNKNOWN ? le : 0.f;
                    so = a.ks == NB_UNKNOWN ? ls : 0.f;
                    f = 1.f;
                    dg = ((lw + le) + (ln + ls)) + wr;
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
    if (threadIdx.x == 0) {      // this block's temporal shares, as the sigma launch left them
        const double *__restrict__ own = tp + ((size_t)blockIdx.z * PCG_PARTS + blockIdx.y * wg.cg + blockIdx.x) * SUBFLOW_ROBUST_PARTIALS;
        s_t += own[0];
        s_uk += own[1];
        s_e += own[2];
    }
    part_store(s_bb, ws[0], wg, bb);
    part_store(s_w, ws[1], wg, sums, VOLUME_ROBUST_SUMS, 0);
    part_store(s_l, ws[2], wg, sums, VOLUME_ROBUST_SUMS, 1);
    part_store(s_t, ws[3], wg, sums, VOLUME_ROBUST_SUMS, 2);
    part_store(s_uk, ws[4], wg, sums, VOLUME_ROBUST_SUMS, 3);
    part_store(s_e, ws[5], wg, sums, VOLUME_ROBUST_SUMS, 4);
}

} // namespace

size_t subflow_robust_partials(int planes) { return (size_t)planes * PCG_PARTS * SUBFLOW_ROBUST_PARTIALS; }

void launch_volume_subflow_robust_setup(const PoissonGeo &g, const PcgGeo &wg, const VolumeGeo &vg, const PoissonJobDev *jobs, const SideArrays *sides, int m,
                                        const RobustTerm &grad, const RobustTerm &time, const RobustTerm &data, const SubflowStore &st, void *lnk,
                                        const float *U, float *LT, float *SG, double *tp, float *R, float *E, float *S, float *F, float *Dg, double *bb,
                                        double *sums, hipStream_t s)
{
    for_side_tables<VolumeJobs>(jobs, sides, m, [&](const VolumeJobs &t, int i0, int cnt) {
        const dim3 grid((unsigned)wg.cg, (unsigned)wg.bands, (unsigned)(g.C * cnt));
        const size_t o = (size_t)g.C * i0 * wg.stride, po = (size_t)g.C * i0 * PCG_PARTS;
        const SubflowLinks L = subflow_links_at(st, lnk, i0);
        const bool now = !t.w[0], lnks = t.sx[0] != nullptr;
        double *b = bb + po, *sm = sums + po * VOLUME_ROBUST_SUMS, *part = tp + po * SUBFLOW_ROBUST_PARTIALS;
        hipLaunchKernelGGL(k_subflow_robust_sigma, grid, dim3(WL), 0, s, g, wg, vg, t, L, time, U + o, LT + o, SG + o, part);
        if (now && lnks)
            hipLaunchKernelGGL((k_subflow_robust_setup<true, true>), grid, dim3(WL), 0, s, g, wg, vg, t, L, grad, data, U + o, (const float *)(SG + o),
                               (const double *)part, R + o, E + o, S + o, F + o, Dg + o, b, sm);
        else if (now)
            hipLaunchKernelGGL((k_subflow_robust_setup<true, false>), grid, dim3(WL), 0, s, g, wg, vg, t, L, grad, data, U + o, (const float *)(SG + o),
                               (const double *)part, R + o, E + o, S + o, F + o, Dg + o, b, sm);
        else if (lnks)
            hipLaunchKernelGGL((k_subflow_robust_setup<false, true>), grid, dim3(WL), 0, s, g, wg, vg, t, L, grad, data, U + o, (const float *)(SG + o),
                               (const double *)part, R + o, E + o, S + o, F + o, Dg + o, b, sm);
        else
            hipLaunchKernelGGL((k_subflow_robust_setup<false, false>), grid, dim3(WL), 0, s, g, wg, vg, t, L, grad, data, U + o, (const float *)(SG + o),
                               (const double *)part, R + o, E + o, S + o, F + o, Dg + o, b, sm);
    });
}

} // namespace sc
