// sc_volume_coupled.hip -- the coupled volume call's two kernels (sc_hip_volume_coupled*, sc_volume_api.cpp: VolumeRobustOperator's
// launches in a reweighting round under a coupling, which RobustRounds::reweigh in sc_robust_api.cpp describes): k_volume_robust_rho
// and k_volume_robust_setup_rho, k_region_robust_rho and k_region_robust_setup_rho (sc_region_robust.hip) on k_volume_robust_setup's
// walk (sc_volume_robust.hip: frames stacked along y, FrameRow, TimeAround, every link computed where it is used, so a band may start
// anywhere inside a frame).  The system of a round is the WLS volume system with s = c rho(M) on every link that shares the magnitude
// M and w' = w rho_q(u - d); a link's share of a magnitude is a = c t^2, t = (u_hi - u_lo) - g, c = smooth_x, smooth_y (NULL: 1, no
// multiply) or lt = tau * smooth_t rounded once (NULL: tau).  The forms (seamlessclone_hip.h, the coupled volume section):
//   SPACE           one magnitude per pixel over its x- and y-link: (a_x + a_y), penalty (p_grad, eps_grad);
//   SPACE | TIME    ... and its forward temporal link: (a_x + a_y) + a_t, the one penalty (p_time = p_grad, eps_time = eps_grad);
//   JOINT           every magnitude is the running sum over channels 0 .. C - 1, only the channels in which the link is live; the
//                   temporal links' is then sum_k a_t under (p_time, eps_time).  Without JOINT and without TIME a temporal link keeps
//                   the uncoupled penalty c_t phi_r(t): its rho is rho_r(t), robust_rho's bits.
// The owner of a link is its low end: the last pixel of a periodic axis owns the wrapping link, the earlier frame a temporal link,
// frame T - 1 the wrapping one; a pixel of a low Dirichlet line owns only its one spatial link into the domain, which forms a magnitude
// of its own and is written by its UNKNOWN end.  A dead link adds nothing to a magnitude; an owner with no live link writes no rho and
// books no energy.  A penalty of exponent 2 has rho 1: its component of the rho planes is neither written nor read, the base value
// passes through without a multiply and its energy is booked link by link, c t^2 in double.
// The rho planes: per unit (a volume under JOINT, else a work plane) up to three components -- xy | t under SPACE, one under SPACE |
// TIME, x | y | t otherwise -- of T frames each, a frame robust_rho_stride of the frame's rectangle apart, addressed [frame][Y][X].
// Every element is written by its owner only: no atomics.  What is read: the robust volume call's elements, and U at UNKNOWN pixels.
#include "sc_region_device.h"
#include <cmath>

namespace sc {

namespace {

// a link's share of a magnitude: c t^2, the square rounded, then the product (c NULL: no multiply)
__device__ __forceinline__ float coupled_sq(const float *__restrict__ c, long long o, float t)
{
    const float q = rounded_product(t, t);
    return c ? rounded_product(c[o], q) : q;
}

// grid: cg x bands x units; esum[(the unit's first plane * PCG_PARTS + part)] = the part's gradient-and-time energy
template <bool LNK, bool PER, bool SPACE, bool TIME, bool JOINT>
__global__ __launch_bounds__(WL) void k_volume_robust_rho(PoissonGeo g, PcgGeo wg, VolumeGeo vg, VolumeJobs t, RobustTerm tg, RobustTerm tt, VolumeRhoGeo rg,
                                                           const float *__restrict__ U, float *__restrict__ Rho, double *__restrict__ esum)
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
    const size_t n2 = (size_t)nx * fny;
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
            // the magnitudes: this pixel's (mx: its x-link's, or under SPACE both spatial links' and under TIME the forward link's too;
            // my: its y-link's; mt: its forward link's), the west Dirichlet pixel's x-link (mw), the north Dirichlet pixel's y-link (mn);
            // has_*: live in a channel;  e2: the energy of the links without a magnitude, link by link
            float mx = 0.f, my = 0.f, mt = 0.f, mw = 0.f, mn = 0.f;
            bool has_x = false, has_y = false, has_t = false, has_w = false, has_n = false;
            double e2 = 0.0;
            for (int k = k0; k < k1; ++k) {
                const long long o = (long long)X * g.cs + (long long)Y * g.rs + (long long)k * g.chs + (long long)fr.t * vg.fs;
                const int kp = state_kind(st[o]);
                if (kp == NB_NONE) continue;
                const bool unk = kp == NB_UNKNOWN;
                const Around a(g, wg, st, X, Y, o, px, py);
                const TimeAround ta(vg, fr.t, o, PER);
                const int kf = time_kind(st, ta.of, ta.hf);
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
                if (live(kf)) {
                    const size_t i_f = !PER || fr.t < vg.T - 1 ? li + n2 : li - (size_t)(vg.T - 1) * n2;
                    const float tr = (value(kf, ta.of, i_f) - uc) - (gt ? gt[o] : 0.f), lt = time_link(smt, o, tau);
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

// k_volume_robust_setup (its walk, its order, its five sums) with every link's rho read from the rho planes -- at the pixel (east,
// south, forward), at its west, north and back owner, only where that link is live: then its owner wrote it.  Field 4 of the sums: the
// data term's energy alone.  gmode, tmode: the modes of the spatial and of the temporal penalty (0: no rho, the base link itself).
template <bool NOW, bool LNK, bool PER, bool SPACE, bool TIME, bool JOINT>
__global__ __launch_bounds__(WL) void k_volume_robust_setup_rho(PoissonGeo g, PcgGeo wg, VolumeGeo vg, VolumeJobs t, int gmode, int tmode, RobustTerm td,
                                                                 VolumeRhoGeo rg, const float *__restrict__ Rho, const float *__restrict__ U,
                                                                 float *__restrict__ R, float *__restrict__ E, float *__restrict__ S,
                                                                 float *__restrict__ F, float *__restrict__ Dg, double *__restrict__ bb,
                                                                 double *__restrict__ sums)
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
    const int nx = wg.nx, x = bd.x;
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
                const TimeAround ta(vg, fr.t, o, PER);
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
                    if (kb != NB_NONE) {
                        const int tb = fr.t > 0 ? fr.t - 1 : vg.T - 1;              // the owner of the back link
                        lb = time_s(ta.ob, (size_t)tb * rg.fstride + (size_t)Y * rg.rw + X);
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

struct CoupledArgs {
    const RobustTerm &grad, &time, &data;
    const float *U;
    float *Rho, *R, *E, *S, *F, *Dg;
    double *bb, *sums, *esum;
    hipStream_t s;
};

template <bool NOW, bool LNK, bool PER, bool SPACE, bool TIME, bool JOINT>
void coupled_launches(const PoissonGeo &g, const PcgGeo &wg, const VolumeGeo &vg, const VolumeJobs &t, int cnt, const VolumeRhoGeo &rg, const CoupledArgs &a)
{
    const unsigned planes = (unsigned)(g.C * cnt);
    hipLaunchKernelGGL((k_volume_robust_rho<LNK, PER, SPACE, TIME, JOINT>), dim3((unsigned)wg.cg, (unsigned)wg.bands, JOINT ? (unsigned)cnt : planes),
                       dim3(WL), 0, a.s, g, wg, vg, t, a.grad, a.time, rg, a.U, a.Rho, a.esum);
    hipLaunchKernelGGL((k_volume_robust_setup_rho<NOW, LNK, PER, SPACE, TIME, JOINT>), dim3((unsigned)wg.cg, (unsigned)wg.bands, planes), dim3(WL), 0,
                       a.s, g, wg, vg, t, a.grad.mode, a.time.mode, a.data, rg, a.Rho, a.U, a.R, a.E, a.S, a.F, a.Dg, a.bb, a.sums);
}

template <bool SPACE, bool TIME, bool JOINT>
void coupled_form(bool now, bool lnk, bool per, const PoissonGeo &g, const PcgGeo &wg, const VolumeGeo &vg, const VolumeJobs &t, int cnt,
                  const VolumeRhoGeo &rg, const CoupledArgs &a)
{
    auto go = now ? (lnk ? (per ? coupled_launches<true, true, true, SPACE, TIME, JOINT> : coupled_launches<true, true, false, SPACE, TIME, JOINT>)
                         : (per ? coupled_launches<true, false, true, SPACE, TIME, JOINT> : coupled_launches<true, false, false, SPACE, TIME, JOINT>))
                  : (lnk ? (per ? coupled_launches<false, true, true, SPACE, TIME, JOINT> : coupled_launches<false, true, false, SPACE, TIME, JOINT>)
                         : (per ? coupled_launches<false, false, true, SPACE, TIME, JOINT> : coupled_launches<false, false, false, SPACE, TIME, JOINT>));
    go(g, wg, vg, t, cnt, rg, a);
}

// The coupled volume forms' launches of every side table: fn(space, time, joint, t, cnt, o, po, ro) -- the form as std::bool_constant,
// for the kernels' template arguments; o, po, ro: the first volume's offset into the work planes, into the parts (per double of a part)
// and into the rho planes
template <class Fn>
void for_volume_coupled_tables(const PoissonGeo &g, const PcgGeo &wg, const VolumeRhoGeo &rg, const PoissonJobDev *jobs, const SideArrays *sides, int m,
                               int coupling, Fn fn)
{
    const bool space = (coupling & ROBUST_ISO) != 0, time = (coupling & ROBUST_TIME) != 0, joint = (coupling & ROBUST_JOINT) != 0;
    for_side_tables<VolumeJobs>(jobs, sides, m, [&](const VolumeJobs &t, int i0, int cnt) {
        const size_t o = (size_t)g.C * i0 * wg.stride, po = (size_t)g.C * i0 * PCG_PARTS;
        const size_t ro = (size_t)(joint ? i0 : g.C * i0) * rg.unit;
        using T = std::true_type;
        using F = std::false_type;
        if (space && time && joint) fn(T(), T(), T(), t, cnt, o, po, ro);
        else if (space && time) fn(T(), T(), F(), t, cnt, o, po, ro);
        else if (space && joint) fn(T(), F(), T(), t, cnt, o, po, ro);
        else if (space) fn(T(), F(), F(), t, cnt, o, po, ro);
        else fn(F(), F(), T(), t, cnt, o, po, ro);
    });
}

} // namespace

void launch_volume_robust_coupled(const PoissonGeo &g, const PcgGeo &wg, const VolumeGeo &vg, const PoissonJobDev *jobs, const SideArrays *sides, int m,
                                  const RobustTerm &grad, const RobustTerm &time, const RobustTerm &data, int coupling, const float *U, float *Rho,
                                  float *R, float *E, float *S, float *F, float *Dg, double *bb, double *sums, double *esum, hipStream_t s)
{
    const VolumeRhoGeo rg = volume_rho_geo(wg, vg, grad, time, coupling);
    for_volume_coupled_tables(g, wg, rg, jobs, sides, m, coupling, [&](auto space, auto tm, auto joint, const VolumeJobs &t, int cnt, size_t o, size_t po, size_t ro) {
        const bool now = !t.w[0], lnk = t.sx[0] || t.smt[0], per = vg.periodic != 0;
        const CoupledArgs a{ grad, time, data, U + o, Rho + ro, R + o, E + o, S + o, F + o, Dg + o, bb + po, sums + po * VOLUME_ROBUST_SUMS, esum + po, s };
        coupled_form<decltype(space)::value, decltype(tm)::value, decltype(joint)::value>(now, lnk, per, g, wg, vg, t, cnt, rg, a);
    });
}

} // namespace sc
