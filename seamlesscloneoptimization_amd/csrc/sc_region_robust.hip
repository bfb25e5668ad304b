// sc_region_robust.hip -- the robust region call's kernels (sc_hip_region_robust*, sc_region_robust_api.cpp: RegionRobustOperator's
// launches in a reweighting round, which RobustRounds::reweigh in sc_robust_api.cpp describes).  The system of a round of
//     minimise  sum w phi_q(u - d) + sum_live x-links c_x phi_p(dx u - gx) + sum_live y-links c_y phi_p(dy u - gy)
// over the UNKNOWN pixels of one image under region states is the region system (sc_region.hip) with s = c rho_p(link residual) on every
// link live in the region and w' = w rho_q(u - d), all at the iterate U on the compact work plane.  k_region_robust_setup is
// k_robust_setup's walk (sc_robust.hip: column groups of 256, bands of rows, a lane owns one column of its band) with k_region_setup's
// state logic (Around, state_kind) and every link computed where it is used, as k_volume_robust_setup does (sc_volume_robust.hip)
// without the time axis; behind it the two launches of the coupled forms (k_region_robust_rho, k_region_robust_setup_rho), k_robust_rho
// and k_robust_setup_rho restricted to the links live in the region.  The penalties' arithmetic, the data term (robust_data), lane_term
// and the coupled forms' helpers are sc_pcg_device.h's.
// The value of u across a link is NOT the work plane's wherever the neighbour is not UNKNOWN -- u0 = M^-1 b and z = M^-1 r fill the
// whole rectangle (sc_region.hip) --: it is data's at a KNOWN pixel, boundary's on a Dirichlet line and U's only at an UNKNOWN one.
// Both ends of a link compute its weight by one expression on the same operands -- t = (u_hi - u_lo) - g, hi / lo by the link's
// direction, then robust_link (the coupled forms: both read one rho and one c) --: the same bits, so E / S of one end and the other
// end's share of Dg agree and L stays symmetric.
// The zero condition of the region family holds after every round: R = E = S = Dg = 0 at every pixel that is not UNKNOWN, and E, S
// are 0 on a link whose other end is not UNKNOWN.
// Where no state differs from 0 the walk, the float32 expressions and the order of every lane's double sums are k_robust_setup's (and
// k_robust_rho's, k_robust_setup_rho's): the call then writes sc_hip_robust's bytes.
// What is read: the region call's elements -- a link weight and its g only where the link is live in the region, weight and (with a
// weight) data at UNKNOWN pixels, data at a KNOWN end of a live link, boundary at a Dirichlet end of one -- and U at UNKNOWN pixels.
#include "sc_region_device.h"
#include <cmath>

namespace sc {

namespace {

// NOW: no weight (w and data at UNKNOWN pixels are not read);  LNK: the call has base link arrays (false: every base link is 1).
// sums[(plane * PCG_PARTS + part) * REGION_ROBUST_SUMS + ..] = the sum of w' | of the live links s | of the UNKNOWN - KNOWN links s |
// the energy of U, in double from the float32 values as robust_phi gives it.  Every live link is counted once, under k_region_stats'
// owner rule: by its low end (the last pixel of a periodic axis owns the wrapping link) whether that end is UNKNOWN or KNOWN, and by
// its UNKNOWN end where the other lies on a low Dirichlet line.
template <bool NOW, bool LNK>
__global__ __launch_bounds__(WL) void k_region_robust_setup(PoissonGeo g, PcgGeo wg, RegionJobs t, RobustTerm tg, RobustTerm td,
                                                             const float *__restrict__ U, float *__restrict__ R, float *__restrict__ E,
                                                             float *__restrict__ S, float *__restrict__ Dg, double *__restrict__ bb,
                                                             double *__restrict__ sums)
{
    __shared__ double ws[REGION_ROBUST_SUMS + 1][4];
    lane_term(tg); lane_term(td);
    const PcgBand bd(g, wg);
    const PoissonJobDev &j = t.j[bd.member];
    const float *__restrict__ w = t.w[bd.member], *__restrict__ st = t.st[bd.member];
    const float *__restrict__ sx = LNK ? t.sx[bd.member] : nullptr, *__restrict__ sy = LNK ? t.sy[bd.member] : nullptr;
    const bool px = wg.ax == MIXED_PERIODIC, py = wg.ay == MIXED_PERIODIC;
    const int nx = wg.nx, ny = wg.ny, x = bd.x;
    const float *__restrict__ ul = U + (size_t)bd.p * wg.stride;
    // this lane's column of the four planes it writes: per-lane pointers, so that the planes' bases need no scalar registers inside the walk
    const size_t col = (size_t)bd.p * wg.stride + (size_t)(x < nx ? x : 0);
    float *__restrict__ rc = R + col, *__restrict__ ec = E + col, *__restrict__ sco = S + col, *__restrict__ dc = Dg + col;
    double s_bb = 0.0, s_w = 0.0, s_l = 0.0, s_uk = 0.0, s_e = 0.0;
    if (x < nx) {
        const int X = wg.x0 + x;
        const int xw = x > 0 ? x - 1 : nx - 1, xe = x < nx - 1 ? x + 1 : 0;      // (read only where the neighbour is UNKNOWN: then a column of the plane)
        for (int y = bd.y0; y < bd.y1; ++y) {
            const int Y = wg.y0 + y;
            const long long o = bd.pixel(g, X, Y);
            const size_t ro = (size_t)y * nx, li = ro + x;
            const int kp = state_kind(st[o]);
            float v = 0.f, e = 0.f, so = 0.f, dg = 0.f;
            if (kp != NB_NONE) {
                const bool unk = kp == NB_UNKNOWN;
                const Around a(g, wg, st, X, Y, o, px, py);
                // u at this pixel and across a link: U at an UNKNOWN pixel, data at a KNOWN one, boundary on a Dirichlet line
                auto value = [&](int k, long long off, size_t i) { return k == NB_UNKNOWN ? ul[i] : k == NB_KNOWN ? j.d[off] : j.b[off]; };
                auto live = [&](int kq) { return kq != NB_NONE && (unk || kq == NB_UNKNOWN); };
                const float uc = value(kp, o, li);
                // the links this pixel owns: east, south -- evaluated at a KNOWN low end as well, for the sums
                RobustLink east{ 0.f, 0.0 }, south{ 0.f, 0.0 }, west{ 0.f, 0.0 }, north{ 0.f, 0.0 };
                float g_e = 0.f, g_s = 0.f, g_w = 0.f, g_n = 0.f, u_e = 0.f, u_s = 0.f, u_w = 0.f, u_n = 0.f;
                if (live(a.ke)) {
                    u_e = value(a.ke, a.oe, ro + xe);
                    g_e = j.gx[o];
                    east = robust_link(tg, LNK ? sx[o] : 1.f, u_e, uc, g_e);
                    if (kp + a.ke == NB_KNOWN) s_uk += (double)east.s;
                }
                if (live(a.ks)) {
                    u_s = value(a.ks, a.os, y < ny - 1 ? li + nx : (size_t)x);
                    g_s = j.gy[o];
                    south = robust_link(tg, LNK ? sy[o] : 1.f, u_s, uc, g_s);
                    if (kp + a.ks == NB_KNOWN) s_uk += (double)south.s;
                }
                double e_d = 0.0;
                if (unk) {
                    if (a.kw != NB_NONE) {
                        u_w = value(a.kw, a.ow, ro + xw);
                        g_w = j.gx[a.ow];
                        west = robust_link(tg, LNK ? sx[a.ow] : 1.f, uc, u_w, g_w);
                    }
                    if (a.kn != NB_NONE) {
                        u_n = value(a.kn, a.on, y > 0 ? li - nx : (size_t)(ny - 1) * nx + x);
                        g_n = j.gy[a.on];
                        north = robust_link(tg, LNK ? sy[a.on] : 1.f, uc, u_n, g_n);
                    }
                    const float lw = west.s, le = east.s, ln = north.s, ls = south.s;
                    const float pa = a.ke == NB_NONE ? 0.f : rounded_product(le, g_e);
                    const float pb = a.kw == NB_NONE ? 0.f : rounded_product(lw, g_w);
                    const float pc = a.ks == NB_NONE ? 0.f : rounded_product(ls, g_s);
                    const float pd = a.kn == NB_NONE ? 0.f : rounded_product(ln, g_n);
                    v = (pa - pb) + (pc - pd);
                    float wr = 0.f;
                    if (!NOW) {
                        wr = robust_data(td, w[o], j.d[o], uc, v, e_d);
                        s_w += (double)wr;
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
                    dg = ((lw + le) + (ln + ls)) + wr;
                }
                // every live link once (k_robust_setup's expressions): by its low end; the links to a low Dirichlet line have no other owner
                const bool dw = unk && a.kw == NB_DIRICHLET, dn = unk && a.kn == NB_DIRICHLET;
                s_l += ((double)east.s + (double)south.s) + ((dw ? (double)west.s : 0.0) + (dn ? (double)north.s : 0.0));
                s_e += e_d + ((east.e + south.e) + ((dw ? west.e : 0.0) + (dn ? north.e : 0.0)));
            }
            rc[ro] = v;
            ec[ro] = e;
            sco[ro] = so;
            dc[ro] = dg;
            s_bb += (double)v * (double)v;
        }
    }
    part_store(s_bb, ws[0], wg, bb);
    part_store(s_w, ws[1], wg, sums, REGION_ROBUST_SUMS, 0);
    part_store(s_l, ws[2], wg, sums, REGION_ROBUST_SUMS, 1);
    part_store(s_uk, ws[3], wg, sums, REGION_ROBUST_SUMS, 2);
    part_store(s_e, ws[4], wg, sums, REGION_ROBUST_SUMS, 3);
}

// ---- the coupled forms (SC_ROBUST_ISOTROPIC, SC_ROBUST_JOINT_CHANNELS; sc_robust.hip: their definitions) restricted to the links live
// in the region: a dead link adds nothing to a magnitude, under JOINT a link's magnitude sums the channels in which it is live (state
// is per channel), and an owner none of whose links is live in any channel of its unit writes no rho and books no energy.
//   k_region_robust_rho        walks every pixel of the rectangle -- UNKNOWN pixels, KNOWN ones (they own their live links to UNKNOWN
//                              pixels) and, through the UNKNOWN pixel next to it, a pixel of a low Dirichlet line -- and writes rho of
//                              every owner with a live link to the rho planes ([Y][X], X < x0 + nx, Y < y0 + ny).  Per part the
//                              gradient energy, every such owner once; under JOINT the job's, booked on its channel-0 plane.
//   k_region_robust_setup_rho  k_region_robust_setup with s = c rho read at the pixel (east, south), at its west owner and at its north
//                              owner, only where that link is live in the region: then its owner wrote it.  Its energy is the data term's.
// grid: cg x bands x units; esum[(the unit's first plane * PCG_PARTS + part)] = the part's gradient energy
template <bool LNK, bool ISO, bool JOINT>
__global__ __launch_bounds__(WL) void k_region_robust_rho(PoissonGeo g, PcgGeo wg, RegionJobs t, RobustTerm tg, RhoGeo rg, const float *__restrict__ U,
                                                           float *__restrict__ Rho, double *__restrict__ esum)
{
    __shared__ double ws[4];
    lane_term(tg);
    const int unit = (int)blockIdx.z, member = JOINT ? unit : unit / g.C;
    const int k0 = JOINT ? 0 : unit - member * g.C, k1 = JOINT ? g.C : k0 + 1;
    const PoissonJobDev &j = t.j[member];
    const float *__restrict__ st = t.st[member];
    const float *__restrict__ sx = LNK ? t.sx[member] : nullptr, *__restrict__ sy = LNK ? t.sy[member] : nullptr;
    const bool px = wg.ax == MIXED_PERIODIC, py = wg.ay == MIXED_PERIODIC;
    const int nx = wg.nx, ny = wg.ny, x = (int)blockIdx.x * WL + (int)threadIdx.x;
    const int y0 = (int)blockIdx.y * wg.rows, y1 = min(y0 + wg.rows, ny);
    float *__restrict__ rx = Rho + (size_t)unit * rg.ncomp * rg.rstride, *__restrict__ ry = ISO ? rx : rx + rg.rstride;
    double s_e = 0.0;
    if (x < nx) {
        const int X = wg.x0 + x, xe = x < nx - 1 ? x + 1 : 0;
        for (int y = y0; y < y1; ++y) {
            const int Y = wg.y0 + y;
            const size_t ro = (size_t)y * nx, li = ro + x;
            // the magnitudes: this pixel's (mx: its x-link's, or under ISO both links'; my: its y-link's), the west Dirichlet pixel's
            // x-link (mw), the north Dirichlet pixel's y-link (mn) -- a Dirichlet pixel owns no other live link; has_*: live in a channel
            float mx = 0.f, my = 0.f, mw = 0.f, mn = 0.f;
            bool has_x = false, has_y = false, has_w = false, has_n = false;
            for (int k = k0; k < k1; ++k) {
                const long long o = (long long)X * g.cs + (long long)Y * g.rs + (long long)k * g.chs;
                const int kp = state_kind(st[o]);
                if (kp == NB_NONE) continue;
                const bool unk = kp == NB_UNKNOWN;
                const Around a(g, wg, st, X, Y, o, px, py);
                const float *__restrict__ ul = U + (size_t)(member * g.C + k) * wg.stride;
                auto value = [&](int kq, long long off, size_t i) { return kq == NB_UNKNOWN ? ul[i] : kq == NB_KNOWN ? j.d[off] : j.b[off]; };
                auto live = [&](int kq) { return kq != NB_NONE && (unk || kq == NB_UNKNOWN); };
                const float uc = value(kp, o, li);
                float ax = 0.f, ay = 0.f;
                if (live(a.ke)) {
                    ax = robust_sq<LNK>(sx, o, (value(a.ke, a.oe, ro + xe) - uc) - j.gx[o]);
                    has_x = true;
                }
                if (live(a.ks)) {
                    ay = robust_sq<LNK>(sy, o, (value(a.ks, a.os, y < ny - 1 ? li + nx : (size_t)x) - uc) - j.gy[o]);
                    has_y = true;
                }
                if (ISO) mx += ax + ay;
                else { mx += ax; my += ay; }
                if (unk && a.kw == NB_DIRICHLET) { mw += robust_sq<LNK>(sx, a.ow, (uc - j.b[a.ow]) - j.gx[a.ow]); has_w = true; }
                if (unk && a.kn == NB_DIRICHLET) { mn += robust_sq<LNK>(sy, a.on, (uc - j.b[a.on]) - j.gy[a.on]); has_n = true; }
            }
            const size_t i = (size_t)Y * rg.rw + X;
            double e_x = 0.0, e_y = 0.0, e_w = 0.0, e_n = 0.0;
            if (ISO ? (has_x || has_y) : has_x) rx[i] = coupled_rho(tg, mx, e_x);
            if (!ISO && has_y) ry[i] = coupled_rho(tg, my, e_y);
            if (has_w) rx[i - 1] = coupled_rho(tg, mw, e_w);              // (a low Dirichlet line: X == 1)
            if (has_n) ry[i - rg.rw] = coupled_rho(tg, mn, e_n);          // (Y == 1)
            s_e += (e_x + e_y) + (e_w + e_n);
        }
    }
    s_e = block_sum(s_e, ws);
    if (threadIdx.x == 0) esum[(size_t)(JOINT ? unit * g.C : unit) * PCG_PARTS + blockIdx.y * wg.cg + blockIdx.x] = s_e;
}

// k_region_robust_setup (its walk, its order, its sums) with the links' rho read from the rho planes; field 3 of the sums: the data term's energy
template <bool NOW, bool LNK, bool ISO, bool JOINT>
__global__ __launch_bounds__(WL) void k_region_robust_setup_rho(PoissonGeo g, PcgGeo wg, RegionJobs t, RobustTerm td, RhoGeo rg,
                                                                 const float *__restrict__ Rho, const float *__restrict__ U, float *__restrict__ R,
                                                                 float *__restrict__ E, float *__restrict__ S, float *__restrict__ Dg,
                                                                 double *__restrict__ bb, double *__restrict__ sums)
{
    __shared__ double ws[REGION_ROBUST_SUMS + 1][4];
    lane_term(td);
    const PcgBand bd(g, wg);
    const PoissonJobDev &j = t.j[bd.member];
    const float *__restrict__ w = t.w[bd.member], *__restrict__ st = t.st[bd.member];
    const float *__restrict__ sx = LNK ? t.sx[bd.member] : nullptr, *__restrict__ sy = LNK ? t.sy[bd.member] : nullptr;
    const bool px = wg.ax == MIXED_PERIODIC, py = wg.ay == MIXED_PERIODIC;
    const int nx = wg.nx, x = bd.x;
    const float *__restrict__ ul = U + (size_t)bd.p * wg.stride;
    const float *__restrict__ rx = Rho + (size_t)(JOINT ? bd.member : bd.p) * rg.ncomp * rg.rstride, *__restrict__ ry = ISO ? rx : rx + rg.rstride;
    const size_t col = (size_t)bd.p * wg.stride + (size_t)(x < nx ? x : 0);
    float *__restrict__ rc = R + col, *__restrict__ ec = E + col, *__restrict__ sco = S + col, *__restrict__ dc = Dg + col;
    double s_bb = 0.0, s_w = 0.0, s_l = 0.0, s_uk = 0.0, s_e = 0.0;
    if (x < nx) {
        const int X = wg.x0 + x;
        const int Xw = X > 0 ? X - 1 : g.W - 1;                                     // the owner of the west link
        for (int y = bd.y0; y < bd.y1; ++y) {
            const int Y = wg.y0 + y;
            const long long o = bd.pixel(g, X, Y);
            const size_t ro = (size_t)y * nx, li = ro + x, rr = (size_t)Y * rg.rw;
            const int kp = state_kind(st[o]);
            float v = 0.f, e = 0.f, so = 0.f, dg = 0.f;
            if (kp != NB_NONE) {
                const bool unk = kp == NB_UNKNOWN;
                const Around a(g, wg, st, X, Y, o, px, py);
                auto live = [&](int kq) { return kq != NB_NONE && (unk || kq == NB_UNKNOWN); };
                float le = 0.f, ls = 0.f, lw = 0.f, ln = 0.f;
                if (live(a.ke)) {
                    le = LNK ? rounded_product(sx[o], rx[rr + X]) : rx[rr + X];
                    if (kp + a.ke == NB_KNOWN) s_uk += (double)le;
                }
                if (live(a.ks)) {
                    ls = LNK ? rounded_product(sy[o], ry[rr + X]) : ry[rr + X];
                    if (kp + a.ks == NB_KNOWN) s_uk += (double)ls;
                }
                double e_d = 0.0;
                if (unk) {
                    const float uc = ul[li];
                    if (a.kw != NB_NONE) lw = LNK ? rounded_product(sx[a.ow], rx[rr + Xw]) : rx[rr + Xw];
                    if (a.kn != NB_NONE) {
                        const size_t rn = (size_t)(Y > 0 ? Y - 1 : g.H - 1) * rg.rw + X;
                        ln = LNK ? rounded_product(sy[a.on], ry[rn]) : ry[rn];
                    }
                    const float pa = a.ke == NB_NONE ? 0.f : rounded_product(le, j.gx[o]);
                    const float pb = a.kw == NB_NONE ? 0.f : rounded_product(lw, j.gx[a.ow]);
                    const float pc = a.ks == NB_NONE ? 0.f : rounded_product(ls, j.gy[o]);
                    const float pd = a.kn == NB_NONE ? 0.f : rounded_product(ln, j.gy[a.on]);
                    v = (pa - pb) + (pc - pd);
                    float wr = 0.f;
                    if (!NOW) {
                        wr = robust_data(td, w[o], j.d[o], uc, v, e_d);
                        s_w += (double)wr;
                    }
                    if (a.kw == NB_DIRICHLET) v -= rounded_product(lw, j.b[a.ow]);
                    if (a.kn == NB_DIRICHLET) v -= rounded_product(ln, j.b[a.on]);
                    if (a.ke == NB_DIRICHLET) v -= rounded_product(le, j.b[a.oe]);
                    if (a.ks == NB_DIRICHLET) v -= rounded_product(ls, j.b[a.os]);
                    if (a.kw == NB_KNOWN) v -= rounded_product(lw, j.d[a.ow]);
                    if (a.kn == NB_KNOWN) v -= rounded_product(ln, j.d[a.on]);
                    if (a.ke == NB_KNOWN) v -= rounded_product(le, j.d[a.oe]);
                    if (a.ks == NB_KNOWN) v -= rounded_product(ls, j.d[a.os]);
                    e = a.ke == NB_UNKNOWN ? le : 0.f;
                    so = a.ks == NB_UNKNOWN ? ls : 0.f;
                    dg = ((lw + le) + (ln + ls)) + wr;
                }
                const bool dw = unk && a.kw == NB_DIRICHLET, dn = unk && a.kn == NB_DIRICHLET;
                s_l += ((double)le + (double)ls) + ((dw ? (double)lw : 0.0) + (dn ? (double)ln : 0.0));
                s_e += e_d;
            }
            rc[ro] = v;
            ec[ro] = e;
            sco[ro] = so;
            dc[ro] = dg;
            s_bb += (double)v * (double)v;
        }
    }
    part_store(s_bb, ws[0], wg, bb);
    part_store(s_w, ws[1], wg, sums, REGION_ROBUST_SUMS, 0);
    part_store(s_l, ws[2], wg, sums, REGION_ROBUST_SUMS, 1);
    part_store(s_uk, ws[3], wg, sums, REGION_ROBUST_SUMS, 2);
    part_store(s_e, ws[4], wg, sums, REGION_ROBUST_SUMS, 3);
}

template <bool NOW, bool LNK, bool ISO, bool JOINT>
void coupled_launches(const PoissonGeo &g, const PcgGeo &wg, const RegionJobs &t, int cnt, const RobustTerm &grad, const RobustTerm &data,
                      const RhoGeo &rg, const float *U, float *Rho, float *R, float *E, float *S, float *Dg, double *bb, double *sums, double *esum,
                      hipStream_t s)
{
    const unsigned planes = (unsigned)(g.C * cnt);
    hipLaunchKernelGGL((k_region_robust_rho<LNK, ISO, JOINT>), dim3((unsigned)wg.cg, (unsigned)wg.bands, JOINT ? (unsigned)cnt : planes), dim3(WL), 0, s,
                       g, wg, t, grad, rg, U, Rho, esum);
    hipLaunchKernelGGL((k_region_robust_setup_rho<NOW, LNK, ISO, JOINT>), dim3((unsigned)wg.cg, (unsigned)wg.bands, planes), dim3(WL), 0, s, g, wg, t,
                       data, rg, Rho, U, R, E, S, Dg, bb, sums);
}

} // namespace

void launch_region_robust_coupled(const PoissonGeo &g, const PcgGeo &wg, const PoissonJobDev *jobs, const SideArrays *sides, int m,
                                  const RobustTerm &grad, const RobustTerm &data, int coupling, const float *U, float *Rho, float *R, float *E,
                                  float *S, float *Dg, double *bb, double *sums, double *esum, hipStream_t s)
{
    for_coupled_tables<RegionJobs>(g, wg, jobs, sides, m, coupling, [&](auto iso, auto joint, const RegionJobs &t, int cnt, const RhoGeo &rg, size_t o, size_t po, size_t ro) {
        constexpr bool ISO = decltype(iso)::value, JOINT = decltype(joint)::value;
        const bool lnk = t.sx[0] != nullptr;
        auto go = !t.w[0] ? (lnk ? coupled_launches<true, true, ISO, JOINT> : coupled_launches<true, false, ISO, JOINT>)
                          : (lnk ? coupled_launches<false, true, ISO, JOINT> : coupled_launches<false, false, ISO, JOINT>);
        go(g, wg, t, cnt, grad, data, rg, U + o, Rho + ro, R + o, E + o, S + o, Dg + o, bb + po, sums + po * REGION_ROBUST_SUMS, esum + po, s);
    });
}

void launch_region_robust_setup(const PoissonGeo &g, const PcgGeo &wg, const PoissonJobDev *jobs, const SideArrays *sides, int m,
                                const RobustTerm &grad, const RobustTerm &data, const float *U, float *R, float *E, float *S, float *Dg,
                                double *bb, double *sums, hipStream_t s)
{
    for_side_tables<RegionJobs>(jobs, sides, m, [&](const RegionJobs &t, int i0, int cnt) {
        const dim3 grid((unsigned)wg.cg, (unsigned)wg.bands, (unsigned)(g.C * cnt));
        const size_t o = (size_t)g.C * i0 * wg.stride, po = (size_t)g.C * i0 * PCG_PARTS;
        const bool now = !t.w[0], lnk = t.sx[0] != nullptr;
        double *b = bb + po, *sm = sums + po * REGION_ROBUST_SUMS;
#define SC_FORM(N, L) hipLaunchKernelGGL((k_region_robust_setup<N, L>), grid, dim3(WL), 0, s, g, wg, t, grad, data, U + o, R + o, E + o, S + o, Dg + o, b, sm)
        if (now) { if (lnk) SC_FORM(true, true); else SC_FORM(true, false); }
        else { if (lnk) SC_FORM(false, true); else SC_FORM(false, false); }
#undef SC_FORM
    });
}

} // namespace sc
