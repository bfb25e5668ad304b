// sc_robust.hip -- the robust call's kernels of its own (sc_hip_robust*, sc_robust_api.cpp: RobustOperator's launches in a reweighting
// round, which RobustRounds::reweigh there describes): k_robust_setup, k_wls_setup (sc_wls.hip) with the links computed from the
// current iterate instead of read from the caller, and behind it the two launches of the coupled forms (isotropic, joint channels:
// k_robust_rho, k_robust_setup_rho).  The system of a round of
//     minimise  sum w phi_q(u - d) + sum_x-links c_x phi_p(u(x+1,y) - u(x,y) - gx) + sum_y-links c_y phi_p(u(x,y+1) - u(x,y) - gy),
//     phi_r(t) = (2 / r) (t^2 + eps^2)^(r/2),
// is the WLS system with s = c rho_p(link residual), w' = w rho_q(u - d), rho_r(t) = (t^2 + eps^2)^((r-2)/2), all at the iterate U on
// the compact work plane (PcgGeo); the value of u beyond a Dirichlet line is boundary's.  The walk is k_wls_setup's: column groups of 256,
// bands of rows, a lane owns one column of its band, no LDS but the sums'; only live links, only unknowns of d, w and U are touched.
// The link to the north is the link to the south of the row above, carried in a register (computed once at the band's first row); the
// link to the west is computed again from the west neighbour's u -- by the same expression on the same operands as that neighbour's east
// link, hence with the same bits: E of the neighbour and this pixel's share of Dg agree and L stays symmetric.
// rho in float32 (sc_pcg_device.h: robust_rho, robust_link, robust_data): r = 2: 1, and the base value passes through without a
// multiply; r = 1: 1 / sqrt(t t + eps eps), square and sum rounded separately; else powf(t t + eps eps, (r - 2) / 2).
#include "sc_pcg_device.h"
#include <cmath>

namespace sc {

namespace {

// BASE: the caller's base links c (t.sx, t.sy); false: all 1
template <bool BASE>
__global__ __launch_bounds__(WL) void k_robust_setup(PoissonGeo g, PcgGeo wg, WlsJobs t, RobustTerm tg, RobustTerm td, const float *__restrict__ U,
                                                      float *__restrict__ R, float *__restrict__ E, float *__restrict__ S, float *__restrict__ Dg,
                                                      double *__restrict__ bb, double *__restrict__ sums)
{
    __shared__ double ws[4][4];
    const PcgBand bd(g, wg);
    const PoissonJobDev &j = t.j[bd.member];
    const float *__restrict__ w = t.w[bd.member], *__restrict__ sx = t.sx[bd.member], *__restrict__ sy = t.sy[bd.member];
    const bool px = wg.ax == MIXED_PERIODIC, py = wg.ay == MIXED_PERIODIC;
    const int nx = wg.nx, ny = wg.ny, x = bd.x;
    const float *__restrict__ ul = U + (size_t)bd.p * wg.stride;
    double s_bb = 0.0, s_w = 0.0, s_l = 0.0, s_e = 0.0;
    if (x < nx) {
        const int X = wg.x0 + x;
        const bool has_e = X < g.W - 1 || px, has_w = X > 0 || px;
        const bool dir_w = X == 1 && mixed_low_d(wg.ax), dir_e = X == g.W - 2 && mixed_high_d(wg.ax);
        const long long west = X > 0 ? -g.cs : (long long)(g.W - 1) * g.cs;        // from a pixel to the element of its west link
        RobustLink north{ 0.f, 0.0 };
        for (int y = bd.y0; y < bd.y1; ++y) {
            const int Y = wg.y0 + y;
            const long long o = bd.pixel(g, X, Y);
            const size_t ro = (size_t)y * nx;
            const bool has_s = Y < g.H - 1 || py, has_n = Y > 0 || py;
            const bool dir_n = Y == 1 && mixed_low_d(wg.ay), dir_s = Y == g.H - 2 && mixed_high_d(wg.ay);
            const float uc = ul[ro + x];
            RobustLink east{ 0.f, 0.0 }, westl{ 0.f, 0.0 }, south{ 0.f, 0.0 };
            float a = 0.f, b = 0.f, cc = 0.f, d = 0.f, b_e = 0.f, b_w = 0.f, b_n = 0.f, b_s = 0.f;
            if (has_e) {
                if (dir_e) b_e = j.b[o + g.cs];
                const float ue = dir_e ? b_e : ul[ro + (x < nx - 1 ? x + 1 : 0)], gv = j.gx[o];
                east = robust_link(tg, BASE ? sx[o] : 1.f, ue, uc, gv);
                a = rounded_product(east.s, gv);
            }
            if (has_w) {
                if (dir_w) b_w = j.b[o - g.cs];
                const float uw = dir_w ? b_w : ul[ro + (x > 0 ? x - 1 : nx - 1)], gv = j.gx[o + west];
                westl = robust_link(tg, BASE ? sx[o + west] : 1.f, uc, uw, gv);
                b = rounded_product(westl.s, gv);
            }
            if (has_s) {
                if (dir_s) b_s = j.b[o + g.rs];
                const float us = dir_s ? b_s : ul[(size_t)(y < ny - 1 ? y + 1 : 0) * nx + x], gv = j.gy[o];
                south = robust_link(tg, BASE ? sy[o] : 1.f, us, uc, gv);
                cc = rounded_product(south.s, gv);
            }
            if (has_n) {
                const long long on = Y > 0 ? o - g.rs : o + (long long)(g.H - 1) * g.rs;
                const float gv = j.gy[on];
                if (dir_n) b_n = j.b[o - g.rs];
                if (y == bd.y0) {
                    const float un = dir_n ? b_n : ul[(size_t)(y > 0 ? y - 1 : ny - 1) * nx + x];
                    north = robust_link(tg, BASE ? sy[on] : 1.f, uc, un, gv);
                }
                d = rounded_product(north.s, gv);
            } else north = RobustLink{ 0.f, 0.0 };
            float v = (a - b) + (cc - d);
            double e_d;
            const float wr = robust_data(td, w[o], j.d[o], uc, v, e_d);
            if (dir_w) v -= rounded_product(westl.s, b_w);
            if (dir_n) v -= rounded_product(north.s, b_n);
            if (dir_e) v -= rounded_product(east.s, b_e);
            if (dir_s) v -= rounded_product(south.s, b_s);
            const size_t i = (size_t)bd.p * wg.stride + ro + x;
            R[i] = v;
            E[i] = (x < nx - 1 || px) ? east.s : 0.f;
            S[i] = (y < ny - 1 || py) ? south.s : 0.f;
            Dg[i] = ((westl.s + east.s) + (north.s + south.s)) + wr;
            s_bb += (double)v * (double)v;
            s_w += (double)wr;
            // every live link once, as k_wls_stats counts them: by its low end, a link to a Dirichlet pixel by its unknown end
            s_l += ((double)east.s + (double)south.s) + ((dir_w ? (double)westl.s : 0.0) + (dir_n ? (double)north.s : 0.0));
            s_e += e_d + ((east.e + south.e) + ((dir_w ? westl.e : 0.0) + (dir_n ? north.e : 0.0)));
            north = south;
        }
    }
    part_store(s_bb, ws[0], wg, bb);
    part_store(s_w, ws[1], wg, sums, ROBUST_SUMS, 0);
    part_store(s_l, ws[2], wg, sums, ROBUST_SUMS, 1);
    part_store(s_e, ws[3], wg, sums, ROBUST_SUMS, 2);
}

// ---- the coupled forms (SC_ROBUST_ISOTROPIC, SC_ROBUST_JOINT_CHANNELS): one penalty psi_p(M) = (2 / p) (M + eps^2)^(p/2) over the
// magnitude M that several links share -- a = c t^2 of a pixel's two forward links (ISO), of all channels of a job (JOINT), or both.
// Every link of a magnitude gets s = c rho_p(M), rho_p(M) = (M + eps^2)^((p-2)/2).  A link's owner is its low end, so a lane needs
// magnitudes its west and north neighbours own, under JOINT every channel of them: two launches per round instead of recomputing them.
//   k_robust_rho        walks the owners -- the unknowns, and through the unknown next to it a pixel of a low-side Dirichlet line --
//                       and writes rho to the rho planes, which are addressed by pixel: [Y][X], X < x0 + nx, Y < y0 + ny.  One plane
//                       per unit (ISO) or two, the x-links' and the y-links' (not ISO); a unit is a job (JOINT) or a plane.  Per part
//                       the gradient energy, every owner once; under JOINT it is the job's, booked on its channel-0 plane.
//   k_robust_setup_rho  k_robust_setup with s = c rho read at the pixel, its west and its north neighbour; its energy is the data term's.
// float32: t t rounded, times c rounded (no base links: no multiply), a_x + a_y within a pixel, then the running sum over the channels
// 0 .. C - 1, Q = M + eps eps, rho = 1 / sqrtf(Q) (p = 1) or powf(Q, (p - 2) / 2), s = c rho rounded.  Both ends of a link read the same
// rho and the same c: the same bits, L stays symmetric.  p = 2 never comes here (RobustRounds::coupling: the bits change nothing then).
// RhoGeo, robust_sq, coupled_rho and the side tables' offsets (for_coupled_tables) are sc_pcg_device.h's: the region call's forms use them too.
// grid: cg x bands x units; esum[(the unit's first plane * PCG_PARTS + part)] = the part's gradient energy
template <bool BASE, bool ISO, bool JOINT>
__global__ __launch_bounds__(WL) void k_robust_rho(PoissonGeo g, PcgGeo wg, WlsJobs t, RobustTerm tg, RhoGeo rg, const float *__restrict__ U,
                                                    float *__restrict__ Rho, double *__restrict__ esum)
{
    __shared__ double ws[4];
    const int unit = (int)blockIdx.z, member = JOINT ? unit : unit / g.C;
    const int k0 = JOINT ? 0 : unit - member * g.C, k1 = JOINT ? g.C : k0 + 1;
    const PoissonJobDev &j = t.j[member];
    const float *__restrict__ sx = t.sx[member], *__restrict__ sy = t.sy[member];
    const bool px = wg.ax == MIXED_PERIODIC, py = wg.ay == MIXED_PERIODIC;
    const int nx = wg.nx, ny = wg.ny, x = (int)blockIdx.x * WL + (int)threadIdx.x;
    const int y0 = (int)blockIdx.y * wg.rows, y1 = min(y0 + wg.rows, ny);
    float *__restrict__ rx = Rho + (size_t)unit * rg.ncomp * rg.rstride, *__restrict__ ry = ISO ? rx : rx + rg.rstride;
    double s_e = 0.0;
    if (x < nx) {
        const int X = wg.x0 + x;
        const bool has_e = X < g.W - 1 || px;
        const bool dir_w = X == 1 && mixed_low_d(wg.ax), dir_e = X == g.W - 2 && mixed_high_d(wg.ax);
        for (int y = y0; y < y1; ++y) {
            const int Y = wg.y0 + y;
            const size_t ro = (size_t)y * nx;
            const bool has_s = Y < g.H - 1 || py;
            const bool dir_n = Y == 1 && mixed_low_d(wg.ay), dir_s = Y == g.H - 2 && mixed_high_d(wg.ay);
            // the magnitudes: this pixel's (mx: its x-link's, or under ISO both links'; my: its y-link's), the west Dirichlet pixel's
            // x-link (mw), the north Dirichlet pixel's y-link (mn) -- a Dirichlet pixel owns no other live link
            float mx = 0.f, my = 0.f, mw = 0.f, mn = 0.f;
            for (int k = k0; k < k1; ++k) {
                const long long o = (long long)X * g.cs + (long long)Y * g.rs + (long long)k * g.chs;
                const float *__restrict__ ul = U + (size_t)(member * g.C + k) * wg.stride;
                const float uc = ul[ro + x];
                float ax = 0.f, ay = 0.f;
                if (has_e) {
                    const float ue = dir_e ? j.b[o + g.cs] : ul[ro + (x < nx - 1 ? x + 1 : 0)];
                    ax = robust_sq<BASE>(sx, o, (ue - uc) - j.gx[o]);
                }
                if (has_s) {
                    const float us = dir_s ? j.b[o + g.rs] : ul[(size_t)(y < ny - 1 ? y + 1 : 0) * nx + x];
                    ay = robust_sq<BASE>(sy, o, (us - uc) - j.gy[o]);
                }
                if (ISO) mx += ax + ay;
                else { mx += ax; my += ay; }
                if (dir_w) mw += robust_sq<BASE>(sx, o - g.cs, (uc - j.b[o - g.cs]) - j.gx[o - g.cs]);
                if (dir_n) mn += robust_sq<BASE>(sy, o - g.rs, (uc - j.b[o - g.rs]) - j.gy[o - g.rs]);
            }
            const size_t i = (size_t)Y * rg.rw + X;
            double e_x = 0.0, e_y = 0.0, e_w = 0.0, e_n = 0.0;
            if (ISO ? (has_e || has_s) : has_e) rx[i] = coupled_rho(tg, mx, e_x);
            if (!ISO && has_s) ry[i] = coupled_rho(tg, my, e_y);
            if (dir_w) rx[i - 1] = coupled_rho(tg, mw, e_w);
            if (dir_n) ry[i - rg.rw] = coupled_rho(tg, mn, e_n);
            s_e += (e_x + e_y) + (e_w + e_n);
        }
    }
    s_e = block_sum(s_e, ws);
    if (threadIdx.x == 0) esum[(size_t)(JOINT ? unit * g.C : unit) * PCG_PARTS + blockIdx.y * wg.cg + blockIdx.x] = s_e;
}

// k_robust_setup (its walk, its order, its sums) with the links' rho read from the rho planes; field 2 of the sums: the data term's energy
template <bool BASE, bool ISO, bool JOINT>
__global__ __launch_bounds__(WL) void k_robust_setup_rho(PoissonGeo g, PcgGeo wg, WlsJobs t, RobustTerm td, RhoGeo rg, const float *__restrict__ Rho,
                                                          const float *__restrict__ U, float *__restrict__ R, float *__restrict__ E,
                                                          float *__restrict__ S, float *__restrict__ Dg, double *__restrict__ bb,
                                                          double *__restrict__ sums)
{
    __shared__ double ws[4][4];
    const PcgBand bd(g, wg);
    const PoissonJobDev &j = t.j[bd.member];
    const float *__restrict__ w = t.w[bd.member], *__restrict__ sx = t.sx[bd.member], *__restrict__ sy = t.sy[bd.member];
    const bool px = wg.ax == MIXED_PERIODIC, py = wg.ay == MIXED_PERIODIC;
    const int nx = wg.nx, ny = wg.ny, x = bd.x;
    const float *__restrict__ ul = U + (size_t)bd.p * wg.stride;
    const float *__restrict__ rx = Rho + (size_t)(JOINT ? bd.member : bd.p) * rg.ncomp * rg.rstride, *__restrict__ ry = ISO ? rx : rx + rg.rstride;
    double s_bb = 0.0, s_w = 0.0, s_l = 0.0, s_e = 0.0;
    if (x < nx) {
        const int X = wg.x0 + x;
        const bool has_e = X < g.W - 1 || px, has_w = X > 0 || px;
        const bool dir_w = X == 1 && mixed_low_d(wg.ax), dir_e = X == g.W - 2 && mixed_high_d(wg.ax);
        const long long west = X > 0 ? -g.cs : (long long)(g.W - 1) * g.cs;        // from a pixel to the element of its west link
        const int Xw = X > 0 ? X - 1 : g.W - 1;                                     // the owner of the west link
        float north = 0.f;
        for (int y = bd.y0; y < bd.y1; ++y) {
            const int Y = wg.y0 + y;
            const long long o = bd.pixel(g, X, Y);
            const size_t ro = (size_t)y * nx, rr = (size_t)Y * rg.rw;
            const bool has_s = Y < g.H - 1 || py, has_n = Y > 0 || py;
            const bool dir_n = Y == 1 && mixed_low_d(wg.ay), dir_s = Y == g.H - 2 && mixed_high_d(wg.ay);
            const float uc = ul[ro + x];
            float east = 0.f, westl = 0.f, south = 0.f;
            float a = 0.f, b = 0.f, cc = 0.f, d = 0.f, b_e = 0.f, b_w = 0.f, b_n = 0.f, b_s = 0.f;
            if (has_e) {
                if (dir_e) b_e = j.b[o + g.cs];
                east = BASE ? rounded_product(sx[o], rx[rr + X]) : rx[rr + X];
                a = rounded_product(east, j.gx[o]);
            }
            if (has_w) {
                if (dir_w) b_w = j.b[o - g.cs];
                westl = BASE ? rounded_product(sx[o + west], rx[rr + Xw]) : rx[rr + Xw];
                b = rounded_product(westl, j.gx[o + west]);
            }
            if (has_s) {
                if (dir_s) b_s = j.b[o + g.rs];
                south = BASE ? rounded_product(sy[o], ry[rr + X]) : ry[rr + X];
                cc = rounded_product(south, j.gy[o]);
            }
            if (has_n) {
                const long long on = Y > 0 ? o - g.rs : o + (long long)(g.H - 1) * g.rs;
                if (dir_n) b_n = j.b[o - g.rs];
                if (y == bd.y0) {
                    const size_t rn = (size_t)(Y > 0 ? Y - 1 : g.H - 1) * rg.rw + X;
                    north = BASE ? rounded_product(sy[on], ry[rn]) : ry[rn];
                }
                d = rounded_product(north, j.gy[on]);
            } else north = 0.f;
            float v = (a - b) + (cc - d);
            double e_d;
            const float wr = robust_data(td, w[o], j.d[o], uc, v, e_d);
            if (dir_w) v -= rounded_product(westl, b_w);
            if (dir_n) v -= rounded_product(north, b_n);
            if (dir_e) v -= rounded_product(east, b_e);
            if (dir_s) v -= rounded_product(south, b_s);
            const size_t i = (size_t)bd.p * wg.stride + ro + x;
            R[i] = v;
            E[i] = (x < nx - 1 || px) ? east : 0.f;
            S[i] = (y < ny - 1 || py) ? south : 0.f;
            Dg[i] = ((westl + east) + (north + south)) + wr;
            s_bb += (double)v * (double)v;
            s_w += (double)wr;
            s_l += ((double)east + (double)south) + ((dir_w ? (double)westl : 0.0) + (dir_n ? (double)north : 0.0));
            s_e += e_d;
            north = south;
        }
    }
    part_store(s_bb, ws[0], wg, bb);
    part_store(s_w, ws[1], wg, sums, ROBUST_SUMS, 0);
    part_store(s_l, ws[2], wg, sums, ROBUST_SUMS, 1);
    part_store(s_e, ws[3], wg, sums, ROBUST_SUMS, 2);
}

template <bool BASE, bool ISO, bool JOINT>
void coupled_launches(const PoissonGeo &g, const PcgGeo &wg, const WlsJobs &t, int cnt, const RobustTerm &grad, const RobustTerm &data,
                      const RhoGeo &rg, const float *U, float *Rho, float *R, float *E, float *S, float *Dg, double *bb, double *sums, double *esum,
                      hipStream_t s)
{
    const unsigned planes = (unsigned)(g.C * cnt);
    hipLaunchKernelGGL((k_robust_rho<BASE, ISO, JOINT>), dim3((unsigned)wg.cg, (unsigned)wg.bands, JOINT ? (unsigned)cnt : planes), dim3(WL), 0, s, g, wg,
                       t, grad, rg, U, Rho, esum);
    hipLaunchKernelGGL((k_robust_setup_rho<BASE, ISO, JOINT>), dim3((unsigned)wg.cg, (unsigned)wg.bands, planes), dim3(WL), 0, s, g, wg, t, data, rg,
                       Rho, U, R, E, S, Dg, bb, sums);
}

} // namespace

void launch_robust_coupled(const PoissonGeo &g, const PcgGeo &wg, const PoissonJobDev *jobs, const SideArrays *sides, int m, const RobustTerm &grad, const RobustTerm &data, int coupling, const float *U, float *Rho,
                           float *R, float *E, float *S, float *Dg, double *bb, double *sums, double *esum, hipStream_t s)
{
    for_coupled_tables<WlsJobs>(g, wg, jobs, sides, m, coupling, [&](auto iso, auto joint, const WlsJobs &t, int cnt, const RhoGeo &rg, size_t o, size_t po, size_t ro) {
        constexpr bool ISO = decltype(iso)::value, JOINT = decltype(joint)::value;
        auto go = t.sx[0] ? coupled_launches<true, ISO, JOINT> : coupled_launches<false, ISO, JOINT>;
        go(g, wg, t, cnt, grad, data, rg, U + o, Rho + ro, R + o, E + o, S + o, Dg + o, bb + po, sums + po * ROBUST_SUMS, esum + po, s);
    });
}

void launch_robust_setup(const PoissonGeo &g, const PcgGeo &wg, const PoissonJobDev *jobs, const SideArrays *sides, int m, const RobustTerm &grad, const RobustTerm &data, const float *U, float *R, float *E, float *S,
                         float *Dg, double *bb, double *sums, hipStream_t s)
{
    for_side_tables<WlsJobs>(jobs, sides, m, [&](const WlsJobs &t, int i0, int cnt) {
        const dim3 grid((unsigned)wg.cg, (unsigned)wg.bands, (unsigned)(g.C * cnt));
        const size_t o = (size_t)g.C * i0 * wg.stride, po = (size_t)g.C * i0 * PCG_PARTS;
        if (t.sx[0]) hipLaunchKernelGGL(k_robust_setup<true>, grid, dim3(WL), 0, s, g, wg, t, grad, data, U + o, R + o, E + o, S + o, Dg + o, bb + po, sums + po * ROBUST_SUMS);
        else hipLaunchKernelGGL(k_robust_setup<false>, grid, dim3(WL), 0, s, g, wg, t, grad, data, U + o, R + o, E + o, S + o, Dg + o, bb + po, sums + po * ROBUST_SUMS);
    });
}

} // namespace sc
