// sc_robust.hip -- the robust call's one kernel of its own (sc_hip_robust*, sc_robust_api.cpp): k_robust_setup, k_wls_setup (sc_wls.hip) with
// the links computed from the current iterate instead of read from the caller.  One reweighting round of
//     minimise  sum w phi_q(u - d) + sum_x-links c_x phi_p(u(x+1,y) - u(x,y) - gx) + sum_y-links c_y phi_p(u(x,y+1) - u(x,y) - gy),
//     phi_r(t) = (2 / r) (t^2 + eps^2)^(r/2),
// is the WLS system with s = c rho_p(link residual), w' = w rho_q(u - d), rho_r(t) = (t^2 + eps^2)^((r-2)/2), all at the iterate U on
// the compact work plane (PcgGeo); the value of u beyond a Dirichlet line is boundary's.  The walk is k_wls_setup's: column groups of 256,
// bands of rows, a lane owns one column of its band, no LDS but the sums'; only live links, only unknowns of d, w and U are touched.
// The link to the north is the link to the south of the row above, carried in a register (computed once at the band's first row); the
// link to the west is computed again from the west neighbour's u -- by the same expression on the same operands as that neighbour's east
// link, hence with the same bits: E of the neighbour and this pixel's share of Dg agree and L stays symmetric.
// rho in float32: r = 2: 1, and the base value passes through without a multiply; r = 1: 1 / sqrt(t t + eps eps), square and sum rounded
// separately; else powf(t t + eps eps, (r - 2) / 2).
#include "sc_pcg_device.h"
#include <cmath>

namespace sc {

namespace {

// rho_r(t), and q = t t + eps eps (r = 2: t t; eps is unused there)
__device__ __forceinline__ float robust_rho(const RobustTerm &r, float t, float &q)
{
    q = rounded_product(t, t);
    if (r.mode == 0) return 1.f;
    q = q + r.eps2;
    return r.mode == 1 ? 1.0f / sqrtf(q) : powf(q, r.half_exp);
}
// one term of the energy, base phi_r(t), in double from rho's float32 values: (2 / r) q rho = (2 / r) q^(r/2)
__device__ __forceinline__ double robust_phi(const RobustTerm &r, float base, float q, float rho)
{
    return (double)base * ((double)r.scale * ((double)q * (double)rho));
}
// a link: its weight s = base rho_p(t), t = (hi - lo) - g, and its energy
struct RobustLink { float s; double e; };
__device__ __forceinline__ RobustLink robust_link(const RobustTerm &r, float base, float hi, float lo, float g)
{
    float q;
    const float t = (hi - lo) - g, rho = robust_rho(r, t, q);
    RobustLink k;
    k.s = r.mode == 0 ? base : rounded_product(base, rho);
    k.e = robust_phi(r, base, q, rho);
    return k;
}

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
            // the data term at the iterate: w' = w rho_q(u - d)
            const float wv = w[o], dv = j.d[o];
            float q;
            const float rho = robust_rho(td, uc - dv, q), wr = td.mode == 0 ? wv : rounded_product(wv, rho);
            v = screened_rhs(v, wr, dv);
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
            s_e += robust_phi(td, wv, q, rho) + ((east.e + south.e) + ((dir_w ? westl.e : 0.0) + (dir_n ? north.e : 0.0)));
            north = south;
        }
    }
    part_store(s_bb, ws[0], wg, bb);
    part_store(s_w, ws[1], wg, sums, ROBUST_SUMS, 0);
    part_store(s_l, ws[2], wg, sums, ROBUST_SUMS, 1);
    part_store(s_e, ws[3], wg, sums, ROBUST_SUMS, 2);
}

} // namespace

void launch_robust_setup(const PoissonGeo &g, const PcgGeo &wg, const PoissonJobDev *jobs, const float *const *w, const float *const *sx,
                         const float *const *sy, int m, const RobustTerm &grad, const RobustTerm &data, const float *U, float *R, float *E, float *S,
                         float *Dg, double *bb, double *sums, hipStream_t s)
{
    for_wls_tables(jobs, w, sx, sy, m, [&](const WlsJobs &t, int i0, int cnt) {
        const dim3 grid((unsigned)wg.cg, (unsigned)wg.bands, (unsigned)(g.C * cnt));
        const size_t o = (size_t)g.C * i0 * wg.stride, po = (size_t)g.C * i0 * PCG_PARTS;
        if (t.sx[0]) hipLaunchKernelGGL(k_robust_setup<true>, grid, dim3(WL), 0, s, g, wg, t, grad, data, U + o, R + o, E + o, S + o, Dg + o, bb + po, sums + po * ROBUST_SUMS);
        else hipLaunchKernelGGL(k_robust_setup<false>, grid, dim3(WL), 0, s, g, wg, t, grad, data, U + o, R + o, E + o, S + o, Dg + o, bb + po, sums + po * ROBUST_SUMS);
    });
}

} // namespace sc
