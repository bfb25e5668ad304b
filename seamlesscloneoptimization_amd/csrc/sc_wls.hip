// sc_wls.hip -- the WLS family's kernels (sc_hip_wls*, sc_wls_api.cpp) under the shared conjugate gradients (sc_pcg.h): statistics, set-up and
// the operator's coefficients for
//     L u = b,     (L u)(p) = sum_q s(p, q) (u(q) - u(p)) - w(p) u(p),     s > 0 the weight of the link p - q,  w >= 0,
// on the compact float32 work planes (PcgGeo; only unknowns, homogeneous Dirichlet lines).  The links of a job come
// as two arrays under the call's layout: sx(x, y) joins (x, y) and (x + 1, y), sy(x, y) joins (x, y) and (x, y + 1); along a periodic
// axis the last column / row holds the link from the last pixel to the first (dct_rhs's convention for gx, gy).  A link is live when at
// least one of its ends is an unknown; no other element of sx, sy is ever read.  Seen from an unknown at pixel (X, Y) its four links are
//     east  sx(X, Y)      where X < W - 1 or the axis wraps           west   sx(X - 1, Y)   where X > 0, sx(W - 1, Y) where X = 0 wraps
//     south sy(X, Y)      where Y < H - 1 or the axis wraps           north  sy(X, Y - 1)   where Y > 0, sy(X, H - 1) where Y = 0 wraps
// -- the neighbour beyond is an unknown or lies on a Dirichlet line, never outside the image -- and 0 (not read) otherwise.
// Set-up folds the caller's arrays into three coefficient planes (w gets none of its own: the operator uses it inside Dg only): E, the
// link to the next unknown column (0 where there is none: a Dirichlet line or a free end follows), S, the link to the next unknown
// row, and Dg, the diagonal: all four incident links, those to Dirichlet pixels included, plus w.  The operator launch is
// sc_pcg_device.h's walk (k_pcg_op) with WlsCoef as its policy: five plane transfers for the weighted operator's three (p, E, S, Dg in,
// q out): the west link is the left neighbour's E, read like the left neighbour's p from the cache lines the wave loads anyway (across
// the 256-column group boundary too), the north link the S of the row above, carried in a register.
#include "sc_pcg_device.h"
#include <cmath>

namespace sc {

namespace {

// the four incident links of the unknown at pixel (X, Y), offset o, of one channel: 0 where there is none (then nothing is read)
struct Links { float west, east, north, south; };
template <bool ONE = false>
__device__ __forceinline__ Links links_at(const PoissonGeo &g, const float *__restrict__ sx, const float *__restrict__ sy, int X, int Y, long long o,
                                          bool px, bool py)
{
    Links k;
    if (ONE) {          // every link that exists is 1: nothing is read
        k.east = (X < g.W - 1 || px) ? 1.f : 0.f;
        k.west = (X > 0 || px) ? 1.f : 0.f;
        k.south = (Y < g.H - 1 || py) ? 1.f : 0.f;
        k.north = (Y > 0 || py) ? 1.f : 0.f;
        return k;
    }
    k.east = (X < g.W - 1 || px) ? sx[o] : 0.f;
    k.west = X > 0 ? sx[o - g.cs] : px ? sx[o + (long long)(g.W - 1) * g.cs] : 0.f;
    k.south = (Y < g.H - 1 || py) ? sy[o] : 0.f;
    k.north = Y > 0 ? sy[o - g.rs] : py ? sy[o + (long long)(g.H - 1) * g.rs] : 0.f;
    return k;
}

__device__ __forceinline__ bool bad_link(float v) { return !(v > 0.f) || v > 3.4028234e38f; }

// Every live link is counted once: by its low end where both ends are unknowns (the last pixel of a periodic axis owns the wrapping
// link), by its unknown end where the other lies on a Dirichlet line.
__global__ __launch_bounds__(WL) void k_wls_stats(PoissonGeo g, PcgGeo wg, WlsJobs t, double *__restrict__ stats)
{
    __shared__ double ws[4][4];
    const PcgBand b(g, wg);
    const float *__restrict__ w = t.w[b.member], *__restrict__ sx = t.sx[b.member], *__restrict__ sy = t.sy[b.member];
    const bool px = wg.ax == MIXED_PERIODIC, py = wg.ay == MIXED_PERIODIC;
    double sw = 0.0, bw = 0.0, ss = 0.0, bs = 0.0;
    if (b.x < wg.nx)
        for (int y = b.y0; y < b.y1; ++y) {
            const int X = wg.x0 + b.x, Y = wg.y0 + y;
            const long long o = b.pixel(g, X, Y);
            const float v = w[o];
            if (!(v >= 0.f) || v > 3.4028234e38f) bw += 1.0;
            sw += (double)v;
            auto link = [&](float s) { if (bad_link(s)) bs += 1.0; ss += (double)s; };
            if (X < g.W - 1 || px) link(sx[o]);
            if (Y < g.H - 1 || py) link(sy[o]);
            if (X == 1 && mixed_low_d(wg.ax)) link(sx[o - g.cs]);
            if (Y == 1 && mixed_low_d(wg.ay)) link(sy[o - g.rs]);
        }
    part_store(sw, ws[0], wg, stats, WLS_STATS, 0);
    part_store(bw, ws[1], wg, stats, WLS_STATS, 1);
    part_store(ss, ws[2], wg, stats, WLS_STATS, 2);
    part_store(bs, ws[3], wg, stats, WLS_STATS, 3);
}

// b in the order the header states: the products s g each rounded on its own, (a - b) + (c - d) as dct_rhs, then - w d as screened_rhs,
// then the Dirichlet neighbours' s * boundary, west, north, east, south, each product rounded on its own.  ONE: every link is 1 and
// t.sx, t.sy are not read (the robust call's quadratic round without base links) -- the bytes of a call given arrays of 1.0f
template <bool LAP, bool ONE>
__global__ __launch_bounds__(WL) void k_wls_setup(PoissonGeo g, PcgGeo wg, WlsJobs t, float *__restrict__ R, float *__restrict__ E,
                                                   float *__restrict__ S, float *__restrict__ Dg, double *__restrict__ bb)
{
    __shared__ double ws[4];
    const PcgBand bd(g, wg);
    const PoissonJobDev &j = t.j[bd.member];
    const float *__restrict__ w = t.w[bd.member];
    const bool px = wg.ax == MIXED_PERIODIC, py = wg.ay == MIXED_PERIODIC;
    double s = 0.0;
    if (bd.x < wg.nx)
        for (int y = bd.y0; y < bd.y1; ++y) {
            const int X = wg.x0 + bd.x, Y = wg.y0 + y;
            const long long o = bd.pixel(g, X, Y);
            const Links k = links_at<ONE>(g, t.sx[bd.member], t.sy[bd.member], X, Y, o, px, py);
            float v;
            if (LAP) v = j.lap[o];
            else {
                const float a = (X < g.W - 1 || px) ? rounded_product(k.east, j.gx[o]) : 0.f;
                const float b = X > 0 ? rounded_product(k.west, j.gx[o - g.cs]) : px ? rounded_product(k.west, j.gx[o + (long long)(g.W - 1) * g.cs]) : 0.f;
                const float cc = (Y < g.H - 1 || py) ? rounded_product(k.south, j.gy[o]) : 0.f;
                const float d = Y > 0 ? rounded_product(k.north, j.gy[o - g.rs]) : py ? rounded_product(k.north, j.gy[o + (long long)(g.H - 1) * g.rs]) : 0.f;
                v = (a - b) + (cc - d);
            }
            const float wv = w[o];
            v = screened_rhs(v, wv, j.d[o]);
            if (X == 1 && mixed_low_d(wg.ax)) v -= rounded_product(k.west, j.b[o - g.cs]);
            if (Y == 1 && mixed_low_d(wg.ay)) v -= rounded_product(k.north, j.b[o - g.rs]);
            if (X == g.W - 2 && mixed_high_d(wg.ax)) v -= rounded_product(k.east, j.b[o + g.cs]);
            if (Y == g.H - 2 && mixed_high_d(wg.ay)) v -= rounded_product(k.south, j.b[o + g.rs]);
            const size_t i = (size_t)bd.p * wg.stride + (size_t)y * wg.nx + bd.x;
            R[i] = v;
            E[i] = (bd.x < wg.nx - 1 || px) ? k.east : 0.f;
            S[i] = (y < wg.ny - 1 || py) ? k.south : 0.f;
            Dg[i] = ((k.west + k.east) + (k.north + k.south)) + wv;
            s += (double)v * (double)v;
        }
    part_store(s, ws, wg, bb);
}

// the coefficients of L for the operator's walk: E and S hold 0 towards a missing right or lower neighbour already; the west link is
// the left neighbour's E, the north link the S of the row above, carried in a register (with wrap at the band start)
struct WlsCoef {
    const float *__restrict__ E, *__restrict__ S, *__restrict__ Dg;
    float s_up = 0.f;
    __device__ __forceinline__ void start(const PcgGeo &wg, size_t base, int x, int ya)
    {
        E += base; S += base;
        s_up = ya >= 0 ? S[(size_t)ya * wg.nx + x] : 0.f;
    }
    __device__ __forceinline__ float value(const PcgGeo &, int x, int xl, int y, size_t ro, size_t i, float l, float r, float up, float dn, float cur)
    {
        const float e_l = xl >= 0 ? E[ro + xl] : 0.f, e_r = E[ro + x], s_dn = S[ro + x];
        const float v = ((e_l * l + e_r * r) + (s_up * up + s_dn * dn)) - Dg[i] * cur;
        s_up = s_dn;
        return v;
    }
};

} // namespace

double wls_live_links(const PcgGeo &wg)
{
    const bool px = wg.ax == MIXED_PERIODIC, py = wg.ay == MIXED_PERIODIC;
    const double per_row = (wg.nx - 1) + (px ? 1 : 0) + (mixed_low_d(wg.ax) ? 1 : 0) + (mixed_high_d(wg.ax) ? 1 : 0);
    const double per_col = (wg.ny - 1) + (py ? 1 : 0) + (mixed_low_d(wg.ay) ? 1 : 0) + (mixed_high_d(wg.ay) ? 1 : 0);
    return per_row * wg.ny + per_col * wg.nx;
}

void launch_wls_stats(const PoissonGeo &g, const PcgGeo &wg, const PoissonJobDev *jobs, const SideArrays *sides, int m, double *stats, hipStream_t s)
{
    for_side_tables<WlsJobs>(jobs, sides, m, [&](const WlsJobs &t, int i0, int cnt) {
        hipLaunchKernelGGL(k_wls_stats, dim3((unsigned)wg.cg, (unsigned)wg.bands, (unsigned)(g.C * cnt)), dim3(WL), 0, s, g, wg, t,
                           stats + (size_t)g.C * i0 * PCG_PARTS * WLS_STATS);
    });
}

void launch_wls_setup(const PoissonGeo &g, const PcgGeo &wg, bool lap, const PoissonJobDev *jobs, const SideArrays *sides, int m, float *R, float *E,
                      float *S, float *Dg, double *bb, hipStream_t s)
{
    for_side_tables<WlsJobs>(jobs, sides, m, [&](const WlsJobs &t, int i0, int cnt) {
        const dim3 grid((unsigned)wg.cg, (unsigned)wg.bands, (unsigned)(g.C * cnt));
        const size_t o = (size_t)g.C * i0 * wg.stride;
        double *b = bb + (size_t)g.C * i0 * PCG_PARTS;
        if (!t.sx[0]) hipLaunchKernelGGL((k_wls_setup<false, true>), grid, dim3(WL), 0, s, g, wg, t, R + o, E + o, S + o, Dg + o, b);
        else if (lap) hipLaunchKernelGGL((k_wls_setup<true, false>), grid, dim3(WL), 0, s, g, wg, t, R + o, E + o, S + o, Dg + o, b);
        else hipLaunchKernelGGL((k_wls_setup<false, false>), grid, dim3(WL), 0, s, g, wg, t, R + o, E + o, S + o, Dg + o, b);
    });
}

void launch_wls_op(const PcgGeo &wg, int planes, bool residual, const float *P, const float *E, const float *S, const float *Dg, float *Q,
                   double *parts, hipStream_t s)
{
    const dim3 grid((unsigned)wg.cg, (unsigned)wg.bands, (unsigned)planes);
    if (residual) hipLaunchKernelGGL((k_pcg_op<true, WlsCoef, float, float, float>), grid, dim3(WL), 0, s, wg, P, Q, parts, E, S, Dg);
    else hipLaunchKernelGGL((k_pcg_op<false, WlsCoef, float, float, float>), grid, dim3(WL), 0, s, wg, P, Q, parts, E, S, Dg);
}

} // namespace sc
