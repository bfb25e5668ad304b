// sc_wls.hip -- the kernels of the WLS solve (sc_hip_wls*, sc_wls_api.cpp): the weighted solve's conjugate gradients on
//     L u = b,     (L u)(p) = sum_q s(p, q) (u(q) - u(p)) - w(p) u(p),     s > 0 the weight of the link p - q,  w >= 0,
// on the same compact float32 work planes (sc_common.h, WeightedGeo; only unknowns, homogeneous Dirichlet lines).  The links of a job come
// as two arrays under the call's layout: sx(x, y) joins (x, y) and (x + 1, y), sy(x, y) joins (x, y) and (x, y + 1); along a periodic
// axis the last column / row holds the link from the last pixel to the first (dct_rhs's convention for gx, gy).  A link is live when at
// least one of its ends is an unknown; no other element of sx, sy is ever read.  Seen from an unknown at pixel (X, Y) its four links are
//     east  sx(X, Y)      where X < W - 1 or the axis wraps           west   sx(X - 1, Y)   where X > 0, sx(W - 1, Y) where X = 0 wraps
//     south sy(X, Y)      where Y < H - 1 or the axis wraps           north  sy(X, Y - 1)   where Y > 0, sy(X, H - 1) where Y = 0 wraps
// -- the neighbour beyond is an unknown or lies on a Dirichlet line, never outside the image -- and 0 (not read) otherwise.
// Set-up folds the caller's arrays into three coefficient planes (w gets none of its own: the operator uses it inside Dg only): E, the link to the next unknown column
// (0 where there is none: a Dirichlet line or a free end follows), S, the link to the next unknown row, and Dg, the diagonal: all four
// incident links, those to Dirichlet pixels included, plus w.  The operator launch is k_w_op's walk -- 256 lanes, a lane owns one column
// of its band and rolls its rows through registers, no LDS, no barrier -- with five plane transfers for the weighted operator's three
// (p, E, S, Dg in, q out): the west link is the left neighbour's E, read like the left neighbour's p from the cache lines the wave
// loads anyway (across the 256-column group boundary too), the north link the S of the row above, carried in a register.
#include "sc_pcg_device.h"
#include <cmath>

namespace sc {

namespace {

// the four incident links of the unknown at pixel (X, Y), offset o, of one channel: 0 where there is none (then nothing is read)
struct Links { float west, east, north, south; };
__device__ __forceinline__ Links links_at(const PoissonGeo &g, const float *__restrict__ sx, const float *__restrict__ sy, int X, int Y, long long o,
                                          bool px, bool py)
{
    Links k;
    k.east = (X < g.W - 1 || px) ? sx[o] : 0.f;
    k.west = X > 0 ? sx[o - g.cs] : px ? sx[o + (long long)(g.W - 1) * g.cs] : 0.f;
    k.south = (Y < g.H - 1 || py) ? sy[o] : 0.f;
    k.north = Y > 0 ? sy[o - g.rs] : py ? sy[o + (long long)(g.H - 1) * g.rs] : 0.f;
    return k;
}

__device__ __forceinline__ bool bad_link(float v) { return !(v > 0.f) || v > 3.4028234e38f; }

// Every live link is counted once: by its low end where both ends are unknowns (the last pixel of a periodic axis owns the wrapping
// link), by its unknown end where the other lies on a Dirichlet line.
__global__ __launch_bounds__(WL) void k_wls_stats(PoissonGeo g, WeightedGeo wg, WlsJobs t, double *__restrict__ stats)
{
    __shared__ double ws[4][4];
    const int p = (int)blockIdx.z, member = p / g.C, c = p - member * g.C, x = (int)blockIdx.x * WL + (int)threadIdx.x;
    const int y0 = (int)blockIdx.y * wg.rows, y1 = min(y0 + wg.rows, wg.ny);
    const float *__restrict__ w = t.w[member], *__restrict__ sx = t.sx[member], *__restrict__ sy = t.sy[member];
    const bool px = wg.ax == MIXED_PERIODIC, py = wg.ay == MIXED_PERIODIC;
    double sw = 0.0, bw = 0.0, ss = 0.0, bs = 0.0;
    if (x < wg.nx)
        for (int y = y0; y < y1; ++y) {
            const int X = wg.x0 + x, Y = wg.y0 + y;
            const long long o = (long long)X * g.cs + (long long)Y * g.rs + (long long)c * g.chs;
            const float v = w[o];
            if (!(v >= 0.f) || v > 3.4028234e38f) bw += 1.0;
            sw += (double)v;
            auto link = [&](float s) { if (bad_link(s)) bs += 1.0; ss += (double)s; };
            if (X < g.W - 1 || px) link(sx[o]);
            if (Y < g.H - 1 || py) link(sy[o]);
            if (X == 1 && mixed_low_d(wg.ax)) link(sx[o - g.cs]);
            if (Y == 1 && mixed_low_d(wg.ay)) link(sy[o - g.rs]);
        }
    sw = block_sum(sw, ws[0]);
    bw = block_sum(bw, ws[1]);
    ss = block_sum(ss, ws[2]);
    bs = block_sum(bs, ws[3]);
    if (threadIdx.x == 0) {
        double *o = stats + ((size_t)p * WEIGHTED_PARTS + blockIdx.y * wg.cg + blockIdx.x) * WLS_STATS;
        o[0] = sw;
        o[1] = bw;
        o[2] = ss;
        o[3] = bs;
    }
}

// b in the order the header states: the products s g each rounded on its own, (a - b) + (c - d) as dct_rhs, then - w d as screened_rhs,
// then the Dirichlet neighbours' s * boundary, west, north, east, south, each product rounded on its own
template <bool LAP>
__global__ __launch_bounds__(WL) void k_wls_setup(PoissonGeo g, WeightedGeo wg, WlsJobs t, float *__restrict__ R, float *__restrict__ E,
                                                   float *__restrict__ S, float *__restrict__ Dg, double *__restrict__ bb)
{
    __shared__ double ws[4];
    const int p = (int)blockIdx.z, member = p / g.C, c = p - member * g.C, x = (int)blockIdx.x * WL + (int)threadIdx.x;
    const int y0 = (int)blockIdx.y * wg.rows, y1 = min(y0 + wg.rows, wg.ny);
    const PoissonJobDev &j = t.j[member];
    const float *__restrict__ w = t.w[member];
    const bool px = wg.ax == MIXED_PERIODIC, py = wg.ay == MIXED_PERIODIC;
    double s = 0.0;
    if (x < wg.nx)
        for (int y = y0; y < y1; ++y) {
            const int X = wg.x0 + x, Y = wg.y0 + y;
            const long long o = (long long)X * g.cs + (long long)Y * g.rs + (long long)c * g.chs;
            const Links k = links_at(g, t.sx[member], t.sy[member], X, Y, o, px, py);
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
            const size_t i = (size_t)p * wg.stride + (size_t)y * wg.nx + x;
            R[i] = v;
            E[i] = (x < wg.nx - 1 || px) ? k.east : 0.f;
            S[i] = (y < wg.ny - 1 || py) ? k.south : 0.f;
            Dg[i] = ((k.west + k.east) + (k.north + k.south)) + wv;
            s += (double)v * (double)v;
        }
    s = block_sum(s, ws);
    if (threadIdx.x == 0) bb[(size_t)p * WEIGHTED_PARTS + blockIdx.y * wg.cg + blockIdx.x] = s;
}

// RES false: Q = L P and the parts of P . Q;  true: Q -= L P and the parts of Q . Q
template <bool RES>
__global__ __launch_bounds__(WL) void k_wls_op(WeightedGeo wg, const float *__restrict__ P, const float *__restrict__ E, const float *__restrict__ S,
                                                const float *__restrict__ Dg, float *__restrict__ Q, double *__restrict__ parts)
{
    __shared__ double ws[4];
    const int x = (int)blockIdx.x * WL + (int)threadIdx.x, nx = wg.nx, ny = wg.ny;
    const int y0 = (int)blockIdx.y * wg.rows, y1 = min(y0 + wg.rows, ny);
    const size_t base = (size_t)blockIdx.z * wg.stride;
    const float *__restrict__ pl = P + base, *__restrict__ el = E + base, *__restrict__ sl = S + base;
    const bool px = wg.ax == MIXED_PERIODIC, py = wg.ay == MIXED_PERIODIC;
    double s = 0.0;
    if (x < nx) {
        // the neighbours of this column: their index, -1 where there is none (the value and its link count 0; E and S hold 0 towards a
        // missing right or lower neighbour already)
        const int xl = x > 0 ? x - 1 : px ? nx - 1 : -1, xr = x < nx - 1 ? x + 1 : px ? 0 : -1;
        auto row_above = [&](int y) { return y > 0 ? y - 1 : py ? ny - 1 : -1; };
        auto row_below = [&](int y) { return y < ny - 1 ? y + 1 : py ? 0 : -1; };
        const int ya = row_above(y0);
        float up = ya >= 0 ? pl[(size_t)ya * nx + x] : 0.f, cur = pl[(size_t)y0 * nx + x];
        float s_up = ya >= 0 ? sl[(size_t)ya * nx + x] : 0.f;          // the north link: the S of the row above (with wrap at the band start)
        for (int y = y0; y < y1; ++y) {
            const int yb = row_below(y);
            const float dn = yb >= 0 ? pl[(size_t)yb * nx + x] : 0.f;
            const size_t ro = (size_t)y * nx;
            const float l = xl >= 0 ? pl[ro + xl] : 0.f, r = xr >= 0 ? pl[ro + xr] : 0.f;
            const float e_l = xl >= 0 ? el[ro + xl] : 0.f, e_r = el[ro + x], s_dn = sl[ro + x];
            const size_t i = base + ro + x;
            const float v = ((e_l * l + e_r * r) + (s_up * up + s_dn * dn)) - Dg[i] * cur;
            if (RES) {
                const float q = Q[i] - v;
                Q[i] = q;
                s += (double)q * (double)q;
            } else {
                Q[i] = v;
                s += (double)cur * (double)v;
            }
            up = cur;
            cur = dn;
            s_up = s_dn;
        }
    }
    s = block_sum(s, ws);
    if (threadIdx.x == 0) parts[(size_t)blockIdx.z * WEIGHTED_PARTS + blockIdx.y * wg.cg + blockIdx.x] = s;
}

__global__ __launch_bounds__(WL) void k_wls_scale(WeightedGeo wg, float *__restrict__ U, float f)
{
    const int tid = (int)threadIdx.x, n = wg.nx * wg.ny;
    const size_t base = (size_t)blockIdx.y * wg.stride;
    int g0, g1;
    segment(wg, (int)blockIdx.x, g0, g1);
    for (int gi = g0 + tid; gi < g1; gi += WL) {
        const size_t i = base + (size_t)gi * 4;
        if (gi * 4 + 3 < n) {
            float4 u = *reinterpret_cast<float4 *>(U + i);
            u.x *= f; u.y *= f; u.z *= f; u.w *= f;
            *reinterpret_cast<float4 *>(U + i) = u;
        } else {
            for (int k = gi * 4; k < n; ++k) U[base + k] *= f;
        }
    }
}

template <typename Fn>
void wls_chunks(const PoissonJobDev *jobs, const float *const *w, const float *const *sx, const float *const *sy, int m, Fn fn)
{
    for (int i0 = 0; i0 < m; i0 += WlsJobs::MAX) {
        WlsJobs t{};
        const int cnt = std::min(m - i0, (int)WlsJobs::MAX);
        for (int i = 0; i < cnt; ++i) { t.j[i] = jobs[i0 + i]; t.w[i] = w[i0 + i]; t.sx[i] = sx[i0 + i]; t.sy[i] = sy[i0 + i]; }
        fn(t, i0, cnt);
    }
}

} // namespace

double wls_live_links(const WeightedGeo &wg)
{
    const bool px = wg.ax == MIXED_PERIODIC, py = wg.ay == MIXED_PERIODIC;
    const double per_row = (wg.nx - 1) + (px ? 1 : 0) + (mixed_low_d(wg.ax) ? 1 : 0) + (mixed_high_d(wg.ax) ? 1 : 0);
    const double per_col = (wg.ny - 1) + (py ? 1 : 0) + (mixed_low_d(wg.ay) ? 1 : 0) + (mixed_high_d(wg.ay) ? 1 : 0);
    return per_row * wg.ny + per_col * wg.nx;
}

void launch_wls_stats(const PoissonGeo &g, const WeightedGeo &wg, const PoissonJobDev *jobs, const float *const *w, const float *const *sx,
                      const float *const *sy, int m, double *stats, hipStream_t s)
{
    wls_chunks(jobs, w, sx, sy, m, [&](const WlsJobs &t, int i0, int cnt) {
        hipLaunchKernelGGL(k_wls_stats, dim3((unsigned)wg.cg, (unsigned)wg.bands, (unsigned)(g.C * cnt)), dim3(WL), 0, s, g, wg, t,
                           stats + (size_t)g.C * i0 * WEIGHTED_PARTS * WLS_STATS);
    });
}

void launch_wls_setup(const PoissonGeo &g, const WeightedGeo &wg, bool lap, const PoissonJobDev *jobs, const float *const *w, const float *const *sx,
                      const float *const *sy, int m, float *R, float *E, float *S, float *Dg, double *bb, hipStream_t s)
{
    wls_chunks(jobs, w, sx, sy, m, [&](const WlsJobs &t, int i0, int cnt) {
        const dim3 grid((unsigned)wg.cg, (unsigned)wg.bands, (unsigned)(g.C * cnt));
        const size_t o = (size_t)g.C * i0 * wg.stride;
        double *b = bb + (size_t)g.C * i0 * WEIGHTED_PARTS;
        if (lap) hipLaunchKernelGGL(k_wls_setup<true>, grid, dim3(WL), 0, s, g, wg, t, R + o, E + o, S + o, Dg + o, b);
        else hipLaunchKernelGGL(k_wls_setup<false>, grid, dim3(WL), 0, s, g, wg, t, R + o, E + o, S + o, Dg + o, b);
    });
}

void launch_wls_op(const WeightedGeo &wg, int planes, bool residual, const float *P, const float *E, const float *S, const float *Dg, float *Q,
                   double *parts, hipStream_t s)
{
    const dim3 grid((unsigned)wg.cg, (unsigned)wg.bands, (unsigned)planes);
    if (residual) hipLaunchKernelGGL(k_wls_op<true>, grid, dim3(WL), 0, s, wg, P, E, S, Dg, Q, parts);
    else hipLaunchKernelGGL(k_wls_op<false>, grid, dim3(WL), 0, s, wg, P, E, S, Dg, Q, parts);
}

void launch_wls_scale(const WeightedGeo &wg, int planes, float *U, float f, hipStream_t s)
{
    hipLaunchKernelGGL(k_wls_scale, dim3((unsigned)wg.eparts, (unsigned)planes), dim3(WL), 0, s, wg, U, f);
}

} // namespace sc
