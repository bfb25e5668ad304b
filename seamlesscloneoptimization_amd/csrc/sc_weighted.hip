// sc_weighted.hip -- the weighted family's kernels (sc_hip_weighted*, sc_weighted_api.cpp) under the shared conjugate gradients (sc_pcg.h):
//     (A - W) u = b,     W = diag(w), w >= 0,     b = lap - w d less the neighbouring Dirichlet values,
// A the 5-point operator under each side's rule, on the compact work planes (PcgGeo): the weights' statistics, the set-up, and the
// operator -- sc_pcg_device.h's walk with the weights as its one coefficient plane (256 lanes and a handful of registers per workgroup:
// full occupancy; the launch is bound by the three plane transfers: p and w in, q out).
#include "sc_pcg_device.h"
#include <cmath>

namespace sc {

namespace {

__global__ __launch_bounds__(WL) void k_w_stats(PoissonGeo g, PcgGeo wg, WeightedJobs t, double *__restrict__ stats)
{
    __shared__ double ws[4], wb[4];
    const PcgBand b(g, wg);
    const float *__restrict__ w = t.w[b.member];
    double s = 0.0, bad = 0.0;
    if (b.x < wg.nx)
        for (int y = b.y0; y < b.y1; ++y) {
            const float v = w[b.pixel(g, wg.x0 + b.x, wg.y0 + y)];
            if (!(v >= 0.f) || v > 3.4028234e38f) bad += 1.0;
            s += (double)v;
        }
    part_store(s, ws, wg, stats, 2, 0);
    part_store(bad, wb, wg, stats, 2, 1);
}

template <bool LAP>
__global__ __launch_bounds__(WL) void k_w_setup(PoissonGeo g, PcgGeo wg, WeightedJobs t, float *__restrict__ R, float *__restrict__ Wc,
                                                 double *__restrict__ bb)
{
    __shared__ double ws[4];
    const PcgBand b(g, wg);
    const PoissonJobDev &j = t.j[b.member];
    const float *__restrict__ w = t.w[b.member];
    const bool px = wg.ax == MIXED_PERIODIC, py = wg.ay == MIXED_PERIODIC;
    double s = 0.0;
    if (b.x < wg.nx)
        for (int y = b.y0; y < b.y1; ++y) {
            const int X = wg.x0 + b.x, Y = wg.y0 + y;
            const long long o = b.pixel(g, X, Y);
            const float wv = w[o];
            float v = screened_rhs(dct_rhs<LAP>(g, j, b.c, X, Y, px, py), wv, j.d[o]);
            if (X == 1 && mixed_low_d(wg.ax)) v -= j.b[o - g.cs];
            if (Y == 1 && mixed_low_d(wg.ay)) v -= j.b[o - g.rs];
            if (X == g.W - 2 && mixed_high_d(wg.ax)) v -= j.b[o + g.cs];
            if (Y == g.H - 2 && mixed_high_d(wg.ay)) v -= j.b[o + g.rs];
            const size_t i = (size_t)b.p * wg.stride + (size_t)y * wg.nx + b.x;
            R[i] = v;
            Wc[i] = wv;
            s += (double)v * (double)v;
        }
    part_store(s, ws, wg, bb);
}

// the coefficients of A - W for the operator's walk: the number of neighbour terms that exist (none beyond a free end) and the weight
struct WeightedCoef {
    const float *__restrict__ Wc;
    float cnt_x = 2.f;
    __device__ __forceinline__ void start(const PcgGeo &wg, size_t, int x, int)
    {
        const bool px = wg.ax == MIXED_PERIODIC;
        cnt_x = 2.f;
        if (x == 0 && !px && !mixed_low_d(wg.ax)) cnt_x -= 1.f;
        if (x == wg.nx - 1 && !px && !mixed_high_d(wg.ax)) cnt_x -= 1.f;
    }
    __device__ __forceinline__ float value(const PcgGeo &wg, int x, int xl, int y, size_t ro, size_t i, float l, float r, float up, float dn, float cur)
    {
        const bool py = wg.ay == MIXED_PERIODIC;
        float cnt = cnt_x + 2.f;
        if (y == 0 && !py && !mixed_low_d(wg.ay)) cnt -= 1.f;
        if (y == wg.ny - 1 && !py && !mixed_high_d(wg.ay)) cnt -= 1.f;
        return (((l + r) + (up + dn)) - cnt * cur) - Wc[i] * cur;
    }
};

} // namespace

void launch_weighted_stats(const PoissonGeo &g, const PcgGeo &wg, const PoissonJobDev *jobs, const SideArrays *sides, int m, double *stats,
                           hipStream_t s)
{
    for_side_tables<WeightedJobs>(jobs, sides, m, [&](const WeightedJobs &t, int i0, int cnt) {
        hipLaunchKernelGGL(k_w_stats, dim3((unsigned)wg.cg, (unsigned)wg.bands, (unsigned)(g.C * cnt)), dim3(WL), 0, s, g, wg, t,
                           stats + (size_t)g.C * i0 * PCG_PARTS * 2);
    });
}

void launch_weighted_setup(const PoissonGeo &g, const PcgGeo &wg, bool lap, const PoissonJobDev *jobs, const SideArrays *sides, int m, float *R,
                           float *Wc, double *bb, hipStream_t s)
{
    for_side_tables<WeightedJobs>(jobs, sides, m, [&](const WeightedJobs &t, int i0, int cnt) {
        const dim3 grid((unsigned)wg.cg, (unsigned)wg.bands, (unsigned)(g.C * cnt));
        const size_t p0 = (size_t)g.C * i0;
        if (lap) hipLaunchKernelGGL(k_w_setup<true>, grid, dim3(WL), 0, s, g, wg, t, R + p0 * wg.stride, Wc + p0 * wg.stride, bb + p0 * PCG_PARTS);
        else hipLaunchKernelGGL(k_w_setup<false>, grid, dim3(WL), 0, s, g, wg, t, R + p0 * wg.stride, Wc + p0 * wg.stride, bb + p0 * PCG_PARTS);
    });
}

void launch_weighted_op(const PcgGeo &wg, int planes, bool residual, const float *P, const float *Wc, float *Q, double *parts, hipStream_t s)
{
    const dim3 grid((unsigned)wg.cg, (unsigned)wg.bands, (unsigned)planes);
    if (residual) hipLaunchKernelGGL((k_pcg_op<true, WeightedCoef, float>), grid, dim3(WL), 0, s, wg, P, Q, parts, Wc);
    else hipLaunchKernelGGL((k_pcg_op<false, WeightedCoef, float>), grid, dim3(WL), 0, s, wg, P, Q, parts, Wc);
}

} // namespace sc
