// sc_volume_flow.hip -- the flow volume call's own kernels (sc_hip_volume_flow*; sc_volume_api.cpp: VolumeFlowOperator): the matching
// that turns a volume's flow arrays into its two link planes, and the operator that gathers its temporal neighbours through them.  The
// statistics and the set-up are sc_volume.hip's in their flow forms; sc_pcg.h says what the link planes hold and states the matching.
//
// Matching, per volume and pair of frames, without regard to state (a volume's channels share it): k_flow_claim lets every candidate
// take an integer minimum on bwd[target] with its own index -- whatever the order, the smallest candidate stays --, k_flow_links keeps
// fwd[p] = target where p won and -1 elsewhere.  So every element has at most one link that leaves it and at most one that arrives,
// fwd and bwd are inverse to each other, the operator is symmetric, and two runs give the same planes.
#include "sc_region_device.h"
#include <climits>

namespace sc {

namespace {

// (Every index of a link plane is below INT_MAX: the entries refuse a larger volume, flow_indexable.  The arithmetic is 64-bit up to the
// one narrowing all the same.)
// the work-plane index that element (x, yy, t)'s link leads to; -1: it is no candidate (no flow in its frame, a component that is not
// finite, not whole or beyond 1e6, a target outside the work rectangle)
__device__ __forceinline__ int flow_target(const PoissonGeo &g, const PcgGeo &wg, const VolumeGeo &vg, const float *__restrict__ fx,
                                           const float *__restrict__ fy, int x, int yy, int t)
{
    if (!(t < vg.T - 1 || vg.periodic)) return -1;
    const size_t e = ((size_t)t * g.H + (wg.y0 + yy)) * g.W + (wg.x0 + x);
    const float dx = fx[e], dy = fy[e];
    if (!(fabsf(dx) <= 1e6f && fabsf(dy) <= 1e6f) || dx != rintf(dx) || dy != rintf(dy)) return -1;      // (NaN fails the first test)
    int tx = x + (int)dx, ty = yy + (int)dy;
    if (wg.ax == MIXED_PERIODIC) { tx %= wg.nx; tx += tx < 0 ? wg.nx : 0; }
    if (wg.ay == MIXED_PERIODIC) { ty %= vg.ny; ty += ty < 0 ? vg.ny : 0; }
    if (tx < 0 || tx >= wg.nx || ty < 0 || ty >= vg.ny) return -1;
    const int tt = t < vg.T - 1 ? t + 1 : 0;
    return (int)(((long long)tt * vg.ny + ty) * wg.nx + tx);
}

// the three launches' grid: column groups x a frame's rows x (volumes T); the element of a lane
struct FlowLane {
    int x, yy, t, k, i;
    __device__ __forceinline__ FlowLane(const PcgGeo &wg, const VolumeGeo &vg)
    {
        x = (int)blockIdx.x * WL + (int)threadIdx.x; yy = (int)blockIdx.y; k = (int)blockIdx.z / vg.T; t = (int)blockIdx.z - k * vg.T;
        i = (int)(((long long)t * vg.ny + yy) * wg.nx + x);
    }
};

__global__ __launch_bounds__(WL) void k_flow_fill(PcgGeo wg, VolumeGeo vg, long long stride, int *__restrict__ bwd)
{
    const FlowLane ln(wg, vg);
    if (ln.x < wg.nx) bwd[(long long)ln.k * stride + ln.i] = INT_MAX;
}

__global__ __launch_bounds__(WL) void k_flow_claim(PoissonGeo g, PcgGeo wg, VolumeGeo vg, FlowArrays a, long long stride, int *__restrict__ bwd)
{
    const FlowLane ln(wg, vg);
    if (ln.x >= wg.nx) return;
    const int j = flow_target(g, wg, vg, a.fx[ln.k], a.fy[ln.k], ln.x, ln.yy, ln.t);
    if (j >= 0) atomicMin(&bwd[(long long)ln.k * stride + j], ln.i);
}

__global__ __launch_bounds__(WL) void k_flow_links(PoissonGeo g, PcgGeo wg, VolumeGeo vg, FlowArrays a, long long stride, int *__restrict__ fwd,
                                                   int *__restrict__ bwd)
{
    const FlowLane ln(wg, vg);
    if (ln.x >= wg.nx) return;
    const long long base = (long long)ln.k * stride;
    const int i = ln.i, j = flow_target(g, wg, vg, a.fx[ln.k], a.fy[ln.k], ln.x, ln.yy, ln.t);
    // (bwd[j] was claimed -- by this element at the least -- and is no INT_MAX: nobody rewrites it below)
    fwd[base + i] = j >= 0 && bwd[base + j] == i ? j : -1;
    if (bwd[base + i] == INT_MAX) bwd[base + i] = -1;
}

// k_volume_op's walk (sc_volume.hip: the rolling rows, the frames' seams) with the temporal neighbours of element i read through the link
// planes of the plane's volume: tb = F[bwd[i]] P[bwd[i]], tf = F[i] P[fwd[i]], 0 where there is none; the wrap of periodic time is in the
// indices.  The same order of arithmetic.  Two int32 loads per element more than k_volume_op and a gather whose coalescing is the
// flow's smoothness.  No atomics, no LDS but the block sum's.
template <bool RES>
__global__ __launch_bounds__(WL) void k_volume_flow_op(PcgGeo wg, VolumeGeo vg, int C, long long lstride, const float *__restrict__ P, float *__restrict__ Q,
                                                        double *__restrict__ parts, const float *__restrict__ E, const float *__restrict__ S,
                                                        const float *__restrict__ F, const float *__restrict__ Dg, const int *__restrict__ fwd,
                                                        const int *__restrict__ bwd)
{
    __shared__ double ws[4];
    const int x = (int)blockIdx.x * WL + (int)threadIdx.x, nx = wg.nx, fny = vg.ny;
    const int y0 = (int)blockIdx.y * wg.rows, y1 = min(y0 + wg.rows, wg.ny);
    const size_t base = (size_t)blockIdx.z * wg.stride, lbase = (size_t)((int)blockIdx.z / C) * (size_t)lstride;
    const float *__restrict__ pl = P + base, *__restrict__ el = E + base, *__restrict__ sl = S + base, *__restrict__ fl = F + base;
    const int *__restrict__ fw = fwd + lbase, *__restrict__ bw = bwd + lbase;
    double s = 0.0;
    if (x < nx) {
        const bool px = wg.ax == MIXED_PERIODIC, py = wg.ay == MIXED_PERIODIC;
        const int xl = x > 0 ? x - 1 : px ? nx - 1 : -1, xr = x < nx - 1 ? x + 1 : px ? 0 : -1;
        FrameRow fr(vg, y0);
        // the row above row y (the yy-th of its frame), -1: none
        auto row_above = [&](int y, int yy) { return yy > 0 ? y - 1 : py ? y + fny - 1 : -1; };
        int ya = row_above(y0, fr.yy);
        float up = ya >= 0 ? pl[(size_t)ya * nx + x] : 0.f, s_up = ya >= 0 ? sl[(size_t)ya * nx + x] : 0.f, cur = pl[(size_t)y0 * nx + x];
        for (int y = y0; y < y1; ++y) {
            const bool last = fr.yy == fny - 1;          // of its frame
            const int yb = !last ? y + 1 : py ? y - (fny - 1) : -1;
            const float dn = yb >= 0 ? pl[(size_t)yb * nx + x] : 0.f;
            const size_t ro = (size_t)y * nx, i = base + ro + x;
            const float l = xl >= 0 ? pl[ro + xl] : 0.f, r = xr >= 0 ? pl[ro + xr] : 0.f;
            const float e_l = xl >= 0 ? el[ro + xl] : 0.f, e_r = el[ro + x], s_dn = sl[ro + x];
            const int jb = bw[ro + x], jf = fw[ro + x];
            const float tb = jb >= 0 ? fl[jb] * pl[jb] : 0.f;
            const float tf = jf >= 0 ? fl[ro + x] * pl[jf] : 0.f;
            const float v = (((e_l * l + e_r * r) + (s_up * up + s_dn * dn)) + (tb + tf)) - Dg[i] * cur;
            if (RES) {
                const float q = Q[i] - v;
                Q[i] = q;
                s += (double)q * (double)q;
            } else {
                Q[i] = v;
                s += (double)cur * (double)v;
            }
            if (!last) {
                up = cur; cur = dn; s_up = s_dn;
                ++fr.yy;
            } else if (y + 1 < y1) {                     // into the next frame
                ++fr.t; fr.yy = 0;
                ya = row_above(y + 1, 0);
                up = ya >= 0 ? pl[(size_t)ya * nx + x] : 0.f;
                s_up = ya >= 0 ? sl[(size_t)ya * nx + x] : 0.f;
                cur = pl[(size_t)(y + 1) * nx + x];
            }
        }
    }
    part_store(s, ws, wg, parts);
}

} // namespace

void launch_flow_links(const PoissonGeo &g, const PcgGeo &wg, const VolumeGeo &vg, const SideArrays *sides, int m, int *fwd, int *bwd, hipStream_t s)
{
    const long long stride = flow_link_stride(wg);
    for (int i0 = 0; i0 < m; i0 += FlowArrays::MAX) {
        const int cnt = std::min(m - i0, (int)FlowArrays::MAX);
        FlowArrays a{};
        for (int i = 0; i < cnt; ++i) a.set(i, sides[i0 + i]);
        const dim3 grid((unsigned)wg.cg, (unsigned)vg.ny, (unsigned)(cnt * vg.T));
        int *f = fwd + stride * i0, *b = bwd + stride * i0;
        hipLaunchKernelGGL(k_flow_fill, grid, dim3(WL), 0, s, wg, vg, stride, b);
        hipLaunchKernelGGL(k_flow_claim, grid, dim3(WL), 0, s, g, wg, vg, a, stride, b);
        hipLaunchKernelGGL(k_flow_links, grid, dim3(WL), 0, s, g, wg, vg, a, stride, f, b);
    }
}

void launch_volume_flow_op(const PcgGeo &wg, const VolumeGeo &vg, int planes, int C, bool residual, const float *P, const float *E, const float *S,
                           const float *F, const float *Dg, const int *fwd, const int *bwd, float *Q, double *parts, hipStream_t s)
{
    const dim3 grid((unsigned)wg.cg, (unsigned)wg.bands, (unsigned)planes);
    const long long ls = flow_link_stride(wg);
    if (residual) hipLaunchKernelGGL(k_volume_flow_op<true>, grid, dim3(WL), 0, s, wg, vg, C, ls, P, Q, parts, E, S, F, Dg, fwd, bwd);
    else hipLaunchKernelGGL(k_volume_flow_op<false>, grid, dim3(WL), 0, s, wg, vg, C, ls, P, Q, parts, E, S, F, Dg, fwd, bwd);
}

} // namespace sc
