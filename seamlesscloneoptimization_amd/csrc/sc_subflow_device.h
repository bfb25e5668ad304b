// sc_subflow_device.h -- what the kernels of the sub-pixel flow calls share (sc_volume_subflow.hip, sc_volume_subflow_robust.hip): the
// taps of a bilinear link, a work-plane index as an offset under the call's layout, the link an element holds as the states judge it,
// and where a launch's first volume lies in the link storage (sc_pcg.h: SubflowLinks, SubflowStore).
#pragma once
#include "sc_region_device.h"

namespace sc {

// The taps of the link that element (x, yy, t) holds under the flow value (dx, dy): j[k] the work-plane index of tap k (-1: the tap is
// no part of the link), b[k] its weight.  x0 = floorf(dx), ax = dx - x0 (exact), the weights the float32 products (1 - ax)(1 - ay),
// ax (1 - ay), (1 - ax) ay, ax ay; a tap of weight 0 is left out; a periodic axis wraps a tap, elsewhere a tap outside the work rectangle
// leaves the pixel without a link.  false: no link (a component that is not finite or beyond 1e6, a tap outside).
__device__ __forceinline__ bool subflow_taps(const PcgGeo &wg, const VolumeGeo &vg, float dx, float dy, int x, int yy, int t, int (&j)[4], float (&b)[4])
{
#pragma unroll
    for (int k = 0; k < 4; ++k) { j[k] = -1; b[k] = 0.f; }
    if (!(fabsf(dx) <= 1e6f && fabsf(dy) <= 1e6f)) return false;      // (NaN fails)
    const float fx0 = floorf(dx), fy0 = floorf(dy), ax = dx - fx0, ay = dy - fy0;
    const float wx0 = 1.f - ax, wy0 = 1.f - ay;
    const int tt = t < vg.T - 1 ? t + 1 : 0;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float w = ((k & 1) ? ax : wx0) * ((k >> 1) ? ay : wy0);
        if (w == 0.f) continue;
        int tx = x + (int)fx0 + (k & 1), ty = yy + (int)fy0 + (k >> 1);
        if (wg.ax == MIXED_PERIODIC) { tx %= wg.nx; tx += tx < 0 ? wg.nx : 0; }
        if (wg.ay == MIXED_PERIODIC) { ty %= vg.ny; ty += ty < 0 ? vg.ny : 0; }
        if (tx < 0 || tx >= wg.nx || ty < 0 || ty >= vg.ny) { ok = false; continue; }
        j[k] = (int)(((long long)tt * vg.ny + ty) * wg.nx + tx);
        b[k] = w;
    }
    if (!ok) {
#pragma unroll
        for (int k = 0; k < 4; ++k) { j[k] = -1; b[k] = 0.f; }
    }
    return ok;
}

// work-plane index j of a volume as the offset of channel c's element under the call's layout
__device__ __forceinline__ long long subflow_offset(const PoissonGeo &g, const PcgGeo &wg, const VolumeGeo &vg, int c, int j)
{
    const int n2 = wg.nx * vg.ny, t = j / n2, r = j - t * n2, y = r / wg.nx, x = r - y * wg.nx;
    return (long long)(wg.x0 + x) * g.cs + (long long)(wg.y0 + y) * g.rs + (long long)c * g.chs + (long long)t * vg.fs;
}

// the link that work-plane element (x, y) of channel c holds, judged by the states: live (neither its source nor any tap OUTSIDE, at
// least one of its points UNKNOWN), the kind of its source, the sum of b over its KNOWN taps and of b * data over them
struct SubflowLink {
    bool live;
    int kp;
    float kb, kd;
    int j[4];
    float b[4];
    __device__ __forceinline__ SubflowLink(const PoissonGeo &g, const PcgGeo &wg, const VolumeGeo &vg, const float *__restrict__ fw, long long n,
                                           const float *__restrict__ st, const float *__restrict__ d, int c, int x, int y, int t, int yy, long long o)
    {
        live = false; kp = NB_NONE; kb = kd = 0.f;
        const long long i = (long long)y * wg.nx + x;
        if (!subflow_taps(wg, vg, fw[i], fw[n + i], x, yy, t, j, b)) return;
        kp = state_kind(st[o]);
        bool dead = kp == NB_NONE, unk = kp == NB_UNKNOWN;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (j[k] >= 0) {
                const long long oq = subflow_offset(g, wg, vg, c, j[k]);
                const int kq = state_kind(st[oq]);
                dead = dead || kq == NB_NONE;
                unk = unk || kq == NB_UNKNOWN;
                if (kq == NB_KNOWN) { kb += b[k]; if (d) kd += b[k] * d[oq]; }
            }
        live = !dead && unk;
    }
};

// the links of the launch's first volume i0 (host)
inline SubflowLinks subflow_links_at(const SubflowStore &st, void *lnk, int i0)
{
    char *p = (char *)lnk;
    return SubflowLinks{ (const long long *)(p + st.off_b) + (long long)i0 * (st.n + 2), (const unsigned long long *)(p + st.ent_b) + (long long)i0 * 4 * st.n,
                         (const float *)(p + st.fw_b) + (long long)i0 * 2 * st.n, st.n };
}

} // namespace sc
