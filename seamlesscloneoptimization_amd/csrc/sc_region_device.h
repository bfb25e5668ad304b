// sc_region_device.h -- what the kernels of the region and the volume families share (sc_region.hip, sc_volume.hip, sc_volume_robust.hip):
// a state element's meaning, the four spatial neighbours of a pixel as the region call sees them, and a volume's frames: the row of a
// work plane of stacked frames, the two temporal neighbours -- one frame away, or at the ends of the flow call's links --, a temporal link's weight.
#pragma once
#include "sc_pcg_device.h"

namespace sc {

// what lies across a link of an UNKNOWN pixel
enum { NB_UNKNOWN = 0, NB_KNOWN = 1, NB_NONE = 2, NB_DIRICHLET = 3 };
__device__ __forceinline__ int state_kind(float v) { return v == 0.f ? NB_UNKNOWN : v == 1.f ? NB_KNOWN : NB_NONE; }

// The four neighbours of the work-plane pixel (X, Y) at offset o: the neighbour's offset (which is also where the west and north
// links and their guidance values are stored; the east and south ones are stored at o) and its kind.
struct Around {
    long long ow, oe, on, os;
    int kw, ke, kn, ks;
    __device__ __forceinline__ Around(const PoissonGeo &g, const PcgGeo &wg, const float *__restrict__ st, int X, int Y, long long o, bool px, bool py)
    {
        ow = X > 0 ? o - g.cs : o + (long long)(g.W - 1) * g.cs;
        oe = X < g.W - 1 ? o + g.cs : o - (long long)(g.W - 1) * g.cs;
        on = Y > 0 ? o - g.rs : o + (long long)(g.H - 1) * g.rs;
        os = Y < g.H - 1 ? o + g.rs : o - (long long)(g.H - 1) * g.rs;
        kw = !(X > 0 || px) ? NB_NONE : (X == 1 && mixed_low_d(wg.ax)) ? NB_DIRICHLET : state_kind(st[ow]);
        ke = !(X < g.W - 1 || px) ? NB_NONE : (X == g.W - 2 && mixed_high_d(wg.ax)) ? NB_DIRICHLET : state_kind(st[oe]);
        kn = !(Y > 0 || py) ? NB_NONE : (Y == 1 && mixed_low_d(wg.ay)) ? NB_DIRICHLET : state_kind(st[on]);
        ks = !(Y < g.H - 1 || py) ? NB_NONE : (Y == g.H - 2 && mixed_high_d(wg.ay)) ? NB_DIRICHLET : state_kind(st[os]);
    }
};

// ---- the volume family (sc_volume.hip, sc_volume_robust.hip): frames stacked along y, temporal neighbours
// row y of a work plane: its frame, its row of unknowns inside the frame
struct FrameRow {
    int t, yy;
    __device__ __forceinline__ FrameRow(const VolumeGeo &vg, int y) { t = y / vg.ny; yy = y - t * vg.ny; }
};

// the pixel across a temporal link: NB_NONE beyond either end of time
__device__ __forceinline__ int time_kind(const float *__restrict__ st, long long o, bool exists) { return exists ? state_kind(st[o]) : NB_NONE; }

// The two temporal neighbours of frame t's element at offset o: where they lie -- the wrap of periodic time included -- and whether
// they exist.  The link to the previous frame, its weight and its guidance value are stored at ob, those to the next frame at o.
struct TimeAround {
    long long ob, of;
    bool hb, hf;
    int jb = -1, jf = -1;      // the flow form: the two ends as work-plane indices (the links' own words), -1: none
    // wraps false (a launch under free time, known at compile time): one frame before and behind, nothing else is computed
    __device__ __forceinline__ TimeAround(const VolumeGeo &vg, int t, long long o, bool wraps)
    {
        if (!wraps) {
            ob = o - vg.fs; of = o + vg.fs;
            hb = t > 0; hf = t < vg.T - 1;
            return;
        }
        const long long wrap = (long long)(vg.T - 1) * vg.fs;
        ob = t > 0 ? o - vg.fs : o + wrap;
        of = t < vg.T - 1 ? o + vg.fs : o - wrap;
        hb = t > 0 || vg.periodic;
        hf = t < vg.T - 1 || vg.periodic;
    }
    // the flow form: the neighbours are the ends of the two links of work-plane element (x, y) of volume `member` of the launch (FlowLinks:
    // fwd, bwd), turned back into offsets of channel c under the call's layout; the wrap of time is in the indices
    __device__ __forceinline__ TimeAround(const PoissonGeo &g, const PcgGeo &wg, const VolumeGeo &vg, const FlowLinks &fl, int member, int c, int y, int x)
    {
        const long long lo = (long long)member * fl.stride + ((long long)y * wg.nx + x);
        const int n2 = wg.nx * vg.ny;
        jb = fl.bwd[lo]; jf = fl.fwd[lo];
        auto offset = [&](int j) {
            const int t = j / n2, r = j - t * n2, y = r / wg.nx, x = r - y * wg.nx;
            return (long long)(wg.x0 + x) * g.cs + (long long)(wg.y0 + y) * g.rs + (long long)c * g.chs + (long long)t * vg.fs;
        };
        hb = jb >= 0; hf = jf >= 0;
        ob = hb ? offset(jb) : 0; of = hf ? offset(jf) : 0;
    }
};
// the temporal neighbours of a launch's form: FLW through the link planes, else one frame before and behind
template <bool FLW, class Flow>
__device__ __forceinline__ TimeAround time_around(const PoissonGeo &g, const PcgGeo &wg, const VolumeGeo &vg, const Flow &fl, int member, int c, int y, int x,
                                                  int t, long long o, bool wraps)
{
    if constexpr (FLW) return TimeAround(g, wg, vg, fl, member, c, y, x);
    else return TimeAround(vg, t, o, wraps);
}
struct NoFlow {};      // the trailing argument of a launch form without link planes
// the weight of the temporal link stored at element e: tau * smooth_t, one rounded product (no array: tau)
__device__ __forceinline__ float time_link(const float *__restrict__ smt, long long e, float tau) { return smt ? rounded_product(tau, smt[e]) : tau; }

// a link's share of a magnitude: c t^2, the square rounded, then the product (c NULL: no multiply)
__device__ __forceinline__ float coupled_sq(const float *__restrict__ c, long long o, float t)
{
    const float q = rounded_product(t, t);
    return c ? rounded_product(c[o], q) : q;
}

} // namespace sc
