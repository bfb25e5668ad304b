// sc_region_device.h -- what the kernels of the region and the volume family share (sc_region.hip, sc_volume.hip): a state element's
// meaning and the four spatial neighbours of a pixel as the region call sees them.
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

} // namespace sc
