// sc_bounded.hip -- the bounded family's kernels (sc_hip_bounded*, sc_bounded_api.cpp) under the shared conjugate gradients (sc_pcg.h): the
// region family's system (sc_region.hip) under lower <= u <= upper at the UNKNOWN pixels, by the primal-dual active set method.  A round
// is a region solve in which the ACTIVE pixels -- those held at a bound -- are treated as KNOWN pixels whose value is that bound, so the
// iteration, the operator launch and the preconditioner are the region family's, untouched, and so is the set-up's condition: at every
// pixel of the work plane that is not a FREE UNKNOWN one, R = E = S = Dg = 0.  The device work of this file is the bookkeeping around it:
//     k_bounded_stats   the judgement of bound arrays: UNKNOWN pixels whose bound is NaN or whose lower > upper;
//     k_bounded_mark    r = L u - b of the original system and the set rule: the next set, how many pixels changed;
//     k_bounded_setup   the round's system: k_region_setup's planes under the set, the bound into the iterate, w-bar's sums;
//     k_bounded_out     the bound's bits at active pixels, the clamped iterate at free ones, data and boundary elsewhere.
// The set lives on two planes of floats (0 free, +1 upper-active, -1 lower-active; 0 at a pixel that is not UNKNOWN): the mark reads its
// neighbours' entries of the current set while it writes its own entry of the next, so no lane reads what another writes, and for the
// same reason the bound goes into the iterate in the set-up launch, which reads no neighbour's iterate.
// No tolerance rule: a pixel whose multiplier is smaller than the inner solves' error can alternate between the sets for ever (seen on
// noisy megapixel clones: one pixel per round).  Keeping a pixel that comes back to the bound it was released from ends that, but on
// the tests' inputs pixels do come back for good reason and holding them broke the KKT conditions at 1e-2: not done.  A lane owns one column of its
// band and walks down it; the neighbours left and right come from the cache lines its wave loads anyway -- no LDS, no barrier inside the
// walk, as in k_region_setup -- and the part's sums go through part_store: the wave's shuffles, four doubles of LDS, one fixed order.
// The launches run once per round beside some tens of iterations: what the call carries (lap, link arrays, a weight) is decided per
// launch on uniform values, not per instantiation.
#include "sc_region_device.h"

namespace sc {

namespace {

// a job's bounds at offset o: its array's element, or the call's scalar
struct Bounds {
    const float *__restrict__ lo, *__restrict__ hi;
    BoundScalars s;
    __device__ __forceinline__ Bounds(const BoundedJobs &t, int member, const BoundScalars &bs) : lo(t.lo[member]), hi(t.hi[member]), s(bs) {}
    __device__ __forceinline__ float lower(long long o) const { return lo ? lo[o] : s.lo; }
    __device__ __forceinline__ float upper(long long o) const { return hi ? hi[o] : s.hi; }
    // the value an entry a != 0 of a set plane holds its pixel at
    __device__ __forceinline__ float held(float a, long long o) const { return a > 0.f ? upper(o) : lower(o); }
};

// the work-plane elements of the four neighbours of unknown (x, y) of the plane that starts at `base` (meaningful where the neighbour
// is an unknown of the border kind: Around says so)
struct AroundIndex {
    size_t w, e, n, s;
    __device__ __forceinline__ AroundIndex(const PcgGeo &wg, size_t base, int x, int y)
    {
        const size_t row = base + (size_t)y * wg.nx;
        w = row + (x > 0 ? x - 1 : wg.nx - 1);
        e = row + (x < wg.nx - 1 ? x + 1 : 0);
        n = base + (size_t)(y > 0 ? y - 1 : wg.ny - 1) * wg.nx + x;
        s = base + (size_t)(y < wg.ny - 1 ? y + 1 : 0) * wg.nx + x;
    }
};

__global__ __launch_bounds__(WL) void k_bounded_stats(PoissonGeo g, PcgGeo wg, BoundedJobs t, BoundScalars bs, double *__restrict__ bad)
{
    __shared__ double ws[4];
    const PcgBand b(g, wg);
    const float *__restrict__ st = t.st[b.member];
    const Bounds bd(t, b.member, bs);
    double n = 0.0;
    if (b.x < wg.nx)
        for (int y = b.y0; y < b.y1; ++y) {
            const long long o = b.pixel(g, wg.x0 + b.x, wg.y0 + y);
            if (st[o] != 0.f) continue;
            const float lo = bd.lower(o), hi = bd.upper(o);
            if (!(lo <= hi)) n += 1.0;          // (NaN on either side fails the comparison)
        }
    part_store(n, ws, wg, bad);
}

__global__ __launch_bounds__(WL) void k_bounded_mark(PoissonGeo g, PcgGeo wg, BoundedJobs t, BoundScalars bs, int lap, const float *__restrict__ U,
                                                      const float *__restrict__ cur, float *__restrict__ next, double *__restrict__ sums)
{
    __shared__ double ws[2][4];
    const PcgBand b(g, wg);
    const PoissonJobDev &j = t.j[b.member];
    const float *__restrict__ w = t.w[b.member], *__restrict__ sx = t.sx[b.member], *__restrict__ sy = t.sy[b.member];
    const float *__restrict__ st = t.st[b.member];
    const Bounds bd(t, b.member, bs);
    const bool px = wg.ax == MIXED_PERIODIC, py = wg.ay == MIXED_PERIODIC;
    const size_t base = (size_t)b.p * wg.stride;
    double changed = 0.0, active = 0.0;
    if (b.x < wg.nx)
        for (int y = b.y0; y < b.y1; ++y) {
            const int X = wg.x0 + b.x, Y = wg.y0 + y;
            const long long o = b.pixel(g, X, Y);
            const size_t i = base + (size_t)y * wg.nx + b.x;
            float an = 0.f;
            if (st[o] == 0.f) {
                const Around a(g, wg, st, X, Y, o, px, py);
                const AroundIndex ix(wg, base, b.x, y);
                const float ao = cur[i], lo = bd.lower(o), hi = bd.upper(o);
                const float u = ao != 0.f ? bd.held(ao, o) : U[i];
                if (ao == 0.f) an = u > hi ? 1.f : u < lo ? -1.f : 0.f;
                else {
                    // u across the link to the neighbour of kind k at offset oq, work-plane element iq
                    auto across = [&](int k, long long oq, size_t iq) {
                        if (k == NB_DIRICHLET) return j.b[oq];
                        if (k == NB_KNOWN) return j.d[oq];
                        const float aq = cur[iq];
                        return aq != 0.f ? bd.held(aq, oq) : U[iq];
                    };
                    // s (u(q) - u) of a link that exists, its weight stored at element e of `arr`
                    auto term = [&](int k, const float *__restrict__ arr, long long e, long long oq, size_t iq) {
                        return k == NB_NONE ? 0.f : (arr ? arr[e] : 1.f) * (across(k, oq, iq) - u);
                    };
                    // the guidance term of a link: s g
                    auto flux = [&](int k, const float *__restrict__ arr, const float *__restrict__ gv, long long e) {
                        return k == NB_NONE ? 0.f : (arr ? arr[e] : 1.f) * gv[e];
                    };
                    float r = (term(a.kw, sx, a.ow, a.ow, ix.w) + term(a.ke, sx, o, a.oe, ix.e)) +
                              (term(a.kn, sy, a.on, a.on, ix.n) + term(a.ks, sy, o, a.os, ix.s));
                    if (w) r -= w[o] * (u - j.d[o]);
                    r -= lap ? j.lap[o] : (flux(a.ke, sx, j.gx, o) - flux(a.kw, sx, j.gx, a.ow)) + (flux(a.ks, sy, j.gy, o) - flux(a.kn, sy, j.gy, a.on));
                    an = ao > 0.f ? (r > 0.f ? 1.f : 0.f) : (r < 0.f ? -1.f : 0.f);
                }
                if (an != ao) changed += 1.0;
                if (an != 0.f) active += 1.0;
            }
            next[i] = an;
        }
    part_store(changed, ws[0], wg, sums, BOUNDED_SUMS, 0);
    part_store(active, ws[1], wg, sums, BOUNDED_SUMS, 1);
}

// k_region_setup's walk and its order of the right-hand side, the kind of an UNKNOWN neighbour that `set` holds at a bound being KNOWN
// and its value that bound; a pixel that `set` holds is no unknown of this round: everything 0 there
__global__ __launch_bounds__(WL) void k_bounded_setup(PoissonGeo g, PcgGeo wg, BoundedJobs t, BoundScalars bs, int lap, const float *__restrict__ set,
                                                       const float *__restrict__ prev, float *__restrict__ U, float *__restrict__ R,
                                                       float *__restrict__ E, float *__restrict__ S, float *__restrict__ Dg,
                                                       double *__restrict__ bb, double *__restrict__ sums)
{
    __shared__ double ws[4][4];
    const PcgBand b(g, wg);
    const PoissonJobDev &j = t.j[b.member];
    const float *__restrict__ w = t.w[b.member], *__restrict__ sx = t.sx[b.member], *__restrict__ sy = t.sy[b.member];
    const float *__restrict__ st = t.st[b.member];
    const Bounds bd(t, b.member, bs);
    const bool px = wg.ax == MIXED_PERIODIC, py = wg.ay == MIXED_PERIODIC;
    const size_t base = (size_t)b.p * wg.stride;
    double s = 0.0, sw = 0.0, uk = 0.0, nf = 0.0;
    if (b.x < wg.nx)
        for (int y = b.y0; y < b.y1; ++y) {
            const int X = wg.x0 + b.x, Y = wg.y0 + y;
            const long long o = b.pixel(g, X, Y);
            const size_t i = base + (size_t)y * wg.nx + b.x;
            float v = 0.f, e = 0.f, so = 0.f, dg = 0.f;
            if (st[o] == 0.f) {
                const float an = set[i], ap = prev[i];
                if (an != 0.f || ap != 0.f) U[i] = bd.held(an != 0.f ? an : ap, o);
                if (an == 0.f) {
                    const Around a(g, wg, st, X, Y, o, px, py);
                    const AroundIndex ix(wg, base, b.x, y);
                    // the neighbour's kind under the set, and the value it is held at: data's, or its bound
                    float vw = 0.f, vn = 0.f, ve = 0.f, vs = 0.f;
                    auto under = [&](int k, long long oq, size_t iq, float &val) {
                        if (k == NB_KNOWN) val = j.d[oq];
                        if (k != NB_UNKNOWN) return k;
                        const float aq = set[iq];
                        if (aq == 0.f) return (int)NB_UNKNOWN;
                        val = bd.held(aq, oq);
                        return (int)NB_KNOWN;
                    };
                    const int kw = under(a.kw, a.ow, ix.w, vw), kn = under(a.kn, a.on, ix.n, vn);
                    const int ke = under(a.ke, a.oe, ix.e, ve), ks = under(a.ks, a.os, ix.s, vs);
                    const float lw = kw == NB_NONE ? 0.f : sx ? sx[a.ow] : 1.f, le = ke == NB_NONE ? 0.f : sx ? sx[o] : 1.f;
                    const float ln = kn == NB_NONE ? 0.f : sy ? sy[a.on] : 1.f, ls = ks == NB_NONE ? 0.f : sy ? sy[o] : 1.f;
                    if (lap) v = j.lap[o];
                    else {
                        const float ta = ke == NB_NONE ? 0.f : rounded_product(le, j.gx[o]);
                        const float tb = kw == NB_NONE ? 0.f : rounded_product(lw, j.gx[a.ow]);
                        const float tc = ks == NB_NONE ? 0.f : rounded_product(ls, j.gy[o]);
                        const float td = kn == NB_NONE ? 0.f : rounded_product(ln, j.gy[a.on]);
                        v = (ta - tb) + (tc - td);
                    }
                    float wv = 0.f;
                    if (w) {
                        wv = w[o];
                        v = screened_rhs(v, wv, j.d[o]);
                    }
                    if (kw == NB_DIRICHLET) v -= rounded_product(lw, j.b[a.ow]);
                    if (kn == NB_DIRICHLET) v -= rounded_product(ln, j.b[a.on]);
                    if (ke == NB_DIRICHLET) v -= rounded_product(le, j.b[a.oe]);
                    if (ks == NB_DIRICHLET) v -= rounded_product(ls, j.b[a.os]);
                    if (kw == NB_KNOWN) { v -= rounded_product(lw, vw); uk += (double)lw; }
                    if (kn == NB_KNOWN) { v -= rounded_product(ln, vn); uk += (double)ln; }
                    if (ke == NB_KNOWN) { v -= rounded_product(le, ve); uk += (double)le; }
                    if (ks == NB_KNOWN) { v -= rounded_product(ls, vs); uk += (double)ls; }
                    e = ke == NB_UNKNOWN ? le : 0.f;
                    so = ks == NB_UNKNOWN ? ls : 0.f;
                    dg = ((lw + le) + (ln + ls)) + wv;
                    sw += (double)wv;
                    nf += 1.0;
                }
            }
            R[i] = v;
            E[i] = e;
            S[i] = so;
            Dg[i] = dg;
            s += (double)v * (double)v;
        }
    part_store(s, ws[0], wg, bb);
    part_store(sw, ws[1], wg, sums, BOUNDED_SUMS, 0);
    part_store(uk, ws[2], wg, sums, BOUNDED_SUMS, 1);
    part_store(nf, ws[3], wg, sums, BOUNDED_SUMS, 2);
}

// k_region_out's walk over every element the layout names
__global__ __launch_bounds__(WL) void k_bounded_out(PoissonGeo g, PcgGeo wg, BoundedJobs t, BoundScalars bs, const float *__restrict__ U,
                                                     const float *__restrict__ set)
{
    const int p = (int)blockIdx.z, member = p / g.C, c = p - member * g.C, x = (int)blockIdx.x * WL + (int)threadIdx.x, y = (int)blockIdx.y;
    if (x >= g.W) return;
    const PoissonJobDev &j = t.j[member];
    const long long o = (long long)x * g.cs + (long long)y * g.rs + (long long)c * g.chs;
    const int ux = x - wg.x0, uy = y - wg.y0;
    if (!(ux >= 0 && ux < wg.nx && uy >= 0 && uy < wg.ny)) { j.out[o] = j.b[o]; return; }
    if (t.st[member][o] != 0.f) { j.out[o] = j.d[o]; return; }
    const Bounds bd(t, member, bs);
    const size_t i = (size_t)p * wg.stride + (size_t)uy * wg.nx + ux;
    const float a = set[i];
    j.out[o] = a != 0.f ? bd.held(a, o) : fminf(fmaxf(U[i], bd.lower(o)), bd.upper(o));
}

} // namespace

void launch_bounded_stats(const PoissonGeo &g, const PcgGeo &wg, const BoundScalars &bs, const PoissonJobDev *jobs, const SideArrays *sides, int m,
                          double *bad, hipStream_t s)
{
    for_side_tables<BoundedJobs>(jobs, sides, m, [&](const BoundedJobs &t, int i0, int cnt) {
        hipLaunchKernelGGL(k_bounded_stats, dim3((unsigned)wg.cg, (unsigned)wg.bands, (unsigned)(g.C * cnt)), dim3(WL), 0, s, g, wg, t, bs,
                           bad + (size_t)g.C * i0 * PCG_PARTS);
    });
}

void launch_bounded_mark(const PoissonGeo &g, const PcgGeo &wg, bool lap, const BoundScalars &bs, const PoissonJobDev *jobs, const SideArrays *sides,
                         int m, const float *U, const float *cur, float *next, double *sums, hipStream_t s)
{
    for_side_tables<BoundedJobs>(jobs, sides, m, [&](const BoundedJobs &t, int i0, int cnt) {
        const size_t o = (size_t)g.C * i0 * wg.stride;
        hipLaunchKernelGGL(k_bounded_mark, dim3((unsigned)wg.cg, (unsigned)wg.bands, (unsigned)(g.C * cnt)), dim3(WL), 0, s, g, wg, t, bs, lap ? 1 : 0,
                           U + o, cur + o, next + o, sums + (size_t)g.C * i0 * PCG_PARTS * BOUNDED_SUMS);
    });
}

void launch_bounded_setup(const PoissonGeo &g, const PcgGeo &wg, bool lap, const BoundScalars &bs, const PoissonJobDev *jobs, const SideArrays *sides,
                          int m, const float *set, const float *prev, float *U, float *R, float *E, float *S, float *Dg, double *bb, double *sums,
                          hipStream_t s)
{
    for_side_tables<BoundedJobs>(jobs, sides, m, [&](const BoundedJobs &t, int i0, int cnt) {
        const size_t o = (size_t)g.C * i0 * wg.stride, po = (size_t)g.C * i0 * PCG_PARTS;
        hipLaunchKernelGGL(k_bounded_setup, dim3((unsigned)wg.cg, (unsigned)wg.bands, (unsigned)(g.C * cnt)), dim3(WL), 0, s, g, wg, t, bs, lap ? 1 : 0,
                           set + o, prev + o, U + o, R + o, E + o, S + o, Dg + o, bb + po, sums + po * BOUNDED_SUMS);
    });
}

void launch_bounded_out(const PoissonGeo &g, const PcgGeo &wg, const BoundScalars &bs, const PoissonJobDev *jobs, const SideArrays *sides, int m,
                        const float *U, const float *set, hipStream_t s)
{
    for_side_tables<BoundedJobs>(jobs, sides, m, [&](const BoundedJobs &t, int i0, int cnt) {
        const size_t o = (size_t)g.C * i0 * wg.stride;
        hipLaunchKernelGGL(k_bounded_out, dim3((unsigned)((g.W + WL - 1) / WL), (unsigned)g.H, (unsigned)(g.C * cnt)), dim3(WL), 0, s, g, wg, t, bs,
                           U + o, set + o);
    });
}

} // namespace sc
