// sc_region.hip -- the region family's kernels (sc_hip_region*, sc_region_api.cpp) under the shared conjugate gradients (sc_pcg.h): the WLS
// family's system (sc_wls.hip) on a domain of any shape.  One more array, state, says of every pixel the border kind calls an unknown
// whether it is solved for (SC_REGION_UNKNOWN, 0), fixed at data's value (SC_REGION_KNOWN, 1) or not there at all (SC_REGION_OUTSIDE,
// 2).  Seen from an UNKNOWN pixel p, the neighbour q across one of its four links is
//     UNKNOWN        the link couples two unknowns: s on p's diagonal, and E or S where q is the next column or row;
//     KNOWN          as a Dirichlet pixel: s on p's diagonal, s * data(q) off the right-hand side;
//     on a Dirichlet line of the border kind: s on p's diagonal, s * boundary(q) off the right-hand side (state is not consulted there);
//     OUTSIDE, or beyond a free end: no link -- nothing is read, nothing counts.
// A link between two pixels of which none is UNKNOWN is dead.  A link is LIVE IN THE REGION when it is live in the WLS sense, neither
// end is OUTSIDE and at least one end is UNKNOWN; link weights and guidance values are read at those links only.
//
// The iteration is the WLS family's, untouched: k_pcg_op with WlsCoef over the whole nx x ny work plane, the shared launches of
// sc_pcg.hip, the direct solve of the whole rectangle as the preconditioner.  What makes that exact is the set-up's one condition:
//     at every pixel of the work plane that is not UNKNOWN,  R = E = S = Dg = 0,
// and E, S are 0 as well on a link from an UNKNOWN pixel to one that is not (E(p) is also q's west coefficient).  Then (L v)(q) = 0 at
// such a pixel q for every finite v -- all five coefficients of its row are 0 -- and at an UNKNOWN pixel (L v)(p) reads v at UNKNOWN
// pixels only.  By induction r and q = L p stay exactly 0 at every pixel that is not UNKNOWN, so every dot product (p . q, r . r,
// r . z) is the sum over the UNKNOWN pixels alone, alpha and beta are those of conjugate gradients on the UNKNOWN pixels preconditioned
// by P M^-1 P^T (P: the restriction to them), and no projection launch is needed.  u and p do take values at the other pixels -- u0 =
// M^-1 b and z = M^-1 r fill the whole rectangle -- but those values are multiplied by coefficients that are 0 and so never reach an
// UNKNOWN pixel, a residual or a dot product; they only have to stay finite (0 * inf is not 0), which they do as sums of finite
// products.  The output launch never reads them: it writes U at UNKNOWN pixels, data's bits at KNOWN and OUTSIDE pixels and
// boundary's bits on the Dirichlet lines.
#include "sc_region_device.h"
#include <cmath>
#include <vector>

namespace sc {

namespace {

__device__ __forceinline__ bool bad_link(float v) { return !(v > 0.f) || v > 3.4028234e38f; }

// Per plane and part (REGION_STATS doubles): the sum of w over the UNKNOWN pixels | how many of those w are invalid | the sum of the
// links live in the region, each counted once -- by its low end (the last pixel of a periodic axis owns the wrapping link), or by its
// UNKNOWN end where the other lies on a low Dirichlet line, as k_wls_stats counts -- | how many of them are invalid | the UNKNOWN
// pixels | the sum of the UNKNOWN - KNOWN links | the state elements that are not exactly 0, 1 or 2 | the links live in the region.
// t.w NULL: no data term; t.sx NULL: every link is 1.
__global__ __launch_bounds__(WL) void k_region_stats(PoissonGeo g, PcgGeo wg, RegionJobs t, double *__restrict__ stats)
{
    __shared__ double ws[REGION_STATS][4];
    const PcgBand b(g, wg);
    const float *__restrict__ w = t.w[b.member], *__restrict__ sx = t.sx[b.member], *__restrict__ sy = t.sy[b.member];
    const float *__restrict__ st = t.st[b.member];
    const bool px = wg.ax == MIXED_PERIODIC, py = wg.ay == MIXED_PERIODIC;
    double sw = 0.0, bw = 0.0, ss = 0.0, bs = 0.0, nu = 0.0, uk = 0.0, bst = 0.0, nl = 0.0;
    if (b.x < wg.nx)
        for (int y = b.y0; y < b.y1; ++y) {
            const int X = wg.x0 + b.x, Y = wg.y0 + y;
            const long long o = b.pixel(g, X, Y);
            const float sv = st[o];
            if (!(sv == 0.f || sv == 1.f || sv == 2.f)) { bst += 1.0; continue; }
            const int kp = state_kind(sv);
            if (kp == NB_NONE) continue;
            const Around a(g, wg, st, X, Y, o, px, py);
            if (kp == NB_UNKNOWN) {
                nu += 1.0;
                if (w) {
                    const float v = w[o];
                    if (!(v >= 0.f) || v > 3.4028234e38f) bw += 1.0;
                    sw += (double)v;
                }
            }
            // the link towards a neighbour of kind kq, stored at element e of its array: live in the region?
            auto link = [&](int kq, const float *__restrict__ arr, long long e) {
                if (kq == NB_NONE || (kp != NB_UNKNOWN && kq != NB_UNKNOWN)) return;
                const float s = arr ? arr[e] : 1.f;
                if (bad_link(s)) bs += 1.0;
                ss += (double)s;
                nl += 1.0;
                if (kp + kq == NB_KNOWN) uk += (double)s;      // one end UNKNOWN (0), the other KNOWN (1)
            };
            link(a.ke, sx, o);
            link(a.ks, sy, o);
            if (a.kw == NB_DIRICHLET) link(a.kw, sx, a.ow);
            if (a.kn == NB_DIRICHLET) link(a.kn, sy, a.on);
        }
    part_store(sw, ws[0], wg, stats, REGION_STATS, 0);
    part_store(bw, ws[1], wg, stats, REGION_STATS, 1);
    part_store(ss, ws[2], wg, stats, REGION_STATS, 2);
    part_store(bs, ws[3], wg, stats, REGION_STATS, 3);
    part_store(nu, ws[4], wg, stats, REGION_STATS, 4);
    part_store(uk, ws[5], wg, stats, REGION_STATS, 5);
    part_store(bst, ws[6], wg, stats, REGION_STATS, 6);
    part_store(nl, ws[7], wg, stats, REGION_STATS, 7);
}

// k_wls_setup's walk.  b in the order the header states: (a - b) + (c - d) of separately rounded products s g (a link that is not live
// in the region counts 0 and is not read), then - w d as screened_rhs (NOW: no data term, w and data are not read here), then the
// Dirichlet lines' terms s * boundary, west, north, east, south, then the KNOWN neighbours' terms s * data likewise, each product
// rounded on its own and subtracted in turn.  ONE: every link is 1, t.sx and t.sy are not read.  Everything is 0 at a pixel that is
// not UNKNOWN, and E, S are kept only where both ends of the link are UNKNOWN (the header comment's condition).
template <bool LAP, bool ONE, bool NOW>
__global__ __launch_bounds__(WL) void k_region_setup(PoissonGeo g, PcgGeo wg, RegionJobs t, float *__restrict__ R, float *__restrict__ E,
                                                      float *__restrict__ S, float *__restrict__ Dg, double *__restrict__ bb)
{
    __shared__ double ws[4];
    const PcgBand bd(g, wg);
    const PoissonJobDev &j = t.j[bd.member];
    const float *__restrict__ w = t.w[bd.member], *__restrict__ sx = t.sx[bd.member], *__restrict__ sy = t.sy[bd.member];
    const float *__restrict__ st = t.st[bd.member];
    const bool px = wg.ax == MIXED_PERIODIC, py = wg.ay == MIXED_PERIODIC;
    double s = 0.0;
    if (bd.x < wg.nx)
        for (int y = bd.y0; y < bd.y1; ++y) {
            const int X = wg.x0 + bd.x, Y = wg.y0 + y;
            const long long o = bd.pixel(g, X, Y);
            float v = 0.f, e = 0.f, so = 0.f, dg = 0.f;
            if (st[o] == 0.f) {
                const Around a(g, wg, st, X, Y, o, px, py);
                const float lw = a.kw == NB_NONE ? 0.f : ONE ? 1.f : sx[a.ow], le = a.ke == NB_NONE ? 0.f : ONE ? 1.f : sx[o];
                const float ln = a.kn == NB_NONE ? 0.f : ONE ? 1.f : sy[a.on], ls = a.ks == NB_NONE ? 0.f : ONE ? 1.f : sy[o];
                if (LAP) v = j.lap[o];
                else {
                    const float ta = a.ke == NB_NONE ? 0.f : rounded_product(le, j.gx[o]);
                    const float tb = a.kw == NB_NONE ? 0.f : rounded_product(lw, j.gx[a.ow]);
                    const float tc = a.ks == NB_NONE ? 0.f : rounded_product(ls, j.gy[o]);
                    const float td = a.kn == NB_NONE ? 0.f : rounded_product(ln, j.gy[a.on]);
                    v = (ta - tb) + (tc - td);
                }
                float wv = 0.f;
                if (!NOW) {
                    wv = w[o];
                    v = screened_rhs(v, wv, j.d[o]);
                }
                if (a.kw == NB_DIRICHLET) v -= rounded_product(lw, j.b[a.ow]);
                if (a.kn == NB_DIRICHLET) v -= rounded_product(ln, j.b[a.on]);
                if (a.ke == NB_DIRICHLET) v -= rounded_product(le, j.b[a.oe]);
                if (a.ks == NB_DIRICHLET) v -= rounded_product(ls, j.b[a.os]);
                if (a.kw == NB_KNOWN) v -= rounded_product(lw, j.d[a.ow]);
                if (a.kn == NB_KNOWN) v -= rounded_product(ln, j.d[a.on]);
                if (a.ke == NB_KNOWN) v -= rounded_product(le, j.d[a.oe]);
                if (a.ks == NB_KNOWN) v -= rounded_product(ls, j.d[a.os]);
                e = a.ke == NB_UNKNOWN ? le : 0.f;
                so = a.ks == NB_UNKNOWN ? ls : 0.f;
                dg = ((lw + le) + (ln + ls)) + wv;
            }
            const size_t i = (size_t)bd.p * wg.stride + (size_t)y * wg.nx + bd.x;
            R[i] = v;
            E[i] = e;
            S[i] = so;
            Dg[i] = dg;
            s += (double)v * (double)v;
        }
    part_store(s, ws, wg, bb);
}

// every element the layout names: U at UNKNOWN pixels, data's bits at KNOWN and OUTSIDE pixels, boundary's bits on the Dirichlet lines
// (out may be data or boundary: the same value again)
__global__ __launch_bounds__(WL) void k_region_out(PoissonGeo g, PcgGeo wg, RegionJobs t, const float *__restrict__ U)
{
    const int p = (int)blockIdx.z, member = p / g.C, c = p - member * g.C, x = (int)blockIdx.x * WL + (int)threadIdx.x, y = (int)blockIdx.y;
    if (x >= g.W) return;
    const PoissonJobDev &j = t.j[member];
    const long long o = (long long)x * g.cs + (long long)y * g.rs + (long long)c * g.chs;
    const int ux = x - wg.x0, uy = y - wg.y0;
    if (ux >= 0 && ux < wg.nx && uy >= 0 && uy < wg.ny)
        j.out[o] = t.st[member][o] == 0.f ? U[(size_t)p * wg.stride + (size_t)uy * wg.nx + ux] : j.d[o];
    else j.out[o] = j.b[o];
}

template <bool LAP, bool ONE> void setup_form(bool now, dim3 grid, hipStream_t s, const PoissonGeo &g, const PcgGeo &wg, const RegionJobs &t, float *R,
                                              float *E, float *S, float *Dg, double *bb)
{
    if (now) hipLaunchKernelGGL((k_region_setup<LAP, ONE, true>), grid, dim3(WL), 0, s, g, wg, t, R, E, S, Dg, bb);
    else hipLaunchKernelGGL((k_region_setup<LAP, ONE, false>), grid, dim3(WL), 0, s, g, wg, t, R, E, S, Dg, bb);
}

} // namespace

void launch_region_stats(const PoissonGeo &g, const PcgGeo &wg, const PoissonJobDev *jobs, const SideArrays *sides, int m, double *stats, hipStream_t s)
{
    for_side_tables<RegionJobs>(jobs, sides, m, [&](const RegionJobs &t, int i0, int cnt) {
        hipLaunchKernelGGL(k_region_stats, dim3((unsigned)wg.cg, (unsigned)wg.bands, (unsigned)(g.C * cnt)), dim3(WL), 0, s, g, wg, t,
                           stats + (size_t)g.C * i0 * PCG_PARTS * REGION_STATS);
    });
}

void launch_region_setup(const PoissonGeo &g, const PcgGeo &wg, bool lap, const PoissonJobDev *jobs, const SideArrays *sides, int m, float *R, float *E,
                         float *S, float *Dg, double *bb, hipStream_t s)
{
    for_side_tables<RegionJobs>(jobs, sides, m, [&](const RegionJobs &t, int i0, int cnt) {
        const dim3 grid((unsigned)wg.cg, (unsigned)wg.bands, (unsigned)(g.C * cnt));
        const size_t o = (size_t)g.C * i0 * wg.stride;
        double *b = bb + (size_t)g.C * i0 * PCG_PARTS;
        const bool one = !t.sx[0], now = !t.w[0];
        if (lap && one) setup_form<true, true>(now, grid, s, g, wg, t, R + o, E + o, S + o, Dg + o, b);
        else if (lap) setup_form<true, false>(now, grid, s, g, wg, t, R + o, E + o, S + o, Dg + o, b);
        else if (one) setup_form<false, true>(now, grid, s, g, wg, t, R + o, E + o, S + o, Dg + o, b);
        else setup_form<false, false>(now, grid, s, g, wg, t, R + o, E + o, S + o, Dg + o, b);
    });
}

void launch_region_out(const PoissonGeo &g, const PcgGeo &wg, const PoissonJobDev *jobs, const SideArrays *sides, int m, const float *U, hipStream_t s)
{
    for_side_tables<RegionJobs>(jobs, sides, m, [&](const RegionJobs &t, int i0, int cnt) {
        hipLaunchKernelGGL(k_region_out, dim3((unsigned)((g.W + WL - 1) / WL), (unsigned)g.H, (unsigned)(g.C * cnt)), dim3(WL), 0, s, g, wg, t,
                           U + (size_t)g.C * i0 * wg.stride);
    });
}

} // namespace sc
