// sc_volume.hip -- the volume families' kernels (sc_hip_volume*, sc_hip_volume_wls*; sc_volume_api.cpp) under the shared conjugate
// gradients (sc_pcg.h): the region family's system (sc_region.hip) on a stack of T frames, plus temporal links between pixel q of frame t
// and pixel q of frame t + 1.  A spatial link weighs sx / sy as in the region family (no arrays: 1), a temporal one lt = tau * smooth_t,
// one rounded float32 product (no array: tau).  A temporal link follows the spatial rule: it is live when neither end is OUTSIDE and at
// least one end is UNKNOWN; a KNOWN temporal neighbour adds lt to the diagonal of its unknown end and lt * data to the right-hand side.
// The two ends of time are free, or -- periodic time -- frame T - 1 is linked to frame 0 by a link like any other, stored with frame
// T - 1.  Pixels on the border kind's Dirichlet lines are no part of a work plane and have no temporal links.
//
// Work planes: one per (volume, channel), the T frames stacked along y -- nx x (T ny), frame t at rows [t ny, (t + 1) ny).  So the
// element-wise launches, the partial sums and the stop rule of sc_pcg.hip see one system per (volume, channel) and need not know about
// frames; the launches here do.  Coefficient planes: E, S, Dg as the region family's (S is 0 in a frame's last row unless y wraps, and
// then joins the frame's own first row) and F, the link to the next frame (in the last frame's rows: the wrapping link, 0 with free
// time).  As in the region family every coefficient and the right-hand side are 0 at a pixel that is not UNKNOWN, and E, S, F are kept
// only where both ends are UNKNOWN, which makes the iteration that of the UNKNOWN pixels alone (sc_region.hip: why).
//
// The preconditioner M = s-bar A - w-bar + tau-bar A_t (A_t: the second difference along the frames, free-ended or circulant) is
// inverted exactly: an orthonormal table product along the frames (k_volume_dct; the DCT-II, or the Hartley table under periodic time)
// turns it into T two-dimensional screened problems, mode k shifted by (w-bar + tau-bar mu_k) / s-bar, which one direct_jobs_solve with
// a shift per plane solves; the transposed product goes back.  The factor 1 / s-bar that is left goes once on u0 (PcgOperator::scale_start).
#include "sc_region_device.h"
#include <cmath>
#include <vector>

namespace sc {

namespace {

__device__ __forceinline__ bool bad_link(float v) { return !(v > 0.f) || v > 3.4028234e38f; }

// Per plane and part (VOLUME_STATS doubles): the sum of w over the UNKNOWN pixels | how many of those w are invalid | the UNKNOWN
// pixels | the sum of the UNKNOWN - KNOWN links' weights, each counted once by its low end (k_region_stats' rule; the earlier frame owns
// a temporal link, frame T - 1 the wrapping one) | the state elements that are not exactly 0, 1 or 2 | the sum of the spatial links
// live in the region, each counted once as k_region_stats counts them | how many | how many of them are invalid | the sum of the live
// temporal links lt | how many | how many of them are invalid (smooth_t or its product with tau not finite or not > 0).
// t.w NULL: no data term; t.sx NULL: every spatial link 1; t.smt NULL: every temporal link tau.  LNK false (a call without any link
// array under free time -- sc_hip_volume's): the links are not looked at, an UNKNOWN - KNOWN link counts 1 or tau, time does not wrap,
// and a part is the first VOLUME_STATS_PLAIN fields alone; true: every other call, VOLUME_STATS fields per part.
// FLW (the flow call; LNK with it): the temporal neighbours come from the link planes fl.fwd / fl.bwd, a part is VOLUME_FLOW_STATS fields,
// the last one the pixel's flow components that are finite and not whole numbers (fa.fx, fa.fy; frames that have a flow only).
template <bool LNK, bool FLW = false>
__global__ __launch_bounds__(WL) void k_volume_stats(PoissonGeo g, PcgGeo wg, VolumeGeo vg, VolumeJobs t, double *__restrict__ stats,
                                                      std::conditional_t<FLW, FlowLinks, NoFlow> fl, std::conditional_t<FLW, FlowArrays, NoFlow> fa)
{
    constexpr int NS = FLW ? VOLUME_FLOW_STATS : LNK ? VOLUME_STATS : VOLUME_STATS_PLAIN;
    __shared__ double ws[NS][4];
    const PcgBand b(g, wg);
    const float *__restrict__ w = t.w[b.member], *__restrict__ st = t.st[b.member];
    const float *__restrict__ sx = t.sx[b.member], *__restrict__ sy = t.sy[b.member], *__restrict__ smt = t.smt[b.member];
    const bool px = wg.ax == MIXED_PERIODIC, py = wg.ay == MIXED_PERIODIC;
    double sw = 0.0, bw = 0.0, nu = 0.0, uk = 0.0, bst = 0.0, ss = 0.0, ns = 0.0, bs = 0.0, sl = 0.0, nt = 0.0, bt = 0.0, bfl = 0.0;
    if (b.x < wg.nx)
        for (int y = b.y0; y < b.y1; ++y) {
            const FrameRow fr(vg, y);
            const int X = wg.x0 + b.x, Y = wg.y0 + fr.yy;
            const long long o = b.pixel(g, X, Y) + (long long)fr.t * vg.fs;
            if constexpr (FLW) {
                if (fr.t < vg.T - 1 || vg.periodic) {
                    const size_t e = ((size_t)fr.t * g.H + Y) * g.W + X;
                    const float vx = fa.fx[b.member][e], vy = fa.fy[b.member][e];
                    if (vx - vx == 0.f && vx != rintf(vx)) bfl += 1.0;
                    if (vy - vy == 0.f && vy != rintf(vy)) bfl += 1.0;
                }
            }
            const float sv = st[o];
            if (!(sv == 0.f || sv == 1.f || sv == 2.f)) { bst += 1.0; continue; }
            const int kp = state_kind(sv);
            if (kp == NB_NONE) continue;
            if (kp == NB_UNKNOWN) {
                nu += 1.0;
                if (w) {
                    const float v = w[o];
                    if (!(v >= 0.f) || v > 3.4028234e38f) bw += 1.0;
                    sw += (double)v;
                }
            }
            const Around a(g, wg, st, X, Y, o, px, py);
            // the spatial link towards a neighbour of kind kq, stored at element e of its array: live in the region?
            auto link = [&](int kq, const float *__restrict__ arr, long long e) {
                if (kq == NB_NONE || (kp != NB_UNKNOWN && kq != NB_UNKNOWN)) return;
                const float s = arr ? arr[e] : 1.f;
                if (bad_link(s)) bs += 1.0;
                ss += (double)s;
                ns += 1.0;
                if (kp + kq == NB_KNOWN) uk += (double)s;      // one end UNKNOWN (0), the other KNOWN (1)
            };
            const TimeAround ta = time_around<FLW>(g, wg, vg, fl, b.member, b.c, y, b.x, fr.t, o, LNK);
            const int kf = time_kind(st, ta.of, ta.hf);
            if (!LNK) {
                if (kp + a.ke == NB_KNOWN) uk += 1.0;
                if (kp + a.ks == NB_KNOWN) uk += 1.0;
                if (kp + kf == NB_KNOWN) uk += (double)vg.tau;
                continue;
            }
            link(a.ke, sx, o);
            link(a.ks, sy, o);
            if (a.kw == NB_DIRICHLET) link(a.kw, sx, a.ow);
            if (a.kn == NB_DIRICHLET) link(a.kn, sy, a.on);
            if (kf != NB_NONE && (kp == NB_UNKNOWN || kf == NB_UNKNOWN)) {
                const float lt = time_link(smt, o, vg.tau);
                if (bad_link(lt) || (smt && bad_link(smt[o]))) bt += 1.0;
                sl += (double)lt;
                nt += 1.0;
                if (kp + kf == NB_KNOWN) uk += (double)lt;
            }
        }
    part_store(sw, ws[0], wg, stats, NS, 0);
    part_store(bw, ws[1], wg, stats, NS, 1);
    part_store(nu, ws[2], wg, stats, NS, 2);
    part_store(uk, ws[3], wg, stats, NS, 3);
    part_store(bst, ws[4], wg, stats, NS, 4);
    if constexpr (LNK) {
        part_store(ss, ws[5], wg, stats, NS, 5);
        part_store(ns, ws[6], wg, stats, NS, 6);
        part_store(bs, ws[7], wg, stats, NS, 7);
        part_store(sl, ws[8], wg, stats, NS, 8);
        part_store(nt, ws[9], wg, stats, NS, 9);
        part_store(bt, ws[10], wg, stats, NS, 10);
    }
    if constexpr (FLW) part_store(bfl, ws[11], wg, stats, NS, 11);
}

// k_region_setup's walk, frame by frame, and the temporal part.  b in the order the header states: the region call's guidance sum
// (a - b) + (c - d) of the rounded products s * g; + (e - f), e = lt * gt_t where the link to the next frame is live, f = lt * gt_(t-1)
// where the one to the previous frame is (gt NULL: zeros; a link that is not live counts 0 and is not read); - w d (NOW: no data term);
// the Dirichlet lines' terms, west, north, east, south; the KNOWN spatial neighbours' likewise; the KNOWN temporal neighbours' lt *
// data, previous frame, then next -- every product rounded on its own and subtracted in turn.  LAP: lap is the whole right-hand side
// before the folded terms, gx, gy, gt are not read.  LNK false (a call without any link array under free time): every spatial link is 1, every
// temporal one tau, no link array is looked at and time does not wrap -- the set-up sc_hip_volume always had; true: each array is a uniform pointer test.  1 * g = g and tau * 1 = tau exactly, so arrays of
// 1.0f give the bytes of no arrays.
// FLW (the flow call; LNK with it): "the next frame" is the end of the link this pixel holds, "the previous frame" the source of the link
// that arrives at it (fl.fwd, fl.bwd) -- whose lt and gt are stored at that source --, F the held link where both ends are UNKNOWN.
template <bool LAP, bool NOW, bool LNK, bool FLW = false>
__global__ __launch_bounds__(WL) void k_volume_setup(PoissonGeo g, PcgGeo wg, VolumeGeo vg, VolumeJobs t, float *__restrict__ R, float *__restrict__ E,
                                                      float *__restrict__ S, float *__restrict__ F, float *__restrict__ Dg, double *__restrict__ bb,
                                                      std::conditional_t<FLW, FlowLinks, NoFlow> fl)
{
    __shared__ double ws[4];
    const PcgBand bd(g, wg);
    const PoissonJobDev &j = t.j[bd.member];
    const float *__restrict__ w = t.w[bd.member], *__restrict__ st = t.st[bd.member], *__restrict__ gt = t.gt[bd.member];
    const float *__restrict__ sx = t.sx[bd.member], *__restrict__ sy = t.sy[bd.member], *__restrict__ smt = t.smt[bd.member];
    const bool px = wg.ax == MIXED_PERIODIC, py = wg.ay == MIXED_PERIODIC;
    const float tau = vg.tau;
    double s = 0.0;
    if (bd.x < wg.nx)
        for (int y = bd.y0; y < bd.y1; ++y) {
            const FrameRow fr(vg, y);
            const int X = wg.x0 + bd.x, Y = wg.y0 + fr.yy;
            const long long o = bd.pixel(g, X, Y) + (long long)fr.t * vg.fs;
            float v = 0.f, e = 0.f, so = 0.f, f = 0.f, dg = 0.f;
            if (st[o] == 0.f) {
                const Around a(g, wg, st, X, Y, o, px, py);
                const TimeAround ta = time_around<FLW>(g, wg, vg, fl, bd.member, bd.c, y, bd.x, fr.t, o, LNK);
                const int kb = time_kind(st, ta.ob, ta.hb), kf = time_kind(st, ta.of, ta.hf);
                const float lw = a.kw == NB_NONE ? 0.f : LNK && sx ? sx[a.ow] : 1.f, le = a.ke == NB_NONE ? 0.f : LNK && sx ? sx[o] : 1.f;
                const float ln = a.kn == NB_NONE ? 0.f : LNK && sy ? sy[a.on] : 1.f, ls = a.ks == NB_NONE ? 0.f : LNK && sy ? sy[o] : 1.f;
                const float lb = kb == NB_NONE ? 0.f : LNK ? time_link(smt, ta.ob, tau) : tau, lf = kf == NB_NONE ? 0.f : LNK ? time_link(smt, o, tau) : tau;
                if (LAP) v = j.lap[o];
                else {
                    const float pa = a.ke == NB_NONE ? 0.f : rounded_product(le, j.gx[o]);
                    const float pb = a.kw == NB_NONE ? 0.f : rounded_product(lw, j.gx[a.ow]);
                    const float pc = a.ks == NB_NONE ? 0.f : rounded_product(ls, j.gy[o]);
                    const float pd = a.kn == NB_NONE ? 0.f : rounded_product(ln, j.gy[a.on]);
                    const float pe = (kf == NB_NONE || !gt) ? 0.f : rounded_product(lf, gt[o]);
                    const float pf = (kb == NB_NONE || !gt) ? 0.f : rounded_product(lb, gt[ta.ob]);
                    v = ((pa - pb) + (pc - pd)) + (pe - pf);
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
                if (kb == NB_KNOWN) v -= rounded_product(lb, j.d[ta.ob]);
                if (kf == NB_KNOWN) v -= rounded_product(lf, j.d[ta.of]);
                e = a.ke == NB_UNKNOWN ? le : 0.f;
                so = a.ks == NB_UNKNOWN ? ls : 0.f;
                f = kf == NB_UNKNOWN ? lf : 0.f;
                dg = (((lw + le) + (ln + ls)) + (lb + lf)) + wv;
            }
            const size_t i = (size_t)bd.p * wg.stride + (size_t)y * wg.nx + bd.x;
            R[i] = v;
            E[i] = e;
            S[i] = so;
            F[i] = f;
            Dg[i] = dg;
            s += (double)v * (double)v;
        }
    part_store(s, ws, wg, bb);
}

// The operator's launch (grid: cg x bands x planes): k_pcg_op's walk with the WLS coefficients over a plane of stacked frames, plus
// F_t(q) P_(t+1)(q) + F_(t-1)(q) P_(t-1)(q).  RES false: Q = L P and the parts of P . Q;  true: Q -= L P and the parts of Q . Q.  A
// lane owns one column of its band and rolls the row above, its own and the row below through registers, with the north link; where
// the band crosses into the next frame the roll starts again (the row above is then the frame's last one where y wraps, else none).
// The two temporal neighbours of its element lie one frame of nx ny floats before and behind it in the same plane.  PER (periodic
// time, decided at compile time: the free-time form is the code it was): the neighbour before frame 0 is frame T - 1, through the
// wrapping link that F holds in the last frame's rows, and the neighbour behind frame T - 1 is frame 0.  No atomics, no LDS but the
// block sum's.
template <bool RES, bool PER>
__global__ __launch_bounds__(WL) void k_volume_op(PcgGeo wg, VolumeGeo vg, const float *__restrict__ P, float *__restrict__ Q, double *__restrict__ parts,
                                                   const float *__restrict__ E, const float *__restrict__ S, const float *__restrict__ F,
                                                   const float *__restrict__ Dg)
{
    __shared__ double ws[4];
    const int x = (int)blockIdx.x * WL + (int)threadIdx.x, nx = wg.nx, fny = vg.ny;
    const int y0 = (int)blockIdx.y * wg.rows, y1 = min(y0 + wg.rows, wg.ny);
    const size_t base = (size_t)blockIdx.z * wg.stride, n2 = (size_t)nx * fny;
    const float *__restrict__ pl = P + base, *__restrict__ el = E + base, *__restrict__ sl = S + base, *__restrict__ fl = F + base;
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
            float tb, tf;
            if (PER) {
                const size_t wrap = (size_t)(vg.T - 1) * n2, ib = fr.t > 0 ? ro + x - n2 : ro + x + wrap;
                tb = fl[ib] * pl[ib];
                tf = fl[ro + x] * pl[fr.t < vg.T - 1 ? ro + x + n2 : ro + x - wrap];
            } else {
                tb = fr.t > 0 ? fl[ro + x - n2] * pl[ro + x - n2] : 0.f;
                tf = fr.t < vg.T - 1 ? fl[ro + x] * pl[ro + x + n2] : 0.f;
            }
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

// One workgroup, lane i of it.  Free time: D[k T + t] = sqrt((k ? 2 : 1) / T) cos(pi (2t + 1) k / (2T)), mu_k = 2 - 2 cos(pi k / T);
// periodic time: the Hartley table D[k T + t] = (cos + sin)(2 pi k t / T) / sqrt(T) -- symmetric, orthonormal, its own inverse, and it
// diagonalises every symmetric circulant --, mu_k = 2 - 2 cos(2 pi k / T).  In double, rounded to float32; the shift of mode k,
// lam[p T + k] = (wbar + tau mu_k) / sbar in double, rounded to float32, for each of the planes
__global__ __launch_bounds__(WL) void k_volume_tables(int T, int planes, int periodic, double wbar, double tau, double sbar, float *__restrict__ D,
                                                       double *__restrict__ lam)
{
    for (int i = (int)threadIdx.x; i < T * T; i += WL) {
        const int k = i / T, t = i - k * T;
        if (periodic) {
            const double a = 2.0 * (double)((k * t) % T) / (double)T;
            D[i] = (float)((cospi(a) + sinpi(a)) / sqrt((double)T));
        } else D[i] = (float)(sqrt((k ? 2.0 : 1.0) / (double)T) * cospi((double)((2 * t + 1) * k) / (2.0 * (double)T)));
    }
    for (int i = (int)threadIdx.x; i < planes * T; i += WL) {
        const int k = i % T;
        const double shift = wbar + tau * (2.0 - 2.0 * cospi((periodic ? 2.0 : 1.0) * (double)k / (double)T));
        lam[i] = (double)(float)(shift / sbar);
    }
}

// The transform along the frames (grid: column groups of a frame's nx ny elements x T x planes): out[k][i] = sum_t D[k][t] in[t][i],
// TR: sum_t D[t][k] in[t][i], t ascending, in float32 -- a dense T x T product per pixel: a lane's T reads are coalesced across the
// wave and shared by the T workgroups of its pixels through the cache.
template <bool TR>
__global__ __launch_bounds__(WL) void k_volume_dct(PcgGeo wg, VolumeGeo vg, const float *__restrict__ D, const float *__restrict__ in, float *__restrict__ out)
{
    const size_t n2 = (size_t)wg.nx * vg.ny, i = (size_t)blockIdx.x * WL + threadIdx.x;
    if (i >= n2) return;
    const int k = (int)blockIdx.y, T = vg.T;
    const size_t base = (size_t)blockIdx.z * wg.stride + i;
    float acc = 0.f;
    for (int t = 0; t < T; ++t) acc += D[TR ? t * T + k : k * T + t] * in[base + (size_t)t * n2];
    out[base + (size_t)k * n2] = acc;
}

// every element the layout names, frame by frame (grid: column groups x H x planes T): U at UNKNOWN pixels, data's bits at KNOWN and
// OUTSIDE pixels, boundary's bits on the Dirichlet lines (out may be data or boundary: the same value again)
__global__ __launch_bounds__(WL) void k_volume_out(PoissonGeo g, PcgGeo wg, VolumeGeo vg, VolumeJobs t, const float *__restrict__ U)
{
    const int z = (int)blockIdx.z, p = z / vg.T, f = z - p * vg.T, member = p / g.C, c = p - member * g.C;
    const int x = (int)blockIdx.x * WL + (int)threadIdx.x, y = (int)blockIdx.y;
    if (x >= g.W) return;
    const PoissonJobDev &j = t.j[member];
    const long long o = (long long)x * g.cs + (long long)y * g.rs + (long long)c * g.chs + (long long)f * vg.fs;
    const int ux = x - wg.x0, uy = y - wg.y0;
    if (ux >= 0 && ux < wg.nx && uy >= 0 && uy < vg.ny)
        j.out[o] = t.st[member][o] == 0.f ? U[(size_t)p * wg.stride + ((size_t)f * vg.ny + uy) * wg.nx + ux] : j.d[o];
    else j.out[o] = j.b[o];
}

template <bool LNK, bool FLW = false, class Flow = NoFlow>
void setup_form(bool lap, bool now, dim3 grid, hipStream_t s, const PoissonGeo &g, const PcgGeo &wg, const VolumeGeo &vg, const VolumeJobs &t, float *R,
                float *E, float *S, float *F, float *Dg, double *b, const Flow &fl = Flow())
{
    if (lap && now) hipLaunchKernelGGL((k_volume_setup<true, true, LNK, FLW>), grid, dim3(WL), 0, s, g, wg, vg, t, R, E, S, F, Dg, b, fl);
    else if (lap) hipLaunchKernelGGL((k_volume_setup<true, false, LNK, FLW>), grid, dim3(WL), 0, s, g, wg, vg, t, R, E, S, F, Dg, b, fl);
    else if (now) hipLaunchKernelGGL((k_volume_setup<false, true, LNK, FLW>), grid, dim3(WL), 0, s, g, wg, vg, t, R, E, S, F, Dg, b, fl);
    else hipLaunchKernelGGL((k_volume_setup<false, false, LNK, FLW>), grid, dim3(WL), 0, s, g, wg, vg, t, R, E, S, F, Dg, b, fl);
}

// the link planes of volumes i0 .. of a launch
FlowLinks flow_links_of(const PcgGeo &wg, int i0, const int *fwd, const int *bwd)
{
    const long long stride = flow_link_stride(wg);
    return FlowLinks{ fwd + stride * i0, bwd + stride * i0, stride };
}

} // namespace

void launch_volume_stats(const PoissonGeo &g, const PcgGeo &wg, const VolumeGeo &vg, const PoissonJobDev *jobs, const SideArrays *sides, int m,
                         double *stats, hipStream_t s, bool full)
{
    for_side_tables<VolumeJobs>(jobs, sides, m, [&](const VolumeJobs &t, int i0, int cnt) {
        const dim3 grid((unsigned)wg.cg, (unsigned)wg.bands, (unsigned)(g.C * cnt));
        const bool general = full || t.sx[0] || t.smt[0] || vg.periodic;
        double *st = stats + (size_t)g.C * i0 * PCG_PARTS * (general ? VOLUME_STATS : VOLUME_STATS_PLAIN);
        if (general) hipLaunchKernelGGL(k_volume_stats<true>, grid, dim3(WL), 0, s, g, wg, vg, t, st, NoFlow(), NoFlow());
        else hipLaunchKernelGGL(k_volume_stats<false>, grid, dim3(WL), 0, s, g, wg, vg, t, st, NoFlow(), NoFlow());
    });
}

void launch_volume_flow_stats(const PoissonGeo &g, const PcgGeo &wg, const VolumeGeo &vg, const PoissonJobDev *jobs, const SideArrays *sides, int m,
                              const int *fwd, const int *bwd, double *stats, hipStream_t s)
{
    static_assert((int)FlowArrays::MAX == (int)VolumeJobs::MAX, "one record of either per volume of a launch");
    for_side_tables<VolumeJobs>(jobs, sides, m, [&](const VolumeJobs &t, int i0, int cnt) {
        const dim3 grid((unsigned)wg.cg, (unsigned)wg.bands, (unsigned)(g.C * cnt));
        FlowArrays fa{};
        for (int i = 0; i < cnt; ++i) fa.set(i, sides[i0 + i]);
        hipLaunchKernelGGL((k_volume_stats<true, true>), grid, dim3(WL), 0, s, g, wg, vg, t, stats + (size_t)g.C * i0 * PCG_PARTS * VOLUME_FLOW_STATS,
                           flow_links_of(wg, i0, fwd, bwd), fa);
    });
}

void launch_volume_flow_setup(const PoissonGeo &g, const PcgGeo &wg, const VolumeGeo &vg, bool lap, const PoissonJobDev *jobs, const SideArrays *sides,
                              int m, const int *fwd, const int *bwd, float *R, float *E, float *S, float *F, float *Dg, double *bb, hipStream_t s)
{
    for_side_tables<VolumeJobs>(jobs, sides, m, [&](const VolumeJobs &t, int i0, int cnt) {
        const dim3 grid((unsigned)wg.cg, (unsigned)wg.bands, (unsigned)(g.C * cnt));
        const size_t o = (size_t)g.C * i0 * wg.stride;
        setup_form<true, true>(lap, !t.w[0], grid, s, g, wg, vg, t, R + o, E + o, S + o, F + o, Dg + o, bb + (size_t)g.C * i0 * PCG_PARTS,
                               flow_links_of(wg, i0, fwd, bwd));
    });
}

void launch_volume_setup(const PoissonGeo &g, const PcgGeo &wg, const VolumeGeo &vg, bool lap, const PoissonJobDev *jobs, const SideArrays *sides, int m,
                         float *R, float *E, float *S, float *F, float *Dg, double *bb, hipStream_t s)
{
    for_side_tables<VolumeJobs>(jobs, sides, m, [&](const VolumeJobs &t, int i0, int cnt) {
        const dim3 grid((unsigned)wg.cg, (unsigned)wg.bands, (unsigned)(g.C * cnt));
        const size_t o = (size_t)g.C * i0 * wg.stride;
        double *b = bb + (size_t)g.C * i0 * PCG_PARTS;
        const bool now = !t.w[0];
        if (t.sx[0] || t.smt[0] || vg.periodic) setup_form<true>(lap, now, grid, s, g, wg, vg, t, R + o, E + o, S + o, F + o, Dg + o, b);
        else setup_form<false>(lap, now, grid, s, g, wg, vg, t, R + o, E + o, S + o, F + o, Dg + o, b);
    });
}

void launch_volume_op(const PcgGeo &wg, const VolumeGeo &vg, int planes, bool residual, const float *P, const float *E, const float *S, const float *F,
                      const float *Dg, float *Q, double *parts, hipStream_t s)
{
    const dim3 grid((unsigned)wg.cg, (unsigned)wg.bands, (unsigned)planes);
    if (vg.periodic) {
        if (residual) hipLaunchKernelGGL((k_volume_op<true, true>), grid, dim3(WL), 0, s, wg, vg, P, Q, parts, E, S, F, Dg);
        else hipLaunchKernelGGL((k_volume_op<false, true>), grid, dim3(WL), 0, s, wg, vg, P, Q, parts, E, S, F, Dg);
    } else if (residual) hipLaunchKernelGGL((k_volume_op<true, false>), grid, dim3(WL), 0, s, wg, vg, P, Q, parts, E, S, F, Dg);
    else hipLaunchKernelGGL((k_volume_op<false, false>), grid, dim3(WL), 0, s, wg, vg, P, Q, parts, E, S, F, Dg);
}

void launch_volume_tables(int T, int planes, bool periodic, double wbar, double tau, double sbar, float *D, double *lam, hipStream_t s)
{
    hipLaunchKernelGGL(k_volume_tables, dim3(1), dim3(WL), 0, s, T, planes, periodic ? 1 : 0, wbar, tau, sbar, D, lam);
}

void launch_volume_dct(const PcgGeo &wg, const VolumeGeo &vg, int planes, bool transposed, const float *D, const float *in, float *out, hipStream_t s)
{
    const dim3 grid((unsigned)(((size_t)wg.nx * vg.ny + WL - 1) / WL), (unsigned)vg.T, (unsigned)planes);
    if (transposed) hipLaunchKernelGGL(k_volume_dct<true>, grid, dim3(WL), 0, s, wg, vg, D, in, out);
    else hipLaunchKernelGGL(k_volume_dct<false>, grid, dim3(WL), 0, s, wg, vg, D, in, out);
}

void launch_volume_out(const PoissonGeo &g, const PcgGeo &wg, const VolumeGeo &vg, const PoissonJobDev *jobs, const SideArrays *sides, int m,
                       const float *U, hipStream_t s)
{
    for_side_tables<VolumeJobs>(jobs, sides, m, [&](const VolumeJobs &t, int i0, int cnt) {
        hipLaunchKernelGGL(k_volume_out, dim3((unsigned)((g.W + WL - 1) / WL), (unsigned)g.H, (unsigned)(g.C * cnt * vg.T)), dim3(WL), 0, s, g, wg, vg, t,
                           U + (size_t)g.C * i0 * wg.stride);
    });
}

} // namespace sc
