// sc_volume_subflow.hip -- the sub-pixel flow volume call's kernels (sc_hip_volume_subflow*; sc_volume_api.cpp: VolumeSubflowOperator):
// sc_hip_volume_wls's system with every temporal link a bilinear stencil of up to four taps in the next frame.  With B the matrix whose
// row of link p holds b_k(p) at its taps and -1 at p, the temporal term is -B^T S B, S = diag(lt): symmetric whatever arrives where, so
// there is no matching -- every candidate holds its link and any number of links may arrive at a pixel.  sc_pcg.h states the storage.
//
// Per call and volume (its channels share them): the cropped flow -- the caller's two arrays on the work rectangle, NaN where a pixel
// holds no link -- and the transpose of B in CSR form: for every target the (source, weight) pairs that arrive, in ascending (source,
// tap) order.  k_subflow_emit writes key = target and value = (source, weight) of every tap slot 4 p + k (an empty slot: key n), a
// stable radix sort by key -- one stable split per key bit, lowest first: k_split_count, k_split_scan, k_split_scatter -- keeps the
// slots' order inside a row, k_subflow_offsets finds every row's start by bisection: the build is linear in the volume (times the
// key's bits) whatever the longest row, uses no atomics at all, and two runs give the same bytes.
// Per solve and work plane: LT, the weight of the link a pixel holds where it is live (else 0), and F, 1 at UNKNOWN pixels (else 0).
// Per application: k_subflow_rho writes rho(p) = LT(p) (sum_k b_k F(q_k) P(q_k) - F(p) P(p)) once per link, k_subflow_op is k_volume_op's
// walk and adds F(i) (rho(i) - sum over the arrivals (s, b) of b rho(s)): "a link's rho written once by its source and read there by the
// pixel it arrives at", the coupled calls' idiom.  The diagonal plane holds the spatial links and w alone: the temporal diagonal is in
// the product.  No float atomics, no LDS but the block sum's.  sc_subflow_device.h holds what these kernels share with the robust
// sub-pixel call's (sc_volume_subflow_robust.hip): the taps, a work-plane index as an offset, the held link as the states judge it.
#include "sc_subflow_device.h"

namespace sc {

namespace {

__device__ __forceinline__ bool bad_link(float v) { return !(v > 0.f) || v > 3.4028234e38f; }

// ---- the build, one volume at a time (grid: column groups x a frame's rows x T)
// fw = the cropped flow (dx | dy, n floats each; NaN: no link), key / val of the four tap slots of every element
__global__ __launch_bounds__(WL) void k_subflow_emit(PoissonGeo g, PcgGeo wg, VolumeGeo vg, const float *__restrict__ fx, const float *__restrict__ fy,
                                                      long long n, float *__restrict__ fw, unsigned int *__restrict__ key,
                                                      unsigned long long *__restrict__ val)
{
    const int x = (int)blockIdx.x * WL + (int)threadIdx.x, yy = (int)blockIdx.y, t = (int)blockIdx.z;
    if (x >= wg.nx) return;
    const long long i = ((long long)t * vg.ny + yy) * wg.nx + x;
    float dx = __builtin_nanf(""), dy = dx;
    if (t < vg.T - 1 || vg.periodic) {
        const size_t e = ((size_t)t * g.H + (wg.y0 + yy)) * g.W + (wg.x0 + x);
        dx = fx[e]; dy = fy[e];
    }
    int j[4];
    float b[4];
    if (!subflow_taps(wg, vg, dx, dy, x, yy, t, j, b)) dx = dy = __builtin_nanf("");
    fw[i] = dx;
    fw[n + i] = dy;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        key[4 * i + k] = j[k] >= 0 ? (unsigned int)j[k] : (unsigned int)n;
        val[4 * i + k] = ((unsigned long long)__float_as_uint(b[k]) << 32) | (unsigned int)i;
    }
}

// ---- the stable split by one key bit (a pass of the sort; N = 4 n slots, a workgroup's tile SPLIT_TILE of them, a lane four
// consecutive ones, so lane order is slot order): the slots whose bit is 0 keep their order in front, the others theirs behind
constexpr int SPLIT_TILE = 4 * WL;

// zeros[b] = the slots of tile b whose bit is 0
__global__ __launch_bounds__(WL) void k_split_count(long long N, int bit, const unsigned int *__restrict__ key, long long *__restrict__ zeros)
{
    __shared__ int sh[WL];
    const long long i0 = ((long long)blockIdx.x * WL + threadIdx.x) * 4;
    int z = 0;
    if (i0 < N) {
        const uint4 k = *reinterpret_cast<const uint4 *>(key + i0);
        z = (int)(~(k.x >> bit) & 1u) + (int)(~(k.y >> bit) & 1u) + (int)(~(k.z >> bit) & 1u) + (int)(~(k.w >> bit) & 1u);
    }
    sh[threadIdx.x] = z;
    __syncthreads();
    for (int o = WL / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) zeros[blockIdx.x] = sh[0];
}

// one workgroup: zeros[0 .. nb) becomes its exclusive prefix sum, zeros[nb] the total
__global__ __launch_bounds__(WL) void k_split_scan(long long nb, long long *__restrict__ zeros)
{
    __shared__ long long sh[WL];
    const long long per = (nb + WL - 1) / WL, b0 = min((long long)threadIdx.x * per, nb), b1 = min(b0 + per, nb);
    long long sum = 0;
    for (long long b = b0; b < b1; ++b) sum += zeros[b];
    sh[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long run = 0;
        for (int t = 0; t < WL; ++t) { const long long v = sh[t]; sh[t] = run; run += v; }
        zeros[nb] = run;
    }
    __syncthreads();
    long long run = sh[threadIdx.x];
    for (long long b = b0; b < b1; ++b) { const long long v = zeros[b]; zeros[b] = run; run += v; }
}

// slot i goes to (the zeros before it) where its bit is 0, else to (all zeros) + (the ones before it) = total + i - (the zeros before it)
__global__ __launch_bounds__(WL) void k_split_scatter(long long N, long long nb, int bit, const unsigned int *__restrict__ kin,
                                                       const unsigned long long *__restrict__ vin, unsigned int *__restrict__ kout,
                                                       unsigned long long *__restrict__ vout, const long long *__restrict__ zeros)
{
    __shared__ int sh[WL];
    const long long i0 = ((long long)blockIdx.x * WL + threadIdx.x) * 4;
    unsigned int k[4] = { 0, 0, 0, 0 };
    int z = 0;
    if (i0 < N) {
        const uint4 q = *reinterpret_cast<const uint4 *>(kin + i0);
        k[0] = q.x; k[1] = q.y; k[2] = q.z; k[3] = q.w;
#pragma unroll
        for (int j = 0; j < 4; ++j) z += (int)(~(k[j] >> bit) & 1u);
    }
    sh[threadIdx.x] = z;
    __syncthreads();
    for (int o = 1; o < WL; o <<= 1) {          // inclusive scan over the lanes
        const int v = (int)threadIdx.x >= o ? sh[threadIdx.x - o] : 0;
        __syncthreads();
        sh[threadIdx.x] += v;
        __syncthreads();
    }
    if (i0 >= N) return;
    long long before = zeros[blockIdx.x] + (sh[threadIdx.x] - z);          // the zeros before slot i0
    const long long total = zeros[nb];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const bool zero = !((k[j] >> bit) & 1u);
        const long long to = zero ? before : total + (i0 + j) - before;
        kout[to] = k[j];
        vout[to] = vin[i0 + j];
        before += zero ? 1 : 0;
    }
}

// off[j] = the first sorted slot whose key is at least j, for j = 0 .. n (off[n]: the slots that hold a tap)
__global__ __launch_bounds__(WL) void k_subflow_offsets(long long n, const unsigned int *__restrict__ key, long long *__restrict__ off)
{
    const long long j = (long long)blockIdx.x * WL + threadIdx.x;
    if (j > n) return;
    long long lo = 0, hi = 4 * n;
    while (lo < hi) {
        const long long mid = lo + (hi - lo) / 2;
        if ((long long)key[mid] < j) lo = mid + 1;
        else hi = mid;
    }
    off[j] = lo;
}

// k_volume_stats in its full form (VOLUME_STATS fields per part, the same spatial rules) with the temporal fields of the bilinear links:
// the sum and the number of the live links' lt, how many of them are invalid, and in the UNKNOWN - KNOWN sum lt * (1 where the source
// is KNOWN, else the sum of b over the KNOWN taps).  Every link is counted once, at its source.
__global__ __launch_bounds__(WL) void k_subflow_stats(PoissonGeo g, PcgGeo wg, VolumeGeo vg, VolumeJobs t, SubflowLinks L, double *__restrict__ stats)
{
    constexpr int NS = VOLUME_STATS;
    __shared__ double ws[NS][4];
    const PcgBand b(g, wg);
    const float *__restrict__ w = t.w[b.member], *__restrict__ st = t.st[b.member];
    const float *__restrict__ sx = t.sx[b.member], *__restrict__ sy = t.sy[b.member], *__restrict__ smt = t.smt[b.member];
    const float *__restrict__ fw = L.fw + (long long)b.member * 2 * L.n;
    const bool px = wg.ax == MIXED_PERIODIC, py = wg.ay == MIXED_PERIODIC;
    double sw = 0.0, bw = 0.0, nu = 0.0, uk = 0.0, bst = 0.0, ss = 0.0, ns = 0.0, bs = 0.0, sl = 0.0, nt = 0.0, bt = 0.0;
    if (b.x < wg.nx)
        for (int y = b.y0; y < b.y1; ++y) {
            const FrameRow fr(vg, y);
            const int X = wg.x0 + b.x, Y = wg.y0 + fr.yy;
            const long long o = b.pixel(g, X, Y) + (long long)fr.t * vg.fs;
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
            auto link = [&](int kq, const float *__restrict__ arr, long long e) {
                if (kq == NB_NONE || (kp != NB_UNKNOWN && kq != NB_UNKNOWN)) return;
                const float s = arr ? arr[e] : 1.f;
                if (bad_link(s)) bs += 1.0;
                ss += (double)s;
                ns += 1.0;
                if (kp + kq == NB_KNOWN) uk += (double)s;
            };
            link(a.ke, sx, o);
            link(a.ks, sy, o);
            if (a.kw == NB_DIRICHLET) link(a.kw, sx, a.ow);
            if (a.kn == NB_DIRICHLET) link(a.kn, sy, a.on);
            const SubflowLink k(g, wg, vg, fw, L.n, st, nullptr, b.c, b.x, y, fr.t, fr.yy, o);
            if (k.live) {
                const float lt = time_link(smt, o, vg.tau);
                if (bad_link(lt) || (smt && bad_link(smt[o]))) bt += 1.0;
                sl += (double)lt;
                nt += 1.0;
                uk += (double)lt * (double)(kp == NB_KNOWN ? 1.f : k.kb);
            }
        }
    part_store(sw, ws[0], wg, stats, NS, 0);
    part_store(bw, ws[1], wg, stats, NS, 1);
    part_store(nu, ws[2], wg, stats, NS, 2);
    part_store(uk, ws[3], wg, stats, NS, 3);
    part_store(bst, ws[4], wg, stats, NS, 4);
    part_store(ss, ws[5], wg, stats, NS, 5);
    part_store(ns, ws[6], wg, stats, NS, 6);
    part_store(bs, ws[7], wg, stats, NS, 7);
    part_store(sl, ws[8], wg, stats, NS, 8);
    part_store(nt, ws[9], wg, stats, NS, 9);
    part_store(bt, ws[10], wg, stats, NS, 10);
}

// The first launch of the set-up, per work-plane element p: LT = lt of the link p holds where it is live, else 0; SG = lt * g', g' the
// link's wanted difference with its KNOWN points folded in: gt (LAP, or gt NULL: 0) less the sum of b * data over its KNOWN taps, plus
// data(p) where the source itself is KNOWN.  gt and smooth_t are read at the source of a live link only.
template <bool LAP>
__global__ __launch_bounds__(WL) void k_subflow_sigma(PoissonGeo g, PcgGeo wg, VolumeGeo vg, VolumeJobs t, SubflowLinks L, float *__restrict__ LT,
                                                       float *__restrict__ SG)
{
    const PcgBand bd(g, wg);
    if (bd.x >= wg.nx) return;
    const PoissonJobDev &j = t.j[bd.member];
    const float *__restrict__ st = t.st[bd.member], *__restrict__ gt = t.gt[bd.member], *__restrict__ smt = t.smt[bd.member];
    const float *__restrict__ fw = L.fw + (long long)bd.member * 2 * L.n;
    for (int y = bd.y0; y < bd.y1; ++y) {
        const FrameRow fr(vg, y);
        const long long o = bd.pixel(g, wg.x0 + bd.x, wg.y0 + fr.yy) + (long long)fr.t * vg.fs;
        const SubflowLink k(g, wg, vg, fw, L.n, st, j.d, bd.c, bd.x, y, fr.t, fr.yy, o);
        float lt = 0.f, sg = 0.f;
        if (k.live) {
            lt = time_link(smt, o, vg.tau);
            float gp = (!LAP && gt) ? gt[o] : 0.f;
            gp -= k.kd;
            if (k.kp == NB_KNOWN) gp += j.d[o];
            sg = lt * gp;
        }
        const size_t i = (size_t)bd.p * wg.stride + (size_t)y * wg.nx + bd.x;
        LT[i] = lt;
        SG[i] = sg;
    }
}

// k_volume_setup's walk and spatial part, word for word; the temporal part of b at an UNKNOWN pixel i is SG(i) less the sum over the
// arrivals (s, b) of b * SG(s), in the rows' order (-B^T S g').  F = 1 at UNKNOWN pixels, Dg = the spatial links and w alone.
template <bool LAP, bool NOW>
__global__ __launch_bounds__(WL) void k_subflow_setup(PoissonGeo g, PcgGeo wg, VolumeGeo vg, VolumeJobs t, SubflowLinks L, const float *__restrict__ SG,
                                                       float *__restrict__ R, float *__restrict__ E, float *__restrict__ S, float *__restrict__ F,
                                                       float *__restrict__ Dg, double *__restrict__ bb)
{
    __shared__ double ws[4];
    const PcgBand bd(g, wg);
    const PoissonJobDev &j = t.j[bd.member];
    const float *__restrict__ w = t.w[bd.member], *__restrict__ st = t.st[bd.member];
    const float *__restrict__ sx = t.sx[bd.member], *__restrict__ sy = t.sy[bd.member];
    const long long *__restrict__ off = L.off + (long long)bd.member * (L.n + 2);
    const unsigned long long *__restrict__ ent = L.ent + (long long)bd.member * 4 * L.n;
    const float *__restrict__ sg = SG + (size_t)bd.p * wg.stride;
    const bool px = wg.ax == MIXED_PERIODIC, py = wg.ay == MIXED_PERIODIC;
    double s = 0.0;
    if (bd.x < wg.nx)
        for (int y = bd.y0; y < bd.y1; ++y) {
            const FrameRow fr(vg, y);
            const int X = wg.x0 + bd.x, Y = wg.y0 + fr.yy;
            const long long o = bd.pixel(g, X, Y) + (long long)fr.t * vg.fs;
            const size_t ip = (size_t)y * wg.nx + bd.x;
            float v = 0.f, e = 0.f, so = 0.f, f = 0.f, dg = 0.f;
            if (st[o] == 0.f) {
                const Around a(g, wg, st, X, Y, o, px, py);
                const float lw = a.kw == NB_NONE ? 0.f : sx ? sx[a.ow] : 1.f, le = a.ke == NB_NONE ? 0.f : sx ? sx[o] : 1.f;
                const float ln = a.kn == NB_NONE ? 0.f : sy ? sy[a.on] : 1.f, ls = a.ks == NB_NONE ? 0.f : sy ? sy[o] : 1.f;
                float arr = 0.f;
                for (long long k = off[ip], k1 = off[ip + 1]; k < k1; ++k) {
                    const unsigned long long en = ent[k];
                    arr += __uint_as_float((unsigned int)(en >> 32)) * sg[(unsigned int)en];
                }
                const float tm = sg[ip] - arr;
                if (LAP) v = j.lap[o] + tm;
                else {
                    const float pa = a.ke == NB_NONE ? 0.f : rounded_product(le, j.gx[o]);
                    const float pb = a.kw == NB_NONE ? 0.f : rounded_product(lw, j.gx[a.ow]);
                    const float pc = a.ks == NB_NONE ? 0.f : rounded_product(ls, j.gy[o]);
                    const float pd = a.kn == NB_NONE ? 0.f : rounded_product(ln, j.gy[a.on]);
                    v = ((pa - pb) + (pc - pd)) + tm;
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
                f = 1.f;
                dg = ((lw + le) + (ln + ls)) + wv;
            }
            const size_t i = (size_t)bd.p * wg.stride + ip;
            R[i] = v;
            E[i] = e;
            S[i] = so;
            F[i] = f;
            Dg[i] = dg;
            s += (double)v * (double)v;
        }
    part_store(s, ws, wg, bb);
}

// rho(p) = LT(p) (sum_k b_k F(q_k) P(q_k) - F(p) P(p)), the taps in their order; 0 where p holds no live link (nothing but LT is read
// there).  Grid: cg x bands x planes; C: the planes per volume.
__global__ __launch_bounds__(WL) void k_subflow_rho(PcgGeo wg, VolumeGeo vg, int C, SubflowLinks L, const float *__restrict__ P, const float *__restrict__ F,
                                                     const float *__restrict__ LT, float *__restrict__ RHO)
{
    const int x = (int)blockIdx.x * WL + (int)threadIdx.x;
    if (x >= wg.nx) return;
    const int y0 = (int)blockIdx.y * wg.rows, y1 = min(y0 + wg.rows, wg.ny);
    const size_t base = (size_t)blockIdx.z * wg.stride;
    const float *__restrict__ fw = L.fw + (long long)((int)blockIdx.z / C) * 2 * L.n;
    const float *__restrict__ pl = P + base, *__restrict__ fl = F + base;
    for (int y = y0; y < y1; ++y) {
        const size_t ip = (size_t)y * wg.nx + x;
        const float lt = LT[base + ip];
        float r = 0.f;
        if (lt != 0.f) {
            const FrameRow fr(vg, y);
            int j[4];
            float b[4];
            subflow_taps(wg, vg, fw[ip], fw[L.n + ip], x, fr.yy, fr.t, j, b);
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (j[k] >= 0) acc += b[k] * (fl[j[k]] * pl[j[k]]);
            r = lt * (acc - fl[ip] * pl[ip]);
        }
        RHO[base + ip] = r;
    }
}

// k_volume_op's walk (sc_volume.hip: the rolling rows, the frames' seams) with the temporal part in product form: at an UNKNOWN element
// i, rho(i) less the sum over the arrivals (s, b) of b rho(s), row i of the volume's transpose in its fixed order.  Per element beyond
// k_volume_op's loads: F, two row offsets (shared with the neighbouring lane), its own rho, and 8 + 4 bytes per arrival.
template <bool RES>
__global__ __launch_bounds__(WL) void k_subflow_op(PcgGeo wg, VolumeGeo vg, int C, SubflowLinks L, const float *__restrict__ P, float *__restrict__ Q,
                                                    double *__restrict__ parts, const float *__restrict__ E, const float *__restrict__ S,
                                                    const float *__restrict__ F, const float *__restrict__ Dg, const float *__restrict__ RHO)
{
    __shared__ double ws[4];
    const int x = (int)blockIdx.x * WL + (int)threadIdx.x, nx = wg.nx, fny = vg.ny;
    const int y0 = (int)blockIdx.y * wg.rows, y1 = min(y0 + wg.rows, wg.ny);
    const size_t base = (size_t)blockIdx.z * wg.stride;
    const int vol = (int)blockIdx.z / C;
    const float *__restrict__ pl = P + base, *__restrict__ el = E + base, *__restrict__ sl = S + base, *__restrict__ fl = F + base;
    const float *__restrict__ rh = RHO + base;
    const long long *__restrict__ off = L.off + (long long)vol * (L.n + 2);
    const unsigned long long *__restrict__ ent = L.ent + (long long)vol * 4 * L.n;
    double s = 0.0;
    if (x < nx) {
        const bool px = wg.ax == MIXED_PERIODIC, py = wg.ay == MIXED_PERIODIC;
        const int xl = x > 0 ? x - 1 : px ? nx - 1 : -1, xr = x < nx - 1 ? x + 1 : px ? 0 : -1;
        FrameRow fr(vg, y0);
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
            float tm = 0.f;
            if (fl[ro + x] != 0.f) {
                float arr = 0.f;
                for (long long k = off[ro + x], k1 = off[ro + x + 1]; k < k1; ++k) {
                    const unsigned long long en = ent[k];
                    arr += __uint_as_float((unsigned int)(en >> 32)) * rh[(unsigned int)en];
                }
                tm = rh[ro + x] - arr;
            }
            const float v = (((e_l * l + e_r * r) + (s_up * up + s_dn * dn)) + tm) - Dg[i] * cur;
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

// the key bits a sort has to look at: those of n, the empty slot's key
int key_bits(long long n)
{
    int bits = 1;
    while (bits < 32 && ((long long)1 << bits) <= n) ++bits;
    return bits;
}

size_t up256(size_t v) { return (v + 255) / 256 * 256; }

} // namespace

SubflowStore subflow_store(const PcgGeo &wg, int per)
{
    SubflowStore st{};
    st.n = (long long)wg.nx * wg.ny;
    st.per = per;
    const size_t n = (size_t)st.n;
    const size_t tmp = sizeof(long long) * ((4 * n + SPLIT_TILE - 1) / SPLIT_TILE + 1);      // a pass's zeros per tile and their total
    st.tmp_bytes = tmp;
    size_t at = 0;
    st.off_b = at; at += up256(sizeof(long long) * (n + 2) * per);
    st.ent_b = at; at += up256(sizeof(unsigned long long) * 4 * n * per);
    st.fw_b = at; at += up256(sizeof(float) * 2 * n * per);
    st.kin_b = at; at += up256(sizeof(unsigned int) * 4 * n);
    st.kout_b = at; at += up256(sizeof(unsigned int) * 4 * n);
    st.vin_b = at; at += up256(sizeof(unsigned long long) * 4 * n);
    st.tmp_b = at; at += up256(tmp);
    st.total = at;
    return st;
}

void launch_subflow_links(const PoissonGeo &g, const PcgGeo &wg, const VolumeGeo &vg, const SideArrays *sides, int m, const SubflowStore &st, void *lnk,
                                hipStream_t s)
{
    char *p = (char *)lnk;
    unsigned int *kin = (unsigned int *)(p + st.kin_b), *kout = (unsigned int *)(p + st.kout_b);
    unsigned long long *vin = (unsigned long long *)(p + st.vin_b);
    const long long n = st.n;
    const long long N = 4 * n, nb = (N + SPLIT_TILE - 1) / SPLIT_TILE;
    long long *zeros = (long long *)(p + st.tmp_b);
    const int bits = key_bits(n);
    for (int k = 0; k < m; ++k) {
        long long *off = (long long *)(p + st.off_b) + (long long)k * (n + 2);
        unsigned long long *ent = (unsigned long long *)(p + st.ent_b) + (long long)k * 4 * n;
        float *fw = (float *)(p + st.fw_b) + (long long)k * 2 * n;
        // the passes go to and fro between two pairs of buffers; the values' last stop is ent
        unsigned int *ka = kin, *kb = kout;
        unsigned long long *va = (bits & 1) ? vin : ent, *vb = (bits & 1) ? ent : vin;
        hipLaunchKernelGGL(k_subflow_emit, dim3((unsigned)wg.cg, (unsigned)vg.ny, (unsigned)vg.T), dim3(WL), 0, s, g, wg, vg, sides[k].fx, sides[k].fy, n,
                           fw, ka, va);
        for (int bit = 0; bit < bits; ++bit) {
            hipLaunchKernelGGL(k_split_count, dim3((unsigned)nb), dim3(WL), 0, s, N, bit, (const unsigned int *)ka, zeros);
            hipLaunchKernelGGL(k_split_scan, dim3(1), dim3(WL), 0, s, nb, zeros);
            hipLaunchKernelGGL(k_split_scatter, dim3((unsigned)nb), dim3(WL), 0, s, N, nb, bit, (const unsigned int *)ka, (const unsigned long long *)va, kb,
                               vb, (const long long *)zeros);
            std::swap(ka, kb);
            std::swap(va, vb);
        }
        hipLaunchKernelGGL(k_subflow_offsets, dim3((unsigned)((n + 1 + WL - 1) / WL)), dim3(WL), 0, s, n, (const unsigned int *)ka, off);
    }
}

void launch_volume_subflow_stats(const PoissonGeo &g, const PcgGeo &wg, const VolumeGeo &vg, const PoissonJobDev *jobs, const SideArrays *sides, int m,
                                 const SubflowStore &st, void *lnk, double *stats, hipStream_t s)
{
    for_side_tables<VolumeJobs>(jobs, sides, m, [&](const VolumeJobs &t, int i0, int cnt) {
        const dim3 grid((unsigned)wg.cg, (unsigned)wg.bands, (unsigned)(g.C * cnt));
        hipLaunchKernelGGL(k_subflow_stats, grid, dim3(WL), 0, s, g, wg, vg, t, subflow_links_at(st, lnk, i0), stats + (size_t)g.C * i0 * PCG_PARTS * VOLUME_STATS);
    });
}

void launch_volume_subflow_setup(const PoissonGeo &g, const PcgGeo &wg, const VolumeGeo &vg, bool lap, const PoissonJobDev *jobs, const SideArrays *sides,
                                 int m, const SubflowStore &st, void *lnk, float *LT, float *SG, float *R, float *E, float *S, float *F, float *Dg,
                                 double *bb, hipStream_t s)
{
    for_side_tables<VolumeJobs>(jobs, sides, m, [&](const VolumeJobs &t, int i0, int cnt) {
        const dim3 grid((unsigned)wg.cg, (unsigned)wg.bands, (unsigned)(g.C * cnt));
        const size_t o = (size_t)g.C * i0 * wg.stride;
        const SubflowLinks L = subflow_links_at(st, lnk, i0);
        double *b = bb + (size_t)g.C * i0 * PCG_PARTS;
        const bool now = !t.w[0];
        if (lap) hipLaunchKernelGGL(k_subflow_sigma<true>, grid, dim3(WL), 0, s, g, wg, vg, t, L, LT + o, SG + o);
        else hipLaunchKernelGGL(k_subflow_sigma<false>, grid, dim3(WL), 0, s, g, wg, vg, t, L, LT + o, SG + o);
        if (lap && now) hipLaunchKernelGGL((k_subflow_setup<true, true>), grid, dim3(WL), 0, s, g, wg, vg, t, L, SG + o, R + o, E + o, S + o, F + o, Dg + o, b);
        else if (lap) hipLaunchKernelGGL((k_subflow_setup<true, false>), grid, dim3(WL), 0, s, g, wg, vg, t, L, SG + o, R + o, E + o, S + o, F + o, Dg + o, b);
        else if (now) hipLaunchKernelGGL((k_subflow_setup<false, true>), grid, dim3(WL), 0, s, g, wg, vg, t, L, SG + o, R + o, E + o, S + o, F + o, Dg + o, b);
        else hipLaunchKernelGGL((k_subflow_setup<false, false>), grid, dim3(WL), 0, s, g, wg, vg, t, L, SG + o, R + o, E + o, S + o, F + o, Dg + o, b);
    });
}

void launch_volume_subflow_op(const PcgGeo &wg, const VolumeGeo &vg, int planes, int C, bool residual, const SubflowStore &st, const void *lnk, const float *P,
                              const float *E, const float *S, const float *F, const float *Dg, const float *LT, float *RHO, float *Q, double *parts,
                              hipStream_t s)
{
    const dim3 grid((unsigned)wg.cg, (unsigned)wg.bands, (unsigned)planes);
    const SubflowLinks L = subflow_links_at(st, const_cast<void *>(lnk), 0);
    hipLaunchKernelGGL(k_subflow_rho, grid, dim3(WL), 0, s, wg, vg, C, L, P, F, LT, RHO);
    if (residual) hipLaunchKernelGGL(k_subflow_op<true>, grid, dim3(WL), 0, s, wg, vg, C, L, P, Q, parts, E, S, F, Dg, (const float *)RHO);
    else hipLaunchKernelGGL(k_subflow_op<false>, grid, dim3(WL), 0, s, wg, vg, C, L, P, Q, parts, E, S, F, Dg, (const float *)RHO);
}

} // namespace sc
