// sc_weighted.hip -- the kernels of the weighted solve (sc_hip_weighted*, sc_weighted_api.cpp): conjugate gradients on
//     (A - W) u = b,     W = diag(w), w >= 0,     b = lap - w d less the neighbouring Dirichlet values,
// A the 5-point operator under each side's rule, on compact float32 planes that hold the unknowns only (sc_common.h, WeightedGeo).
// Both A - W and the preconditioner A - lambda-bar are negative definite; the iteration is the textbook one with both signs
// flipped, which changes no quotient: alpha = (r . z) / (p . (A - W) p), beta = (r . z)' / (r . z).
// Every launch covers all planes of the chunk.  The operator rolls rows through registers: a lane owns one column of its band, keeps
// the row above, its own and the row below, and reads the left and right neighbours from the cache lines its wave loads anyway -- no
// LDS, no barrier inside the walk, 256 lanes and a handful of registers per workgroup (full occupancy; the launch is bound by the
// three plane transfers: p and w in, q out).  Reductions: a lane's running sum in double, the wave's by sc_wave.h's shuffles, the four
// waves' through LDS in a fixed order; a plane's total is added up from its parts by every workgroup that needs it, again in one
// order -- two runs of a call give the same bytes.
#include "sc_pcg_device.h"
#include <cmath>

namespace sc {

namespace {

// a plane's total from its n parts: the calling wave's 64 lanes stride through them, then the butterfly
__device__ __forceinline__ double parts_sum(const double *__restrict__ p, int n, int lane)
{
    double m = 0.0;
    for (int i = lane; i < n; i += 64) m += p[i];
    return wave_sum(m);
}

// a / b as the float the update multiplies by; 0 when the quotient is not finite (a plane whose residual is exactly zero)
__device__ __forceinline__ float safe_ratio(double a, double b)
{
    const double q = a / b;
    return (q == q && fabs(q) <= 3.0e38) ? (float)q : 0.f;
}

__global__ __launch_bounds__(WL) void k_w_stats(PoissonGeo g, WeightedGeo wg, WeightedJobs t, double *__restrict__ stats)
{
    __shared__ double ws[4], wb[4];
    const int p = (int)blockIdx.z, member = p / g.C, c = p - member * g.C, x = (int)blockIdx.x * WL + (int)threadIdx.x;
    const int y0 = (int)blockIdx.y * wg.rows, y1 = min(y0 + wg.rows, wg.ny);
    const float *__restrict__ w = t.w[member];
    double s = 0.0, bad = 0.0;
    if (x < wg.nx)
        for (int y = y0; y < y1; ++y) {
            const float v = w[(long long)(wg.x0 + x) * g.cs + (long long)(wg.y0 + y) * g.rs + (long long)c * g.chs];
            if (!(v >= 0.f) || v > 3.4028234e38f) bad += 1.0;
            s += (double)v;
        }
    s = block_sum(s, ws);
    bad = block_sum(bad, wb);
    if (threadIdx.x == 0) {
        double *o = stats + ((size_t)p * WEIGHTED_PARTS + blockIdx.y * wg.cg + blockIdx.x) * 2;
        o[0] = s;
        o[1] = bad;
    }
}

template <bool LAP>
__global__ __launch_bounds__(WL) void k_w_setup(PoissonGeo g, WeightedGeo wg, WeightedJobs t, float *__restrict__ R, float *__restrict__ Wc,
                                                 double *__restrict__ bb)
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
            const float wv = w[o];
            float v = screened_rhs(dct_rhs<LAP>(g, j, c, X, Y, px, py), wv, j.d[o]);
            if (X == 1 && mixed_low_d(wg.ax)) v -= j.b[o - g.cs];
            if (Y == 1 && mixed_low_d(wg.ay)) v -= j.b[o - g.rs];
            if (X == g.W - 2 && mixed_high_d(wg.ax)) v -= j.b[o + g.cs];
            if (Y == g.H - 2 && mixed_high_d(wg.ay)) v -= j.b[o + g.rs];
            const size_t i = (size_t)p * wg.stride + (size_t)y * wg.nx + x;
            R[i] = v;
            Wc[i] = wv;
            s += (double)v * (double)v;
        }
    s = block_sum(s, ws);
    if (threadIdx.x == 0) bb[(size_t)p * WEIGHTED_PARTS + blockIdx.y * wg.cg + blockIdx.x] = s;
}

// RES false: Q = (A - W) P and the parts of P . Q;  true: Q -= (A - W) P and the parts of Q . Q
template <bool RES>
__global__ __launch_bounds__(WL) void k_w_op(WeightedGeo wg, const float *__restrict__ P, const float *__restrict__ Wc, float *__restrict__ Q,
                                              double *__restrict__ parts)
{
    __shared__ double ws[4];
    const int x = (int)blockIdx.x * WL + (int)threadIdx.x, nx = wg.nx, ny = wg.ny;
    const int y0 = (int)blockIdx.y * wg.rows, y1 = min(y0 + wg.rows, ny);
    const size_t base = (size_t)blockIdx.z * wg.stride;
    const float *__restrict__ pl = P + base;
    const bool px = wg.ax == MIXED_PERIODIC, py = wg.ay == MIXED_PERIODIC;
    double s = 0.0;
    if (x < nx) {
        // the neighbours of this column: its index (-1: none, the value is 0) and whether the term exists at all (it does not beyond a free end)
        int xl = x - 1, xr = x + 1;
        float cnt_x = 2.f;
        if (x == 0) { xl = px ? nx - 1 : -1; if (!px && !mixed_low_d(wg.ax)) cnt_x -= 1.f; }
        if (x == nx - 1) { xr = px ? 0 : -1; if (!px && !mixed_high_d(wg.ax)) cnt_x -= 1.f; }
        auto row_above = [&](int y) { return y > 0 ? y - 1 : py ? ny - 1 : -1; };
        auto row_below = [&](int y) { return y < ny - 1 ? y + 1 : py ? 0 : -1; };
        int ya = row_above(y0);
        float up = ya >= 0 ? pl[(size_t)ya * nx + x] : 0.f, cur = pl[(size_t)y0 * nx + x];
        for (int y = y0; y < y1; ++y) {
            const int yb = row_below(y);
            const float dn = yb >= 0 ? pl[(size_t)yb * nx + x] : 0.f;
            const float *__restrict__ row = pl + (size_t)y * nx;
            const float l = xl >= 0 ? row[xl] : 0.f, r = xr >= 0 ? row[xr] : 0.f;
            float cnt = cnt_x + 2.f;
            if (y == 0 && !py && !mixed_low_d(wg.ay)) cnt -= 1.f;
            if (y == ny - 1 && !py && !mixed_high_d(wg.ay)) cnt -= 1.f;
            const size_t i = base + (size_t)y * nx + x;
            const float v = (((l + r) + (up + dn)) - cnt * cur) - Wc[i] * cur;
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
        }
    }
    s = block_sum(s, ws);
    if (threadIdx.x == 0) parts[(size_t)blockIdx.z * WEIGHTED_PARTS + blockIdx.y * wg.cg + blockIdx.x] = s;
}

__global__ __launch_bounds__(WL) void k_w_update(WeightedGeo wg, float *__restrict__ U, float *__restrict__ R, const float *__restrict__ P,
                                                  const float *__restrict__ Q, const double *__restrict__ rz, const double *__restrict__ pq,
                                                  double *__restrict__ rr)
{
    __shared__ double ws[4];
    __shared__ float s_alpha;
    const int tid = (int)threadIdx.x, plane = (int)blockIdx.y, n = wg.nx * wg.ny;
    if (tid < 64) {
        const double rho = parts_sum(rz + (size_t)plane * WEIGHTED_PARTS, wg.eparts, tid);
        const double den = parts_sum(pq + (size_t)plane * WEIGHTED_PARTS, wg.cg * wg.bands, tid);
        if (tid == 0) s_alpha = safe_ratio(rho, den);
    }
    __syncthreads();
    const float alpha = s_alpha;
    const size_t base = (size_t)plane * wg.stride;
    int g0, g1;
    segment(wg, (int)blockIdx.x, g0, g1);
    double s = 0.0;
    for (int gi = g0 + tid; gi < g1; gi += WL) {
        const size_t i = base + (size_t)gi * 4;
        if (gi * 4 + 3 < n) {
            float4 u = *reinterpret_cast<float4 *>(U + i), r = *reinterpret_cast<float4 *>(R + i);
            const float4 p = *reinterpret_cast<const float4 *>(P + i), q = *reinterpret_cast<const float4 *>(Q + i);
            u.x += alpha * p.x; u.y += alpha * p.y; u.z += alpha * p.z; u.w += alpha * p.w;
            r.x -= alpha * q.x; r.y -= alpha * q.y; r.z -= alpha * q.z; r.w -= alpha * q.w;
            *reinterpret_cast<float4 *>(U + i) = u;
            *reinterpret_cast<float4 *>(R + i) = r;
            s += ((double)r.x * r.x + (double)r.y * r.y) + ((double)r.z * r.z + (double)r.w * r.w);
        } else {
            for (int k = gi * 4; k < n; ++k) {
                const size_t e = base + k;
                U[e] += alpha * P[e];
                const float r = R[e] - alpha * Q[e];
                R[e] = r;
                s += (double)r * r;
            }
        }
    }
    s = block_sum(s, ws);
    if (tid == 0) rr[(size_t)plane * WEIGHTED_PARTS + blockIdx.x] = s;
}

__global__ __launch_bounds__(WL) void k_w_dot(WeightedGeo wg, const float *__restrict__ R, const float *__restrict__ Z, double *__restrict__ rz,
                                               const double *__restrict__ rr, int nrr, double *__restrict__ rr_tot)
{
    __shared__ double ws[4];
    const int tid = (int)threadIdx.x, plane = (int)blockIdx.y, n = wg.nx * wg.ny;
    if (blockIdx.x == 0 && tid < 64) {
        const double t = parts_sum(rr + (size_t)plane * WEIGHTED_PARTS, nrr, tid);
        if (tid == 0) rr_tot[plane] = t;
    }
    const size_t base = (size_t)plane * wg.stride;
    int g0, g1;
    segment(wg, (int)blockIdx.x, g0, g1);
    double s = 0.0;
    for (int gi = g0 + tid; gi < g1; gi += WL) {
        const size_t i = base + (size_t)gi * 4;
        if (gi * 4 + 3 < n) {
            const float4 r = *reinterpret_cast<const float4 *>(R + i), z = *reinterpret_cast<const float4 *>(Z + i);
            s += ((double)r.x * z.x + (double)r.y * z.y) + ((double)r.z * z.z + (double)r.w * z.w);
        } else {
            for (int k = gi * 4; k < n; ++k) s += (double)R[base + k] * Z[base + k];
        }
    }
    s = block_sum(s, ws);
    if (tid == 0) rz[(size_t)plane * WEIGHTED_PARTS + blockIdx.x] = s;
}

__global__ __launch_bounds__(WL) void k_w_dir(WeightedGeo wg, float *__restrict__ P, const float *__restrict__ Z, const double *__restrict__ rz,
                                               const double *__restrict__ rz_old)
{
    __shared__ float s_beta;
    const int tid = (int)threadIdx.x, plane = (int)blockIdx.y, n = wg.nx * wg.ny;
    if (tid < 64) {
        float beta = 0.f;
        if (rz_old) {
            const double a = parts_sum(rz + (size_t)plane * WEIGHTED_PARTS, wg.eparts, tid);
            const double b = parts_sum(rz_old + (size_t)plane * WEIGHTED_PARTS, wg.eparts, tid);
            beta = safe_ratio(a, b);
        }
        if (tid == 0) s_beta = beta;
    }
    __syncthreads();
    const float beta = s_beta;
    const size_t base = (size_t)plane * wg.stride;
    int g0, g1;
    segment(wg, (int)blockIdx.x, g0, g1);
    for (int gi = g0 + tid; gi < g1; gi += WL) {
        const size_t i = base + (size_t)gi * 4;
        if (gi * 4 + 3 < n) {
            float4 p = *reinterpret_cast<float4 *>(P + i);
            const float4 z = *reinterpret_cast<const float4 *>(Z + i);
            p.x = z.x + beta * p.x; p.y = z.y + beta * p.y; p.z = z.z + beta * p.z; p.w = z.w + beta * p.w;
            *reinterpret_cast<float4 *>(P + i) = p;
        } else {
            for (int k = gi * 4; k < n; ++k) P[base + k] = Z[base + k] + beta * P[base + k];
        }
    }
}

__global__ __launch_bounds__(WL) void k_w_out(PoissonGeo g, WeightedGeo wg, PoissonJobs t, const float *__restrict__ U)
{
    const int p = (int)blockIdx.z, member = p / g.C, c = p - member * g.C, x = (int)blockIdx.x * WL + (int)threadIdx.x, y = (int)blockIdx.y;
    if (x >= g.W) return;
    const PoissonJobDev &j = t.j[member];
    const long long o = (long long)x * g.cs + (long long)y * g.rs + (long long)c * g.chs;
    const int ux = x - wg.x0, uy = y - wg.y0;
    if (ux >= 0 && ux < wg.nx && uy >= 0 && uy < wg.ny) j.out[o] = U[(size_t)p * wg.stride + (size_t)uy * wg.nx + ux];
    else j.out[o] = j.b[o];          // a Dirichlet line (out may be boundary: the same value again)
}

template <typename Fn>
void w_chunks(const PoissonJobDev *jobs, const float *const *w, int m, Fn fn)
{
    for (int i0 = 0; i0 < m; i0 += WeightedJobs::MAX) {
        WeightedJobs t{};
        const int cnt = std::min(m - i0, (int)WeightedJobs::MAX);
        for (int i = 0; i < cnt; ++i) { t.j[i] = jobs[i0 + i]; t.w[i] = w ? w[i0 + i] : nullptr; }
        fn(t, i0, cnt);
    }
}

} // namespace

WeightedGeo weighted_geo(const MixedGeo &mg)
{
    WeightedGeo wg{};
    wg.nx = mg.nx; wg.ny = mg.ny; wg.ax = mg.ax; wg.ay = mg.ay;
    wg.x0 = mixed_low_d(mg.ax) ? 1 : 0;
    wg.y0 = mixed_low_d(mg.ay) ? 1 : 0;
    wg.cg = (mg.nx + WL - 1) / WL;                               // <= 32 at 8192 unknowns
    const int max_bands = std::max(1, WEIGHTED_PARTS / wg.cg);
    wg.bands = std::min(max_bands, (mg.ny + 7) / 8);             // at least 8 rows per band: the two halo rows cost a quarter at most
    wg.rows = (mg.ny + wg.bands - 1) / wg.bands;
    wg.bands = (mg.ny + wg.rows - 1) / wg.rows;
    const long long n = (long long)mg.nx * mg.ny;
    wg.egroups = (int)((n + 3) / 4);
    wg.eparts = (int)std::min<long long>(WEIGHTED_PARTS, (wg.egroups + 4 * WL - 1) / (4 * WL));      // 16 floats per lane at least, where the plane has them
    wg.stride = (n + 63) / 64 * 64;                             // planes start on a 256-byte boundary
    return wg;
}

void launch_weighted_stats(const PoissonGeo &g, const WeightedGeo &wg, const PoissonJobDev *jobs, const float *const *w, int m, double *stats,
                           hipStream_t s)
{
    w_chunks(jobs, w, m, [&](const WeightedJobs &t, int i0, int cnt) {
        hipLaunchKernelGGL(k_w_stats, dim3((unsigned)wg.cg, (unsigned)wg.bands, (unsigned)(g.C * cnt)), dim3(WL), 0, s, g, wg, t,
                           stats + (size_t)g.C * i0 * WEIGHTED_PARTS * 2);
    });
}

void launch_weighted_setup(const PoissonGeo &g, const WeightedGeo &wg, bool lap, const PoissonJobDev *jobs, const float *const *w, int m, float *R,
                           float *Wc, double *bb, hipStream_t s)
{
    w_chunks(jobs, w, m, [&](const WeightedJobs &t, int i0, int cnt) {
        const dim3 grid((unsigned)wg.cg, (unsigned)wg.bands, (unsigned)(g.C * cnt));
        const size_t p0 = (size_t)g.C * i0;
        if (lap) hipLaunchKernelGGL(k_w_setup<true>, grid, dim3(WL), 0, s, g, wg, t, R + p0 * wg.stride, Wc + p0 * wg.stride, bb + p0 * WEIGHTED_PARTS);
        else hipLaunchKernelGGL(k_w_setup<false>, grid, dim3(WL), 0, s, g, wg, t, R + p0 * wg.stride, Wc + p0 * wg.stride, bb + p0 * WEIGHTED_PARTS);
    });
}

void launch_weighted_op(const WeightedGeo &wg, int planes, bool residual, const float *P, const float *Wc, float *Q, double *parts, hipStream_t s)
{
    const dim3 grid((unsigned)wg.cg, (unsigned)wg.bands, (unsigned)planes);
    if (residual) hipLaunchKernelGGL(k_w_op<true>, grid, dim3(WL), 0, s, wg, P, Wc, Q, parts);
    else hipLaunchKernelGGL(k_w_op<false>, grid, dim3(WL), 0, s, wg, P, Wc, Q, parts);
}

void launch_weighted_update(const WeightedGeo &wg, int planes, float *U, float *R, const float *P, const float *Q, const double *rz, const double *pq,
                            double *rr, hipStream_t s)
{
    hipLaunchKernelGGL(k_w_update, dim3((unsigned)wg.eparts, (unsigned)planes), dim3(WL), 0, s, wg, U, R, P, Q, rz, pq, rr);
}

void launch_weighted_dot(const WeightedGeo &wg, int planes, const float *R, const float *Z, double *rz, const double *rr, int nrr, double *rr_tot,
                         hipStream_t s)
{
    hipLaunchKernelGGL(k_w_dot, dim3((unsigned)wg.eparts, (unsigned)planes), dim3(WL), 0, s, wg, R, Z, rz, rr, nrr, rr_tot);
}

void launch_weighted_dir(const WeightedGeo &wg, int planes, float *P, const float *Z, const double *rz, const double *rz_old, hipStream_t s)
{
    hipLaunchKernelGGL(k_w_dir, dim3((unsigned)wg.eparts, (unsigned)planes), dim3(WL), 0, s, wg, P, Z, rz, rz_old);
}

void launch_weighted_out(const PoissonGeo &g, const WeightedGeo &wg, const PoissonJobDev *jobs, int m, const float *U, hipStream_t s)
{
    w_chunks(jobs, nullptr, m, [&](const WeightedJobs &t, int i0, int cnt) {
        PoissonJobs pj{};
        for (int i = 0; i < cnt; ++i) pj.j[i] = t.j[i];
        hipLaunchKernelGGL(k_w_out, dim3((unsigned)((g.W + WL - 1) / WL), (unsigned)g.H, (unsigned)(g.C * cnt)), dim3(WL), 0, s, g, wg, pj,
                           U + (size_t)g.C * i0 * wg.stride);
    });
}

} // namespace sc
