// sc_pcg.hip -- the kernels every conjugate-gradient family launches (sc_pcg.cpp drives them): update, dot, direction, the one-off scale
// of the start, the jobs' output, and the work planes' geometry.  Both L and the preconditioner A - lam are negative definite; the
// iteration is the textbook one with both signs flipped, which changes no quotient: alpha = (r . z) / (p . L p), beta = (r . z)' / (r . z).
// Every launch covers all planes of the chunk.  Reductions: a lane's running sum in double, the wave's by sc_wave.h's shuffles, the four
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

__global__ __launch_bounds__(WL) void k_pcg_update(PcgGeo wg, float *__restrict__ U, float *__restrict__ R, const float *__restrict__ P,
                                                    const float *__restrict__ Q, const double *__restrict__ rz, const double *__restrict__ pq,
                                                    double *__restrict__ rr)
{
    __shared__ double ws[4];
    __shared__ float s_alpha;
    const int tid = (int)threadIdx.x, plane = (int)blockIdx.y;
    if (tid < 64) {
        const double rho = parts_sum(rz + (size_t)plane * PCG_PARTS, wg.eparts, tid);
        const double den = parts_sum(pq + (size_t)plane * PCG_PARTS, wg.cg * wg.bands, tid);
        if (tid == 0) s_alpha = safe_ratio(rho, den);
    }
    __syncthreads();
    const float alpha = s_alpha;
    double s = 0.0;
    pcg_elements(wg, [&](size_t i) {
        float4 u = ld4(U + i), r = ld4(R + i);
        const float4 p = ld4(P + i), q = ld4(Q + i);
        u.x += alpha * p.x; u.y += alpha * p.y; u.z += alpha * p.z; u.w += alpha * p.w;
        r.x -= alpha * q.x; r.y -= alpha * q.y; r.z -= alpha * q.z; r.w -= alpha * q.w;
        st4(U + i, u);
        st4(R + i, r);
        s += dot4(r, r);
    }, [&](size_t e) {
        U[e] += alpha * P[e];
        const float r = R[e] - alpha * Q[e];
        R[e] = r;
        s += (double)r * r;
    });
    s = block_sum(s, ws);
    if (tid == 0) rr[(size_t)plane * PCG_PARTS + blockIdx.x] = s;
}

__global__ __launch_bounds__(WL) void k_pcg_dot(PcgGeo wg, const float *__restrict__ R, const float *__restrict__ Z, double *__restrict__ rz,
                                                 const double *__restrict__ rr, int nrr, double *__restrict__ rr_tot)
{
    __shared__ double ws[4];
    const int tid = (int)threadIdx.x, plane = (int)blockIdx.y;
    if (blockIdx.x == 0 && tid < 64) {
        const double t = parts_sum(rr + (size_t)plane * PCG_PARTS, nrr, tid);
        if (tid == 0) rr_tot[plane] = t;
    }
    double s = 0.0;
    pcg_elements(wg, [&](size_t i) { s += dot4(ld4(R + i), ld4(Z + i)); }, [&](size_t e) { s += (double)R[e] * Z[e]; });
    s = block_sum(s, ws);
    if (tid == 0) rz[(size_t)plane * PCG_PARTS + blockIdx.x] = s;
}

__global__ __launch_bounds__(WL) void k_pcg_dir(PcgGeo wg, float *__restrict__ P, const float *__restrict__ Z, const double *__restrict__ rz,
                                                 const double *__restrict__ rz_old)
{
    __shared__ float s_beta;
    const int tid = (int)threadIdx.x, plane = (int)blockIdx.y;
    if (tid < 64) {
        float beta = 0.f;
        if (rz_old) {
            const double a = parts_sum(rz + (size_t)plane * PCG_PARTS, wg.eparts, tid);
            const double b = parts_sum(rz_old + (size_t)plane * PCG_PARTS, wg.eparts, tid);
            beta = safe_ratio(a, b);
        }
        if (tid == 0) s_beta = beta;
    }
    __syncthreads();
    const float beta = s_beta;
    pcg_elements(wg, [&](size_t i) {
        float4 p = ld4(P + i);
        const float4 z = ld4(Z + i);
        p.x = z.x + beta * p.x; p.y = z.y + beta * p.y; p.z = z.z + beta * p.z; p.w = z.w + beta * p.w;
        st4(P + i, p);
    }, [&](size_t e) { P[e] = Z[e] + beta * P[e]; });
}

__global__ __launch_bounds__(WL) void k_pcg_scale(PcgGeo wg, float *__restrict__ U, float f)
{
    pcg_elements(wg, [&](size_t i) {
        float4 u = ld4(U + i);
        u.x *= f; u.y *= f; u.z *= f; u.w *= f;
        st4(U + i, u);
    }, [&](size_t e) { U[e] *= f; });
}

__global__ __launch_bounds__(WL) void k_pcg_out(PoissonGeo g, PcgGeo wg, PoissonJobs t, const float *__restrict__ U)
{
    const int p = (int)blockIdx.z, member = p / g.C, c = p - member * g.C, x = (int)blockIdx.x * WL + (int)threadIdx.x, y = (int)blockIdx.y;
    if (x >= g.W) return;
    const PoissonJobDev &j = t.j[member];
    const long long o = (long long)x * g.cs + (long long)y * g.rs + (long long)c * g.chs;
    const int ux = x - wg.x0, uy = y - wg.y0;
    if (ux >= 0 && ux < wg.nx && uy >= 0 && uy < wg.ny) j.out[o] = U[(size_t)p * wg.stride + (size_t)uy * wg.nx + ux];
    else j.out[o] = j.b[o];          // a Dirichlet line (out may be boundary: the same value again)
}

} // namespace

PcgGeo pcg_geo(const MixedGeo &mg)
{
    PcgGeo wg{};
    wg.nx = mg.nx; wg.ny = mg.ny; wg.ax = mg.ax; wg.ay = mg.ay;
    wg.x0 = mixed_low_d(mg.ax) ? 1 : 0;
    wg.y0 = mixed_low_d(mg.ay) ? 1 : 0;
    wg.cg = (mg.nx + WL - 1) / WL;                               // <= 32 at 8192 unknowns
    const int max_bands = std::max(1, PCG_PARTS / wg.cg);
    wg.bands = std::min(max_bands, (mg.ny + 7) / 8);             // at least 8 rows per band: the two halo rows cost a quarter at most
    wg.rows = (mg.ny + wg.bands - 1) / wg.bands;
    wg.bands = (mg.ny + wg.rows - 1) / wg.rows;
    const long long n = (long long)mg.nx * mg.ny;
    wg.egroups = (int)((n + 3) / 4);
    wg.eparts = (int)std::min<long long>(PCG_PARTS, (wg.egroups + 4 * WL - 1) / (4 * WL));      // 16 floats per lane at least, where the plane has them
    wg.stride = (n + 63) / 64 * 64;                             // planes start on a 256-byte boundary
    return wg;
}

void launch_pcg_update(const PcgGeo &wg, int planes, float *U, float *R, const float *P, const float *Q, const double *rz, const double *pq, double *rr, hipStream_t s)
{
    hipLaunchKernelGGL(k_pcg_update, dim3((unsigned)wg.eparts, (unsigned)planes), dim3(WL), 0, s, wg, U, R, P, Q, rz, pq, rr);
}

void launch_pcg_dot(const PcgGeo &wg, int planes, const float *R, const float *Z, double *rz, const double *rr, int nrr, double *rr_tot, hipStream_t s)
{
    hipLaunchKernelGGL(k_pcg_dot, dim3((unsigned)wg.eparts, (unsigned)planes), dim3(WL), 0, s, wg, R, Z, rz, rr, nrr, rr_tot);
}

void launch_pcg_dir(const PcgGeo &wg, int planes, float *P, const float *Z, const double *rz, const double *rz_old, hipStream_t s)
{
    hipLaunchKernelGGL(k_pcg_dir, dim3((unsigned)wg.eparts, (unsigned)planes), dim3(WL), 0, s, wg, P, Z, rz, rz_old);
}

void launch_pcg_scale(const PcgGeo &wg, int planes, float *U, float f, hipStream_t s)
{
    hipLaunchKernelGGL(k_pcg_scale, dim3((unsigned)wg.eparts, (unsigned)planes), dim3(WL), 0, s, wg, U, f);
}

void launch_pcg_out(const PoissonGeo &g, const PcgGeo &wg, const PoissonJobDev *jobs, int m, const float *U, hipStream_t s)
{
    for_job_tables<PoissonJobs>(m, [&](PoissonJobs &t, int i, int k) { t.j[i] = jobs[k]; }, [&](const PoissonJobs &t, int i0, int cnt) {
        hipLaunchKernelGGL(k_pcg_out, dim3((unsigned)((g.W + WL - 1) / WL), (unsigned)g.H, (unsigned)(g.C * cnt)), dim3(WL), 0, s, g, wg, t,
                           U + (size_t)g.C * i0 * wg.stride);
    });
}

} // namespace sc
