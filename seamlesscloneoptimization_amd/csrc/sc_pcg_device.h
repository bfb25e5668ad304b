// sc_pcg_device.h -- what the kernels of the conjugate-gradient families share (sc_pcg.hip, sc_weighted.hip, sc_wls.hip): the workgroup's
// size and its sum in one fixed order, and one walk of each kind over the work planes (sc_pcg.h, PcgGeo) -- the element-wise walk of a
// segment's float4 groups, the band of a statistics or set-up launch, and the operator's walk with a family's coefficients as a policy,
// and the robust penalties' arithmetic with the coupled forms' side tables (sc_robust.hip, sc_region_robust.hip, sc_volume_robust.hip).
#pragma once
#include "sc_pcg.h"
#include "sc_wave.h"
#include <algorithm>
#include <type_traits>

namespace sc {

constexpr int WL = 256;      // lanes per workgroup

// the workgroup's sum (valid in every lane after the barrier); ws: 4 doubles of LDS of this call's own
__device__ __forceinline__ double block_sum(double v, double *ws)
{
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = v;
    __syncthreads();
    return (ws[0] + ws[1]) + (ws[2] + ws[3]);
}

// a * b rounded to float32 on its own: never one half of a fused multiply-add, whatever the translation unit's contraction setting
// (the product is opaque to the optimiser, as in screened_rhs)
__device__ __forceinline__ float rounded_product(float a, float b)
{
    float t = a * b;
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(t));
#endif
    return t;
}

// The element-wise walk (grid: eparts x planes): segment blockIdx.x of plane blockIdx.y is `per` float4 groups, a lane takes every
// WL-th of them; group(i) for a whole group at float offset i, tail(e) for each float of the plane's last, partial group.
template <class Group, class Tail>
__device__ __forceinline__ void pcg_elements(const PcgGeo &wg, Group group, Tail tail)
{
    const int n = wg.nx * wg.ny, per = (wg.egroups + wg.eparts - 1) / wg.eparts;
    const int g0 = (int)blockIdx.x * per, g1 = min(g0 + per, wg.egroups);
    const size_t base = (size_t)blockIdx.y * wg.stride;
    for (int gi = g0 + (int)threadIdx.x; gi < g1; gi += WL) {
        if (gi * 4 + 3 < n) group(base + (size_t)gi * 4);
        else
            for (int k = gi * 4; k < n; ++k) tail(base + k);
    }
}
__device__ __forceinline__ float4 ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ void st4(float *p, float4 v) { *reinterpret_cast<float4 *>(p) = v; }
// a group's share of a lane's double sum, in the one order every such sum is added
__device__ __forceinline__ double dot4(float4 a, float4 b)
{
    return ((double)a.x * b.x + (double)a.y * b.y) + ((double)a.z * b.z + (double)a.w * b.w);
}

// The band of a statistics or set-up launch (grid: cg x bands x planes): plane p = member C + channel c, this lane's column x of the
// unknowns (one only where x < nx), rows [y0, y1); pixel(g, X, Y): the offset of pixel (X, Y) = (x0 + x, y0 + y) of the channel under
// the call's layout.  (The kernels keep their own row loop and work-plane index: behind a helper that takes the geometry they cost
// scalar registers.)
struct PcgBand {
    int p, member, c, x, y0, y1;
    __device__ __forceinline__ PcgBand(const PoissonGeo &g, const PcgGeo &wg)
    {
        p = (int)blockIdx.z; member = p / g.C; c = p - member * g.C; x = (int)blockIdx.x * WL + (int)threadIdx.x;
        y0 = (int)blockIdx.y * wg.rows; y1 = min(y0 + wg.rows, wg.ny);
    }
    __device__ __forceinline__ long long pixel(const PoissonGeo &g, int X, int Y) const { return (long long)X * g.cs + (long long)Y * g.rs + (long long)c * g.chs; }
};
// the workgroup's sum of v into field f of its part: parts[(plane * PCG_PARTS + band * cg + column group) * per + f]
__device__ __forceinline__ void part_store(double v, double *ws, const PcgGeo &wg, double *__restrict__ parts, int per = 1, int f = 0)
{
    v = block_sum(v, ws);
    if (threadIdx.x == 0) parts[((size_t)blockIdx.z * PCG_PARTS + blockIdx.y * wg.cg + blockIdx.x) * per + f] = v;
}

// ---- the robust penalties (sc_robust.hip, sc_region_robust.hip, sc_volume_robust.hip): one term as RobustTerm states it (sc_pcg.h)
// rho_r(t), and q = t t + eps eps (r = 2: t t; eps is unused there)
__device__ __forceinline__ float robust_rho(const RobustTerm &r, float t, float &q)
{
    q = rounded_product(t, t);
    if (r.mode == 0) return 1.f;
    q = q + r.eps2;
    return r.mode == 1 ? 1.0f / sqrtf(q) : powf(q, r.half_exp);
}
// one term of the energy, base phi_r(t), in double from rho's float32 values: (2 / r) q rho = (2 / r) q^(r/2)
__device__ __forceinline__ double robust_phi(const RobustTerm &r, float base, float q, float rho)
{
    return (double)base * ((double)r.scale * ((double)q * (double)rho));
}
// a link: its weight s = base rho_p(t), t = (hi - lo) - g, and its energy
struct RobustLink { float s; double e; };
__device__ __forceinline__ RobustLink robust_link(const RobustTerm &r, float base, float hi, float lo, float g)
{
    float q;
    const float t = (hi - lo) - g, rho = robust_rho(r, t, q);
    RobustLink k;
    k.s = r.mode == 0 ? base : rounded_product(base, rho);
    k.e = robust_phi(r, base, q, rho);
    return k;
}

// the penalties' constants in vector registers: the region and volume walks are short of scalar ones
__device__ __forceinline__ void lane_term(RobustTerm &r)
{
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(r.eps2), "+v"(r.half_exp), "+v"(r.scale));
#endif
}
// The data term at the iterate: w' = w rho_q(u - d) (the return value), rhs = screened_rhs(rhs, w', d), e = the term's energy
__device__ __forceinline__ float robust_data(const RobustTerm &r, float wv, float dv, float uc, float &rhs, double &e)
{
    float q;
    const float rho = robust_rho(r, uc - dv, q), wr = r.mode == 0 ? wv : rounded_product(wv, rho);
    rhs = screened_rhs(rhs, wr, dv);
    e = robust_phi(r, wv, q, rho);
    return wr;
}

// ---- the coupled forms (sc_robust.hip: their definitions): the rho planes' geometry, a link's share c t^2 of a magnitude (BASE: with
// the base link c[o]; false: 1, no multiply), rho_p(M) with the magnitude's energy (2 / p) Q rho in double from the float32 Q and rho
struct RhoGeo { int rw, ncomp; long long rstride; };
template <bool BASE>
__device__ __forceinline__ float robust_sq(const float *__restrict__ c, long long o, float t)
{
    const float q = rounded_product(t, t);
    return BASE ? rounded_product(c[o], q) : q;
}
__device__ __forceinline__ float coupled_rho(const RobustTerm &r, float m, double &e)
{
    const float q = m + r.eps2, rho = r.mode == 1 ? 1.0f / sqrtf(q) : powf(q, r.half_exp);
    e = (double)r.scale * ((double)q * (double)rho);
    return rho;
}
// The coupled forms' launches of every side table (host): fn(iso, joint, t, cnt, rg, o, po, ro) -- iso, joint: the form as
// std::bool_constant, for the kernels' template arguments; o, po, ro: the first job's offset into the work planes, into the parts (per
// double of a part) and into the rho planes
template <class Table, class Fn>
void for_coupled_tables(const PoissonGeo &g, const PcgGeo &wg, const PoissonJobDev *jobs, const SideArrays *sides, int m, int coupling, Fn fn)
{
    const bool iso = (coupling & ROBUST_ISO) != 0, joint = (coupling & ROBUST_JOINT) != 0;
    const RhoGeo rg{ wg.x0 + wg.nx, iso ? 1 : 2, robust_rho_stride(wg) };
    for_side_tables<Table>(jobs, sides, m, [&](const Table &t, int i0, int cnt) {
        const size_t o = (size_t)g.C * i0 * wg.stride, po = (size_t)g.C * i0 * PCG_PARTS;
        const size_t ro = (size_t)(joint ? i0 : g.C * i0) * rg.ncomp * rg.rstride;
        if (iso && joint) fn(std::true_type(), std::true_type(), t, cnt, rg, o, po, ro);
        else if (iso) fn(std::true_type(), std::false_type(), t, cnt, rg, o, po, ro);
        else fn(std::false_type(), std::true_type(), t, cnt, rg, o, po, ro);
    });
}

// The operator's launch (grid: cg x bands x planes), one kernel for every family.  RES false: Q = L P and the parts of P . Q;  true:
// Q -= L P and the parts of Q . Q.  A lane owns one column of its band, keeps the row above, its own and the row below in registers, and
// reads the left and right neighbours from the cache lines its wave loads anyway -- no LDS, no barrier inside the walk.  A neighbour that
// does not exist (beyond a free end or a Dirichlet line) has index -1 and the value 0.  The family's coefficients are the policy K, built
// from the launch's coefficient planes `coef` (the kernel has no others to read): start(wg, base, x, ya) once per lane (base: the
// plane's first element, ya: the row above the band, -1: none), then per row value(wg, x, xl, y, ro, i, l, r, up, dn, cur) = (L P) at element i = base + ro + x (ro = y nx; xl: the left column, -1: none), which loads the
// row's coefficients and rolls whatever the policy carries from row to row.  (The walk is the kernel itself and not a function under
// two kernels: inlined from a function it cost the WLS instantiation two scalar registers.)
template <bool RES, class K, class... C>
__global__ __launch_bounds__(WL) void k_pcg_op(PcgGeo wg, const float *__restrict__ P, float *__restrict__ Q, double *__restrict__ parts,
                                                const C *__restrict__... coef)
{
    __shared__ double ws[4];
    K k{ coef... };
    const int x = (int)blockIdx.x * WL + (int)threadIdx.x, nx = wg.nx, ny = wg.ny;
    const int y0 = (int)blockIdx.y * wg.rows, y1 = min(y0 + wg.rows, ny);
    const size_t base = (size_t)blockIdx.z * wg.stride;
    const float *__restrict__ pl = P + base;
    double s = 0.0;
    if (x < nx) {
        const bool px = wg.ax == MIXED_PERIODIC, py = wg.ay == MIXED_PERIODIC;
        const int xl = x > 0 ? x - 1 : px ? nx - 1 : -1, xr = x < nx - 1 ? x + 1 : px ? 0 : -1;
        auto row_above = [&](int y) { return y > 0 ? y - 1 : py ? ny - 1 : -1; };
        auto row_below = [&](int y) { return y < ny - 1 ? y + 1 : py ? 0 : -1; };
        const int ya = row_above(y0);
        float up = ya >= 0 ? pl[(size_t)ya * nx + x] : 0.f, cur = pl[(size_t)y0 * nx + x];
        k.start(wg, base, x, ya);
        for (int y = y0; y < y1; ++y) {
            const int yb = row_below(y);
            const float dn = yb >= 0 ? pl[(size_t)yb * nx + x] : 0.f;
            const size_t ro = (size_t)y * nx;
            const float l = xl >= 0 ? pl[ro + xl] : 0.f, r = xr >= 0 ? pl[ro + xr] : 0.f;
            const size_t i = base + ro + x;
            const float v = k.value(wg, x, xl, y, ro, i, l, r, up, dn, cur);
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
    part_store(s, ws, wg, parts);
}

} // namespace sc
