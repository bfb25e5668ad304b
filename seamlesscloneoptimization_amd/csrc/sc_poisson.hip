// sc_poisson.hip -- the two launches around the solve of sc_hip_poisson (host side in sc_poisson_api.cpp): the pre-process reads
// the caller's strided float32 arrays into the fields the solvers expect, the output launch writes the solution back.
//
// The field contract is k_edit_preprocess's: U0 = boundary on the whole image (frame and interior, 0 in the pad columns up to the
// next multiple of four), F = the right-hand side on the interior, 0 on the frame and in the pads.  Member k of a group owns
// channels C k .. C k + C - 1 of the fields (blockIdx.z = k inside a launch of up to 16 members).
//
// Lanes: one element (x, c) of an image row per lane, ROWS rows per workgroup walked top to bottom.  The lane space of a row is
// (x, c) with c inner when the layout interleaves the channels (channel_stride < col_stride: HWC, RGBA-strided) and x inner
// otherwise (planar CHW), so consecutive lanes read consecutive floats of the two common layouts.  Element (x - 1, c) of the same
// row is then D lanes to the left (D = C interleaved, 1 planar): gx(q - x) comes from that lane through LDS, and gy(q - y) stays in
// a register from the row before -- every guidance element is read once by one lane (plus one row and D elements of halo per
// workgroup).
#include "sc_common.h"
#include "sc_wave.h"
#include <hip/hip_runtime.h>
#include <algorithm>
#include <type_traits>

namespace sc {

constexpr int PS_LANES = 256, PS_ROWS = 16;

// the lane's element of the row space: (x, c); false beyond the row (E elements)
__device__ __forceinline__ bool ps_lane(const PoissonGeo &g, bool inter, int wcols, int &x, int &c)
{
    const int e = (int)blockIdx.x * PS_LANES + (int)threadIdx.x;
    if (inter) { x = e / g.C; c = e - x * g.C; }
    else { c = e / wcols; x = e - c * wcols; }
    return inter ? x < wcols : c < g.C;
}

// SCR: a screened solve's right-hand side, F = lap - lam d on the interior (screened_rhs; d is read there only, once per element)
template <bool INTER, bool LAP, bool SCR>
__device__ __forceinline__ void poisson_pre_block(const PoissonGeo &g, const PoissonJobDev &j, const Field &U0, const Field &F, int c0, float lam)
{
    __shared__ float gxs[2][PS_LANES];
    const int W = g.W, H = g.H, Wp = (W + 3) & ~3;
    int x, c;
    const bool lane = ps_lane(g, INTER, Wp, x, c);
    const int D = INTER ? g.C : 1;
    const int tid = (int)threadIdx.x;
    const bool img = lane && x < W, in_x = lane && x >= 1 && x <= W - 2;
    const long long xo = (long long)x * g.cs + (long long)c * g.chs;
    float *const u0 = U0.p + (size_t)(c0 + c) * U0.plane + x, *const f = F.p + (size_t)(c0 + c) * F.plane + x;
    const int y0 = (int)blockIdx.y * PS_ROWS, y1 = min(y0 + PS_ROWS, H);
    float gyu = 0.f;
    if (!LAP && in_x && y0 >= 1) gyu = j.gy[xo + (long long)(y0 - 1) * g.rs];
    for (int y = y0; y < y1; ++y) {
        const long long o = xo + (long long)y * g.rs;
        const bool in_y = y >= 1 && y <= H - 2, in = in_x && in_y;
        float lap = 0.f;
        if constexpr (LAP) {
            if (in) lap = j.lap[o];
        } else {
            const float gxv = (lane && x <= W - 2 && in_y) ? j.gx[o] : 0.f;      // column 0 too: the lane to its right needs it
            const float gyv = (in_x && y <= H - 2) ? j.gy[o] : 0.f;              // row 0 too: the row below needs it
            float *const s = gxs[y & 1];
            s[tid] = gxv;
            __syncthreads();         // (double-buffered: a lane writes the other half next row, which every lane finished reading before this barrier)
            if (in) {
                const float gxl = tid >= D ? s[tid - D] : j.gx[o - g.cs];
                lap = (gxv - gxl) + (gyv - gyu);
            }
            gyu = gyv;
        }
        if constexpr (SCR) {
            if (in) lap = screened_rhs(lap, lam, j.d[o]);
        }
        if (lane) {
            const size_t fo = (size_t)y * U0.pitch;
            u0[fo] = (img && !(SCR && in)) ? j.b[o] : 0.f;      // (a screened solve is direct: boundary's interior is never read)
            f[fo] = lap;
        }
    }
}

template <bool INTER, bool LAP, bool SCR>
__global__ __launch_bounds__(PS_LANES) void k_poisson_pre(PoissonGeo g, PoissonJobDev j, Field U0, Field F, float lam)
{
    poisson_pre_block<INTER, LAP, SCR>(g, j, U0, F, 0, lam);
}

template <bool INTER, bool LAP, bool SCR>
__global__ __launch_bounds__(PS_LANES) void k_poisson_pre_group(PoissonGeo g, PoissonJobs t, Field U0, Field F, float lam)
{
    poisson_pre_block<INTER, LAP, SCR>(g, t.j[blockIdx.z], U0, F, g.C * (int)blockIdx.z, lam);
}

// the solution field's interior into out, the frame from boundary (bit for bit); only the W x H x C elements the layout names
template <bool INTER>
__device__ __forceinline__ void poisson_out_block(const PoissonGeo &g, const PoissonJobDev &j, const Field &U, int c0)
{
    const int W = g.W, H = g.H;
    int x, c;
    if (!ps_lane(g, INTER, W, x, c)) return;
    const bool in_x = x >= 1 && x <= W - 2;
    const long long xo = (long long)x * g.cs + (long long)c * g.chs;
    const float *const u = U.p + (size_t)(c0 + c) * U.plane + x;
    const int y0 = (int)blockIdx.y * PS_ROWS, y1 = min(y0 + PS_ROWS, H);
    for (int y = y0; y < y1; ++y) {
        const long long o = xo + (long long)y * g.rs;
        j.out[o] = (in_x && y >= 1 && y <= H - 2) ? u[(size_t)y * U.pitch] : j.b[o];
    }
}

template <bool INTER>
__global__ __launch_bounds__(PS_LANES) void k_poisson_out(PoissonGeo g, PoissonJobDev j, Field U)
{
    poisson_out_block<INTER>(g, j, U, 0);
}

template <bool INTER>
__global__ __launch_bounds__(PS_LANES) void k_poisson_out_group(PoissonGeo g, PoissonJobs t, Field U)
{
    poisson_out_block<INTER>(g, t.j[blockIdx.z], U, g.C * (int)blockIdx.z);
}

// The Neumann solve's free constant (sc_fft.hip, direct_jobs_solve): sums of boundary in double.  Workgroup (i, c, k): rows [i H / np, (i + 1) H / np)
// of channel c of member k, x inner; a lane's running sum, the wave's by shuffles, the four waves' through LDS -- one order of
// additions per (W, H), whatever the batch, so a member's mean is its solo run's to the bit.  A job without boundary: zeros.
__global__ __launch_bounds__(PS_LANES) void k_poisson_mean(PoissonGeo g, PoissonJobs t, double *__restrict__ parts)
{
    __shared__ double ws[PS_LANES / 64];
    const PoissonJobDev &j = t.j[blockIdx.z];
    const int c = (int)blockIdx.y, i = (int)blockIdx.x, np = (int)gridDim.x, tid = (int)threadIdx.x;
    const int y0 = (int)((long long)i * g.H / np), y1 = (int)((long long)(i + 1) * g.H / np);
    double s = 0.0;
    if (j.b) {
        const float *__restrict__ b = j.b + (long long)c * g.chs;
        for (int y = y0; y < y1; ++y) {
            const float *__restrict__ row = b + (long long)y * g.rs;
#pragma unroll 4
            for (int x = tid; x < g.W; x += PS_LANES) s += (double)row[(long long)x * g.cs];
        }
    }
    s = wave_sum(s);
    if ((tid & 63) == 0) ws[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) parts[((size_t)blockIdx.z * g.C + c) * np + i] = (ws[0] + ws[1]) + (ws[2] + ws[3]);
}

// ---------------------------------------------------------------- launchers
static bool interleaved(const PoissonGeo &g) { return g.C > 1 && g.chs < g.cs; }
static dim3 ps_grid(const PoissonGeo &g, int wcols, int members)
{
    return dim3((unsigned)((wcols * g.C + PS_LANES - 1) / PS_LANES), (unsigned)((g.H + PS_ROWS - 1) / PS_ROWS), (unsigned)members);
}

// the instantiation for (interleaved, lap given, screened): fn(std::integral_constant<bool, .>...) launches it
template <typename Fn>
static void ps_pre_dispatch(bool inter, bool lap, bool scr, Fn fn)
{
    auto pick = [&](auto i, auto l) {
        if (scr) fn(i, l, std::true_type());
        else fn(i, l, std::false_type());
    };
    if (inter) { if (lap) pick(std::true_type(), std::true_type()); else pick(std::true_type(), std::false_type()); }
    else { if (lap) pick(std::false_type(), std::true_type()); else pick(std::false_type(), std::false_type()); }
}

void launch_poisson_pre(const PoissonGeo &g, bool lap, const PoissonJobDev &j, Field U0, Field F, hipStream_t s, float lam)
{
    const dim3 grid = ps_grid(g, (g.W + 3) & ~3, 1);
    ps_pre_dispatch(interleaved(g), lap, lam > 0.f, [&](auto i, auto l, auto sc) {
        hipLaunchKernelGGL((k_poisson_pre<decltype(i)::value, decltype(l)::value, decltype(sc)::value>), grid, dim3(PS_LANES), 0, s, g, j, U0, F, lam);
    });
}

void launch_poisson_pre_group(const PoissonGeo &g, bool lap, const PoissonJobDev *jobs, int n, Field U0, Field F, hipStream_t s, float lam)
{
    for_job_tables<PoissonJobs>(n, [&](PoissonJobs &t, int i, int k) { t.j[i] = jobs[k]; }, [&](const PoissonJobs &t, int i0, int cnt) {
        const dim3 grid = ps_grid(g, (g.W + 3) & ~3, cnt);
        Field u = U0, f = F;      // this launch's first member owns channel C i0
        u.p = U0.p + (size_t)g.C * i0 * U0.plane;
        f.p = F.p + (size_t)g.C * i0 * F.plane;
        ps_pre_dispatch(interleaved(g), lap, lam > 0.f, [&](auto i, auto l, auto sc) {
            hipLaunchKernelGGL((k_poisson_pre_group<decltype(i)::value, decltype(l)::value, decltype(sc)::value>), grid, dim3(PS_LANES), 0, s, g, t, u, f, lam);
        });
    });
}

int poisson_mean_parts(int H) { return std::min(H, 256); }

void launch_poisson_mean(const PoissonGeo &g, const PoissonJobDev *jobs, int n, double *parts, hipStream_t s)
{
    const int np = poisson_mean_parts(g.H);
    for_job_tables<PoissonJobs>(n, [&](PoissonJobs &t, int i, int k) { t.j[i] = jobs[k]; }, [&](const PoissonJobs &t, int i0, int cnt) {
        hipLaunchKernelGGL(k_poisson_mean, dim3((unsigned)np, (unsigned)g.C, (unsigned)cnt), dim3(PS_LANES), 0, s, g, t,
                           parts + (size_t)g.C * i0 * np);
    });
}

void launch_poisson_out(const PoissonGeo &g, const PoissonJobDev &j, Field U, hipStream_t s)
{
    const dim3 grid = ps_grid(g, g.W, 1);
    if (interleaved(g)) hipLaunchKernelGGL(k_poisson_out<true>, grid, dim3(PS_LANES), 0, s, g, j, U);
    else hipLaunchKernelGGL(k_poisson_out<false>, grid, dim3(PS_LANES), 0, s, g, j, U);
}

void launch_poisson_out_group(const PoissonGeo &g, const PoissonJobDev *jobs, int n, Field U, hipStream_t s)
{
    for_job_tables<PoissonJobs>(n, [&](PoissonJobs &t, int i, int k) { t.j[i] = jobs[k]; }, [&](const PoissonJobs &t, int i0, int cnt) {
        const dim3 grid = ps_grid(g, g.W, cnt);
        Field u = U;
        u.p = U.p + (size_t)g.C * i0 * U.plane;
        if (interleaved(g)) hipLaunchKernelGGL(k_poisson_out_group<true>, grid, dim3(PS_LANES), 0, s, g, t, u);
        else hipLaunchKernelGGL(k_poisson_out_group<false>, grid, dim3(PS_LANES), 0, s, g, t, u);
    });
}

} // namespace sc
