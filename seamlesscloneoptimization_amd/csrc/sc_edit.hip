// sc_edit.hip -- the kernels of the whole-image gradient edits (sc_hip_edit: cv::colorChange, cv::illuminationChange,
// cv::textureFlattening; host side in sc_edit_api.cpp): the whole-image erode of the mask, the Canny edge detector of texture
// flattening (Sobel + channel choice + non-maximum suppression in one launch, hysteresis as repeated tile launches), the
// pre-process that forms the edited right-hand side and the copy of the image's frame into the destination.
//
// PARITY UNPINNED: OpenCV is not available to this project and the reference has no fixture of these functions.  What the
// kernels compute is the restatement in tests/photo_edits_np.py, bit for bit except the powf of
// illuminationChange.
#include "sc_common.h"
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>

namespace sc {

// ---------------------------------------------------------------- whole-image erode
// cv::erode of the whole mask with a 3 x 3 rectangle, three iterations = a 7 x 7 minimum filter.  Pixels outside the image are
// ignored (morphologyDefaultBorderValue: +inf for erosion), so a mask that is 255 up to the image's edge stays 255 there --
// unlike k_mask_erode_min7, which reads zeros outside a bounding box.  64 x 16 outputs per workgroup, 70 x 22 bytes in LDS.
__device__ __forceinline__ void edit_erode_block(const uint8_t *__restrict__ mask, int mstep, int W, int H, uint8_t *__restrict__ M, int mpitch)
{
    __shared__ uint8_t in[22][72];
    __shared__ uint8_t hm[22][64];
    const int x0 = blockIdx.x * 64, y0 = blockIdx.y * 16;
    for (int i = threadIdx.x; i < 22 * 70; i += 256) {
        const int ry = i / 70, rx = i - ry * 70;
        const int y = y0 - 3 + ry, x = x0 - 3 + rx;
        in[ry][rx] = (y >= 0 && y < H && x >= 0 && x < W) ? mask[(size_t)y * mstep + x] : (uint8_t)255;
    }
    __syncthreads();
    const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
    for (int r = ly; r < 22; r += 4) {
        unsigned m = 255u;
#pragma unroll
        for (int d = 0; d < 7; ++d) m = min(m, (unsigned)in[r][lx + d]);
        hm[r][lx] = (uint8_t)m;
    }
    __syncthreads();
    for (int r = ly; r < 16; r += 4) {
        unsigned m = 255u;
#pragma unroll
        for (int d = 0; d < 7; ++d) m = min(m, (unsigned)hm[r + d][lx]);
        const int y = y0 + r, x = x0 + lx;
        if (y < H && x < W) M[(size_t)y * mpitch + x] = (uint8_t)m;
    }
}

__global__ __launch_bounds__(256) void k_edit_erode(const uint8_t *__restrict__ mask, int mstep, int W, int H, uint8_t *__restrict__ M, int mpitch)
{
    edit_erode_block(mask, mstep, W, H, M, mpitch);
}

// a group of same-size images (sc_edit_batch.cpp): blockIdx.z = member, whose eroded mask is plane z of M (planes mplane bytes apart)
__global__ __launch_bounds__(256) void k_edit_erode_group(EditJobs t, int W, int H, uint8_t *__restrict__ M, int mpitch, size_t mplane)
{
    const EditJob &j = t.j[blockIdx.z];
    edit_erode_block(j.mask, j.mstep, W, H, M + mplane * blockIdx.z, mpitch);
}

void launch_edit_erode(const uint8_t *mask, int mstep, int W, int H, uint8_t *M, int mpitch, hipStream_t s)
{
    hipLaunchKernelGGL(k_edit_erode, dim3((W + 63) / 64, (H + 15) / 16), dim3(256), 0, s, mask, mstep, W, H, M, mpitch);
}

// ---------------------------------------------------------------- Canny (OpenCV 3.4.5 cv::Canny, L2gradient = false)
// k_canny_nms: one workgroup per CN_TW x CN_TH tile.  The tile's source pixels with a halo of R + 1 (R = aperture / 2; replicated
// borders: coordinates clamped into the image) go to LDS as three planes; a vertical pass forms the smoothed (for dx) and the
// differentiated (for dy) columns, a horizontal pass dx and dy -- int32 sums, saturated once to int16 as cv::Sobel(CV_16S) does --
// for the tile and a one-pixel ring around it.  Per pixel the channel with the largest |dx| + |dy| wins (the first on a tie); the
// ring's magnitudes outside the image are 0.  Non-maximum suppression then writes the class map: 0 none, 1 weak, 2 strong.
constexpr int CN_TW = 64, CN_TH = 16;

template <int R> struct SobelK;
template <> struct SobelK<1> { static constexpr int s[3] = { 1, 2, 1 }, d[3] = { -1, 0, 1 }; };
template <> struct SobelK<2> { static constexpr int s[5] = { 1, 4, 6, 4, 1 }, d[5] = { -1, -2, 0, 2, 1 }; };
template <> struct SobelK<3> { static constexpr int s[7] = { 1, 6, 15, 20, 15, 6, 1 }, d[7] = { -1, -4, -5, 0, 5, 4, 1 }; };

__device__ __forceinline__ int sat16(int v) { return v > 32767 ? 32767 : (v < -32768 ? -32768 : v); }

template <int R>
__device__ __forceinline__ void canny_nms_block(const uint8_t *__restrict__ src, int sstep, int W, int H, int lo, int hi,
                                                uint8_t *__restrict__ C, int cpitch)
{
    constexpr int IW = CN_TW + 2 + 2 * R, IH = CN_TH + 2 + 2 * R;      // staged source: tile + ring + Sobel halo
    constexpr int RW = CN_TW + 2, RH = CN_TH + 2;                       // tile + ring
    __shared__ short in[3][IH][IW];
    __shared__ short vs[3][RH][IW], vd[3][RH][IW];
    __shared__ short sdx[RH][RW], sdy[RH][RW];
    __shared__ int smag[RH][RW];
    const int tx0 = blockIdx.x * CN_TW, ty0 = blockIdx.y * CN_TH;
    for (int i = threadIdx.x; i < IH * IW; i += 256) {
        const int ry = i / IW, rx = i - ry * IW;
        const int y = min(max(ty0 - 1 - R + ry, 0), H - 1), x = min(max(tx0 - 1 - R + rx, 0), W - 1);
        const uint8_t *p = src + (size_t)y * sstep + 3 * (size_t)x;
        in[0][ry][rx] = p[0]; in[1][ry][rx] = p[1]; in[2][ry][rx] = p[2];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 3 * RH * IW; i += 256) {
        const int c = i / (RH * IW), r = i - c * (RH * IW), ry = r / IW, rx = r - ry * IW;
        int a = 0, b = 0;
#pragma unroll
        for (int j = 0; j <= 2 * R; ++j) {
            const int v = in[c][ry + j][rx];
            a += SobelK<R>::s[j] * v;
            b += SobelK<R>::d[j] * v;
        }
        vs[c][ry][rx] = (short)a;      // |a| <= 255 * 64, |b| <= 255 * 10: exact in int16
        vd[c][ry][rx] = (short)b;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < RH * RW; i += 256) {
        const int ry = i / RW, rx = i - ry * RW;
        const int y = ty0 - 1 + ry, x = tx0 - 1 + rx;
        int bdx = 0, bdy = 0, bm = -1;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            int a = 0, b = 0;
#pragma unroll
            for (int k = 0; k <= 2 * R; ++k) {
                a += SobelK<R>::d[k] * (int)vs[c][ry][rx + k];
                b += SobelK<R>::s[k] * (int)vd[c][ry][rx + k];
            }
            a = sat16(a); b = sat16(b);
            const int m = abs(a) + abs(b);
            if (m > bm) { bm = m; bdx = a; bdy = b; }
        }
        if (y < 0 || y >= H || x < 0 || x >= W) bm = 0;
        sdx[ry][rx] = (short)bdx; sdy[ry][rx] = (short)bdy; smag[ry][rx] = bm;
    }
    __syncthreads();
    constexpr long long TG22 = 13573;      // round(tan(22.5 deg) * 2^15)
    for (int i = threadIdx.x; i < CN_TW * CN_TH; i += 256) {
        const int ly = i / CN_TW, lx = i - ly * CN_TW;
        const int y = ty0 + ly, x = tx0 + lx;
        if (y >= H || x >= W) continue;
        const int ry = ly + 1, rx = lx + 1;
        const int m = smag[ry][rx];
        uint8_t cls = 0;
        if (m > lo) {
            const int dx = sdx[ry][rx], dy = sdy[ry][rx];
            const long long xs = dx < 0 ? -(long long)dx : dx, ys = dy < 0 ? -(long long)dy : dy;
            const long long tg22x = xs * TG22, yy = ys << 15;       // 64-bit: OpenCV's int32 form overflows at aperture 7 only
            bool keep;
            if (yy < tg22x) {
                keep = m > smag[ry][rx - 1] && m >= smag[ry][rx + 1];
            } else if (yy > tg22x + (xs << 16)) {
                keep = m > smag[ry - 1][rx] && m >= smag[ry + 1][rx];
            } else {
                const int s = (dx ^ dy) < 0 ? -1 : 1;
                keep = m > smag[ry - 1][rx - s] && m > smag[ry + 1][rx + s];
            }
            if (keep) cls = m > hi ? 2 : 1;
        }
        C[(size_t)y * cpitch + x] = cls;
    }
}

template <int R>
__global__ __launch_bounds__(256) void k_canny_nms(const uint8_t *__restrict__ src, int sstep, int W, int H, int lo, int hi,
                                                   uint8_t *__restrict__ C, int cpitch)
{
    canny_nms_block<R>(src, sstep, W, H, lo, hi, C, cpitch);
}

// a group: member blockIdx.z's source into plane z of the class maps (all members have one W x H, so one grid serves them all)
template <int R>
__global__ __launch_bounds__(256) void k_canny_nms_group(EditJobs t, int W, int H, int lo, int hi, uint8_t *__restrict__ C, int cpitch, size_t cplane)
{
    const EditJob &j = t.j[blockIdx.z];
    canny_nms_block<R>(j.src, j.sstep, W, H, lo, hi, C + cplane * blockIdx.z, cpitch);
}

void launch_canny_nms(const uint8_t *src, int sstep, int W, int H, int lo, int hi, int aperture, uint8_t *C, int cpitch, hipStream_t s)
{
    const dim3 grid((W + CN_TW - 1) / CN_TW, (H + CN_TH - 1) / CN_TH);
    if (aperture == 7) hipLaunchKernelGGL(k_canny_nms<3>, grid, dim3(256), 0, s, src, sstep, W, H, lo, hi, C, cpitch);
    else if (aperture == 5) hipLaunchKernelGGL(k_canny_nms<2>, grid, dim3(256), 0, s, src, sstep, W, H, lo, hi, C, cpitch);
    else hipLaunchKernelGGL(k_canny_nms<1>, grid, dim3(256), 0, s, src, sstep, W, H, lo, hi, C, cpitch);
}

// k_canny_hyst: one launch of the hysteresis.  A workgroup loads its HY_TW x HY_TH tile of the class map and a one-pixel ring (0
// outside the image) into LDS and turns weak pixels with a strong 8-neighbour strong until nothing changes inside the tile; each
// pass that goes on has changed a pixel, so there are at most HY_TW * HY_TH + 1 passes.  Changed pixels are written back.  A tile
// whose edge pixel changed stores the launch's number `round` into the host's pinned mailbox: the neighbouring tile may have read
// the old value as its ring.  Tiles read each other's edges while they are being written within one launch; either value is
// correct (a pixel only ever goes weak -> strong), and a change that a neighbour may have missed is an edge change, which the
// mailbox reports.  So the map is final after a launch that stored nothing: every ring it read was final, every tile ended at
// its fixed point.  No workgroup waits for another.
constexpr int HY_TW = 64, HY_TH = 16;

__device__ __forceinline__ void canny_hyst_block(uint8_t *__restrict__ C, int cpitch, int W, int H, unsigned *mailbox, unsigned round)
{
    __shared__ uint8_t t[HY_TH + 2][HY_TW + 2];
    const int tx0 = blockIdx.x * HY_TW, ty0 = blockIdx.y * HY_TH;
    for (int i = threadIdx.x; i < (HY_TH + 2) * (HY_TW + 2); i += 256) {
        const int ry = i / (HY_TW + 2), rx = i - ry * (HY_TW + 2);
        const int y = ty0 - 1 + ry, x = tx0 - 1 + rx;
        t[ry][rx] = (y >= 0 && y < H && x >= 0 && x < W) ? C[(size_t)y * cpitch + x] : (uint8_t)0;
    }
    __syncthreads();
    // four pixels per lane: one row, columns 4 (lane % 16) .. + 3
    const int ly = threadIdx.x >> 4, lx0 = 4 * (threadIdx.x & 15);
    unsigned changed = 0u;      // bit k: pixel lx0 + k went weak -> strong
    for (int pass = 0; pass <= HY_TW * HY_TH; ++pass) {
        int any = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int ry = ly + 1, rx = lx0 + k + 1;
            if (t[ry][rx] != 1) continue;
            const bool s = t[ry - 1][rx - 1] == 2 || t[ry - 1][rx] == 2 || t[ry - 1][rx + 1] == 2 || t[ry][rx - 1] == 2 ||
                           t[ry][rx + 1] == 2 || t[ry + 1][rx - 1] == 2 || t[ry + 1][rx] == 2 || t[ry + 1][rx + 1] == 2;
            if (s) { t[ry][rx] = 2; changed |= 1u << k; any = 1; }
        }
        if (!__syncthreads_or(any)) break;
    }
    int edge = 0;
    const int y = ty0 + ly;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!(changed >> k & 1u)) continue;
        const int lx = lx0 + k, x = tx0 + lx;       // (a weak pixel lies inside the image)
        C[(size_t)y * cpitch + x] = 2;
        if (lx == 0 || lx == HY_TW - 1 || ly == 0 || ly == HY_TH - 1) edge = 1;
    }
    if (__syncthreads_or(edge) && threadIdx.x == 0) __hip_atomic_store(mailbox, round, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

__global__ __launch_bounds__(256) void k_canny_hyst(uint8_t *__restrict__ C, int cpitch, int W, int H, unsigned *mailbox, unsigned round)
{
    canny_hyst_block(C, cpitch, W, H, mailbox, round);
}

// every member's map in one launch (blockIdx.z = plane), ONE mailbox for the group: a launch that stored nothing left every member's
// map final (the argument above holds per plane; planes never read each other)
__global__ __launch_bounds__(256) void k_canny_hyst_group(uint8_t *__restrict__ C, int cpitch, size_t cplane, int W, int H, unsigned *mailbox, unsigned round)
{
    canny_hyst_block(C + cplane * blockIdx.z, cpitch, W, H, mailbox, round);
}

void launch_canny_hyst(uint8_t *C, int cpitch, int W, int H, unsigned *mailbox, unsigned round, hipStream_t s)
{
    hipLaunchKernelGGL(k_canny_hyst, dim3((W + HY_TW - 1) / HY_TW, (H + HY_TH - 1) / HY_TH), dim3(256), 0, s, C, cpitch, W, H, mailbox, round);
}

// ---------------------------------------------------------------- pre-process of an edit
// One lane per pixel of the whole image (columns up to the next multiple of four, as k_preprocess writes them).  U0 = src (0 in
// the pad columns); F = the divergence of the edited field on the interior, 0 on the frame.  At a pixel q, per channel:
//   (gx, gy) = forward differences of src, m = M (1/255f), mi = (255 - M)(1/255f) (M: the eroded mask),
//   P' = COLOR        (P m) k_c
//        ILLUMINATION Q = P m, (Q ab) |Q|^-beta (ab = alpha^beta, from the host), NaN -> 0 (cv::patchNaNs)
//        TEXTURE      (edge(q) ? P : 0) m
//   G = (gx, gy) mi + P',  lap = (Gx(q) - Gx(q - x)) + (Gy(q) - Gy(q - y)).
// The interior's neighbours q + x, q + y, q - x, q - y are all inside the image.  Byte loads: the kernel is not a hot one (the
// solve behind it reads the fields tens of times).
struct EditArgs { int op; float k[3]; float ab, nbeta; };

template <int OP>
__device__ __forceinline__ float2 edit_field(const uint8_t *__restrict__ src, int sstep, const uint8_t *__restrict__ M, int mpitch,
                                             const uint8_t *__restrict__ E, int x, int y, int c, const EditArgs &a)
{
    const uint8_t *p = src + (size_t)y * sstep + 3 * (size_t)x + c;
    const float i0 = (float)p[0], gx = (float)p[3] - i0, gy = (float)p[sstep] - i0;
    const unsigned mb = M[(size_t)y * mpitch + x];
    const float m = (float)mb * (1.0f / 255.0f), mi = (float)(255u - mb) * (1.0f / 255.0f);
    float px, py;
    if constexpr (OP == 1) {
        px = (gx * m) * a.k[c];
        py = (gy * m) * a.k[c];
    } else if constexpr (OP == 2) {
        const float qx = gx * m, qy = gy * m;
        const float mag = sqrtf(qx * qx + qy * qy);
        const float w = powf(mag, a.nbeta);
        px = (qx * a.ab) * w;
        py = (qy * a.ab) * w;
        if (px != px) px = 0.f;
        if (py != py) py = 0.f;
    } else {
        const bool e = E[(size_t)y * mpitch + x] == 2;
        px = (e ? gx : 0.f) * m;
        py = (e ? gy : 0.f) * m;
    }
    return make_float2(gx * mi + px, gy * mi + py);
}

template <int OP>
__device__ __forceinline__ void edit_preprocess_block(const uint8_t *__restrict__ src, int sstep, const uint8_t *__restrict__ M, int mpitch,
                                                      const uint8_t *__restrict__ E, const Field &U0, const Field &F, int c0, const EditArgs &a)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int W = U0.W, H = U0.H;
    if (x >= ((W + 3) & ~3) || y >= H) return;
    const size_t o = (size_t)y * U0.pitch + x;
    const bool in = x >= 1 && x <= W - 2 && y >= 1 && y <= H - 2;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        U0.at(c0 + c)[o] = x < W ? (float)src[(size_t)y * sstep + 3 * (size_t)x + c] : 0.f;
        float lap = 0.f;
        if (in) {
            const float2 g = edit_field<OP>(src, sstep, M, mpitch, E, x, y, c, a);
            const float2 gl = edit_field<OP>(src, sstep, M, mpitch, E, x - 1, y, c, a);
            const float2 gu = edit_field<OP>(src, sstep, M, mpitch, E, x, y - 1, c, a);
            lap = (g.x - gl.x) + (g.y - gu.y);
        }
        F.at(c0 + c)[o] = lap;
    }
}

template <int OP>
__global__ __launch_bounds__(256) void k_edit_preprocess(const uint8_t *__restrict__ src, int sstep, const uint8_t *__restrict__ M, int mpitch,
                                                         const uint8_t *__restrict__ E, Field U0, Field F, EditArgs a)
{
    edit_preprocess_block<OP>(src, sstep, M, mpitch, E, U0, F, 0, a);
}

// a group: member blockIdx.z writes channels 3z..3z+2 of U0 / F from its own source, eroded mask (plane z of M) and class map
// (plane z of E) -- the single image's arithmetic, so the same bits
template <int OP>
__global__ __launch_bounds__(256) void k_edit_preprocess_group(EditJobs t, const uint8_t *__restrict__ M, int mpitch, size_t mplane,
                                                               const uint8_t *__restrict__ E, Field U0, Field F, EditArgs a)
{
    const EditJob &j = t.j[blockIdx.z];
    edit_preprocess_block<OP>(j.src, j.sstep, M + mplane * blockIdx.z, mpitch, E ? E + mplane * blockIdx.z : nullptr, U0, F, 3 * blockIdx.z, a);
}

void launch_edit_preprocess(int op, const float k[3], float ab, float nbeta, const uint8_t *src, int sstep, const uint8_t *M, int mpitch,
                            const uint8_t *E, Field U0, Field F, hipStream_t s)
{
    EditArgs a;
    a.op = op; a.k[0] = k[0]; a.k[1] = k[1]; a.k[2] = k[2]; a.ab = ab; a.nbeta = nbeta;
    const dim3 grid(((U0.W + 3) / 4 * 4 + 63) / 64, (U0.H + 3) / 4);
    if (op == 1) hipLaunchKernelGGL(k_edit_preprocess<1>, grid, dim3(256), 0, s, src, sstep, M, mpitch, E, U0, F, a);
    else if (op == 2) hipLaunchKernelGGL(k_edit_preprocess<2>, grid, dim3(256), 0, s, src, sstep, M, mpitch, E, U0, F, a);
    else hipLaunchKernelGGL(k_edit_preprocess<3>, grid, dim3(256), 0, s, src, sstep, M, mpitch, E, U0, F, a);
}

// ---------------------------------------------------------------- the frame of src into dst
// The post-process writes the interior; dst's one-pixel frame is src's (the Dirichlet data).  One lane per frame pixel.
__device__ __forceinline__ void edit_frame_block(const uint8_t *__restrict__ src, int sstep, uint8_t *__restrict__ dst, int dstep, int W, int H)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    int x, y;
    if (i < W) { x = i; y = 0; }
    else if (i < 2 * W) { x = i - W; y = H - 1; }
    else if (i < 2 * W + (H - 2)) { x = 0; y = 1 + (i - 2 * W); }
    else if (i < 2 * W + 2 * (H - 2)) { x = W - 1; y = 1 + (i - 2 * W - (H - 2)); }
    else return;
    const uint8_t *s = src + (size_t)y * sstep + 3 * (size_t)x;
    uint8_t *d = dst + (size_t)y * dstep + 3 * (size_t)x;
    d[0] = s[0]; d[1] = s[1]; d[2] = s[2];
}

__global__ __launch_bounds__(256) void k_edit_frame(const uint8_t *__restrict__ src, int sstep, uint8_t *__restrict__ dst, int dstep, int W, int H)
{
    edit_frame_block(src, sstep, dst, dstep, W, H);
}

// a group: member blockIdx.z's frame (members whose dst is their src have nothing to copy: the launcher leaves them out)
__global__ __launch_bounds__(256) void k_edit_frame_group(EditJobs t, int W, int H)
{
    const EditJob &j = t.j[blockIdx.z];
    edit_frame_block(j.src, j.sstep, j.dst, j.dstep, W, H);
}

void launch_edit_frame(const uint8_t *src, int sstep, uint8_t *dst, int dstep, int W, int H, hipStream_t s)
{
    const int n = 2 * W + 2 * (H - 2);
    hipLaunchKernelGGL(k_edit_frame, dim3((n + 255) / 256), dim3(256), 0, s, src, sstep, dst, dstep, W, H);
}

// ---------------------------------------------------------------- launchers of the group forms (one launch per 16 members)
template <typename F>
static void for_chunks(const EditJob *jobs, int n, F f)
{
    for (int i0 = 0; i0 < n; i0 += EditJobs::MAX) {
        EditJobs t{};
        const int cnt = std::min(n - i0, (int)EditJobs::MAX);
        for (int i = 0; i < cnt; ++i) t.j[i] = jobs[i0 + i];
        f(t, i0, cnt);
    }
}

void launch_edit_erode_group(const EditJob *jobs, int n, int W, int H, uint8_t *M, int mpitch, size_t mplane, hipStream_t s)
{
    for_chunks(jobs, n, [&](const EditJobs &t, int i0, int cnt) {
        hipLaunchKernelGGL(k_edit_erode_group, dim3((W + 63) / 64, (H + 15) / 16, cnt), dim3(256), 0, s, t, W, H, M + mplane * i0, mpitch, mplane);
    });
}

void launch_canny_nms_group(const EditJob *jobs, int n, int W, int H, int lo, int hi, int aperture, uint8_t *C, int cpitch, size_t cplane, hipStream_t s)
{
    for_chunks(jobs, n, [&](const EditJobs &t, int i0, int cnt) {
        const dim3 grid((W + CN_TW - 1) / CN_TW, (H + CN_TH - 1) / CN_TH, cnt);
        uint8_t *c = C + cplane * i0;
        if (aperture == 7) hipLaunchKernelGGL(k_canny_nms_group<3>, grid, dim3(256), 0, s, t, W, H, lo, hi, c, cpitch, cplane);
        else if (aperture == 5) hipLaunchKernelGGL(k_canny_nms_group<2>, grid, dim3(256), 0, s, t, W, H, lo, hi, c, cpitch, cplane);
        else hipLaunchKernelGGL(k_canny_nms_group<1>, grid, dim3(256), 0, s, t, W, H, lo, hi, c, cpitch, cplane);
    });
}

void launch_canny_hyst_group(uint8_t *C, int cpitch, size_t cplane, int n, int W, int H, unsigned *mailbox, unsigned round, hipStream_t s)
{
    hipLaunchKernelGGL(k_canny_hyst_group, dim3((W + HY_TW - 1) / HY_TW, (H + HY_TH - 1) / HY_TH, n), dim3(256), 0, s, C, cpitch, cplane, W, H, mailbox, round);
}

void launch_edit_preprocess_group(int op, const float k[3], float ab, float nbeta, const EditJob *jobs, int n, const uint8_t *M, int mpitch,
                                  size_t mplane, const uint8_t *E, Field U0, Field F, hipStream_t s)
{
    EditArgs a;
    a.op = op; a.k[0] = k[0]; a.k[1] = k[1]; a.k[2] = k[2]; a.ab = ab; a.nbeta = nbeta;
    for_chunks(jobs, n, [&](const EditJobs &t, int i0, int cnt) {
        const dim3 grid(((U0.W + 3) / 4 * 4 + 63) / 64, (U0.H + 3) / 4, cnt);
        Field u = U0, f = F;      // this launch's first member owns channel 3 i0
        u.p = U0.p + (size_t)3 * i0 * U0.plane;
        f.p = F.p + (size_t)3 * i0 * F.plane;
        const uint8_t *m = M + mplane * i0, *e = E ? E + mplane * i0 : nullptr;
        if (op == 1) hipLaunchKernelGGL(k_edit_preprocess_group<1>, grid, dim3(256), 0, s, t, m, mpitch, mplane, e, u, f, a);
        else if (op == 2) hipLaunchKernelGGL(k_edit_preprocess_group<2>, grid, dim3(256), 0, s, t, m, mpitch, mplane, e, u, f, a);
        else hipLaunchKernelGGL(k_edit_preprocess_group<3>, grid, dim3(256), 0, s, t, m, mpitch, mplane, e, u, f, a);
    });
}

void launch_edit_frame_group(const EditJob *jobs, int n, int W, int H, hipStream_t s)
{
    const int px = 2 * W + 2 * (H - 2);
    for_chunks(jobs, n, [&](const EditJobs &t, int, int cnt) {
        hipLaunchKernelGGL(k_edit_frame_group, dim3((px + 255) / 256, 1, cnt), dim3(256), 0, s, t, W, H);
    });
}

} // namespace sc
