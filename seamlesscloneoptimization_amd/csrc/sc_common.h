// sc_common.h -- shared host-side declarations of libseamlessclone_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <algorithm>
#include <string>
#include <vector>
#include "../../include/seamlessclone_hip_testing.h"

namespace sc {

// Planar float32 field: C planes of H rows, row pitch in floats (multiple of 64 = 256 B so
// every row starts on a cache-line / float4 boundary; the ring column x=0 sits at the row
// start, so float4 groups are aligned in ROI coordinates).
struct Field {
    float *p = nullptr;
    int W = 0, H = 0, C = 0;
    int pitch = 0;      // floats per row
    size_t plane = 0;   // floats per plane (pitch * H rounded up to 64)
    __host__ __device__ float *at(int c) const { return p + (size_t)c * plane; }
    size_t bytes() const { return plane * (size_t)C * sizeof(float); }
};

static inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// ROI geometry (seamlessClone_imp.cpp:1014-1016,1066)
struct Geo { int x0, y0, W, H, ltx, lty; };

// 8-bit interleaved image view (cv::Mat {data, cols, rows, step})
struct Img8 {
    const uint8_t *p; int cols, rows, step;
};

// mask stage of one member of a group of clones (launch_mask_*_group): the scan uses mask/mw/mh/mstep/rect, the erode
// additionally g/M/mpitch (mask_bytes is filled in by the launcher)
struct MaskJob {
    const uint8_t *mask; int mw, mh, mstep;
    int *rect;
    int *rect_host;      // (group scans) the same four words in the host's pinned mailbox, written by the fold: no copy command (may be nullptr)
    size_t mask_bytes;
    Geo g;
    uint8_t *M; int mpitch;
};
struct MaskJobs { enum { MAX = 16 }; MaskJob j[MAX]; };     // by value in the kernel arguments
// pre- / post-process of the members of a group: ROI origins in the images and the member's eroded mask; member i owns
// channels 3i..3i+2 of the fields (blockIdx.z = i)
// body_org: where the member's output is WRITTEN; body_src: where its destination pixels are READ (the pre-process), at the same
// step -- body_org itself, or the same ROI of the restore source when the group restores only the destination's frame (sc_batch.cpp)
struct ImageJob { const uint8_t *face_org; int fstep; uint8_t *body_org; const uint8_t *body_src; int bstep; const uint8_t *M;
                  const int *d_rect; int rx0, rx1, ry0, ry1;
                  int W, H; };      // W > 0: the member's own ROI size inside fields laid out for a larger one (a size class, RagMember); 0: the fields' size   // d_rect != nullptr: the member ran on a PREDICTED bounding box and is spliced only if the device found exactly that box (RectGuard semantics)
struct ImageJobs { enum { MAX = 16 }; ImageJob j[MAX]; };

// ---------------------------------------------------------------- kernel launchers (sc_kernels.hip)
// single-mask bounding box: per-workgroup parts folded by the last workgroup to arrive (sc_kernels.hip, mask_bbox_block);
// nbx / nblocks are filled in by the launchers
struct BboxFold { int *parts = nullptr; unsigned *counter = nullptr; int *rect_dev = nullptr; int *rect_host = nullptr; int nbx = 0, nblocks = 0; };
int  mask_bbox_blocks(int mw, int mh);                               // workgroups of the scan = parts (4 ints each) it needs
void launch_mask_bbox(const uint8_t *mask, int mw, int mh, int mstep, BboxFold fold, hipStream_t s);
void launch_mask_erode3(const uint8_t *mask, int mstep, int mask_rows, Geo g, uint8_t *M, int mpitch, hipStream_t s);
void launch_mask_erode_min7(const uint8_t *mask, int mstep, Geo g, uint8_t *M, int mpitch, hipStream_t s);   // OpenCV's grey-mask erode (SC_FLAG_OPENCV_GREY_MASK)
// the whole-image edits (sc_edit.hip): 7 x 7 minimum filter that ignores pixels outside the image; Canny's class map (0 / 1 weak /
// 2 strong) and one hysteresis launch (stores `round` into *mailbox when a tile's edge pixel changed); the edit's pre-process (op:
// SC_EDIT_*, k = per-channel factors B, G, R, ab = alpha^beta, nbeta = -beta; E: the class map after hysteresis); src's frame into dst
void launch_edit_erode(const uint8_t *mask, int mstep, int W, int H, uint8_t *M, int mpitch, hipStream_t s);
void launch_canny_nms(const uint8_t *src, int sstep, int W, int H, int lo, int hi, int aperture, uint8_t *C, int cpitch, hipStream_t s);
void launch_canny_hyst(uint8_t *C, int cpitch, int W, int H, unsigned *mailbox, unsigned round, hipStream_t s);
void launch_edit_frame(const uint8_t *src, int sstep, uint8_t *dst, int dstep, int W, int H, hipStream_t s);
void launch_edit_preprocess(int op, const float k[3], float ab, float nbeta, const uint8_t *src, int sstep, const uint8_t *M, int mpitch,
                            const uint8_t *E, Field U0, Field F, hipStream_t s);
// ... their group forms (sc_edit_batch.cpp: same-size images as one field of 3n channels): member k's eroded mask and class map are
// plane k of M / C (planes mplane / cplane bytes apart, pitch mpitch), its fields channels 3k..3k+2; one launch per 16 members (the
// table goes by value), the hysteresis one launch for all of them with one mailbox
struct EditJob { const uint8_t *src; int sstep; const uint8_t *mask; int mstep; uint8_t *dst; int dstep; };
struct EditJobs { enum { MAX = 16 }; EditJob j[MAX]; };
void launch_edit_erode_group(const EditJob *jobs, int n, int W, int H, uint8_t *M, int mpitch, size_t mplane, hipStream_t s);
void launch_canny_nms_group(const EditJob *jobs, int n, int W, int H, int lo, int hi, int aperture, uint8_t *C, int cpitch, size_t cplane, hipStream_t s);
void launch_canny_hyst_group(uint8_t *C, int cpitch, size_t cplane, int n, int W, int H, unsigned *mailbox, unsigned round, hipStream_t s);
void launch_edit_preprocess_group(int op, const float k[3], float ab, float nbeta, const EditJob *jobs, int n, const uint8_t *M, int mpitch,
                                  size_t mplane, const uint8_t *E, Field U0, Field F, hipStream_t s);
void launch_edit_frame_group(const EditJob *jobs, int n, int W, int H, hipStream_t s);     // members whose dst is not their src
// the Poisson solve on caller arrays (sc_poisson.hip, sc_poisson_api.cpp): one layout (W x H x C elements, strides in floats) for
// every array of a call; pre-process into U0 / F (lap: the right-hand side given, else from gx, gy), the solution U back into out.
// Group forms: member k owns channels C k .. C k + C - 1, one launch per 16 members (the table goes by value)
struct PoissonGeo { int W, H, C; long long cs, rs, chs; };
struct PoissonJobDev { const float *gx, *gy, *lap, *b; float *out; const float *d = nullptr; };      // d: a screened solve's data term
struct PoissonJobs { enum { MAX = 16 }; PoissonJobDev j[MAX]; };
// m jobs through tables of Table::MAX that go by value in the kernel arguments: fill(table, i, k) sets slot i from job k, fn(table, i0, cnt)
// launches jobs i0 .. i0 + cnt - 1
template <class Table, class Fill, class Fn> void for_job_tables(int m, Fill fill, Fn fn)
{
    for (int i0 = 0; i0 < m; i0 += Table::MAX) {
        Table t{};
        const int cnt = std::min(m - i0, (int)Table::MAX);
        for (int i = 0; i < cnt; ++i) fill(t, i, i0 + i);
        fn(t, i0, cnt);
    }
}
// A call with free (reflecting) sides on some but not all of the four borders (SC_POISSON_FREE_*): per axis its kind -- 0: Dirichlet
// lines at both ends, 1: both ends free, 2: a Dirichlet line at the low end (column or row 0) and a free high end, 3: the reverse --
// and its number of unknowns, pixels less the axis's Dirichlet lines.  (Kind 0 on both axes is the Dirichlet call, kind 1 on both the
// Neumann call: neither comes here.)  Kind 4 (SC_POISSON_PERIODIC_X / _Y): the axis wraps -- no Dirichlet line, every pixel an unknown, the
// neighbour beyond either end is the pixel at the other end.
struct MixedGeo { int ax, ay, nx, ny; };
constexpr int MIXED_PERIODIC = 4;
__host__ __device__ __forceinline__ bool mixed_low_d(int k) { return k == 0 || k == 2; }
__host__ __device__ __forceinline__ bool mixed_high_d(int k) { return k == 0 || k == 3; }
// the axis's operator has the eigenvalue 0 (its constant vector): no Dirichlet line at either end.  Both axes: the unscreened system is
// singular (the Neumann call, and any pairing of a periodic axis with a periodic or free-free one)
__host__ __device__ __forceinline__ bool mixed_zero_eig(int k) { return k == 1 || k == MIXED_PERIODIC; }
// a screened solve's right-hand side (sc_screened_api.cpp): rhs - lam d in float32, one multiply, then one subtract -- never one fused
// multiply-add, whatever the translation unit's contraction setting (the product is opaque to the optimiser)
__device__ __forceinline__ float screened_rhs(float rhs, float lam, float d)
{
    float t = lam * d;
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(t));
#endif
    return rhs - t;
}
#if defined(__HIPCC__)
// the reflecting system's right-hand side at pixel (x, y) of channel c: given, or (a - b) + (c - d) of the guidance field in float32
// (px / py: that axis wraps -- the difference stored in the last column / row runs from the last pixel to the first, and column / row 0
// takes it as its backward difference)
template <bool LAP>
__device__ __forceinline__ float dct_rhs(const PoissonGeo &g, const PoissonJobDev &j, int c, int x, int y, bool px, bool py)
{
    const long long o = (long long)x * g.cs + (long long)y * g.rs + (long long)c * g.chs;
    if (LAP) return j.lap[o];
    const float a = (x < g.W - 1 || px) ? j.gx[o] : 0.f, b = x > 0 ? j.gx[o - g.cs] : px ? j.gx[o + (long long)(g.W - 1) * g.cs] : 0.f;
    const float cc = (y < g.H - 1 || py) ? j.gy[o] : 0.f, d = y > 0 ? j.gy[o - g.rs] : py ? j.gy[o + (long long)(g.H - 1) * g.rs] : 0.f;
    return (a - b) + (cc - d);
}
#endif
// lam > 0: the screened right-hand side F = lap - lam d (d: PoissonJobDev::d, read on the interior); lam = 0: the launches as they were
void launch_poisson_pre(const PoissonGeo &g, bool lap, const PoissonJobDev &j, Field U0, Field F, hipStream_t s, float lam = 0.f);
void launch_poisson_pre_group(const PoissonGeo &g, bool lap, const PoissonJobDev *jobs, int n, Field U0, Field F, hipStream_t s, float lam = 0.f);
void launch_poisson_out(const PoissonGeo &g, const PoissonJobDev &j, Field U, hipStream_t s);
void launch_poisson_out_group(const PoissonGeo &g, const PoissonJobDev *jobs, int n, Field U, hipStream_t s);
// the Neumann solve's free constant: parts[(k C + c) np + i] = the sum in double of rows [i H / np, (i + 1) H / np) of channel c of member k's
// boundary (0 where the job has none); np = poisson_mean_parts(H); one launch per 16 members
int poisson_mean_parts(int H);
void launch_poisson_mean(const PoissonGeo &g, const PoissonJobDev *jobs, int n, double *parts, hipStream_t s);
size_t mask_bbox_group_parts(const MaskJob *jobs, int n);            // ints of scratch the group scan needs (one set of extrema per workgroup)
void launch_mask_bbox_group(const MaskJob *jobs, int n, hipStream_t s, int *parts);
void launch_mask_erode3_group(const MaskJob *jobs, int n, hipStream_t s);
// body_org: pointer to the pixel that corresponds to ROI (0,0); face_org likewise (patch + offset)
// scan: the clone's bounding-box scan rides in this launch as extra workgroups (fold.nbx / nblocks / scan_rows are filled in here)
// g, mask_bytes: the launch's tiles also form the eroded mask of the (predicted) ROI `g` themselves, from the mask bytes (mask_bytes of them are
// the caller's), and leave it in M as k_mask_erode3 would -- no erode launch in front of the pre-process
struct BboxTask { const uint8_t *mask = nullptr; int mw = 0, mh = 0, mstep = 0; BboxFold fold; int scan_rows = 0; Geo g{}; size_t mask_bytes = 0; uint8_t *M_out = nullptr; };     // M_out: where the tiles leave the eroded mask (the buffer the launch's M argument names)
void launch_preprocess(const uint8_t *body_org, int bstep, const uint8_t *face_org, int fstep,
                       const uint8_t *M, int mpitch, Field U0, Field U1, Field F, hipStream_t s, bool f_half = false, bool u_half = false, bool grey = false,
                       const BboxTask *scan = nullptr, int mode = SC_NORMAL_CLONE);     // mode: SC_NORMAL_CLONE / SC_MIXED_CLONE / SC_MONOCHROME_TRANSFER
// bounding box the host assumed when it launched a clone before the device's answer was back (d_rect == nullptr: none)
struct RectGuard { const int *d_rect = nullptr; int x0 = 0, x1 = 0, y0 = 0, y1 = 0; };
// "Do not write": a device word the launches of one solve may set to that solve's generation number (a 16-bit fixed-point store
// of the field saturated, k_cycle0 with C0_Q16_OUT); the output launches of the same solve then write nothing and the host repeats
// the clone on float fields.  A generation instead of a flag: nothing has to be reset between solves.  p == nullptr: none.
// `host`: a second copy of the word in pinned host memory, for the host to read without a copy command (the device copy is the
// one the output launches test: a million threads polling a word across PCIe made the splice 170 times slower).
struct AbortFlag { unsigned *p = nullptr; unsigned gen = 0; unsigned *host = nullptr; };
#if defined(__HIPCC__)
__device__ __forceinline__ bool abort_set(const AbortFlag &a) { return a.p && *reinterpret_cast<const volatile unsigned *>(a.p) == a.gen; }
#endif
// float-table correction at the nodes = every 8th field row and column (sc_lowmode.hip): CN[c][Y][X], ny rows of npitch
// floats per channel; the post-process adds the bilinear interpolation between the four nodes around a pixel.
// CN == nullptr: none.
struct LmNodes { const float *CN = nullptr; int ny = 0, npitch = 0; };
#if defined(__HIPCC__)
// the correction at the four pixels x .. x + 3 (x a multiple of 4: one 8-column cell) of row y, added to v; and the output
// byte of a value: clamp to [0, 255], truncate (seamlessClone_imp.cpp:2091-2096).  One definition for the post-process and for
// the multigrid launch that writes output bytes itself: the same operations in the same order.
// (p00, p01: the two nodes of the cell's upper node row, p10, p11: of its lower one)
__device__ __forceinline__ void lm_add4_nodes(float p00, float p01, float p10, float p11, int x, int y, float4 &v)
{
    const float ty = 0.125f * (float)(y & 7);
    const float l = __builtin_fmaf(ty, p10 - p00, p00), r = __builtin_fmaf(ty, p11 - p01, p01);
    const float dx = 0.125f * (r - l), a0 = __builtin_fmaf((float)(x & 7), dx, l);
    v.x += a0;
    v.y += a0 + dx;
    v.z += __builtin_fmaf(2.0f, dx, a0);
    v.w += __builtin_fmaf(3.0f, dx, a0);
}
__device__ __forceinline__ void lm_add4(const LmNodes &lm, int c, int x, int y, float4 &v)
{
    const float *__restrict__ p = lm.CN + ((size_t)c * lm.ny + (y >> 3)) * lm.npitch + (x >> 3);
    lm_add4_nodes(p[0], p[1], p[lm.npitch], p[lm.npitch + 1], x, y, v);
}
__device__ __forceinline__ unsigned lm_byte(float d)
{
    d = d > 255.0f ? 255.0f : d;
    d = d < 0.0f ? 0.0f : d;
    return (unsigned)(unsigned char)d;
}
__device__ __forceinline__ float lm_bilinear(const LmNodes &lm, int c, int x, int y)
{
    const float *__restrict__ p = lm.CN + ((size_t)c * lm.ny + (y >> 3)) * lm.npitch + (x >> 3);
    const float tx = 0.125f * (float)(x & 7), ty = 0.125f * (float)(y & 7);
    const float top = __builtin_fmaf(tx, p[1] - p[0], p[0]), bot = __builtin_fmaf(tx, p[lm.npitch + 1] - p[lm.npitch], p[lm.npitch]);
    return __builtin_fmaf(ty, bot - top, top);
}
#endif
void launch_postprocess(Field U, uint8_t *body_org, int bstep, hipStream_t s, RectGuard guard = RectGuard(), LmNodes lm = LmNodes(), AbortFlag ab = AbortFlag());
// the same for a group (fields of 3n channels), one launch per 16 members
// store_u0 = false (float16 fields only): the initial field is not stored -- the first level-0 launch reads the destinations' bytes (C0_IN3)
void launch_preprocess_group(const ImageJob *jobs, int n, int mpitch, Field U0, Field F, hipStream_t s, bool f_half, bool u_half, int mode, bool store_u0 = true);
// ... and the launch that stores those float16 planes after all (what the pre-process would have stored), for a solve whose first launch has no bytes form
void launch_u0_half_group(const ImageJob *jobs, int n, Field U0, hipStream_t s);
void launch_postprocess_group(Field U, const ImageJob *jobs, int n, hipStream_t s, LmNodes lm = LmNodes(), AbortFlag ab = AbortFlag());
// splice of output bytes a multigrid launch left planar in Q's memory (launch_cycle0, out_bytes): interleave into the destination
void launch_splice_planar(Field Q, uint8_t *body_org, int bstep, hipStream_t s, RectGuard guard = RectGuard(), AbortFlag ab = AbortFlag());
void launch_splice_planar_group(Field Q, const ImageJob *jobs, int n, hipStream_t s, AbortFlag ab = AbortFlag());
void launch_half_to_float(const void *src_half, float *dst, size_t n, hipStream_t s);
// The FRAME of a destination whose ROI interior a clone is going to write: every byte of the image's step x rows except the interior
// columns of the interior rows.  In memory that is a head [0, head_end), `mids` runs of mid_len bytes `stride` apart from mid_first
// (the bytes behind one interior row's last interior pixel up to the next row's first), and a tail [tail_begin, bytes).  A ROI
// without interior: the head is the whole image (head_end == bytes, no mids, tail_begin == bytes).
struct FrameSpans { size_t bytes, head_end, mid_first, mid_len, stride, tail_begin; int mids; };
// the one place that computes them (host only): image of `step` bytes x `rows`, ROI of W x H pixels (3 bytes each) at (ltx, lty)
FrameSpans frame_spans(size_t step, int rows, int ltx, int lty, int W, int H);
// up to 16 device-to-device copies in one launch (16-byte aligned pointers).  frame[i].bytes != 0: only that frame of member i is
// copied (frame[i].bytes == bytes[i]); 0, as CopyJobs{} leaves it: all of bytes[i]
struct CopyJobs { enum { MAX = 16 }; void *dst[MAX]; const void *src[MAX]; size_t bytes[MAX]; FrameSpans frame[MAX]; };
void launch_copy_group(const CopyJobs &t, int n, hipStream_t s);

void launch_jacobi(Field Uin, Field Uout, Field F, hipStream_t s, bool tag = false, int lds_tile_rows = 0);
void launch_rb_half(Field U, Field F, int color, float omega, hipStream_t s, bool tag = false);
// fused temporally-blocked kernels (sc_sweep_tb.hip); return false when the shape is unsupported
bool launch_jacobi_tb(Field Uin, Field Uout, Field F, int sweeps, hipStream_t s, bool tag = false);
bool launch_rb_tb(Field Uin, Field Uout, Field F, int sweeps, float omega, hipStream_t s, bool tag = false);
int  tb_max_depth(int method);
int  tb_hard_max_depth(int method);
long tb_big_side();
// Column tiling of a coarse-level launch (k_cycle0's GEN forms, k_rb_tb's GEN forms): a plane is cut into column tiles one wave wide that
// own `uw` = 256 - 2 hx columns each, and row tiles that own `rows` rows.  The LAST column tile of a level whose width lies just above a
// multiple of uw owns a few columns only (widths 1025, 513, 257 of a 2048^2 ROI: 97, 49, 25 of 232); where it needs at most half a wave --
// its own columns and hx halo columns on either side -- one workgroup serves that tile of K planes: the wave is cut into K slots of `lps`
// lanes (a power of two), slot k holds plane c0 + k at columns x_res - hx + 4 (lane % lps).  Rows stay wave-uniform.  Workgroups are
// numbered full tiles first (column tile fastest, then row tile, then plane), packed tiles behind them (row tile fastest, then pack).
// One definition for the launchers and the kernels: what is counted is what runs.  A size class never packs (its members differ in width
// and leave empty tiles early), nor does a launch asked for the unpacked tiling (SC_LEGACY_UNPACKED_TILES).
struct TilePlan { int nbx, nby, full, lps, lg, K, blocks; };      // full: column tiles served one plane per workgroup (nbx, or nbx - 1 when the last one is packed); lps = 1 << lg
__host__ __device__ inline TilePlan coarse_tile_plan(int W, int H, int C, int uw, int hx, int rows, bool size_class, bool pack = true)
{
    TilePlan p;
    p.nbx = (W + uw - 1) / uw; p.nby = (H + rows - 1) / rows;
    p.full = p.nbx; p.lps = 64; p.lg = 6; p.K = 1;
    const int need = (W - (p.nbx - 1) * uw + 2 * hx + 3) / 4;      // float4 lanes of the last tile: the columns it owns and a halo on either side (at least 3)
    if (pack && !size_class && need <= 32) {
        p.lg = 32 - __builtin_clz((unsigned)(need - 1));            // the smallest power of two that holds them
        p.lps = 1 << p.lg; p.K = 64 >> p.lg; p.full = p.nbx - 1;
    }
    p.blocks = p.nby * (p.full * C + (p.nbx - p.full) * ((C + p.K - 1) >> (6 - p.lg)));
    return p;
}
// what lane `lane` of workgroup `tile` (the logical number, after xcd_tile) serves: row tile, plane (>= C: an empty slot of the last pack),
// first column, lane index inside its slot and the slot's width in lanes (a full tile: the lane itself, 64).  Two integer divisions on
// either path (the kernels decode their workgroup number with this: a division is some forty instructions of a launch's prologue).
struct TileLane { int by, c, x, sl, lps; };
__host__ __device__ inline TileLane coarse_tile_lane(const TilePlan &p, int C, int uw, int hx, int tile, int lane)
{
    TileLane t;
    const int nfull = p.full * p.nby * C;
    if (tile < nfull) {
        const int q = tile / p.full;
        t.c = q / p.nby; t.by = q - t.c * p.nby;
        t.x = (tile - q * p.full) * uw - hx + 4 * lane; t.sl = lane; t.lps = 64;
    } else {
        const int k = tile - nfull, g = k / p.nby;
        t.by = k - g * p.nby; t.lps = p.lps; t.sl = lane & (p.lps - 1);
        t.c = (g << (6 - p.lg)) + (lane >> p.lg);
        t.x = p.full * uw - hx + 4 * t.sl;
    }
    return t;
}
// band height (rows per lane) of a coarse-level launch; pack: the launch packs its last column tiles (coarse_tile_plan) where the band
// height is at most pack_rows (k_cycle0's coarse forms pack with 4- and 6-row bands: 8-row bands have no registers left for a plane per lane)
int  tb_gen_rows(int W, int H, int C, int hx, int hy, bool pack = false, int pack_rows = 8);
int  tb_gen_rows_deep(int W, int H, int C, int hx, int hy, bool pack = false);   // the same for launches of depth 3 or 4: 4 or 6
struct MGGeom;
struct ComposeArgs;
struct RagMember;
constexpr int TBM_PLAIN = 0, TBM_PROLONG = 1, TBM_ZEROIN = 4;   // mode of launch_rb_tb_gen
bool launch_rb_tb_gen(Field Uin, Field Uout, Field F, int sweeps, const MGGeom &g, int mode, Field E, hipStream_t s, const RagMember *rag = nullptr, int lev = 0,
                      bool pack = true);      // pack = false: every column tile in a workgroup of its own (SC_LEGACY_UNPACKED_TILES)
int  launch_rb_tb_prolong0(Field Uin, Field Uout, Field F, int sweeps, const MGGeom &g, Field E, float *partial, hipStream_t s);
int  tb_blocks_level0(int W, int H, int C, int sweeps);
void launch_max_final(const float *d_partial, int n, unsigned *d_out, hipStream_t s);
void launch_max_final2(const float *d_a, int na, const float *d_b, int nb, unsigned *d_out2, hipStream_t s, const unsigned *flag = nullptr);   // out[0] = max a, out[1] = max b (-1: b empty), out[2] = *flag (0 without one)
// tiling of a level-0 launch (sc_cycle0.hip, launch_cycle0 below)
void cycle0_row_geometry(int H, int sweeps, int &nby, int &step, int &hy);
int  cycle0_blocks(int W, int H, int C, int sweeps);
// host only (sc_hip_cycle0_plan): head[8] = nbx, nby, column step, row step, hx, hy, waves per tile, rows per wave; verdicts[(by nbx + bx) waves + wave] =
// what k_cycle0's `inner` test answers there (restated beside cycle0_plan, sc_cycle0.hip); ncx .. n2y: coarse unknowns of levels 1 and 2.  -1: no such launch.
int  cycle0_plan(int W, int H, int sweeps, bool prolong, bool composed, int ncx, int ncy, int n2x, int n2y, int head[8], int *verdicts, int capacity);
// coarse level: zero-guess pre-smoothing + residual + restriction fused (Uout = smoothed correction, Fc = next RHS)
bool launch_cycle_coarse(Field Uout, Field F, Field Fc, const MGGeom &g, int sweeps, hipStream_t s, bool half_io = false,
                         const RagMember *rag = nullptr, int lev = 0, bool pack = true);

// residual: d_out[0] = sum r^2, d_out[1] = sum lap^2 (double); d_partials holds >= 2*max_blocks doubles
int  residual_max_blocks();
void launch_residual(Field U, Field F, double *d_partials, double *d_out, hipStream_t s);

// ---------------------------------------------------------------- multigrid (sc_mg_kernels.hip)
// One grid direction of a level pair.  Level l has n interior points at unit spacing (in
// level units) except the LAST gap, from point n to the Dirichlet boundary, which is alpha
// (0.5 <= alpha <= 1.5).  That one irregular interval lets any ROI size coarsen without
// moving the boundary: coarse points sit on the even fine points 2,4,..,2*nc.
struct MGDim {
    int n, nc;        // interior points on this level / on the next coarser one
    float alpha;      // last gap of this level
    float cw_last;    // stencil weight of the inner neighbour at the last point: 2/(1+alpha)
    float d_last;     // diagonal contribution at the last point: 2/alpha (regular: 2)
    float tw1, tw2;   // interpolation weights of the fine tail points 2nc+1, 2nc+2 (0 if absent)
    float inv_last;   // 1 / (row sum of the transposed interpolation at coarse point nc)
};
struct MGGeom { MGDim x, y; };
// Composed prolongation source (sc_mg_device.h): the level interpolated from ran without post-smoothing and without a
// prolongation launch of its own; E2 = finished correction of the level below it, g1 = its geometry (transfer to that level).
struct ComposeArgs { Field E2; MGGeom g1; };

// The bits of k_cycle0's template parameter TAG: the FORM of a launch (sc_cycle0.hip).
constexpr int C0_TIMING   = 1;      // the same code under a second symbol, for isolated timing (sc_hip_time_cycle0_form)
constexpr int C0_F_HALF   = 2;      // F holds float16 (level 0 only: the clone's right-hand side as the pre-process stored it)
constexpr int C0_U_HALF   = 4;      // Uin holds float16: the first launch of a clone reads the 8-bit destination values the pre-process stored so
constexpr int C0_FINAL    = 8;      // the cycle the stop rule judges: no residual / restriction; leaves the float-table correction's cell shares in `bands` if not null
constexpr int C0_COMPOSED = 16;     // level 0 only: E is level 1's correction after pre-smoothing, the interpolated level-2 correction is added on the fly (ComposeArgs)
constexpr int C0_OUT      = 32;     // a final cycle leaving as bytes: Uout's memory receives planar 8-bit output values (node correction added, clamped, truncated)
constexpr int C0_BANDS    = 64;     // a full cycle that leaves the float-table correction's cell shares of the field it writes in `bands`
constexpr int C0_L1_HALF  = 128;    // LEVEL 1's right-hand side and correction are float16: what level 0 restricts to and interpolates from, the level-1 launch's own F and Uout
constexpr int C0_Q16_IN   = 256;    // Uin holds 16-bit fixed point (c0_load_q16): the field between the first level-0 launches of the fast path
constexpr int C0_Q16_OUT  = 512;    // ... and so will Uout; a store that saturates reports itself (AbortFlag)
constexpr int C0_PACK_ROWS = 6;     // ... with bands of at most this many rows per lane
constexpr int C0_PACK     = 2048;   // coarse levels only (GEN, ZEROIN): the last column tile of several planes in one workgroup, plane and column per lane (coarse_tile_plan)
constexpr int C0_OUT3     = 4096;   // with C0_OUT | C0_FINAL, a same-size group: one workgroup per (member, tile) runs the member's three channels in turn and writes the tile's interleaved bytes into the destination itself (ImageJobs); nothing planar is stored, no splice launch follows
constexpr int C0_IN3      = 8192;   // the first launch of a same-size group, member-major like C0_OUT3: the initial field is read from the members' destination bytes (ImageJob::body_src) instead of float16 planes; Uin carries geometry only
constexpr int C0_RAG      = 1024;   // a SIZE CLASS (RagMember): strides and grid are the class's, all else the member's, read from rag[channel / 3]; tiles beyond its extent leave

// One level-0 launch (sc_cycle0.hip): [prolongation of E +] `sweeps` red-black GS sweeps [+ residual + restriction into Fc]; launch_cycle0 derives (T, PRO, TAG) from these facts
struct Cycle0Launch {
    Field Uin, Uout, F, Fc, E;         // E: the correction interpolated from (composed: level 1's after its pre-smoothing); Fc: level 1's right-hand side
    MGGeom g{};
    int sweeps = 0;                    // post + pre (full cycle), post (final cycle) or pre (first launch, catch-up)
    bool prolong = false;              // add P E first and write the per-workgroup max |P E| to `partial`
    bool f_half = false, u_half = false, q16_in = false, q16_out = false;      // F / Uin hold float16; Uin / Uout hold 16-bit fixed point
    bool final_cycle = false, out_bytes = false;      // the judged cycle: nothing restricted; ... leaving as planar output bytes in Uout's memory, `lm` added
    bool out_interleaved = false;      // ... leaving as interleaved bytes in the destinations of `jobs` instead (C0_OUT3): members 0 .. njobs - 1 <= ImageJobs::MAX own channels 3i .. 3i + 2; `sat` set: nothing is written
    bool in_bytes = false;             // the first launch of a same-size group reads the initial field from the destinations of `jobs` (their body_src) instead of Uin (C0_IN3): not u_half, Uin is geometry only
    const ImageJob *jobs = nullptr; int njobs = 0;
    bool composed = false;             // the prolongation source is composed from E and comp.E2 (comp.g1: level 1's geometry)
    bool l1_half = false, timing = false;      // level 1 keeps float16 fields (mg_level1_half); the form's twin under a second symbol
    ComposeArgs comp{};
    float4 *bands = nullptr;           // final cycle or full cycle of four sweeps: receives the correction's cell shares, two float4 per (channel, tile row, wave, cell)
    float *partial = nullptr;
    LmNodes lm{};
    AbortFlag sat{};                   // where a saturating 16-bit store reports itself
    const RagMember *rag = nullptr;    // the launch serves a size class
    hipStream_t s = nullptr;
};
bool cycle0_form(const Cycle0Launch &d, int &T, bool &PRO, int &TAG);      // the form of the launch: false if the library does not instantiate it
int  cycle0_form_at(int i, int &T, bool &PRO, int &TAG);                   // entry i of the table of instantiated forms (if any); returns its length
int  launch_cycle0(const Cycle0Launch &d);      // the number of partial maxima written, 0 without a prolongation, -1: form not instantiated, nothing launched

// ---- size classes ("ragged groups", round 5): clones of DIFFERENT ROI sizes through one set of solver launches -----------------
// The members of a class share the fields' strides (pitch and plane of the class's largest width / height on every level), the
// launch grids (sized for the class) and every compile-time choice (hierarchy depth, the bottom solve's operand padding, the
// correction's mode-block counts); everything that depends on a member's own W x H is read from this table by member index
// (channel / 3: a wave-uniform scalar load) at kernel entry: its field size on every level, the level geometries, its bottom
// matrices, its float-table correction tables.  Tiles beyond a member's extent exit.  Every member's arithmetic is, operation for
// operation, that of its solo run: same bytes alone, in a same-size group or in a class.
constexpr int RAG_MAX_LEVELS = 12;
struct RagMember {
    int W, H;                                  // level-0 field, ring included
    int lw[RAG_MAX_LEVELS], lh[RAG_MAX_LEVELS]; // level-l field, ring included (lw[0] = W): clamp bounds of a member's loads
    MGGeom g[RAG_MAX_LEVELS];                  // level l and its transfer to l + 1
    const unsigned char *mm;                   // matrix-core operands of the member's directly solved level (k_mg_tail)
    int npx, npy;                              // ... padded to this many per side (32 or 64): the member's own, as in its solo run
    // float-table correction (sc_lowmode.hip): the member's node grid, its split of the projection and its tables
    int lm_nx, lm_ny, lm_cells_y, lm_nxt, lm_nrs, lm_nparts, lm_Kx, lm_Ky;     // nodes, cell rows, column tiles / row splits / parts of the projection, modes kept
    const float *lm_Sx, *lm_Sy, *lm_R;
    const int *lm_map[2];                      // parts of each cell row for the 2- and the 4-sweep tiling of a level-0 launch
};

void launch_rb_half_gen(Field U, Field F, int color, float omega, MGGeom g, hipStream_t s);
void launch_residual_restrict(Field U, Field F, Field Fc, MGGeom g, hipStream_t s); // Fc = 4 * normalised P^T (F - A U)
int  prolong_blocks(int nx, int ny, int C);
// Uf += P Uc; with d_partial (>= prolong_blocks floats) also *d_maxcorr = bits of max |P Uc|
void launch_prolong_add(Field Uc, Field Uf, MGGeom g, float *d_partial, unsigned *d_maxcorr, hipStream_t s);
void launch_fill_zero(Field U, hipStream_t s);

// bottom of the V-cycle fused into one launch (one workgroup per channel, levels LDS resident)
constexpr int MG_BOTTOM_MAX_LEVELS = 12;
constexpr int MG_BOTTOM_LDS_BYTES = 152 * 1024;   // of the CU's 160 KiB
struct MGBottomLevel { MGGeom g; float omega; int offU, offF, pitch; };   // LDS offsets / row pitch in floats
// Direct solve of one bottom level by fast diagonalisation (sc_mg_levels.cpp has the matrices built: build_fd):
// the level's operator is a tensor sum Tx (x) I + I (x) Ty of two tridiagonal 1-D operators, so with
// Tx = Vx Lx Vx^-1, Ty = Vy Ly Vy^-1 the solution of A U = F is
//     U = Vy [ (Vy^-1 F Vx^-T) / (ly_j + lx_i) ] Vx^T      -- four small dense products in LDS.
// fd_mats (HBM, padded to multiples of 4, zero padded): Mx1[nxp][nxp], My1T[nyp][nyp], My2T[nyp][nyp],
// Mx2[nxp][nxp], Dinv[nyp][nxp].  fd_level < 0: no direct solve (V-cycle down to the coarsest level).
struct MGBottomArgs {
    int nlevels, pre, post, coarse_sweeps, lds_floats;
    int fd_level, fd_nxp, fd_nyp, fd_off;   // level index inside the bottom, padded sizes, LDS offset of the FD region
    const float *fd_mats;
    Field Ftop, Utop;       // HBM planes of the first bottom level: RHS in, correction out
    MGBottomLevel lv[MG_BOTTOM_MAX_LEVELS];
};
__host__ __device__ static inline long fd_mat_floats(int nxp, int nyp) { return 2L * nxp * nxp + 2L * nyp * nyp + (long)nxp * nyp; }
__host__ __device__ static inline long fd_lds_floats(int nxp, int nyp) { return fd_mat_floats(nxp, nyp) + 2L * nxp * nyp; }
hipError_t mg_bottom_prepare();
// per-size state built on the device (sc_mg_kernels.hip): the direct solve's matrices from the closed-form eigenpairs of the
// level's two 1-D operators (nx, ny <= 128), and the zeroing of every plane of the levels >= 1 in one launch
// mm != nullptr: also the operands of the matrix-core form (k_mg_bottom_mm), padded to NPX / NPY (32, 64 or 96)
void launch_fd_build(float *mats, const MGGeom &g, int nxp, int nyp, hipStream_t s, unsigned char *mm = nullptr, int NPX = 0, int NPY = 0);
void launch_fd_build_rag(const RagMember *rag, int members, int lev, hipStream_t s);   // the operands of every member of a size class (each at its own padding), one launch
__host__ __device__ static inline long fd_mm_bytes(int NPX, int NPY) { return 4L * (2L * NPX * NPX + 2L * NPY * NPY + (long)NPX * NPY); }   // AX1 | AX2 | AY1 | AY2 | Dinv, float
// the bottom's first level solved directly on the matrix cores: right-hand side in (Ftop), correction out (Utop), nx x ny unknowns
struct MGBottomMM { const unsigned char *mm; Field Ftop, Utop; int nx, ny; };
bool launch_mg_bottom_mm(const MGBottomMM &a, int NPX, int NPY, int C, hipStream_t s);
// the level above the bottom (F: its right-hand side, U: receives its finished correction) and the bottom in one launch
// (sc_mg_kernels.hip, k_mg_tail); false: not a shape this path serves (the caller launches the three kernels it replaces)
struct MGTail { const unsigned char *mm; Field F, U; MGGeom g; int pre, post; unsigned long long *stamps;
                const RagMember *rag; int lev; bool rag_uniform; };      // (rag_uniform: every member of the class has the class's operand padding)      // rag != nullptr: a size class -- g, mm and F's row count are member (channel / 3)'s own, at its level `lev`   // stamps: measurement only (11 shader-clock values of channel 0), else nullptr
bool launch_mg_tail(const MGTail &a, int NPX, int NPY, int C, hipStream_t s);
struct ZeroJobs { enum { MAX = 48 }; void *p[MAX]; size_t n16[MAX]; int count; };     // n16: 16-byte units
void launch_zero_multi(const ZeroJobs &z, hipStream_t s);
void launch_mg_bottom(const MGBottomArgs &a, int C, hipStream_t s);

} // namespace sc
