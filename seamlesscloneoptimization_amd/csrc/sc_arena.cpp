// sc_arena.cpp -- an instance's memory: the grow-only device arena and its page-locked staging, the row transfers between
// caller images and the device, and the solution fields carved out of the arena.
#include "sc_instance.h"
#include <algorithm>
#include <cstring>
#include <thread>

namespace sc {

int hip_fail(Instance *I, hipError_t e, const char *what)
{
    if (I) {
        I->err = std::string(what) + ": " + hipGetErrorString(e);
        I->scan_counter_dirty = true;      // a launch that never completed may have left the scan's arrival counter non-zero
    }
    return SC_ERR_HIP;
}

// Grow-only, amortised (the reference's SCImage::resize, seamlessClone_imp.h:83,119-121,137-149).  Round 5: growth stays off the
// stream's critical path -- the new block is allocated FIRST, with no wait on the stream, and the block it replaces is RETIRED, not
// freed: launches already queued keep reading and writing it, and hipFree (a device-wide synchronisation that also stalls the other
// instances of a pool) happens once, when the instance is destroyed.  Capacities double, so the retired blocks of a buffer add up to
// less than its final size.  (Rounds 1-4: stream synchronisation + hipFree + hipMalloc + a memset of the whole new capacity inside
// the call that happened to need more -- the p95 / max of the first call at a new ROI size: 1.6x / 4.0x the steady call.)
// zero: the caller reads the block before it writes it (tables with zero padding, accumulation buffers); the large blocks -- fields,
// level planes, image staging -- are written before they are read (or their unwritten parts only ever reach masked lanes) and skip it.
int ensure(Instance *I, DevBuf &b, size_t bytes, bool zero)
{
    if (bytes <= b.cap) {
        // (testing: a buffer that is RE-USED without zeroing holds what the previous call left -- here: NaN bytes, in place before any
        //  stream touches it; every stream of the instance has drained first, the previous call may still be reading)
        if (!zero && bytes && (I->opts.flags & SC_FLAG_POISON_ARENA)) {
            SC_HIP(I, hipStreamSynchronize(I->stream));
            if (I->aux) SC_HIP(I, hipStreamSynchronize(I->aux));
            if (I->aux2) SC_HIP(I, hipStreamSynchronize(I->aux2));
            SC_HIP(I, hipMemsetAsync(b.p, 0xFF, bytes, I->stream));
            SC_HIP(I, hipStreamSynchronize(I->stream));
        }
        return SC_OK;
    }
    size_t ncap = bytes > 2 * b.cap ? bytes : 2 * b.cap;
    ncap = (ncap + 4095) & ~(size_t)4095;
    void *np = nullptr;
    bool own = true;
    constexpr size_t SLAB_FIRST = (size_t)16 << 20, SLAB_PIECE_MAX = (size_t)8 << 20;
    if (ncap <= SLAB_PIECE_MAX) {          // a piece of a slab: no hipMalloc unless the slabs are used up
        if (I->slabs.empty() || I->slabs.back().cap - I->slabs.back().used < ncap) {
            Instance::Slab sl;
            sl.cap = I->slabs.empty() ? SLAB_FIRST : 2 * I->slabs.back().cap;
            SC_HIP(I, hipMalloc((void **)&sl.base, sl.cap));
            I->arena_bytes += sl.cap;
            I->slabs.push_back(sl);
        }
        Instance::Slab &sl = I->slabs.back();
        np = sl.base + sl.used;
        sl.used += ncap;                   // (ncap is a multiple of 4096: every piece is page aligned)
        own = false;
    } else {
        SC_HIP(I, hipMalloc(&np, ncap));
        I->arena_bytes += ncap;
    }
    if (zero) SC_HIP(I, hipMemsetAsync(np, 0, ncap, I->stream));
    else if (I->opts.flags & SC_FLAG_POISON_ARENA) {      // (testing: what recycled memory may hold; in place before ANY stream uses the block)
        SC_HIP(I, hipMemsetAsync(np, 0xFF, ncap, I->stream));
        SC_HIP(I, hipStreamSynchronize(I->stream));
    }
    if (b.p && b.own) {                              // (a replaced slab piece simply stays unused)
        I->retired.push_back(b);
        I->retired_bytes += b.cap;
        // ... unless the retired blocks have become large (an instance walking up through multi-gigabyte ROI sizes): then, and only
        // then, wait for the stream and give them back -- a growth step of that size is milliseconds of hipMalloc anyway
        if (I->retired_bytes > ((size_t)1 << 30)) {
            SC_HIP(I, hipStreamSynchronize(I->stream));
            if (I->aux) SC_HIP(I, hipStreamSynchronize(I->aux));
            if (I->aux2) SC_HIP(I, hipStreamSynchronize(I->aux2));
            for (DevBuf &r : I->retired) { I->arena_bytes -= r.cap; dev_release(r); }
            I->retired.clear();
            I->retired_bytes = 0;
        }
    }
    b.p = np;
    b.cap = ncap;
    b.own = own;
    return SC_OK;
}

// Page-locked host staging, grow-only.  At least 256 KB per buffer (round 5): the small ones -- eigenvalue tables, ratio tables, part
// maps, the stop rule's maxima -- used to start at a page and re-grow (stream wait + hipHostFree + hipHostMalloc: ~0.3 ms) whenever a
// caller's ROI size set a new record: the slowest first calls of the new_size leg (2.4-3.0x the steady call) were exactly those.
int ensure_pinned(Instance *I, DevBuf &b, size_t bytes)
{
    if (bytes <= b.cap) return SC_OK;
    size_t ncap = bytes > 2 * b.cap ? bytes : 2 * b.cap;
    ncap = std::max(ncap, (size_t)256 << 10);
    ncap = (ncap + 4095) & ~(size_t)4095;
    if (b.p) {
        SC_HIP(I, hipStreamSynchronize(I->stream));
        SC_HIP(I, hipHostFree(b.p));
        b.p = nullptr; b.cap = 0;
    }
    SC_HIP(I, hipHostMalloc(&b.p, ncap, hipHostMallocDefault));
    b.cap = ncap;
    if (I->opts.flags & SC_FLAG_POISON_ARENA) memset(b.p, 0x5A, ncap);      // (testing: what recycled host memory may hold -- the pad bytes of packed rows are never written; 0x5A: neither "inside the mask" nor "outside")
    return SC_OK;
}

static bool is_pinned(const void *p)
{
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return attr.type == hipMemoryTypeHost;
}

// Row-wise host copy between a caller image and the pinned staging.  A single core moves ~14 GB/s, which
// would make the packing (not PCIe, not the GPU) the longest part of a 2048^2 call, so copies above 512 KB are
// shared between the calling thread and the instance's parked helpers (sc_hostcopy.h) in ~256 KB pieces.
// (1 MB until late in round 5: the splice of a 592^2 output, 1 037 232 bytes, ran on one core: 71 us of a 0.37-ms call, 25 shared;
//  256 KB loses: waking the helpers costs more than they save on the 0.4-MB pieces of a small call's upload)
void copy_rows(Instance *I, uint8_t *dst, size_t dpitch, const uint8_t *src, size_t spitch, size_t row_bytes, int rows)
{
    const size_t total = row_bytes * (size_t)rows;
    auto span = [=](int y0, int y1) {
        if (dpitch == row_bytes && spitch == row_bytes) {
            memcpy(dst + (size_t)y0 * row_bytes, src + (size_t)y0 * row_bytes, row_bytes * (size_t)(y1 - y0));
            return;
        }
        for (int y = y0; y < y1; ++y) memcpy(dst + (size_t)y * dpitch, src + (size_t)y * spitch, row_bytes);
    };
    if (total < ((size_t)512 << 10)) { span(0, rows); return; }
    if (!I->copier) {
        const unsigned hw = std::thread::hardware_concurrency();
        int n = 8;                         // measured: packing saturates near 8 threads
        if (hw && (unsigned)n > hw) n = (int)hw;
        I->copier.reset(new RowCopier(n - 1));
    }
    const int rows_per = (int)std::max<size_t>(1, ((size_t)256 << 10) / std::max<size_t>(row_bytes, 1));
    const int parts = (rows + rows_per - 1) / rows_per;
    I->copier->parallel(parts, [&](int i) { span(i * rows_per, std::min(rows, (i + 1) * rows_per)); });
}

// rows x row_bytes from caller memory (pitch hpitch) to device memory (pitch dpitch).
// The library issues NO 2-D copies.  hipMemcpy2DAsync becomes one DMA per row (~6 us each, measured with
// rocprofv3: 384 copies per 298x192 clone), and under rocprofv3's copy interception the row DMAs of the SECOND of two
// back-to-back 2-D copies were released out of stream order (they landed after the kernels
// that read them had started, the last ones after teardown had freed the arena -> GPU memory-access fault).  So
// every strided host image -- pageable or caller-pinned -- is packed into the instance's pinned staging AT THE
// DEVICE PITCH and crosses PCIe as linear copies; only a caller-pinned image that already has the device pitch is
// copied in place.  The caller must not reuse `stage` before the stream has passed these copies.
int upload_rows(Instance *I, DevBuf &stage, void *d, size_t dpitch, const uint8_t *h, size_t hpitch,
                size_t row_bytes, int rows)
{
    if (rows <= 0 || row_bytes == 0) return SC_OK;
    if (hpitch == dpitch && is_pinned(h)) {
        SC_HIP(I, hipMemcpyAsync(d, h, dpitch * (size_t)(rows - 1) + row_bytes, hipMemcpyHostToDevice, I->stream));
        return SC_OK;
    }
    int rc = ensure_pinned(I, stage, dpitch * (size_t)rows);
    if (rc) return rc;
    uint8_t *s = (uint8_t *)stage.p;
    // Pieces: the DMA of piece k runs while piece k+1 is being packed.  The first piece is small (1 MB: the link starts moving
    // early), the following ones grow to 8 MB.  (Measured against equal 4 MB pieces on one box: no difference beyond noise --
    // the packing itself, 33-45 GB/s with eight threads, is what paces this path, not the DMA commands.)
    size_t piece = (size_t)1 << 20;
    for (int y0 = 0; y0 < rows;) {
        const int n = std::min((int)std::max<size_t>(1, piece / dpitch), rows - y0);
        copy_rows(I, s + (size_t)y0 * dpitch, dpitch, h + (size_t)y0 * hpitch, hpitch, row_bytes, n);
        SC_HIP(I, hipMemcpyAsync((uint8_t *)d + (size_t)y0 * dpitch, s + (size_t)y0 * dpitch, dpitch * (size_t)(n - 1) + row_bytes,
                                 hipMemcpyHostToDevice, I->stream));
        y0 += n;
        piece = std::min(piece * 4, (size_t)8 << 20);
    }
    return SC_OK;
}

// rows x row_bytes from device memory (pitch dpitch) into caller memory (pitch hpitch): ONE linear device-to-host copy
// into the pinned staging, a wait, then the rows are spliced on the host (no 2-D copy, see upload_rows).  Synchronous.
int download_rows(Instance *I, DevBuf &stage, uint8_t *h, size_t hpitch, const void *d, size_t dpitch,
                  size_t row_bytes, int rows)
{
    if (rows <= 0 || row_bytes == 0) return SC_OK;
    const size_t total = dpitch * (size_t)(rows - 1) + row_bytes;
    int rc = ensure_pinned(I, stage, total);
    if (rc) return rc;
    SC_HIP(I, hipMemcpyAsync(stage.p, d, total, hipMemcpyDeviceToHost, I->stream));
    SC_HIP(I, hipStreamSynchronize(I->stream));
    copy_rows(I, h, hpitch, (const uint8_t *)stage.p, dpitch, row_bytes, rows);
    return SC_OK;
}

static Field make_field(void *p, int W, int H, int C)
{
    Field f;
    f.p = (float *)p; f.W = W; f.H = H; f.C = C;
    f.pitch = round_up(W, 64);
    f.plane = (size_t)f.pitch * H;
    return f;
}

int setup_fields(Instance *I, int W, int H, int C)
{
    field_moved(I);
    I->out_direct = false;             // new fields are about to be built (a clone's pre-process, sc_hip_build_rhs, sc_hip_field_load)
    Field proto = make_field(nullptr, W, H, C);
    const size_t bytes = proto.bytes() + 4096;
    int rc;
    if ((rc = ensure(I, I->d_U0, bytes, false))) return rc;
    if ((rc = ensure(I, I->d_U1, bytes, false))) return rc;
    if ((rc = ensure(I, I->d_F, bytes, false))) return rc;
    const bool same = I->F.p == I->d_F.p && I->U0.p == I->d_U0.p && I->U1.p == I->d_U1.p && I->F.W == W &&
                      I->F.H == H && I->F.C == C;
    I->U0 = make_field(I->d_U0.p, W, H, C);
    I->U1 = make_field(I->d_U1.p, W, H, C);
    I->F = make_field(I->d_F.p, W, H, C);
    I->result_in_U1 = false;
    I->f_half = false;        // whoever fills F next says what it holds
    I->u_half = I->u0_bytes = false;
    if (!same) I->mg.clear(); // the multigrid hierarchy is rebuilt only when the ROI shape changes
    return SC_OK;
}

} // namespace sc
