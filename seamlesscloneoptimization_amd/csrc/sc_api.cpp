// sc_api.cpp -- the extern "C" boundary of libseamlessclone_hip.so (include/seamlessclone_hip.h): the instance's lifecycle,
// options and memory entries and the single clone.  The batch path is in sc_batch.cpp, the arena and row transfers in
// sc_arena.cpp, the test and measurement hooks (include/seamlessclone_hip_testing.h) in sc_hooks.cpp.
//
// Host orchestration of one clone (reference call stack: seamlessClone_imp.cu:265-352 ->
// seamlessClone_imp.cpp:430-486 seamlessCloneGPU -> :2105-2135 run()):
//   H2D mask -> bbox kernel -> 16-byte read-back (the one mid-pipeline sync the reference also
//   has, :1012) -> H2D of the face/body ROI only -> fused erode -> fused pre-process and
//   iterative solve (solve_step, sc_solver.cpp) -> fused post-process into the body ROI -> D2H of the interior straight
//   into the caller's image (replaces the reference's D2H + host splice loop, :470-483).
#include "sc_pcg.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

using namespace sc;

namespace sc {

Instance *get(void *p)
{
    Instance *I = (Instance *)p;
    if (!I || !I->ok()) return nullptr;
    return I;
}

// The prologue of the clone entries: a live instance, no error left from an earlier call, the per-call statistics reset, the instance's
// device current.  Enqueues nothing.
int begin_call(void *p, Instance *&I)
{
    I = get(p);
    if (!I) return SC_ERR_BAD_ARG;
    I->err.clear();
    I->info.field_retry = 0; I->info.new_size = 0; I->info.group_members = 0; I->info.group_ragged = 0;
    SC_HIP(I, hipSetDevice(I->gpu));
    return SC_OK;
}

int validate_images(Instance *I, const void *face, int fc, int fr, int fs, const void *body, int bc, int br,
                    int bs, const void *mask, int mc, int mr, int ms)
{
    if (!face || !body || !mask) { I->err = "null image pointer"; return SC_ERR_BAD_ARG; }
    if (fc <= 0 || fr <= 0 || bc <= 0 || br <= 0 || mc <= 0 || mr <= 0) { I->err = "empty image"; return SC_ERR_BAD_SIZE; }
    if (fc != mc || fr != mr) { I->err = "face and mask sizes differ"; return SC_ERR_BAD_SIZE; }
    if (fs < 3 * fc || bs < 3 * bc || ms < mc) { I->err = "row step smaller than the row"; return SC_ERR_BAD_SIZE; }
    if (I->clone_mode != SC_NORMAL_CLONE && (I->opts.flags & SC_FLAG_OPENCV_GREY_MASK)) {
        I->err = "SC_FLAG_OPENCV_GREY_MASK supports SC_NORMAL_CLONE only";
        return SC_ERR_BAD_ARG;
    }
    return SC_OK;
}

// bbox kernel + read-back of the rectangle into h_rect[4..7] (enqueue only).  mask is a device pointer.
// Stage mark k of the run's timeline (finish_timing).  An empty stage reuses the previous mark instead of recording an
// event: every hipEventRecord is a few microseconds of host time in front of the next launch.
static int tmark(Instance *I, int k, bool empty_stage = false)
{
    if (!I->stage_marks) { I->tm[k] = nullptr; return SC_OK; }    // asynchronous device call: nobody reads the timeline
    if (I->marks_ends_only && k != 0 && k != 7) empty_stage = true;   // SC_FLAG_NO_STAGE_MARKS: first and last mark only
    if (empty_stage && k > 0) { I->tm[k] = I->tm[k - 1]; return SC_OK; }
    I->tm[k] = I->ev[k];
    SC_HIP(I, hipEventRecord(I->ev[k], I->stream));
    return SC_OK;
}

// With `predicted` the same launch also erodes that ROI (the whole mask stage in one kernel: the erode of a predicted box
// does not depend on the box being computed); device_clone then skips its own erode launch.
int bbox_enqueue(Instance *I, const uint8_t *d_mask, int mc, int mr, int ms, const Geo *predicted)
{
    // The scan's workgroups leave their extrema as parts, the last one to finish folds them into the rectangle (seeded like the
    // reference's, seamlessClone_imp.cpp:1006) and stores it in device memory AND in the pinned mailbox h_rect[4..7]: no seed
    // upload and no read-back copy in the stream (each was a command of its own in front of / behind the launch).
    int rc = ensure(I, I->d_bbox_parts, sizeof(int) * 4 * (size_t)mask_bbox_blocks(mc, mr));
    if (rc) return rc;
    BboxFold fold;
    fold.parts = (int *)I->d_bbox_parts.p;
    fold.counter = (unsigned *)(I->d_rect + 32);      // a line of its own; zero between launches (the folding workgroup resets it)
    fold.rect_dev = I->d_rect;
    fold.rect_host = I->h_rect + 4;
    I->erode_done = false;
    I->scan_pending = false;
    I->scan_fence = nullptr;
    if (I->scan_counter_dirty) {      // after a HIP error: the folding workgroup is the only one that resets the counter, and it may never have run
        SC_HIP(I, hipMemsetAsync(fold.counter, 0, sizeof(unsigned), I->stream));
        I->scan_counter_dirty = false;
    }
    if (predicted && !(I->opts.flags & SC_FLAG_OPENCV_GREY_MASK)) {
        // A clone launched on a predicted box needs the scan's answer only at its end: the erode of the predicted ROI goes out
        // alone and the scan rides in the pre-process launch behind it (device_clone, launch_preprocess) -- off the critical path.
        I->mpitch = round_up(predicted->W, 64);
        rc = ensure(I, I->d_M, (size_t)I->mpitch * predicted->H, false);
        if (rc) return rc;
        // (round 4, late: no erode launch either -- the pre-process tiles form the eroded mask themselves and leave it in d_M)
        I->erode_done = true;
        I->pending_scan = BboxTask();
        I->pending_scan.mask = d_mask; I->pending_scan.mw = mc; I->pending_scan.mh = mr; I->pending_scan.mstep = ms;
        I->pending_scan.fold = fold;
        I->pending_scan.g = *predicted;
        I->pending_scan.mask_bytes = (size_t)ms * (mr - 1) + (size_t)(predicted->x0 + predicted->W + 1);      // as launch_mask_erode3 counts them
        I->scan_pending = true;
    } else
    launch_mask_bbox(d_mask, mc, mr, ms, fold, I->stream);
    SC_HIP(I, hipGetLastError());
    return tmark(I, 2);
}

int geo_from_rect(Instance *I, const int r[4], int cx, int cy, Geo &g)
{
    const int x0 = r[0], x1 = r[1], y0 = r[2], y1 = r[3];
    if (!((x1 - x0) > 0 && (y1 - y0) > 0)) { I->err = "mask has no usable non-zero region"; return SC_ERR_EMPTY_MASK; }
    g.x0 = x0; g.y0 = y0; g.W = x1 - x0 + 1; g.H = y1 - y0 + 1;
    g.ltx = cx - (g.W >> 1); // seamlessClone_imp.cpp:1066
    g.lty = cy - (g.H >> 1);
    return SC_OK;
}

// synchronous form: waits for the device's rectangle (the reference does the same, seamlessClone_imp.cpp:1012)
int device_bbox(Instance *I, const uint8_t *d_mask, int mc, int mr, int ms, int cx, int cy, Geo &g)
{
    int rc = bbox_enqueue(I, d_mask, mc, mr, ms);
    if (rc) return rc;
    SC_HIP(I, hipStreamSynchronize(I->stream));
    return geo_from_rect(I, I->h_rect + 4, cx, cy, g);
}

// Predicted bounding box for a clone launched before the device's answer is back: the previous rectangle when the
// mask has the size of the previous call's (a sequence of clones with one mask), else the whole interior (every
// mask that touches its four inner borders, all-255 masks in particular).  After a wrong guess speculation pauses
// for a few calls, so a stream of unpredictable masks pays at most one wasted clone in nine.
static bool predict_rect(Instance *I, int mc, int mr, int r[4])
{
    if ((I->opts.flags & SC_FLAG_NO_SPECULATE) || mc < 3 || mr < 3) return false;
    if (I->spec_cooldown > 0) { --I->spec_cooldown; return false; }
    if (I->last_mc == mc && I->last_mr == mr) { memcpy(r, I->last_rect, sizeof(int) * 4); return true; }
    r[0] = 1; r[1] = mc - 2; r[2] = 1; r[3] = mr - 2;
    return true;
}

static void remember_rect(Instance *I, int mc, int mr, const int r[4])
{
    I->last_mc = mc; I->last_mr = mr;
    memcpy(I->last_rect, r, sizeof(int) * 4);
}

static RectGuard make_guard(Instance *I, const int r[4])
{
    RectGuard g;
    g.d_rect = I->d_rect; g.x0 = r[0]; g.x1 = r[1]; g.y0 = r[2]; g.y1 = r[3];
    return g;
}

int check_roi(Instance *I, const Geo &g, int bc, int br)
{
    if (g.ltx < 0 || g.lty < 0 || g.ltx + g.W > bc || g.lty + g.H > br) {
        I->err = "ROI leaves the destination image";
        return SC_ERR_ROI_OOB;
    }
    return SC_OK;
}

// the erode of ROI g of the device mask into I->d_M: the reference's thresholded 3x erode, or OpenCV's minimum filters
void erode_mask(Instance *I, const uint8_t *d_mask, int ms, int mr, const Geo &g)
{
    if (I->opts.flags & SC_FLAG_OPENCV_GREY_MASK) launch_mask_erode_min7(d_mask, ms, g, (uint8_t *)I->d_M.p, I->mpitch, I->stream);
    else launch_mask_erode3(d_mask, ms, mr, g, (uint8_t *)I->d_M.p, I->mpitch, I->stream);
}

bool launch_clone_preprocess(Instance *I, const uint8_t *body_org, int bstep, const uint8_t *face_org, int fstep)
{
    const bool grey = (I->opts.flags & SC_FLAG_OPENCV_GREY_MASK) != 0;
    if (I->scan_pending) I->pending_scan.M_out = (uint8_t *)I->d_M.p;      // the launch's tiles erode the mask themselves and leave it here
    const bool had_scan = I->scan_pending;
    launch_preprocess(body_org, bstep, face_org, fstep, (const uint8_t *)I->d_M.p, I->mpitch, I->U0, I->U1, I->F,
                      I->stream, I->f_half, I->u_half, grey, I->scan_pending ? &I->pending_scan : nullptr, I->clone_mode);
    I->scan_pending = false;
    return had_scan;
}

// erode -> pre-process -> solve -> post-process on device-resident ROI origins
// out_org / ostep: where the output bytes go (ROI origin, row step): the destination itself for device-resident images; the
// host path hands a compact buffer of its own so that what comes back across PCIe is the ROI and nothing else
static int device_clone(Instance *I, const uint8_t *d_mask, int ms, int mr, const uint8_t *face_org, int fstep,
                        uint8_t *body_org, int bstep, const Geo &g, int passes, uint8_t *out_org = nullptr, int ostep = 0,
                        bool fence_at_end = true)
{
    // fence_at_end: the event behind which the scan's rectangle may be read (scan_fence) is the clone's LAST mark, not one of its
    // own behind the pre-process launch -- every event in the stream is a ~5 us bubble, and a caller that waits for the whole clone
    // anyway (a device-resident synchronous call, a host call whose output needs no copy command) loses nothing by it.  false: the
    // host call that still has device-to-host copies to enqueue behind the clone checks the rectangle while the clone's tail runs.
    if (!out_org) { out_org = body_org; ostep = bstep; }
    CallScope scope{ I };
    bool fence_pending = false;
    int rc;
    I->mpitch = round_up(g.W, 64);
    if ((rc = ensure(I, I->d_M, (size_t)I->mpitch * g.H, false))) return rc;
    if ((rc = setup_fields(I, g.W, g.H, 3))) return rc;
    const bool eroded = I->erode_done;
    if (!eroded) erode_mask(I, d_mask, ms, mr, g);
    I->erode_done = false;
    if ((rc = tmark(I, 4, eroded))) return rc;
    const SolveTarget to{ out_org, ostep };
    int solve_rc = SC_OK;
    for (int pass = 0; pass < passes; ++pass) {
        const bool last = pass == passes - 1;
        solve_rc = solve_step(I, to, [&]() -> int {
            const bool had_scan = launch_clone_preprocess(I, body_org, bstep, face_org, fstep);
            if (last && (rc = tmark(I, 5))) return rc;
            if (had_scan) {
                // the host compares the scan's rectangle (pinned mailbox) with its guess once THIS point of the stream has passed: mark 5
                // when it was really recorded just now, else the clone's last mark (fence_at_end), else an event of its own
                if (last && I->stage_marks && I->tm[5] == I->ev[5]) I->scan_fence = I->ev[5];
                else if (fence_at_end && I->stage_marks) fence_pending = true;
                else { SC_HIP(I, hipEventRecord(I->ev_scan, I->stream)); I->scan_fence = I->ev_scan; }
            }
            return SC_OK;
        });
        if (solve_rc != SC_OK && solve_rc != SC_ERR_NOT_CONVERGED) return solve_rc;
        if (!I->spec_post.done) {          // otherwise the solver already enqueued it behind its last cycle
            if (last && (rc = tmark(I, 6))) return rc;
            if ((rc = write_output(I, to))) return rc;      // (a solve that got here stored no 16-bit field or kept it in range)
        } else if (last) {
            I->tm[6] = nullptr;            // no mark between the last cycle and the post-process (an event there costs a
        }                                  // ~5 us bubble): ms_post is reported as 0 and ms_solve includes it
        SC_HIP(I, hipGetLastError());
    }
    if ((rc = tmark(I, 7))) return rc;
    if (!I->tm[6]) I->tm[6] = I->tm[7];
    if (fence_pending) {
        if (I->tm[7]) I->scan_fence = I->tm[7];
        else { SC_HIP(I, hipEventRecord(I->ev_scan, I->stream)); I->scan_fence = I->ev_scan; }
    }
    return solve_rc;
}

void fill_info_geo(Instance *I, const Geo &g)
{
    I->info.x0 = g.x0; I->info.y0 = g.y0; I->info.W = g.W; I->info.H = g.H; I->info.ltx = g.ltx; I->info.lty = g.lty;
    I->info.device_bytes = I->arena_bytes;
    I->info.device = I->gpu;
}

float ev_ms(hipEvent_t a, hipEvent_t b)
{
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, a, b) != hipSuccess) return 0.f;
    return ms;
}

} // namespace sc

extern "C" {

void sc_hip_default_opts(sc_solver_opts *o)
{
    if (!o) return;
    memset(o, 0, sizeof(*o));
    o->method = SC_METHOD_AUTO;
    o->max_sweeps = 30;      // V-cycles
    o->tol = 0.f;            // MULTIGRID stops on update_tol; the sweep methods on tol
    o->check_every = 1;
    o->omega = 0.f;
    o->sweeps_per_launch = 0;
    o->reference_warmup = 0;
    o->mg_pre = 2;
    o->mg_post = 2;
    o->update_tol = 0.25f;   // residual error ~0.01 grey levels (measured: tools/mg_convergence.py)
}

int sc_hip_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int sc_hip_device_pci_bus_id(int gpu_id, char *buf, int len)
{
    if (!buf || len < 16) return SC_ERR_BAD_ARG;
    buf[0] = 0;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || gpu_id < 0 || gpu_id >= n) { (void)hipGetLastError(); return SC_ERR_BAD_ARG; }
    if (hipDeviceGetPCIBusId(buf, len, gpu_id) != hipSuccess) { (void)hipGetLastError(); buf[0] = 0; return SC_ERR_HIP; }
    return SC_OK;
}

void *my_seamlessclone_api_imp_create_instance(int gpu_id)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || gpu_id < 0 || gpu_id >= n) {
        fprintf(stderr, "seamlessclone_hip: cannot use GPU %d (%d visible)\n", gpu_id, n);
        return nullptr;
    }
    if (hipSetDevice(gpu_id) != hipSuccess) return nullptr;
    Instance *I = new (std::nothrow) Instance();
    if (!I) return nullptr;
    if (!(I->pcg = new (std::nothrow) PcgState())) { delete I; return nullptr; }
    I->gpu = gpu_id;
    sc_hip_default_opts(&I->opts);
    bool ok = hipStreamCreateWithFlags(&I->stream, hipStreamNonBlocking) == hipSuccess;
    ok = ok && hipStreamCreateWithFlags(&I->aux, hipStreamNonBlocking) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&I->ev_fork, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&I->ev_join, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&I->ev_fd_fork, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&I->ev_fd, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&I->ev_scan, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipHostMalloc((void **)&I->h_rect, 8 * sizeof(int), hipHostMallocDefault) == hipSuccess;
    ok = ok && hipHostMalloc((void **)&I->h_red, 2 * sizeof(double), hipHostMallocDefault) == hipSuccess;
    ok = ok && hipMalloc((void **)&I->d_rect, 64 * sizeof(int)) == hipSuccess;       // the rectangle; word 32: the scan's arrival counter
    ok = ok && hipMemset(I->d_rect, 0, 64 * sizeof(int)) == hipSuccess;
    ok = ok && hipMalloc((void **)&I->d_partials, 2 * sizeof(double) * residual_max_blocks()) == hipSuccess;
    ok = ok && hipMalloc((void **)&I->d_red, 2 * sizeof(double)) == hipSuccess;
    ok = ok && hipMalloc((void **)&I->d_maxcorr, 4 * sizeof(unsigned)) == hipSuccess;
    ok = ok && hipHostMalloc((void **)&I->h_maxcorr, 4 * sizeof(unsigned), hipHostMallocDefault) == hipSuccess;
    ok = ok && mg_bottom_prepare() == hipSuccess;   // opt in to >64 KiB dynamic LDS for the bottom kernel
    for (int i = 0; ok && i < 8; ++i) ok = hipEventCreate(&I->ev[i]) == hipSuccess;
    ok = ok && hipEventCreate(&I->ev_k0) == hipSuccess && hipEventCreate(&I->ev_k1) == hipSuccess;
    for (int i = 0; ok && i < 8; ++i) ok = hipEventCreate(&I->ev_chunk[i]) == hipSuccess;
    if (!ok) {
        fprintf(stderr, "seamlessclone_hip: instance creation failed on GPU %d: %s\n", gpu_id,
                hipGetErrorString(hipGetLastError()));
        my_seamlessclone_api_imp_destroy(I);
        return nullptr;
    }
    return I;
}

void my_seamlessclone_api_imp_destroy(void *p)
{
    Instance *I = get(p);
    if (!I) return;
    (void)hipSetDevice(I->gpu);
    if (I->stream) (void)hipStreamSynchronize(I->stream);
    if (I->aux) (void)hipStreamSynchronize(I->aux);
    if (I->aux2) (void)hipStreamSynchronize(I->aux2);
    for (DevBuf &b : I->retired) dev_release(b);                    // blocks that growth replaced (ensure)
    for (Instance::Slab &sl : I->slabs) if (sl.base) (void)hipFree(sl.base);
    DevBuf *bufs[] = { &I->d_face, &I->d_body_roi, &I->d_out, &I->d_mask, &I->d_in, &I->d_M, &I->d_edge, &I->d_pois, &I->d_U0, &I->d_U1, &I->d_F };
    for (DevBuf *b : bufs) dev_release(*b);
    for (DevBuf &b : I->mg_bufs) dev_release(b);
    dev_release(I->mg_partial);
    if (I->h_partial.p) (void)hipHostFree(I->h_partial.p);
    for (DevBuf *b : { &I->lm.P, &I->lm.E, &I->lm.CN, &I->lm.B, &I->lm.maps[0].d, &I->lm.maps[1].d }) dev_release(*b);
    for (LowMode::Tables &t : I->lm.tables) {          // (lm.Sx / Sy / R are views of one of these)
        for (DevBuf *b : { &t.Sx, &t.Sy, &t.R }) dev_release(*b);
        if (t.hR.p) (void)hipHostFree(t.hR.p);
        if (t.ev) (void)hipEventDestroy(t.ev);
    }
    for (auto &m : I->lm.maps) if (m.h.p) (void)hipHostFree(m.h.p);
    for (DevBuf *b : { &I->dst.Sw, &I->dst.Sh, &I->dst.fxy, &I->dst.G, &I->dst.T1, &I->dst.T2 }) dev_release(*b);
    if (I->dst.hfxy.p) (void)hipHostFree(I->dst.hfxy.p);
    for (DevBuf *b : { &I->fft.A, &I->fft.B, &I->fft.tw64 }) dev_release(*b);
    for (FftDim &d : I->fft.dims) dev_release(d.chirp);
    if (I->fft.hst_all.p) (void)hipHostFree(I->fft.hst_all.p);
    for (FftFxy &f : I->fft.fxy) {
        dev_release(f.d);
        if (f.hst.p) (void)hipHostFree(f.hst.p);
        if (f.ev) (void)hipEventDestroy(f.ev);
    }
    if (I->fft.ev_fork) (void)hipEventDestroy(I->fft.ev_fork);
    if (I->fft.ev_built) (void)hipEventDestroy(I->fft.ev_built);
    pcg_release(I);
    dev_release(I->mg_fd);
    dev_release(I->rag.d_aux);
    if (I->rag.h_stage.p) (void)hipHostFree(I->rag.h_stage.p);
    if (I->rag.ev) (void)hipEventDestroy(I->rag.ev);
    if (I->rag.ev_ready) (void)hipEventDestroy(I->rag.ev_ready);
    if (I->ev_fd_fork) (void)hipEventDestroy(I->ev_fd_fork);
    if (I->ev_fd) (void)hipEventDestroy(I->ev_fd);
    if (I->ev_scan) (void)hipEventDestroy(I->ev_scan);
    if (I->d_rect) (void)hipFree(I->d_rect);
    dev_release(I->d_rects);
    dev_release(I->d_bbox_parts);
    if (I->h_rects.p) (void)hipHostFree(I->h_rects.p);
    if (I->d_partials) (void)hipFree(I->d_partials);
    if (I->d_red) (void)hipFree(I->d_red);
    if (I->d_maxcorr) (void)hipFree(I->d_maxcorr);
    if (I->h_maxcorr) (void)hipHostFree(I->h_maxcorr);
    if (I->h_rect) (void)hipHostFree(I->h_rect);
    if (I->h_red) (void)hipHostFree(I->h_red);
    for (DevBuf *b : { &I->h_face, &I->h_body, &I->h_mask, &I->h_out, &I->h_in, &I->h_hyst, &I->h_sx, &I->h_sy, &I->h_state, &I->h_gt, &I->h_smt, &I->h_lo, &I->h_hi, &I->h_fx, &I->h_fy }) if (b->p) (void)hipHostFree(b->p);
    for (int i = 0; i < 8; ++i) if (I->ev[i]) (void)hipEventDestroy(I->ev[i]);
    for (int i = 0; i < 8; ++i) if (I->ev_chunk[i]) (void)hipEventDestroy(I->ev_chunk[i]);
    if (I->ev_k0) (void)hipEventDestroy(I->ev_k0);
    if (I->ev_k1) (void)hipEventDestroy(I->ev_k1);
    if (I->ev_rects) (void)hipEventDestroy(I->ev_rects);
    if (I->ev_fork) (void)hipEventDestroy(I->ev_fork);
    if (I->ev_join) (void)hipEventDestroy(I->ev_join);
    if (I->aux) (void)hipStreamDestroy(I->aux);
    if (I->aux2) (void)hipStreamDestroy(I->aux2);
    if (I->stream) (void)hipStreamDestroy(I->stream);
    I->magic = 0;
    delete I;
}

void my_seamlessclone_api_imp_sync(void *p)
{
    Instance *I = get(p);
    if (!I) return;
    (void)hipSetDevice(I->gpu);
    (void)hipStreamSynchronize(I->stream);
}

int sc_hip_set_solver(void *p, const sc_solver_opts *o)
{
    Instance *I = get(p);
    if (!I || !o) return SC_ERR_BAD_ARG;
    if (o->method < SC_METHOD_JACOBI || o->method > SC_METHOD_FFT || o->max_sweeps < 0) {
        I->err = "bad solver options";
        return SC_ERR_BAD_ARG;
    }
    if (o->jacobi_tile_rows != 0 && o->jacobi_tile_rows != 16 && o->jacobi_tile_rows != 32 && o->jacobi_tile_rows != 64) {
        I->err = "jacobi_tile_rows must be 0, 16, 32 or 64";
        return SC_ERR_BAD_ARG;
    }
    if (o->mg_level1_sweeps != 0 && (o->mg_level1_sweeps < 2 || o->mg_level1_sweeps > 4)) {
        I->err = "mg_level1_sweeps must be 0 or 2..4";
        return SC_ERR_BAD_ARG;
    }
    if (((o->flags ^ I->opts.flags) & SC_FLAG_VCYCLE_BOTTOM) || legacy_path(*o, SC_LEGACY_BOTTOM_F32) != legacy_path(I->opts, SC_LEGACY_BOTTOM_F32) || o->mg_direct_max != I->opts.mg_direct_max) I->mg.clear();   // the hierarchy (which bottom level is solved directly) depends on these only
    if (o->mg_direct_max < 0) { I->err = "mg_direct_max must be >= 0"; return SC_ERR_BAD_ARG; }
    I->opts = *o;
    return SC_OK;
}

int sc_hip_set_clone_mode(void *p, int mode)
{
    Instance *I = get(p);
    if (!I) return SC_ERR_BAD_ARG;
    if (mode != SC_NORMAL_CLONE && mode != SC_MIXED_CLONE && mode != SC_MONOCHROME_TRANSFER) {
        I->err = "clone mode must be SC_NORMAL_CLONE, SC_MIXED_CLONE or SC_MONOCHROME_TRANSFER";
        return SC_ERR_BAD_ARG;
    }
    I->clone_mode = mode;
    return SC_OK;
}

int sc_hip_get_clone_mode(void *p)
{
    Instance *I = get(p);
    return I ? I->clone_mode : SC_ERR_BAD_ARG;
}

int sc_hip_get_solver(void *p, sc_solver_opts *o)
{
    Instance *I = get(p);
    if (!I || !o) return SC_ERR_BAD_ARG;
    *o = I->opts;
    return SC_OK;
}

int sc_hip_get_info(void *p, sc_run_info *info)
{
    Instance *I = get(p);
    if (!I || !info) return SC_ERR_BAD_ARG;
    I->info.device_bytes = I->arena_bytes;
    I->info.device = I->gpu;
    *info = I->info;
    return SC_OK;
}

const char *sc_hip_last_error(void *p)
{
    Instance *I = get(p);
    if (!I) return "bad instance";
    return I->err.c_str();
}

void *sc_hip_malloc(void *p, size_t bytes)
{
    Instance *I = get(p);
    if (!I) return nullptr;
    (void)hipSetDevice(I->gpu);
    void *d = nullptr;
    if (hipMalloc(&d, bytes) != hipSuccess) return nullptr;
    return d;
}

void sc_hip_free(void *p, void *d)
{
    Instance *I = get(p);
    if (!I || !d) return;
    (void)hipSetDevice(I->gpu);
    (void)hipStreamSynchronize(I->stream);
    (void)hipFree(d);
}

void *sc_hip_host_alloc(void *p, size_t bytes)
{
    Instance *I = get(p);
    if (!I || bytes == 0) return nullptr;
    (void)hipSetDevice(I->gpu);
    void *h = nullptr;
    if (hipHostMalloc(&h, bytes, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return h;
}

void sc_hip_host_free(void *p, void *h)
{
    Instance *I = get(p);
    if (!I || !h) return;
    (void)hipSetDevice(I->gpu);
    (void)hipStreamSynchronize(I->stream);
    (void)hipHostFree(h);
}

int sc_hip_memcpy_h2d(void *p, void *d, const void *h, size_t bytes)
{
    Instance *I = get(p);
    if (!I || !d || !h) return SC_ERR_BAD_ARG;
    SC_HIP(I, hipSetDevice(I->gpu));
    SC_HIP(I, hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, I->stream));
    SC_HIP(I, hipStreamSynchronize(I->stream));
    return SC_OK;
}

int sc_hip_memcpy_d2h(void *p, void *h, const void *d, size_t bytes)
{
    Instance *I = get(p);
    if (!I || !d || !h) return SC_ERR_BAD_ARG;
    SC_HIP(I, hipSetDevice(I->gpu));
    SC_HIP(I, hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, I->stream));
    SC_HIP(I, hipStreamSynchronize(I->stream));
    return SC_OK;
}

int sc_hip_memcpy_d2d_async(void *p, void *dst, const void *src, size_t bytes)
{
    Instance *I = get(p);
    if (!I || !dst || !src) return SC_ERR_BAD_ARG;
    SC_HIP(I, hipSetDevice(I->gpu));
    SC_HIP(I, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, I->stream));
    return SC_OK;
}

static void finish_timing(Instance *I, bool staged)
{
    // ev: 0 start | 1 mask on device | 2 bbox done | 3 ROI images on device | 4 erode done |
    //     5 pre-process done | 6 solve done | 7 post-process done ; ev_k1 = D2H done
    I->info.ms_h2d = staged ? ev_ms(I->tm[0], I->tm[1]) + ev_ms(I->tm[2], I->tm[3]) : 0.f;
    I->info.ms_mask = ev_ms(I->tm[1], I->tm[2]) + ev_ms(I->tm[3], I->tm[4]);
    I->info.ms_pre = ev_ms(I->tm[4], I->tm[5]);
    I->info.ms_solve = ev_ms(I->tm[5], I->tm[6]);
    I->info.ms_post = ev_ms(I->tm[6], I->tm[7]);
    I->info.ms_d2h = staged ? ev_ms(I->tm[7], I->ev_k1) : 0.f;
    I->info.ms_device_total = I->info.ms_mask + I->info.ms_pre + I->info.ms_solve + I->info.ms_post;
}

int my_seamlessclone_api_imp_run(void *p, const uint8_t *face, int fc, int fr, int fs, uint8_t *body, int bc, int br,
                                 int bs, const uint8_t *mask, int mc, int mr, int ms, int cx, int cy, int gpu_id,
                                 bool bSync)
{
    (void)gpu_id; // the instance already owns its device (the reference ignores it as well, seamlessClone_imp.cu:265)
    Instance *I;
    int rc = begin_call(p, I);
    if (rc) return rc;
    rc = validate_images(I, face, fc, fr, fs, body, bc, br, bs, mask, mc, mr, ms);
    if (rc) return rc;
    // --- the predicted box (the previous one for this mask size, else the mask's interior), if any
    int guess[4];
    Geo gp{};
    bool predicted = predict_rect(I, mc, mr, guess);
    if (predicted) {
        predicted = geo_from_rect(I, guess, cx, cy, gp) == SC_OK && check_roi(I, gp, bc, br) == SC_OK;
        I->err.clear();                               // a guess that does not fit the destination is not an error
    }
    // --- SMALL calls (the reference's own patches: 154 x 100 ... 592^2 into 1600 x 898): what the clone reads -- mask, patch ROI,
    //     destination ROI -- is packed row by row into ONE pinned block and crosses PCIe as ONE copy into one device block.  Three
    //     copies out of pageable memory cost 12-40 us EACH before a byte moves (the runtime stages them itself): h2d 0.037 / 0.050 /
    //     0.131 ms at 154 x 100 / 300 x 194 / 592^2 for 0.1 / 0.4 / 2.4 MB.  Needs the box before the first copy: predicted calls only.
    struct PreIn { const uint8_t *face = nullptr; uint8_t *body = nullptr; int pitch = 0; } pre;
    constexpr size_t SMALL_CALL_MAX = (size_t)1 << 20;      // (measured: 0.138 -> 0.117 ms per call at 154 x 100, 0.177 -> 0.166 at 300 x 194; at 592^2 -- 2.4 MB -- packing on the host loses: 0.415 -> 0.425)
    const uint8_t *dmask = nullptr;                   // the mask on the device, its row step
    int dms = 0;
    I->stage_marks = true;         // a host-image call is synchronous whatever bSync says: its timeline is always read
    I->marks_ends_only = (I->opts.flags & SC_FLAG_NO_STAGE_MARKS) != 0;      // (... unless the caller gives the per-stage figures up for their ~5 us bubbles)
    if (predicted && !I->opts.reference_warmup) {
        const int sdms = round_up(mc, 256), sdfs = round_up(3 * gp.W, 256);
        const size_t bm = (size_t)sdms * mr, bi = (size_t)sdfs * gp.H, total = bm + 2 * bi;
        if (total <= SMALL_CALL_MAX) {
            if ((rc = ensure(I, I->d_in, total + 64, false))) return rc;
            if ((rc = ensure_pinned(I, I->h_in, total))) return rc;
            if ((rc = tmark(I, 0))) return rc;
            uint8_t *const hs = (uint8_t *)I->h_in.p, *const ds = (uint8_t *)I->d_in.p;
            copy_rows(I, hs, (size_t)sdms, mask, (size_t)ms, (size_t)mc, mr);
            copy_rows(I, hs + bm, (size_t)sdfs, face + (size_t)gp.y0 * fs + 3 * (size_t)gp.x0, (size_t)fs, 3 * (size_t)gp.W, gp.H);
            copy_rows(I, hs + bm + bi, (size_t)sdfs, body + (size_t)gp.lty * bs + 3 * (size_t)gp.ltx, (size_t)bs, 3 * (size_t)gp.W, gp.H);
            {   // ... by a KERNEL that reads the pinned block across PCIe (k_copy_group: sixteen bytes per lane, four loads in flight): a copy
                // command takes ~20 us before its first byte moves, whatever its size (h2d stage at 154 x 100: 24 us for 0.1 MB)
                CopyJobs cj{};
                cj.dst[0] = ds; cj.src[0] = hs; cj.bytes[0] = total;
                launch_copy_group(cj, 1, I->stream);
                SC_HIP(I, hipGetLastError());
            }
            dmask = ds; dms = sdms;
            pre.face = ds + bm; pre.body = ds + bm + bi; pre.pitch = sdfs;
            if ((rc = tmark(I, 1))) return rc;
        }
    }
    if (!dmask) {
        // --- mask to the device
        const bool whole_m = 4 * (size_t)mc >= 3 * (size_t)ms;      // (not a narrow view of a much wider image): one linear copy at the caller's step
        dms = whole_m ? ms : round_up(mc, 256);
        if ((rc = ensure(I, I->d_mask, (size_t)dms * mr + 64, false))) return rc;
        if ((rc = tmark(I, 0))) return rc;
        if (whole_m) SC_HIP(I, hipMemcpyAsync(I->d_mask.p, mask, (size_t)ms * (mr - 1) + mc, hipMemcpyHostToDevice, I->stream));
        else if ((rc = upload_rows(I, I->h_mask, I->d_mask.p, dms, mask, ms, mc, mr))) return rc;
        dmask = (const uint8_t *)I->d_mask.p;
        if ((rc = tmark(I, 1))) return rc;
    }
    // One attempt on a given geometry: ROI of face/body to the device (the reference uploads both images whole),
    // clone, [check the predicted box], result back into the caller's image.  SC_GUESS_WRONG = the device found a
    // different box than `guess`; nothing has been written anywhere the caller can see.
    constexpr int SC_GUESS_WRONG = 1;
    auto attempt = [&](const Geo &g, const int *guess, const PreIn *in) -> int {      // in: the ROIs are on the device already (the small call's one copy)
        int r;
        const int dfs = round_up(3 * g.W, 256);
        // An image whose ROI covers most of its rows (>= 3/4 of the row step: the patch always, the destination often) crosses
        // PCIe as ONE linear copy of whole rows straight from the caller's memory at the caller's row step -- no packing pass,
        // no helper threads; the kernels take any origin and step.  Packing 29 MB with eight threads ran at 33-45 GB/s on the
        // boxes measured, under the link's 55; the direct copy: h2d 0.90 -> 0.67 ms of a 2048^2 call on the slower box.  A small
        // ROI of a large image is still packed (row by row into pinned staging, one DMA per piece).  The library still issues
        // no 2-D copies (appendix B).
        // ... or the rows' bytes outside the ROI are few in all (a small ROI of a larger image -- the reference's published table:
        // patches into a 1600 x 898 destination): the packed path has ~0.1 ms of fixed cost (helper threads, staging, the splice
        // behind the last DMA), 3 MB more on the link cost 0.055 (600^2 ROI of a 1600-wide image: 0.475 -> 0.36 ms per call)
        // -- but not more than twice the ROI's own bytes: a 300 x 194 patch of a 1600-wide image (0.76 MB around 0.17) is faster packed
        // (0.20 against 0.25 ms)
        constexpr size_t WHOLE_EXTRA_MAX = (size_t)3 << 20;
        auto few_extra = [&](int step) { const size_t extra = ((size_t)step - 3 * (size_t)g.W) * g.H; return extra <= WHOLE_EXTRA_MAX && extra <= 2 * 3 * (size_t)g.W * g.H; };
        const bool whole_f = !in && (4 * 3 * (size_t)g.W >= 3 * (size_t)fs || few_extra(fs));
        const bool whole_b = !in && (4 * 3 * (size_t)g.W >= 3 * (size_t)bs || few_extra(bs));
        const int fpitch = in ? in->pitch : whole_f ? fs : dfs, bpitch = in ? in->pitch : whole_b ? bs : dfs;
        const size_t foff = whole_f ? 3 * (size_t)g.x0 : 0, boff = whole_b ? 3 * (size_t)g.ltx : 0;
        if ((r = ensure(I, I->d_out, (size_t)dfs * g.H + 64, false))) return r;
        if (!in) {
            if ((r = ensure(I, I->d_face, (size_t)fpitch * g.H + 64, false))) return r;
            if ((r = ensure(I, I->d_body_roi, (size_t)bpitch * g.H + 64, false))) return r;
            if (whole_f) SC_HIP(I, hipMemcpyAsync(I->d_face.p, face + (size_t)g.y0 * fs, (size_t)fs * (g.H - 1) + foff + 3 * (size_t)g.W, hipMemcpyHostToDevice, I->stream));
            else if ((r = upload_rows(I, I->h_face, I->d_face.p, dfs, face + (size_t)g.y0 * fs + 3 * g.x0, fs, 3 * (size_t)g.W, g.H))) return r;
            if (whole_b) SC_HIP(I, hipMemcpyAsync(I->d_body_roi.p, body + (size_t)g.lty * bs, (size_t)bs * (g.H - 1) + boff + 3 * (size_t)g.W, hipMemcpyHostToDevice, I->stream));
            else if ((r = upload_rows(I, I->h_body, I->d_body_roi.p, dfs, body + (size_t)g.lty * bs + 3 * g.ltx, bs, 3 * (size_t)g.W, g.H))) return r;
        }
        const uint8_t *const d_face_roi = in ? in->face : (const uint8_t *)I->d_face.p + foff;
        uint8_t *const d_body_roi = in ? in->body : (uint8_t *)I->d_body_roi.p + boff;
        if ((r = tmark(I, 3))) return r;
        const int passes = I->opts.reference_warmup ? 2 : 1;
        // the output bytes go to a compact buffer of their own (the interior only is written, and only that comes back); the
        // reference's warm-up pass (two applications in place) needs the first result where the second reads it: the body buffer
        // SC_FLAG_ROWS_RETURN (opt-in since round 5): a destination uploaded as whole rows takes the output bytes in place as well and the
        // rows come back as ONE linear copy straight into the caller's image -- no pinned staging, no splice on the host behind the
        // last DMA.  What it overwrites outside the ROI's columns are the caller's own bytes, uploaded a moment ago: harmless only
        // while nobody else writes those pixels during the call, which the library cannot know (two calls cloning into disjoint ROIs
        // of one image would lose each other's result) -- so the default writes ROI bytes only, as the reference does
        // (seamlessClone_imp.cpp:470-483).
        const bool inplace = whole_b && passes == 1 && (size_t)bs == 3 * (size_t)bc && (I->opts.flags & SC_FLAG_ROWS_RETURN);      // (a view into a wider array keeps the staged path: nothing beyond the view's own pixels is ever written)
        constexpr size_t DIRECT_OUT_MAX = (size_t)2 << 20;
        // a SMALL output: the output launch writes the ROI's bytes straight into the pinned staging (three words per lane, coalesced: posted
        // writes across PCIe) -- no device-to-host copy command (~10 us before its first byte moves) behind the last kernel
        const bool direct_out = passes == 1 && !inplace && (size_t)dfs * g.H <= DIRECT_OUT_MAX;
        if (direct_out && (r = ensure_pinned(I, I->h_out, (size_t)dfs * g.H + 64))) return r;
        uint8_t *const out_dev = (passes > 1 || inplace) ? d_body_roi : direct_out ? (uint8_t *)I->h_out.p : (uint8_t *)I->d_out.p;
        const int out_pitch = (passes > 1 || inplace) ? bpitch : dfs;
        r = device_clone(I, dmask, dms, mr, d_face_roi, fpitch, d_body_roi, bpitch, g, passes, out_dev, out_pitch, direct_out);
        if (r != SC_OK && r != SC_ERR_NOT_CONVERGED) return r;
        // direct_out: nothing is enqueued behind the clone -- ONE wait for the stream, then the rectangle is compared, then the rows are
        // spliced (a wrong guess: the guarded output launch wrote nothing, the staging holds nothing the caller will see)
        const bool check_after_sync = guess && direct_out;
        if (guess && !check_after_sync) {      // the scan rode in the pre-process launch and finished long ago: this wait on the event behind that launch is free
            if (I->scan_fence) SC_HIP(I, hipEventSynchronize(I->scan_fence));
            else SC_HIP(I, hipStreamSynchronize(I->stream));      // (cannot happen: a clone launched on a guess always carries its scan)
            I->scan_fence = nullptr;
            if (memcmp(guess, I->h_rect + 4, 4 * sizeof(int)) != 0) return SC_GUESS_WRONG;
        }
        // Interior back into the caller's image: linear D2H pieces of the compact ROI buffer into pinned staging
        // (a 2-D copy would be one DMA per row), each spliced into the image row by row while the next one is
        // still crossing PCIe.  The call completes before returning whatever bSync says: the result has to be in
        // caller memory (the reference is effectively synchronous too: its D2H + host splice, imp.cpp:471).
        const int orows = g.H - 2;
        const size_t ob = 3 * (size_t)(g.W - 2);
        if (orows > 0 && g.W > 2 && inplace) {
            SC_HIP(I, hipMemcpyAsync(body + (size_t)(g.lty + 1) * bs + 3 * (size_t)(g.ltx + 1), out_dev + (size_t)out_pitch + 3,
                                     (size_t)bs * (orows - 1) + ob, hipMemcpyDeviceToHost, I->stream));
            SC_HIP(I, hipEventRecord(I->ev_k1, I->stream));
        } else if (orows > 0 && g.W > 2 && direct_out) {
            SC_HIP(I, hipEventRecord(I->ev_k1, I->stream));
            SC_HIP(I, hipStreamSynchronize(I->stream));              // the kernel's stores are in host memory when it has ended
            if (check_after_sync) {
                I->scan_fence = nullptr;
                if (memcmp(guess, I->h_rect + 4, 4 * sizeof(int)) != 0) return SC_GUESS_WRONG;
            }
            copy_rows(I, body + (size_t)(g.lty + 1) * bs + 3 * (g.ltx + 1), (size_t)bs, (const uint8_t *)I->h_out.p + dfs + 3, (size_t)dfs, ob, orows);
        } else if (orows > 0 && g.W > 2) {
            const int dfs = out_pitch;            // (shadows the compact pitch: the warm-up variant returns at the body buffer's)
            if ((r = ensure_pinned(I, I->h_out, (size_t)dfs * g.H + 64))) return r;
            uint8_t *dst_org = body + (size_t)(g.lty + 1) * bs + 3 * (g.ltx + 1);
            const uint8_t *src = out_dev + dfs;                                   // ROI row 1
            uint8_t *stage = (uint8_t *)I->h_out.p + dfs;
            // pieces that SHRINK towards the end: the splice of piece k runs while piece k + 1 crosses the link, and what is left
            // after the last DMA is the splice of a small piece only (equal pieces left 1/3 of the image to splice behind the link)
            int starts[9], pieces = 0;
            {
                const size_t total = (size_t)dfs * orows;
                size_t left = total;
                int yy = 0;
                while (yy < orows && pieces < 7) {
                    size_t want = left > ((size_t)3 << 20) ? left / 2 : left;          // halves, down to ~1.5-3 MB
                    int n = (int)std::max<size_t>(1, want / dfs);
                    if (orows - yy - n < 8) n = orows - yy;
                    starts[pieces++] = yy;
                    yy += n; left = (size_t)dfs * (orows - yy);
                }
                if (yy < orows) starts[pieces++] = yy;
                starts[pieces] = orows;
            }
            for (int k = 0; k < pieces; ++k) {
                const int y0 = starts[k], n = starts[k + 1] - y0;
                SC_HIP(I, hipMemcpyAsync(stage + (size_t)y0 * dfs, src + (size_t)y0 * dfs, (size_t)dfs * (n - 1) + 3 + ob,
                                         hipMemcpyDeviceToHost, I->stream));
                SC_HIP(I, hipEventRecord(I->ev_chunk[k], I->stream));
            }
            SC_HIP(I, hipEventRecord(I->ev_k1, I->stream));
            for (int k = 0; k < pieces; ++k) {
                const int y0 = starts[k], n = starts[k + 1] - y0;
                SC_HIP(I, hipEventSynchronize(I->ev_chunk[k]));
                copy_rows(I, dst_org + (size_t)y0 * bs, (size_t)bs, stage + (size_t)y0 * dfs + 3, (size_t)dfs, ob, n);
            }
        } else {
            SC_HIP(I, hipEventRecord(I->ev_k1, I->stream));
        }
        SC_HIP(I, hipStreamSynchronize(I->stream));
        if (check_after_sync && I->scan_fence) {      // (an ROI without interior rows: nothing was spliced above)
            I->scan_fence = nullptr;
            if (memcmp(guess, I->h_rect + 4, 4 * sizeof(int)) != 0) return SC_GUESS_WRONG;
        }
        return r;
    };
    Geo g{};
    bool done = false;
    I->guard = RectGuard();
    if (predicted) {
        // launch on the predicted box; the bbox kernel's answer is checked before anything reaches the caller
        if ((rc = bbox_enqueue(I, dmask, mc, mr, dms, &gp))) return rc;
        I->guard = make_guard(I, guess);
        rc = attempt(gp, guess, pre.face ? &pre : nullptr);
        I->guard = RectGuard();
        if (rc == SC_GUESS_WRONG) {               // repeat on the true box (the mask stays where it is, the ROIs go up the ordinary way), pause speculation for a while
            I->spec_cooldown = 8;
            if ((rc = geo_from_rect(I, I->h_rect + 4, cx, cy, g))) return rc;
            fill_info_geo(I, g);
            if ((rc = check_roi(I, g, bc, br))) return rc;
            rc = attempt(g, nullptr, nullptr);
        } else {
            g = gp;
        }
        if (rc != SC_OK && rc != SC_ERR_NOT_CONVERGED) return rc;
        done = true;
    }
    if (!done) {                                      // no usable prediction: wait for the device's box first
        if ((rc = device_bbox(I, dmask, mc, mr, dms, cx, cy, g))) return rc;
        fill_info_geo(I, g);
        if ((rc = check_roi(I, g, bc, br))) return rc;
        rc = attempt(g, nullptr, nullptr);
        if (rc != SC_OK && rc != SC_ERR_NOT_CONVERGED) return rc;
    }
    fill_info_geo(I, g);
    remember_rect(I, mc, mr, I->h_rect + 4);
    finish_timing(I, true);
    I->info.ms_call = ev_ms(I->tm[0], I->ev_k1);
    if (bSync) {      // the reference's bSync: time the call on the stream and say so (seamlessClone_imp.cu:336-349)
        printf("Compute stage performance time= %.3f msec, patch size=%dx%d\n", I->info.ms_call, g.W, g.H);      // the reference's ucMask has the ROI's size by then (seamlessClone_imp.cpp:1024)
        printf("total device memory used: %zu\n", I->arena_bytes);
        fflush(stdout);
    }
    return rc;
}

int sc_hip_run_device(void *p, const uint8_t *d_face, int fc, int fr, int fs, uint8_t *d_body, int bc, int br, int bs,
                      const uint8_t *d_mask, int mc, int mr, int ms, int cx, int cy, bool bSync)
{
    Instance *I;
    int rc = begin_call(p, I);
    if (rc) return rc;
    rc = validate_images(I, d_face, fc, fr, fs, d_body, bc, br, bs, d_mask, mc, mr, ms);
    if (rc) return rc;
    I->stage_marks = bSync;        // the stage timeline (sc_run_info::ms_*) is filled for synchronous calls only, like the
                                   // reference's bSync timing: each mark is an event in the stream and a ~5 us bubble behind it
    I->marks_ends_only = bSync && (I->opts.flags & SC_FLAG_NO_STAGE_MARKS);
    if ((rc = tmark(I, 0))) return rc;
    if ((rc = tmark(I, 1, true))) return rc;       // nothing to upload: images are device resident
    const int passes = I->opts.reference_warmup ? 2 : 1;
    auto attempt = [&](const Geo &g) -> int {
        int r = tmark(I, 3, true);
        if (r) return r;
        r = device_clone(I, d_mask, ms, mr, roi_at(d_face, fs, g.x0, g.y0), fs, roi_at(d_body, bs, g.ltx, g.lty), bs, g, passes);
        if (r != SC_OK && r != SC_ERR_NOT_CONVERGED) return r;
        SC_HIP(I, hipEventRecord(I->ev_k1, I->stream));
        return r;
    };
    Geo g{};
    bool done = false;
    int guess[4];
    I->guard = RectGuard();
    // a predicted box needs the final wait to be checked against the device's answer: synchronous calls only
    if (bSync && predict_rect(I, mc, mr, guess)) {
        Geo gp{};
        if (geo_from_rect(I, guess, cx, cy, gp) == SC_OK && check_roi(I, gp, bc, br) == SC_OK) {
            if ((rc = bbox_enqueue(I, d_mask, mc, mr, ms, &gp))) return rc;
            I->guard = make_guard(I, guess);
            rc = attempt(gp);
            I->guard = RectGuard();
            if (rc != SC_OK && rc != SC_ERR_NOT_CONVERGED) return rc;
            SC_HIP(I, hipStreamSynchronize(I->stream));
            if (memcmp(guess, I->h_rect + 4, sizeof(guess)) == 0) {
                g = gp;
            } else {                                  // wrong guess: the destination was not touched
                I->spec_cooldown = 8;
                if ((rc = geo_from_rect(I, I->h_rect + 4, cx, cy, g))) return rc;
                fill_info_geo(I, g);
                if ((rc = check_roi(I, g, bc, br))) return rc;
                rc = attempt(g);
                if (rc != SC_OK && rc != SC_ERR_NOT_CONVERGED) return rc;
                SC_HIP(I, hipStreamSynchronize(I->stream));
            }
            done = true;
        }
        I->err.clear();
    }
    if (!done) {
        if ((rc = device_bbox(I, d_mask, mc, mr, ms, cx, cy, g))) return rc;
        fill_info_geo(I, g);
        if ((rc = check_roi(I, g, bc, br))) return rc;
        rc = attempt(g);
        if (rc != SC_OK && rc != SC_ERR_NOT_CONVERGED) return rc;
        if (bSync) SC_HIP(I, hipStreamSynchronize(I->stream));
    }
    fill_info_geo(I, g);
    remember_rect(I, mc, mr, I->h_rect + 4);
    if (bSync) finish_timing(I, false);
    else I->info.ms_h2d = I->info.ms_mask = I->info.ms_pre = I->info.ms_solve = I->info.ms_post = I->info.ms_d2h = I->info.ms_device_total = 0.f;
    return rc;
}

} // extern "C"
