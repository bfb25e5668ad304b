// sc_instance.h -- the per-GPU instance behind the C ABI: one HIP stream, a grow-only device
// arena (the role SCImage plays in the reference, seamlessClone_imp.h:90-457: capacity only
// ever grows, steady state does no hipMalloc), pinned mailboxes for the two small read-backs
// (bounding box, residual norm) and hipEvents for per-stage timing.
#pragma once
#include "sc_common.h"
#include "sc_hostcopy.h"
#include <algorithm>
#include <memory>
#include <cmath>

namespace sc {

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    bool own = true;       // false: a piece of one of the instance's slabs (Instance::slabs) -- not a hipMalloc block of its own, never hipFree'd
};
// releases a device buffer on instance teardown: its own hipMalloc block, or nothing for a piece of a slab
inline void dev_release(DevBuf &b) { if (b.p && b.own) (void)hipFree(b.p); b.p = nullptr; b.cap = 0; }

// eigen-decomposition of one 1-D level operator (sc_fd_selftest.cpp: the host reference of the fast-diagonalisation bottom solve)
struct FD1 {
    int n = 0;
    float cw_last = 0.f, d_last = 0.f;     // together with n: the key
    std::vector<double> lam, q, ee;          // eigenvalues; q[k*n + i] = component i of eigenvector k; diagonal of E
};

// float-table correction (sc_lowmode.hip): sine tables and coefficient buffers for the current ROI size
struct LowMode {
    int w = 0, h = 0, C = 0;               // interior size the tables were built for; channels the buffers hold
    int Kx = 0, Ky = 0, Kxp = 0, Kyp = 0;  // modes per direction, padded to the register block
    int nx = 0, ny = 0, npitch = 0;        // nodes (every 8th field column / row) and the row pitch of CN
    bool singular = false;                 // the reference's float denominator of the lowest mode is zero at this size: no correction
    double max_ratio = 0.0;                // max |den_exact / den_float - 1| over the corrected modes
    DevBuf B;                              // cell-share parts left by a level-0 launch [C][band rows][cells_x][2] float4
    struct PartMap { DevBuf d, h; int H = 0, sweeps = 0; } maps[2];      // parts of each cell row (device, pinned) for the 2- and the 4-sweep tiling
    PartMap *map_used = nullptr;
    int rag_tiling = 0;                    // a size class: which of the members' two maps the last bands buffer belongs to (0: 2 sweeps, 1: 4)
    int band_rows = 0;
    const float *bands_of = nullptr;       // the field whose parts B holds (nullptr: none); cleared whenever a solve starts or moves on
    DevBuf Sx, Sy, R, P, E, CN;            // Sx[nx][Kxp], Sy[ny][Kyp] (sines at the nodes), R[Kyp][Kxp] -- views of the current entry of `tables` --, P = cell shares float4[C][cells_y][cells_x], E = partial products of the coarse projection [parts][C][Kyp][Kxp], CN[C][ny][npitch]
    // the per-size tables, kept in a small LRU (a caller alternating between a few ROI sizes rebuilds nothing): Sx, Sy built on
    // the device, R on the host into the entry's own pinned staging (no stream synchronisation; the upload event is waited for
    // only when the entry is reused for another size)
    struct Tables { int w = 0, h = 0; bool singular = false; double max_ratio = 0.0; DevBuf Sx, Sy, R, hR; hipEvent_t ev = nullptr; unsigned long long used = 0; };
    enum { TABLES = 4 };
    Tables tables[TABLES];
    unsigned long long tick = 0;
};

// direct DST solve (sc_dst.hip): DST matrices, the reference's float tables and the double work planes
struct DstState {
    int w = 0, h = 0, wp = 0, hp = 0;      // interior size the tables were built for, padded to the 128 x 128 tiles
    bool singular = false;                 // the reference's float tables are singular at this size: exact denominators instead
    DevBuf Sw, Sh, fxy, G, T1, T2;         // Sw[wp][wp], Sh[hp][hp] double; fx[wp] + fy[hp] float; G, T1, T2: [C][hp][wp] double
    DevBuf hfxy;                           // pinned staging of the float tables
};

// FFT direct solve (sc_fft.hip): per-direction chirp / transform tables and the two work planes.  The tables of a transform
// length are built ON THE DEVICE (k_fft_build: both directions of a solve in one launch) and kept in a small LRU: a caller whose mask changes with every
// frame meets new ROI sizes all the time, and alternating between a few sizes costs nothing.
struct FftDim { int n = 0, logM = 0, r = 1; bool dbl = false; int kind = 0; DevBuf chirp; unsigned long long used = 0; };   // M = r 2^logM (r = 1, 3, 5); kind 0 (DST-I, chirp of period 2(n+1)): chirp[n+1] | bhat[M] | tw[M] | tw2[2^logM] (complex float or double); kind 1 (DCT-II / III, period 2n): chirp[n+1] | half-sample twiddle[n+1] | bhat | tw | tw2; kinds 2 (one Dirichlet end, period 2n+1) and 4 (periodic, Hartley, period n): two tables of n+1 in those places
struct FftFxy { int w = 0, h = 0; bool singular = false; DevBuf d, hst; hipEvent_t ev = nullptr; unsigned long long used = 0; };   // the reference's float tables fx[w] + fy[h]: device, pinned staging of its own, upload event
struct FftState {
    enum { DIMS = 8, FXY = 4 };
    FftDim dims[DIMS];
    FftFxy fxy[FXY];
    unsigned long long tick = 0;
    DevBuf A, B;                           // work planes [C][h][w]
    DevBuf hst_all;                        // pinned staging of all FXY eigenvalue-table entries (one block; FftFxy::hst is unused since round 5)
    DevBuf mean;                           // the Neumann solve's partial sums of boundary, double [planes][parts] (direct_jobs_solve)
    DevBuf tw64;                           // double twiddles of the build's own transform (float tables are built through a double FFT)
    hipEvent_t ev_fork = nullptr, ev_built = nullptr;   // the build runs on the instance's second stream
    bool pending = false;                  // ... and `stream` has not waited for ev_built yet
    FftDim *req[2] = { nullptr, nullptr }; // tables queued for a build by the current solve (its two directions), launched together
    int nreq = 0;
    bool forked = false;                   // this solve has already put the second stream behind the main one (one fork per solve: both directions' tables and the eigenvalue tables ride on it)
};

struct PcgState;      // the conjugate-gradient families' work planes and mailbox (sc_pcg.h)

struct MGLevel {
    Field U, F, T;   // correction, RHS, scratch (residual field); level 0 aliases the instance fields
    MGGeom g;        // geometry of this level and of its transfer to the next coarser one
    float omega = 1.f; // SOR factor used when this is the coarsest level
};

// ---- size classes (sc_ragged.cpp; RagMember in sc_common.h) -------------------------------------------------------------------
// What one ROI size needs in order to share a set of launches with OTHER sizes: host arithmetic only.
struct SizePlan {
    int W = 0, H = 0;
    bool ok = false;                    // the default fast path serves this size inside a class (else: same-size groups, or alone)
    bool conditional = false;           // the float-table correction's a-priori bound does not hold at this size (plan_size): classes of such members only
    bool solo_differs = false;          // ... on another hierarchy than its solo run's (small ROIs whose level 1 a solo clone solves directly): within one grey level of it, not the same bytes
    int nl = 0, tail = 0;               // levels of its hierarchy; the level k_mg_tail holds (the one below it is solved directly)
    int npx = 0, npy = 0;               // padding of the directly solved level's operands (32 or 64 per side)
    int Kx = 0, Ky = 0, Kxp = 0, Kyp = 0, nx = 0, ny = 0, cells_y = 0, nxt = 0, nrs = 0;     // float-table correction
    double max_ratio = 0.0;
    // the heavy part, shared between copies (plans are memoised per size: sc_ragged.cpp): level geometries, the correction's ratio
    // table R[Kyp][Kxp] and the part maps of the 2- and the 4-sweep tiling
    struct Tables { std::vector<MGGeom> g; };
    std::shared_ptr<const Tables> t;
    // (what only the per-call setup needs -- the correction's ratio table, its part maps -- is computed into the staging by every call: rag_begin_table)
    // same compile-time choices and launch shapes (the spread of a group's sizes is plan_groups' business)
    bool same_class(const SizePlan &o) const
    {
        // (levels below the directly solved one are never visited: their number is free; operand paddings are per member:
        //  k_mg_tail_any; the correction's mode-block padding is the class's largest: a member's extra blocks are exact zeros)
        return ok && o.ok && tail == o.tail && conditional == o.conditional;
    }
};
bool plan_size(const sc_solver_opts &o, int W, int H, SizePlan &p);     // fills p; returns p.ok
// members (any order) -> groups that can each share one set of launches: a size class (two or more DIFFERENT sizes), a same-size
// group, or a single; `cap` = most members per group.  groups[k] lists indices into `plans`.
void plan_cache_clear();                                         // forgets every memoised plan and table (tests, measurements)
void pool_group_caps(int group, int n, int streams, int &cap, int &cap_max, long &budget_px);      // the pool's group policy (group 0: automatic)
void plan_groups(std::vector<SizePlan> &plans, int cap, std::vector<std::vector<int>> &groups, int cap_max = 0, long budget_px = 0);      // (may rewrite a member's plan: sc_ragged.cpp)

struct RagState {
    const RagMember *dev = nullptr;     // the members' table on the device WHILE a size class is being processed, else nullptr
    std::vector<RagMember> host;        // the same table (device pointers filled in)
    int n = 0;
    int nl = 0, tail = 0, npx = 0, npy = 0, Kxp = 0, Kyp = 0;     // the class's constants
    int max_nx = 0, max_ny = 0, max_nxt = 0, max_nrs = 0, max_cells_y = 0;
    double max_ratio = 0.0;
    DevBuf d_aux, h_stage;              // RagMember[n], R tables, part maps | Sx, Sy, bottom operands; pinned staging of what the host writes (the head of d_aux)
    bool pad_uniform = false;           // every member's operand padding of the directly solved level is the class's (k_mg_tail<SKX, SKY, true> instead of k_mg_tail_any)
    bool levels_built = false;          // the class's hierarchy is in I->mg (mg_build_levels_rag, called from rag_begin_builds)
    hipEvent_t ev = nullptr;            // behind the upload out of h_stage
    hipEvent_t ev_ready = nullptr;      // second stream: the level planes are zeroed and the correction's tables built (the matrices follow: Instance::ev_fd)
    bool ready_pending = false;         // ... and the main stream has not waited for that yet
};

// Where a solve's output bytes go (solve_step, write_output): one destination, or one per member of a group.  Neither: the solver
// writes no output bytes (the Poisson call writes its own).
struct SolveTarget {
    uint8_t *org = nullptr; int step = 0;            // one destination: ROI origin and row step (the post-process checks Instance::guard)
    const std::vector<ImageJob> *group = nullptr;    // one destination per member (channels 3i..3i+2) of a group
    bool writes() const { return org || group; }
};

struct Instance {
    uint32_t magic = 0x5C10E001u;
    int gpu = 0;
    hipStream_t stream = nullptr;
    // second stream of the instance: the float-table node correction of the next-to-last iterate (three latency-bound launches)
    // runs here beside the coarse levels of the last cycle; forked and joined with events, see mg_solve
    hipStream_t aux = nullptr;
    hipStream_t aux2 = nullptr;            // a size class's matrix build (rag_begin_builds), beside aux's zeroing and tables; created on first use
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    bool aux_pending = false;              // work on aux that `stream` has not waited for yet
    sc_solver_opts opts{};
    int clone_mode = SC_NORMAL_CLONE;      // sc_hip_set_clone_mode; apart from opts: sc_hip_set_solver does not touch it
    bool edit_call = false;                // an edit (sc_edit_api.cpp) is solving: its right-hand side is float (mg_reads_half_rhs)
    sc_run_info info{};
    std::string err;

    // staging copies for host-pointer runs
    DevBuf d_in, h_in;                             // a SMALL host-image call: mask | patch ROI | destination ROI packed in one pinned block, one copy, one device block
    DevBuf d_face, d_body_roi, d_mask, d_out;      // d_out: the host path's compact output buffer (ROI bytes that go back across PCIe)
    // page-locked host staging (grow-only): pageable caller images are packed here row by row so
    // each image crosses PCIe as ONE DMA instead of one slow pageable 2-D copy
    DevBuf h_face, h_body, h_mask, h_out;
    DevBuf h_sx, h_sy;                             // a WLS host call's two link arrays (float_stage)
    DevBuf h_state;                                // a region host call's state array (float_stage)
    DevBuf h_gt, h_smt;                            // a volume host call's temporal guidance and temporal link weights (float_stage)
    DevBuf h_lo, h_hi;                             // a bounded host call's bound arrays (float_stage)
    DevBuf h_fx, h_fy;                             // a flow volume host call's two flow arrays (sc_hip_volume_flow)
    std::unique_ptr<RowCopier> copier;   // helper threads for the packing / splicing copies (created on first use)
    hipEvent_t ev_chunk[8]{};            // D2H chunk completions (host path): splice chunk k while k+1 is in flight
    // ROI mask after 3x erode
    DevBuf d_M;
    int mpitch = 0;
    // edits (sc_edit_api.cpp): Canny's class map (pitch mpitch), the hysteresis mailbox (pinned), the last edit's hysteresis counts
    DevBuf d_edge, h_hyst;
    int hyst_launches = 0, hyst_reads = 0;
    // the Poisson solve on caller arrays (sc_poisson_api.cpp): the host call's device copies of the arrays' spans
    DevBuf d_pois;
    bool auto_as_single = false;           // ... one problem of up to 4 channels: SC_METHOD_AUTO decides as for a single clone (effective_method)
    float screen_lambda = 0.f;             // a screened call (sc_screened_api.cpp) is solving: fft_solve divides by eigenvalue - lambda
    // fields
    DevBuf d_U0, d_U1, d_F;
    Field U0, U1, F;      // current views into the buffers above
    bool result_in_U1 = false;
    int bytes_writer = 0;                  // sc_hip_bytes_writer (which clears it): judged bytes left bit 0 planar + a splice launch, bit 1 interleaved from the judged launch
    bool out_direct = false;               // the last solve wrote output bytes from its last cycle: result(I) is the iterate before it, not the solution
    bool f_half = false;      // F currently holds float16 values (written by the pre-process for the fused multigrid path)
    bool u_half = false;      // ... and so does the initial field U0 until the first cycle has consumed it
    // ... unless u0_bytes: a same-size group whose pre-process stores no U0 at all -- the first level-0 launch reads the members' destination
    // bytes itself (k_cycle0 with C0_IN3).  Decided once per attempt by solve_prepare, before the pre-process is enqueued.
    bool u0_bytes = false;
    int u0_reader = 0;        // sc_hip_u0_reader (which clears it): the first launches read bit 0 float16 planes, bit 1 destination bytes, bit 2 planes a safety-net launch filled
    bool u_q16 = false;       // multigrid fast path, during a solve: the current field is 16-bit fixed point (sc_cycle0.hip, C0_Q16_IN / C0_Q16_OUT)
    bool mg_q16_last = false; // ... the last solve kept its field so (sc_hip_time_cycle0 times the same form)
    // 16-bit stores check their range: `sat` is the current solve's report word + generation (sc_common.h AbortFlag; p == nullptr:
    // the solve stores no 16-bit field); a solve whose word was set returns SC_RETRY_FLOAT_FIELD and solve_step repeats the
    // pre-process and the solve with force_float_field set
    AbortFlag sat;
    unsigned sat_counter = 0;
    bool force_float_field = false;
    // Speculative epilogue: the multigrid driver enqueues the post-process right behind the cycle whose
    // convergence check it is about to wait for, so the host round trip of the check overlaps useful work.
    // If the check then fails the solve simply continues and the post-process runs again at the end.
    // Armed by solve_step for the solve of a target that takes output bytes; done: the solver wrote them.
    struct SpecPost { SolveTarget to; bool armed = false, done = false; } spec_post;
    // Speculative geometry: a clone may be launched on a predicted bounding box (the previous one for the same
    // mask size, else the whole mask interior) while the bbox kernel's answer is still in flight; `guard` makes
    // the post-process a no-op on a wrong guess and the host then repeats the clone (sc_api.cpp, sc_batch.cpp).
    RectGuard guard;
    int last_mc = -1, last_mr = -1, last_rect[4] = { 0, 0, 0, 0 };
    int spec_cooldown = 0;
    bool erode_done = false;   // the ROI device_clone is about to process has been eroded already (a clone launched on a predicted box)
    BboxTask pending_scan;     // ... and its bounding-box scan has not gone out yet: it rides in the pre-process launch
    bool scan_pending = false;
    bool scan_counter_dirty = false;   // a call failed with a HIP error: zero the scan's arrival counter before the next scan (hip_fail)
    // completion fence of a scan that rode in a pre-process launch: an event recorded right behind that launch, whatever the
    // stage marks do (a stage mark is not a fence: SC_FLAG_NO_STAGE_MARKS records none there); nullptr: no scan went out
    hipEvent_t ev_scan = nullptr, scan_fence = nullptr;
    bool bench_tag = false;   // sc_hip_field_time_sweeps: launch the second-symbol instantiations
    // multigrid hierarchy (level 0 aliases U0/U1/F)
    std::vector<DevBuf> mg_bufs;
    DevBuf mg_partial;    // per-block maxima of the level-0 correction
    DevBuf h_partial;     // pinned copy of the same (small grids are folded on the host: no reduction launch)
    std::vector<MGLevel> mg;
    size_t mg_bottom = 0;  // first level run by the fused bottom kernel (== mg.size(): none)
    bool mg_l1_half = false;   // level 1's planes currently hold float16 values (sc_multigrid.cpp: mg_level1_half; re-zeroed when the mode flips)
    // direct (fast-diagonalisation) solve inside the bottom kernel: level index relative to mg_bottom, or -1
    int fd_level = -1, fd_nxp = 0, fd_nyp = 0;
    DevBuf mg_fd;          // its matrices (built on the device, k_fd_build)
    bool fd_mm = false;    // ... the matrix-core form serves it (k_mg_bottom_mm): operands at float offset fd_mm_off, padded to fd_npx x fd_npy
    int fd_npx = 0, fd_npy = 0;
    size_t fd_mm_off = 0;
    hipEvent_t ev_fd_fork = nullptr, ev_fd = nullptr;   // the build runs on `aux`: started behind ev_fd_fork, finished at ev_fd
    bool fd_pending = false;                            // ... and `stream` has not waited for ev_fd yet
    LowMode lm;
    RagState rag;
    DstState dst;
    FftState fft;
    PcgState *pcg = nullptr;     // made with the instance (sc_api.cpp: creation fails without it), freed by pcg_release: never null in a call
    bool fft_lds_float = false, fft_lds_double = false;   // this instance's device has the FFT kernels opted in to > 64 KB of LDS (sc_fft.hip)
    // reductions / mailboxes
    DevBuf d_rects, h_rects;     // bounding boxes of a group of clones (sc_hip_run_device_batch): device, pinned
    DevBuf d_bbox_parts;         // per-workgroup extrema of the group's scans (folded by a second launch instead of atomics)
    hipEvent_t ev_rects = nullptr;   // behind the read-back of a group's bounding boxes
    int group_spec_cooldown = 0;     // calls left without a predicted bounding box after a wrong guess in a group
    int *d_rect = nullptr;
    int *h_rect = nullptr;       // pinned
    double *d_partials = nullptr;
    double *d_red = nullptr;
    double *h_red = nullptr;     // pinned
    unsigned *d_maxcorr = nullptr;     // max correction of the last cycle and of the one before (bits of a float), the solve's saturation word (four words allocated)
    unsigned *h_maxcorr = nullptr;     // pinned, the same
    hipEvent_t ev[8]{};
    bool stage_marks = true;   // record the stage marks (synchronous calls); tmark() in sc_api.cpp
    bool marks_ends_only = false;   // ... but only the first and the last one (SC_FLAG_NO_STAGE_MARKS)
    hipEvent_t tm[8]{};   // stage marks of the current run: ev[k], or the previous mark where a stage is empty (no record call)
    hipEvent_t ev_k0 = nullptr, ev_k1 = nullptr;
    size_t arena_bytes = 0;
    std::vector<DevBuf> retired;           // device blocks that growth replaced: freed when the instance goes, or once they add up to 1 GB (ensure, sc_arena.cpp)
    size_t retired_bytes = 0;
    // Small device buffers are pieces of a few SLABS (16 MB, then doubling) instead of hipMalloc blocks of their own: an instance owns
    // ~40 grow-only buffers, and a caller whose ROI sizes wander re-sizes several of them in one call -- each a hipMalloc of 30-100 us
    struct Slab { uint8_t *base = nullptr; size_t cap = 0, used = 0; };
    std::vector<Slab> slabs;

    bool ok() const { return magic == 0x5C10E001u; }
};

// The per-call solve state a driver may set, put back on every way out of it: a call finds no edit, no forced float fields, the
// splice disarmed and SC_METHOD_AUTO deciding by channel count, whatever the call before it returned from.
struct CallScope {
    Instance *I;
    ~CallScope()
    {
        I->edit_call = false;
        I->force_float_field = false;
        I->spec_post = Instance::SpecPost();
        I->auto_as_single = false;
        I->screen_lambda = 0.f;
    }
};

// a superseded launch form asked for (SC_FLAG_LEGACY_PATHS + sc_solver_opts.legacy_paths)
inline bool legacy_path(const sc_solver_opts &o, int which) { return (o.flags & SC_FLAG_LEGACY_PATHS) && (o.legacy_paths & which); }
// The judged bytes launch of a same-size group writes the destinations itself (k_cycle0 with C0_OUT3, sc_cycle0.hip) from this many
// (member, level-0 tile) workgroups on; below, and for size classes, groups of more than ImageJobs::MAX members and single clones, it
// leaves planar bytes and a splice launch follows.  The cut is measured (profiles/out3_threshold.txt): from 200 on -- two
// members at 1024^2, the smallest group measured -- the new form is never slower than the splice beyond the runs' spread, and it gains from
// 720 on (two members at 2048^2: 1.4 %; sixteen: 2.8 %).  Nothing smaller was measured: it keeps the splice.
constexpr long SC_OUT3_MIN_TILES = 200;
// The first launch of such a group reads the destinations' bytes (C0_IN3), and its pre-process stores no float16 initial field, from this
// many (member, level-0 tile) workgroups on; below, the planes as ever.  Measured (profiles/in3_threshold.txt): 60 and 120
// tiles (2 and 4 members at 512^2) are 5.3 and 3.7 % SLOWER with the bytes; from 200 (2 x 1024^2: +0.3 %, inside the runs' spread) the new form
// is never slower beyond the spread, and it gains from 720 on (2 x 2048^2: 0.8 %, 8 x 1024^2: 1.7 %, 16 x 2048^2: 1.2 %).
constexpr long SC_IN3_MIN_TILES = 200;

// internal return code of a solve (never crosses the C ABI): a 16-bit fixed-point store saturated, no output was written;
// solve_step repeats the pre-process and the solve with Instance::force_float_field set
constexpr int SC_RETRY_FLOAT_FIELD = 1;

// error helper: records the message, returns SC_ERR_HIP
int hip_fail(Instance *I, hipError_t e, const char *what);
#define SC_HIP(I, call)                                                   \
    do {                                                                  \
        hipError_t e_ = (call);                                           \
        if (e_ != hipSuccess) return hip_fail((I), e_, #call);            \
    } while (0)

int ensure(Instance *I, DevBuf &b, size_t bytes, bool zero = true);
int ensure_pinned(Instance *I, DevBuf &b, size_t bytes);
double fd_selftest_error();   // sc_fd_selftest.cpp
double fd_closed_selftest_error();
int setup_fields(Instance *I, int W, int H, int C);

// ---- what the entry points share (sc_api.cpp, sc_batch.cpp, sc_hooks.cpp) --------------------------------------------------------
// sc_api.cpp
Instance *get(void *p);                                   // the instance behind a handle, nullptr if it is none
int begin_call(void *p, Instance *&I);                    // a clone entry's prologue: get, clear the error and per-call statistics, set the device
int validate_images(Instance *I, const void *face, int fc, int fr, int fs, const void *body, int bc, int br,
                    int bs, const void *mask, int mc, int mr, int ms);
int geo_from_rect(Instance *I, const int r[4], int cx, int cy, Geo &g);
int check_roi(Instance *I, const Geo &g, int bc, int br);
int device_bbox(Instance *I, const uint8_t *d_mask, int mc, int mr, int ms, int cx, int cy, Geo &g);   // waits for the device's rectangle
void erode_mask(Instance *I, const uint8_t *d_mask, int ms, int mr, const Geo &g);                    // ROI g of the mask into I->d_M
// the scan of a device mask into the instance's rectangle (d_rect, pinned mailbox h_rect[4..7]), enqueue only.  predicted: the scan does not
// go out -- it is left in pending_scan (with the erode's geometry and byte count) to ride in the clone's pre-process launch
int bbox_enqueue(Instance *I, const uint8_t *d_mask, int mc, int mr, int ms, const Geo *predicted = nullptr);
// the pre-process launch of a single clone on its ROI origins, into the instance's fields in the formats f_half / u_half name; a pending
// scan rides in it, its tiles then erode the mask themselves into d_M.  Returns whether it carried the scan.
bool launch_clone_preprocess(Instance *I, const uint8_t *body_org, int bstep, const uint8_t *face_org, int fstep);
// pixel (x, y) of an interleaved 8-bit BGR image: where a ROI's origin lies
template <class T> inline T *roi_at(T *img, int step, int x, int y) { return img + (size_t)y * step + 3 * x; }
// sc_batch.cpp: the jobs of a group's launches.  GROUP_RS: ints between the rectangles of a group's scans, one 128-byte line each (eight
// rectangles in one line: 162 us for the group's scan instead of 20)
constexpr int GROUP_RS = 32;
// the scans of the usable members of a call: rectangles to d_r and to the pinned h_out, GROUP_RS ints apart, at the member's index
std::vector<MaskJob> group_scan_jobs(const sc_batch_job *jobs, int n, const std::vector<char> &usable, int *d_r, int *h_out);
// erode and image jobs of members idx[0..) as one field (run_group_members): member k's eroded mask is plane k (mplane bytes) of d_M
void group_member_jobs(Instance *I, const sc_batch_job *jobs, const std::vector<int> &idx, const std::vector<Geo> &geo, const int *guess, int *d_r,
                       bool size_class, const std::vector<char> &frame, size_t mplane, std::vector<MaskJob> &mj, std::vector<ImageJob> &ij);
void fill_info_geo(Instance *I, const Geo &g);
float ev_ms(hipEvent_t a, hipEvent_t b);
// stage mark k of an edit or a Poisson call (synchronous calls only; a failed record leaves the mark's time unread)
inline void stage_mark(Instance *I, int k)
{
    if (I->stage_marks) (void)hipEventRecord(I->ev[k], I->stream);
}
// a batch's code: the first real error, else SC_ERR_NOT_CONVERGED if any member did not converge, else SC_OK
inline int worse(int worst, int rc) { return (rc != SC_OK && (worst == SC_OK || worst == SC_ERR_NOT_CONVERGED)) ? rc : worst; }
// sc_edit_api.cpp: the whole-image edits' stages (the test hooks drive them too)
int edit_validate(Instance *I, const sc_edit_params *p, const void *src, int cols, int rows, int ss, const void *mask, int ms,
                  const void *dst, int ds);
int canny_stage(Instance *I, const uint8_t *d_src, int W, int H, int ss, float low, float high, int aperture, uint8_t *C_out);
int edit_stage(Instance *I, const sc_edit_params *p, const uint8_t *d_src, int W, int H, int ss, const uint8_t *d_mask, int ms);
void edit_preprocess(Instance *I, const sc_edit_params *p, const uint8_t *d_src, int ss);     // into I->U0, I->F (setup_fields first)
// ... the same for a group of n same-size images (sc_edit_batch.cpp): member k's eroded mask / class map in plane k of d_M / d_edge
int canny_stage_group(Instance *I, const EditJob *jobs, int n, int W, int H, size_t mplane, float low, float high, int aperture);
void edit_preprocess_group(Instance *I, const sc_edit_params *p, const EditJob *jobs, int n, size_t mplane);
// sc_poisson_api.cpp: the Poisson call's validation (host-only; why: the reason) ...
int poisson_validate(const sc_poisson_params *p, const sc_poisson_layout *l, const char **why);
// ... and the front end the float32 families share (sc_poisson_api.cpp, sc_screened_api.cpp, sc_weighted_api.cpp; DESIGN.md "float32
// call front end"): validation, job intake, host staging, the chunk loop and the way back.
// A kind's parts.  The free sides as a mask (1 left, 2 right, 4 top, 8 bottom; SC_POISSON_NEUMANN: all four); the periodic axes as a
// mask (1 x, 2 y); the base kind (anything but GUIDANCE or LAPLACIAN there is a bad kind); the kind the entry points hand on: all four
// sides free reads SC_POISSON_NEUMANN alone, so one test of that bit finds the Neumann call and any SC_POISSON_FREE_* bit left a call
// with one to three free sides; the periodic bits pass through.
constexpr int SC_POISSON_FREE_ALL = SC_POISSON_FREE_LEFT | SC_POISSON_FREE_RIGHT | SC_POISSON_FREE_TOP | SC_POISSON_FREE_BOTTOM;
constexpr int SC_POISSON_PERIODIC_ALL = SC_POISSON_PERIODIC_X | SC_POISSON_PERIODIC_Y;
inline int poisson_free_sides(int kind) { return (kind & SC_POISSON_NEUMANN) ? 15 : (kind & SC_POISSON_FREE_ALL) >> 12; }
inline int poisson_periodic(int kind) { return (kind & SC_POISSON_PERIODIC_ALL) >> 17; }
inline int poisson_base(int kind) { return kind & ~(SC_POISSON_NEUMANN | SC_POISSON_FREE_ALL | SC_POISSON_PERIODIC_ALL); }
inline int poisson_norm_kind(int kind)
{
    const int f = poisson_free_sides(kind);
    return poisson_base(kind) | (f == 15 ? SC_POISSON_NEUMANN : f << 12) | (kind & SC_POISSON_PERIODIC_ALL);
}
// a call the transforms on caller arrays serve (direct_jobs_solve): a free side or a periodic axis
inline bool poisson_direct(int kind) { return poisson_free_sides(kind) || poisson_periodic(kind); }
// the axis kinds and unknowns of a call with free sides `f` (f = 0, the Dirichlet frame, and f = 15 included) and periodic axes `per`
// (a periodic axis has no free side: poisson_validate)
inline MixedGeo poisson_mixed_geo(int f, int cols, int rows, int per)
{
    auto axis = [](bool lo, bool hi) { return lo ? (hi ? 1 : 3) : (hi ? 2 : 0); };
    MixedGeo mg;
    mg.ax = (per & 1) ? MIXED_PERIODIC : axis(f & 1, f & 2);
    mg.ay = (per & 2) ? MIXED_PERIODIC : axis(f & 4, f & 8);
    mg.nx = cols - (mixed_low_d(mg.ax) ? 1 : 0) - (mixed_high_d(mg.ax) ? 1 : 0);
    mg.ny = rows - (mixed_low_d(mg.ay) ? 1 : 0) - (mixed_high_d(mg.ay) ? 1 : 0);
    return mg;
}
// no side of the kind (poisson_norm_kind's) keeps a Dirichlet line: boundary is read for its mean alone (unscreened; may be NULL) or not at all
inline bool poisson_no_dirichlet(int kind)
{
    const MixedGeo mg = poisson_mixed_geo(poisson_free_sides(kind), 4, 4, poisson_periodic(kind));
    return mixed_zero_eig(mg.ax) && mixed_zero_eig(mg.ay);
}
// lam > 0: a screened call -- the jobs carry their data term (PoissonJobDev::d), the solve is the direct one with shifted denominators
struct PoissonCall { int kind; float tol, lam; };      // kind: poisson_norm_kind's
size_t poisson_span(const sc_poisson_layout *l);          // floats from an array's pointer to one past its last element
// What a family's jobs carry beyond the Poisson call's arrays, and one job's arrays (host or device pointers; absent ones NULL).
enum { FLOAT_DATA = 1, FLOAT_WEIGHT = 2, FLOAT_SMOOTH = 4, FLOAT_STATE = 8, FLOAT_GT = 16, FLOAT_SMOOTH_T = 32, FLOAT_LOWER = 64, FLOAT_UPPER = 128, FLOAT_FLOW = 256 };
struct FloatArrays {
    const float *gx, *gy, *lap, *data, *weight, *boundary; float *out; const float *smooth_x = nullptr, *smooth_y = nullptr;
    const float *state = nullptr;      // FLOAT_STATE: the region call's state array
    const float *gt = nullptr;         // FLOAT_GT: the volume call's temporal guidance (may be NULL: zeros)
    const float *smooth_t = nullptr;   // FLOAT_SMOOTH_T: the WLS volume call's temporal link weights
    const char *refuse = nullptr;      // the family's own reason against this job (float_job_validate: SC_ERR_BAD_ARG with it)
    const float *lower = nullptr, *upper = nullptr;      // FLOAT_LOWER, FLOAT_UPPER: the bounded call's per-pixel bounds
    const float *flow_x = nullptr, *flow_y = nullptr;    // FLOAT_FLOW: the flow volume call's two dense flow arrays (no channel axis, their own length)
};
// A screened or weighted family's validation around poisson_validate: params (their kind) and layout non-null, `own` (the reason the
// family's own parameters fail, or NULL), the Poisson call's checks, then the direct solve's side limit under a frame with `limit_why`.
int family_validate(const int *kind, const sc_poisson_layout *l, const char *own, const char *limit_why, const char **why);
// The instance's word on a direct solve before anything runs: the method must be SC_METHOD_AUTO or SC_METHOD_FFT (`method_why`), and
// under SC_FLAG_FFT_FP64 no axis may have more unknowns than the double transforms take (`fp64_why`, SC_ERR_BAD_SIZE).
int direct_instance_check(Instance *I, int kind, const sc_poisson_layout *l, const char *method_why, const char *fp64_why);
// A job's own code: the pointers its kind (poisson_norm_kind's) and family need, each 4-byte aligned.  Without a Dirichlet line on any
// side a Poisson job may come without boundary (mean zero) and the other families do not read it: float_dev_job drops it there.
// FLOAT_SMOOTH: the two link arrays as well, and -- span > 0, the floats an array occupies under the call's layout (poisson_span) --
// neither they nor weight may share a float of their span with out's.  FLOAT_STATE: the state array as well, under the same span rule
// (which then holds for whichever of weight and the link arrays the call carries).  FLOAT_SMOOTH_T: the temporal link array as well; it
// occupies tspan floats (the call's temporal frames) and may share none of them with out's span.  FLOAT_LOWER, FLOAT_UPPER: that bound
// array as well, under state's span rule.  FLOAT_FLOW: the two flow arrays as well; each occupies fspan floats (dense: the call's temporal
// frames of cols x rows) and may share none of them with out's span.
int float_job_validate(int kind, int carries, const FloatArrays &a, const char **why, size_t span = 0, size_t tspan = 0, size_t fspan = 0);
PoissonJobDev float_dev_job(int kind, int carries, const FloatArrays &a);
// A job's side arrays: what a family's set-up reads beside the job's PoissonJobDev -- data weights, spatial link weights, the region
// and volume calls' state, the volume calls' temporal guidance and temporal link weights, the bounded call's bound arrays.  Device pointers; an array the call does not
// carry (its FLOAT_* bit is not in `carries`) is NULL: float_intake and float_stage say so, nobody behind them asks again.  One record
// per job, beside its PoissonJobDev from there to the kernels' tables (sc_pcg.h: PcgOperator::ds, for_side_tables).
struct SideArrays {
    const float *w = nullptr, *sx = nullptr, *sy = nullptr, *st = nullptr, *gt = nullptr, *smt = nullptr, *lo = nullptr, *hi = nullptr;
    const float *fx = nullptr, *fy = nullptr;      // the flow volume call's two dense flow arrays
};
// The validated jobs of a device call: their device forms (contiguous: the Poisson and the screened call hand dj.data() to the solve),
// their side arrays and where each one's code goes.
struct FloatJobs { std::vector<PoissonJobDev> dj; std::vector<SideArrays> side; std::vector<int *> rcs; };
// A device call's job intake: arrays_of(job) names one public job's arrays.  A job that fails float_job_validate gets its code; the
// others go into v with SC_ERR_HIP until their chunk has run.  Returns the worst validation code, I->err the first reason (v.rcs
// empty: nothing to run).
template <class Job, class ArraysOf> int float_intake(Instance *I, int kind, int carries, Job *jobs, int n, ArraysOf arrays_of, FloatJobs &v,
                                                      size_t span = 0, size_t tspan = 0, size_t fspan = 0)
{
    if (!jobs || n <= 0) { I->err = "no jobs"; return SC_ERR_BAD_ARG; }
    int worst = SC_OK;
    const char *why = "";
    for (int i = 0; i < n; ++i) {
        Job &j = jobs[i];
        const FloatArrays a = arrays_of(j);
        const int vrc = float_job_validate(kind, carries, a, &why, span, tspan, fspan);
        if (vrc != SC_OK) {
            j.rc = vrc;
            if (worst == SC_OK) { worst = vrc; I->err = why; }
            continue;
        }
        j.rc = SC_ERR_HIP;          // until its chunk has run
        v.dj.push_back(float_dev_job(kind, carries, a));
        const bool smooth = (carries & FLOAT_SMOOTH) != 0;
        v.side.push_back(SideArrays{ carries & FLOAT_WEIGHT ? a.weight : nullptr, smooth ? a.smooth_x : nullptr, smooth ? a.smooth_y : nullptr,
                                     carries & FLOAT_STATE ? a.state : nullptr, carries & FLOAT_GT ? a.gt : nullptr,
                                     carries & FLOAT_SMOOTH_T ? a.smooth_t : nullptr, carries & FLOAT_LOWER ? a.lower : nullptr,
                                     carries & FLOAT_UPPER ? a.upper : nullptr });
        if (carries & FLOAT_FLOW) { v.side.back().fx = a.flow_x; v.side.back().fy = a.flow_y; }
        v.rcs.push_back(&j.rc);
    }
    return worst;
}
// A host call's staging: the arrays' spans into one block of I->d_pois, each at a 256-byte boundary -- gx, gy or lap | data | weight |
// boundary unless it is data | out unless it is data or boundary (in place) | smooth_x | smooth_y | state | lower | upper | flow_x | flow_y --, uploaded in that order.  job: the
// device job (float_dev_job's rules; job.out is what poisson_download reads), side: the staged side arrays (NULL where the call carries none).
// frames > 1 (the volume call): every array is `frames` images frame_stride floats apart -- one span of all of them is staged; the
// temporal arrays -- gt, FLOAT_GT and not NULL, and smooth_t, FLOAT_SMOOTH_T -- hold tframes of them (0: frames - 1) and go behind
// state, each through a pinned block of its own.  FLOAT_FLOW: the two flow arrays, flow_floats floats each (at most a slot: they
// have no channel axis), in the last two slots, through h_fx and h_fy.
struct FloatStaged { PoissonJobDev job; SideArrays side; };
int float_stage(Instance *I, const sc_poisson_layout *l, int kind, int carries, const FloatArrays &a, FloatStaged &s, int frames = 1,
                long long frame_stride = 0, int tframes = 0, size_t flow_floats = 0);
// nv validated jobs of C channels through chunks of at most SC_POISSON_MAX_PLANES planes: chunk(i0, m) runs jobs i0 .. i0 + m - 1 and
// sets their codes.  SC_OK and SC_ERR_NOT_CONVERGED let the call go on; any other code ends it: that chunk's jobs and every one not
// yet run read it, after SC_ERR_HIP the ones already run too.  Returns that code, else the worst.
template <class Chunk> int run_chunks(Instance *I, int C, int *const *rcs, int nv, Chunk chunk)
{
    const int per = std::max(1, SC_POISSON_MAX_PLANES / C);
    int worst = SC_OK;
    for (int i0 = 0; i0 < nv; i0 += per) {
        const int m = std::min(per, nv - i0);
        const int rc = chunk(i0, m);
        if (rc != SC_OK && rc != SC_ERR_NOT_CONVERGED) {
            for (int k = rc == SC_ERR_HIP ? 0 : i0; k < nv; ++k) *rcs[k] = rc;
            return rc;
        }
        worst = worse(worst, rc);
        I->info.group_members = m > 1 ? m : 0;
    }
    return worst;
}
int poisson_run(Instance *I, const PoissonCall &p, const sc_poisson_layout *l, const PoissonJobDev *dj, int *const *rcs, int nv, bool timed, float t[4]);
void poisson_set_timing(Instance *I, const float t[4]);
int poisson_download(Instance *I, const sc_poisson_layout *l, const float *d_out, float *out, const float t[4], int rc_solve, int frames = 1,
                     long long frame_stride = 0);
// sc_arena.cpp: row copies between caller memory, pinned staging and the device (no 2-D copies)
void copy_rows(Instance *I, uint8_t *dst, size_t dpitch, const uint8_t *src, size_t spitch, size_t row_bytes, int rows);
int upload_rows(Instance *I, DevBuf &stage, void *d, size_t dpitch, const uint8_t *h, size_t hpitch, size_t row_bytes, int rows);
int download_rows(Instance *I, DevBuf &stage, uint8_t *h, size_t hpitch, const void *d, size_t dpitch, size_t row_bytes, int rows);

// solver drivers (sc_solver.cpp) -- operate on I->U0/U1/F, leave the answer in result(I)
int solve(Instance *I);
// One solve of every driver that writes through the solver (clones, edits, their groups, Poisson chunks) into target t: pre()
// enqueues the pre-process for the current I->f_half / I->u_half (and the caller's own marks) and returns a code.  A solve whose
// 16-bit field saturated wrote nothing: pre() and the solve go again on float fields (info.field_retry).  Unless the solver wrote
// the output itself (spec_post.done), the caller then writes it with write_output.  Run under a CallScope.
void solve_prepare(Instance *I, const SolveTarget &t = SolveTarget());      // the field formats the pre-process is to write (t: u0_bytes is a group's)
int solve_attempt(Instance *I, const SolveTarget &t);    // SC_RETRY_FLOAT_FIELD: force_float_field is set, repeat both
template <class Pre> int solve_step(Instance *I, const SolveTarget &t, Pre &&pre)
{
    int rc;
    do {
        solve_prepare(I, t);
        if ((rc = pre())) return rc;
    } while ((rc = solve_attempt(I, t)) == SC_RETRY_FLOAT_FIELD);
    return rc;
}
int write_output(Instance *I, const SolveTarget &t, AbortFlag sat = AbortFlag());   // the post-process of result(I) into t
bool mg_reads_half_rhs(const Instance *I);
bool mg_level1_half(const Instance *I);      // sc_multigrid.cpp: level 1's right-hand side and correction are stored as float16 in the solve configured in I
bool mg_composes_level1(const Instance *I);   // sc_multigrid.cpp: level 1 runs pre-smoothing only, the level-0 launch composes its prolongation source
// the cycle's sweeps, the stop rule's threshold and the budget of cycles: the options, or their defaults
struct MGParams { int pre, post, budget; float utol; };
inline MGParams mg_params(const sc_solver_opts &o)
{
    return { o.mg_pre > 0 ? o.mg_pre : 2, o.mg_post > 0 ? o.mg_post : 2, o.max_sweeps > 0 ? o.max_sweeps : 30, o.update_tol > 0.f ? o.update_tol : 0.25f };
}
// the bottom's matrices may still be in the making on the second stream (build_fd, rag_begin_builds): the main stream waits for them once
inline int fd_wait(Instance *I)
{
    if (I->fd_pending) {
        SC_HIP(I, hipStreamWaitEvent(I->stream, I->ev_fd, 0));
        I->fd_pending = false;
    }
    return SC_OK;
}
// sc_multigrid.cpp, for the measurement hooks (sc_hooks.cpp): one cycle from level l down and up again; the level above the bottom and
// the bottom in one launch (done: the launch serves this shape), and whether the solve runs level l so
int vcycle(Instance *I, size_t l, int pre, int post, unsigned no_post = 0);
int run_tail(Instance *I, size_t l, int pre, int post, bool &done, unsigned long long *stamps = nullptr);
bool tail_serves(const Instance *I, size_t l);

// ---- the schedule of a fused multigrid solve (sc_multigrid.cpp): which level-0 launch comes next, as a function of the solve's facts
// and of what the stop rule answered so far.  No instance, no pointer, no HIP call: mg_solve_fused launches what it says, the
// measurement hooks time four of its steps, sc_hip_fused_schedule lists them.
// Steps: the first launch (pre-smoothing + residual + restriction, no prolongation) | the full cycle | the full cycle before the judged
// one (16-bit field in, float out, may leave the node correction's cell shares) | the judged cycle leaving output bytes | ... leaving
// its field | the catch-up launch behind a rejected judged cycle (the form of the first launch)
enum { FUSED_DONE = 0, FUSED_FIRST, FUSED_FULL, FUSED_BEFORE_JUDGED, FUSED_JUDGED_BYTES, FUSED_JUDGED_FIELD, FUSED_CATCH_UP };
// REJECT_EARLY: by FusedSchedule::early_cond; NO_FORM: the bytes form is not instantiated, nothing was launched
enum { VERDICT_NONE = -1, VERDICT_ACCEPT = 0, VERDICT_REJECT, VERDICT_REJECT_EARLY, VERDICT_SATURATED, VERDICT_NO_FORM };
enum { NODES_NONE = 0, NODES_MAIN, NODES_SECOND, NODES_NOTHING };
struct FusedFacts {
    int pre, post, budget;
    bool tol;                  // a residual tolerance is set: every cycle is judged
    bool out_wanted, q16;      // the judged cycle may leave output bytes; the field starts as 16-bit fixed point (mg_solve_fused)
    bool u_half, composed;     // the initial field is float16; mg_composes_level1
    bool separate_restrict;    // SC_LEGACY_SEPARATE_RESTRICT: no launch leaves cell shares
    bool small;                // more than 3 planes, or fewer than 3 << 18 pixels: the early node correction stays on the main stream
};
struct FusedStep {
    int kind = FUSED_DONE, sweeps = 0;
    bool prolong = false, final_cycle = false, out_bytes = false, u_half = false, q16_in = false, q16_out = false, composed = false;
    bool coarse_first = false; // the step opens a cycle: levels 1 .. bottom run in front of it
    int bands_sweeps = 0;      // ... and the cycle's bands buffer is asked for then, sized for this many sweeps (0: none)
    int bands = 0;             // the launch receives that buffer (sweeps it is sized for; 0: it does not)
    bool ask_early = false;    // lowmode_early_kind's answer decides the rest of the step: fused_early, in front of the bands buffer
    bool lm = false;           // the launch carries the early node correction (the main stream waits for it first)
    int nodes = NODES_NONE;    // the correction the next cycle's bytes carry is computed from this launch's result: on the main stream, the second, or there is none to add
    bool judged = false;       // the stop rule reads the launch's maxima; the next fused_next takes its verdict
    bool sat = false;          // the launch is given the solve's saturation word
};
struct FusedSchedule {
    FusedFacts f;
    int last = -1, cyc = 0;    // kind of the step handed out last (-1: none yet); cycles completed in front of it
    int sweep_launches = 0;    // as sc_run_info counts them (a bytes form counts once it is accepted)
    int result = SC_OK;        // at FUSED_DONE: SC_OK, SC_ERR_NOT_CONVERGED or SC_RETRY_FLOAT_FIELD
    bool early_ready = false;  // the node correction for the judged cycle's bytes is on its way
    bool early_cond = false;   // ... and the bytes stand only if the judged update is small enough (lowmode_early_kind 3)
    bool u_q16 = false;        // the field is 16-bit fixed point
};
FusedStep fused_next(FusedSchedule &S, int verdict = VERDICT_NONE);
void fused_early(FusedSchedule &S, FusedStep &s, int early_kind);
Cycle0Launch level0_launch(Instance *I, bool composed = false);   // sc_multigrid.cpp: what every level-0 launch on I's fields and hierarchy says alike
Cycle0Launch step_launch(Cycle0Launch d, const FusedStep &s);     // ... and what step s adds to it: everything but buffers, `timing` and `rag`
int lowmode_correct(Instance *I, const Field &U, const Field &Out);   // sc_lowmode.hip: Out = U + float-table correction
int lowmode_nodes(Instance *I, const Field &U, LmNodes &lm, hipStream_t on = nullptr);      // on: another stream than the instance's          // the correction of U at the node rows (what the post-process adds)
float4 *lowmode_bands_buffer(Instance *I, int sweeps);               // where a final level-0 launch leaves the correction's cell shares (nullptr: not wanted)
inline void field_moved(Instance *I) { I->lm.bands_of = nullptr; }   // anything that writes the solution field outside the judged multigrid launch calls this
int lowmode_part_map_selftest();                                     // host-only check of the parts-per-cell-row map against the launch geometry
int lowmode_early_kind(Instance *I, float update_tol);                // see sc_lowmode.hip
void lowmode_bands_written(Instance *I, const float *field);       // the launch went in: B describes `field` (nullptr: nothing)
int lowmode_count(int n);
bool lowmode_ratio(int w, int h, int Kx, int Ky, int Kxp, float *R, double &max_ratio);   // the correction's ratio table (R may be nullptr: statistics only); false: singular
bool lowmode_part_map(int H, int sweeps, std::vector<int> &m, int &band_rows);
bool lowmode_part_map(int H, int sweeps, int *m, int &band_rows);      // ... into 4 ints per cell row, all -1 on entry
int lowmode_projection_splits(int nxt, int nkb);                      // row splits of the coarse projection for a ROI with nxt column tiles
void launch_lm_tables_rag(const RagMember *rag, int members, int max_rows, int Kxp, int Kyp, hipStream_t s);
void mg_plan_levels(int W, int H, std::vector<MGGeom> &g);           // sc_mg_levels.cpp
size_t mg_default_tail_level(const std::vector<MGGeom> &g);
size_t mg_plan_bottom(const std::vector<MGGeom> &g, bool default_rule);      // first level of the cycle's bottom (g.size(): none)
bool mg_ladder_composes(size_t levels, size_t bottom);                       // the ladder allows the composed level 1 (mg_composes_level1)
MGDim make_dim(int n, double a, int nc);                             // one direction of a level: n unknowns, last interval a, nc coarse unknowns
int bottom_pitch(const MGLevel &L);                                  // row pitch of a level inside the bottom kernel's LDS
int build_levels(Instance *I);                                       // the hierarchy of the fields bound to I (kept while their size stays)
int mg_build_levels_rag(Instance *I, hipStream_t zero_on);           // the class's level planes, zeroed on the given stream
int rag_begin_table(Instance *I, const std::vector<SizePlan> &members);      // the members' table and host tables, uploaded on the instance's stream (sets I->rag.dev)
int rag_begin_builds(Instance *I);                                           // ... then everything the device builds per call, on two more streams
void rag_end(Instance *I);
int dst_solve(Instance *I);                                           // sc_dst.hip: SC_METHOD_DST
int fft_solve(Instance *I, bool fp64);                                // sc_fft.hip: SC_METHOD_FFT (fp64: SC_FLAG_FFT_FP64)
bool fft_supported(int w, int h, bool fp64);
// sc_fft.hip: the problem with free sides on some or all of the borders or periodic axes (SC_POISSON_FREE_*, SC_POISSON_NEUMANN,
// SC_POISSON_PERIODIC_*; mg: poisson_mixed_geo) on caller arrays: m same-size jobs as C m planes, straight from the jobs' arrays into their out arrays, each axis under its own transform
// (marks: 5 behind the boundary-mean reduction of an unscreened singular solve -- no Dirichlet line on any side --, else at the start; 6 behind the last transform launch)
// (lam > 0: the screened solve, sc_screened_api.cpp: the jobs' data term read with the right-hand side, no mean)
// lam_tab (device; NULL: none): one shift per plane in lam's place, lam_tab[member C + channel], each a float's value; a plane whose
// shift is 0 in a system without any Dirichlet line is the singular solve (its coefficient (0, 0) is set to 0)
int direct_jobs_solve(Instance *I, const PoissonGeo &g, const MixedGeo &mg, bool lap, const PoissonJobDev *jobs, int m, bool fp64, float lam = 0.f,
                      const double *lam_tab = nullptr);
bool wants_float_tables(const Instance *I);
int effective_method(const Instance *I);                              // sc_solver.cpp: what SC_METHOD_AUTO resolves to for the fields bound to I
int output_nodes(Instance *I, LmNodes &lm);  // sc_solver.cpp: the float-table correction the post-process of result(I) has to add (none: lm.CN == nullptr)
int run_sweeps(Instance *I, int method, int sweeps, float omega, int sweeps_per_launch);
int fused_depth(int method, int sweeps_per_launch); // 0 = plain kernels
int eval_residual(Instance *I, double out[2]);
Field &result(Instance *I);
float optimal_omega(int W, int H);

} // namespace sc
