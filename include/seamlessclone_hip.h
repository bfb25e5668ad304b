/*
 * seamlessclone_hip.h -- C ABI of libseamlessclone_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for the seamless-clone (Poisson image editing, NORMAL_CLONE) hot path of
 * wujinzhong/seamlessCloneOptimization.  The four my_seamlessclone_api_imp_* symbols keep the
 * names the reference exports from seamlessClone-CUDA/seamlessclone_cuda.h:4-63 (thin
 * wrappers over seamlessClone_imp.cu:239,265,354,365) and that its Python binding re-declares
 * at seamlessClone-python-binding/SeamlessClone.cpp:37-44.  The reference passes cv::Mat* as
 * void* and returns a cv::Mat by value; a C ABI cannot, so each cv::Mat becomes the
 * {data, cols, rows, step} quadruple it wraps and the result is written in place into `body`
 * (the reference's returned Mat aliases the caller's dest buffer, seamlessClone_imp.cpp:470).
 *
 * Images are 8-bit, BGR interleaved (CV_8UC3) for face/body and single channel (CV_8UC1)
 * for mask, `step` = bytes per row.  All sc_hip_* entry points are additions: solver
 * options, a device-resident run for callers whose images already live in HBM, run
 * statistics and a batch driver.  The stage-level hooks used by the parity tests are in
 * seamlessclone_hip_testing.h, which integrators do not need.
 *
 * Threading: one instance <-> one HIP stream <-> one host thread at a time (reference:
 * one instance per stream, not re-entrant).  No process-global state.
 */
#ifndef SEAMLESSCLONE_HIP_H
#define SEAMLESSCLONE_HIP_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__GNUC__)
#define SC_API __attribute__((visibility("default")))
#else
#define SC_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* ---- return codes (the reference aborts / asserts instead: seamlessClone_imp.cu:272-275,
 *      seamlessClone_imp.cpp:432-436,1013) */
#define SC_OK                 0
#define SC_ERR_BAD_ARG       -1   /* null pointer, bad instance, bad option value          */
#define SC_ERR_BAD_SIZE      -2   /* face/mask size mismatch, step too small, empty image  */
#define SC_ERR_EMPTY_MASK    -3   /* bbox of mask!=0 degenerate (reference assert :1013)   */
#define SC_ERR_ROI_OOB       -4   /* ROI leaves body (unchecked in the reference)          */
#define SC_ERR_HIP           -5   /* HIP runtime error; see sc_hip_last_error()            */
#define SC_ERR_NOT_CONVERGED -6   /* tol not reached within max_sweeps; result still written */

/* OpenCV clone flags (cv::NORMAL_CLONE, cv::MIXED_CLONE, cv::MONOCHROME_TRANSFER, same values).  The reference hard-codes
 * NORMAL_CLONE (seamlessClone_imp.cu:301); the other two are additions, selected per instance with sc_hip_set_clone_mode.
 * Inside the mask the blended gradient field is
 *   NORMAL       the patch's (gx, gy)
 *   MIXED        per channel and pixel, the patch's (gx, gy) where |gx - gy| of the patch exceeds the destination's, else the destination's
 *   MONOCHROME   the (gx, gy) of the patch's grey image, (1868 B + 9617 G + 4899 R + 8192) >> 14, in all three channels
 * and the destination's (gx, gy) outside it (OpenCV 3.4.5 Cloning::normalClone).  PARITY UNPINNED for MIXED and MONOCHROME:
 * checked against a restatement of that arithmetic, not against OpenCV or a fixture of the reference. */
#define SC_NORMAL_CLONE        1
#define SC_MIXED_CLONE         2
#define SC_MONOCHROME_TRANSFER 3

/* ---- solver selection */
enum sc_method {
    SC_METHOD_JACOBI = 0,    /* U' = 1/4 (l+r+u+d - lap), ping-pong                         */
    SC_METHOD_RBGS   = 1,    /* red-black Gauss-Seidel (omega = 1)                          */
    SC_METHOD_SOR    = 2,    /* red-black SOR, omega from opts (<=0: optimal for the ROI)   */
    SC_METHOD_MULTIGRID = 3, /* V-cycles with red-black GS smoothing (converges at any ROI)  */
    SC_METHOD_DST    = 4,    /* the reference's direct solve (seamlessClone_imp.cpp:1814-1896; matrix form :1266-1334):
                                u = S_h ((S_h g S_w) / den) S_w with den = filter_X + filter_Y - 4 from the float
                                tables of :596-599, four double-precision products on the matrix cores.  O(n^3):
                                milliseconds at 2048^2; the non-iterative cross-check of the default path          */
    SC_METHOD_AUTO   = 5,    /* DEFAULT.  A direct solve -- SC_METHOD_FFT with double transforms -- for ROIs of at most
                                SC_AUTO_DIRECT_MAX unknowns per side (there it is faster than the cycles and has no iteration
                                error: diff sum against the float-table CPU port 2 instead of 129 at the reference's 300x194
                                patch, whose own published deviation from OpenCV is 44, PDF p3) and for thin ROIs
                                (SC_AUTO_THIN_MAX) -- single clones only: a group of clones (sc_hip_run_device_batch) is about
                                throughput, where the cycles win at every size --, SC_METHOD_MULTIGRID above and whenever
                                tol > 0 asks for a residual-based stop.  sc_run_info.method says which one ran.                                      */
    SC_METHOD_FFT    = 6     /* the reference's DEFAULT direct back-end (poissonSolver2D_FFT, seamlessClone_imp.cpp:1694-1918):
                                the same u = S_h ((S_h g S_w) / den) S_w in float32 with FFT-based transforms, O(n^2 log n).
                                The DST-I of each row is a chirp-z transform over a power-of-two FFT held in LDS (sc_fft.hip);
                                at most 8192 unknowns per side (SC_ERR_BAD_SIZE beyond).  float32 like cuFFT / OpenCV's dft:
                                within +-1 of the float-table port, diff sums of the size the reference publishes for its
                                own cuFFT path against OpenCV (PDF p3)                                           */
};
#define SC_AUTO_DIRECT_MAX 720        /* round 4 (900 in round 3): the cycles got faster (0.222 against 0.231 ms at 750^2, 0.228 against 0.268 at 900^2) */
#define SC_AUTO_DIRECT_AREA 450000   /* round 4: ... also where the ROI has at most this many unknowns in all, whatever its shape (an elongated ROI's
                                       transforms are short in one direction: 900 x 100 takes 0.10 ms directly, 0.19 in cycles), ... */
#define SC_AUTO_NARROW_MAX 140      /* ... and where it is at most this many unknowns across -- both up to SC_AUTO_THIN_LONG_MAX along (the double
                                       transform's limit): 4000 x 130 takes 0.37 ms directly, 0.45 in cycles                          */
#define SC_AUTO_THIN_MAX 4          /* ... and for thin ROIs (at most this many unknowns across, up to SC_AUTO_THIN_LONG_MAX along) */
#define SC_AUTO_THIN_LONG_MAX 4096

typedef struct sc_solver_opts {
    int   method;            /* enum sc_method                                              */
    int   max_sweeps;        /* sweeps (JACOBI/RBGS/SOR) or V-cycles (MULTIGRID) budget; MULTIGRID
                                reports SC_ERR_NOT_CONVERGED when the budget ends first         */
    float tol;               /* stop when ||lap - A u||_2 / ||lap||_2 <= tol; <=0: run
                                exactly max_sweeps                                         */
    int   check_every;       /* sweeps between residual checks (tol>0)                      */
    float omega;             /* SOR relaxation; <=0 -> optimum for the rectangle,
                                2/(1+sqrt(1-rho^2)), rho = (cos(pi/(w+1))+cos(pi/(h+1)))/2            */
    int   sweeps_per_launch; /* 0: library default (register-blocked fused kernels, deepest depth);
                                1: one sweep per launch with the plain kernels; -1: fused kernel, depth 1;
                                >=2: fused kernel at that depth (Jacobi 1-4, 6, 8; red-black 1-2).  All variants
                                give bit-identical fields.                                          */
    int   reference_warmup;  /* 1: clone twice in place, as the reference's run() does
                                (warm-up + 1, seamlessClone_imp.cu:303-318)                */
    int   mg_pre, mg_post;   /* multigrid smoothing sweeps per level (0 = default 2/2)      */
    float update_tol;        /* MULTIGRID stop rule, in grey levels.  The error a V-cycle leaves is
                                ~rho/(1-rho) times the largest coarse-grid correction it applied to
                                the ROI (rho = contraction per cycle, 0.05-0.1).  From the third cycle
                                on the driver measures rho from two successive corrections and stops
                                once that predicted error is <= 0.1 x update_tol; with only one
                                correction known (max_sweeps = 1) it stops once the correction itself
                                is <= update_tol.  Default 0.25 (error <= 0.025): normally 3 cycles,
                                max |delta| 1 on 0.004-0.1 % of channels vs the exact solution -- below
                                the reference's own float32 deviation from OpenCV (0.16 % at 2400x1552,
                                PDF p3).  0.02 costs one or two more cycles.
                                The float32 residual norm stalls earlier and is only reported. */
    int   flags;             /* SC_FLAG_* bits below; 0 = the default paths                  */
    int   jacobi_tile_rows;  /* single-sweep Jacobi launches (sweeps_per_launch = 1): 0 = rows rolling through
                                registers (k_jacobi_roll, default); 16, 32 or 64 = the LDS-staged 256 x rows tile
                                with a 1-pixel halo (k_jacobi<rows>).  Bit-identical fields.              */
    int   mg_level1_sweeps;  /* multigrid, default schedule (level 1 without post-smoothing, SC_FLAG_NO_COMPOSE_L1 clear): sweeps
                                level 1 does before its restriction; 0 = default (4), 2..4                        */
    int   mg_direct_max;     /* multigrid bottom kernel: the first level whose sides are both at most this many unknowns is solved
                                directly (fast diagonalisation); the LDS-resident levels above it cycle.  0 = default
                                (SC_MG_DIRECT_MAX_DEFAULT); at most 128.  Same fixed point, slightly different iterates        */
    int   legacy_paths;      /* read only with SC_FLAG_LEGACY_PATHS (seamlessclone_hip_testing.h): SC_LEGACY_* bits, the superseded launch forms to run instead of
                                the defaults (A/B measurements and cross-checks of kernels whose decision is made)              */
} sc_solver_opts;
#define SC_MG_DIRECT_MAX_DEFAULT 128

/* ---- sc_solver_opts.flags: non-default variants of the same path, selectable per instance so one process (one
 *      test run) can drive every variant.  Unless noted a variant gives the default path's result bit for bit. */
#define SC_FLAG_NO_SPECULATE   (1 << 0)  /* wait for the device's bounding box before launching the clone (the
                                            reference's order, seamlessClone_imp.cpp:1012) instead of launching on
                                            a predicted box                                                      */
#define SC_FLAG_FLOAT_RHS      (1 << 1)  /* multigrid: keep the right-hand side as float32 (default: float16,
                                            exact -- it is an integer in [-1020, 1020]) AND level 1's right-hand side and
                                            correction as float32 (default: float16 -- a correction scheme tolerates it, the
                                            fixed point is level 0's).  Same fixed point, iterates a relative 5e-4 of a
                                            correction apart: results within one grey level of the default's, not bit-identical */
#define SC_FLAG_FLOAT_U0       (1 << 2)  /* multigrid: initial field as float32 (default: float16, exact -- 8-bit
                                            values)                                                             */
#define SC_FLAG_NO_COMPOSE_L1  (1 << 3)  /* multigrid: level 1 gets its own post-smoothing launch (textbook V(2,2));
                                            default: the level-0 launch composes its prolongation source from
                                            levels 1 and 2.  Same fixed point, slightly different iterates      */
#define SC_FLAG_VCYCLE_BOTTOM  (1 << 4)  /* multigrid: cycle down to the coarsest level inside the bottom kernel
                                            instead of solving its first level directly (fast diagonalisation).
                                            Same fixed point, slightly different iterates                       */
#define SC_FLAG_EXACT_TABLES   (1 << 5)  /* MULTIGRID / DST: return the exact solution of the 5-point
                                            system (DST: double denominators 2cos + 2cos - 4 instead of the float tables).  Default: the answer OpenCV and the reference compute, whose
                                            eigenvalue tables are stored and combined in float32
                                            (seamlessClone_imp.cpp:596-599, :1651-1653) -- see DESIGN.md sec. 5,
                                            "float-table correction"                                            */
/* bits 6, 7 and 14 are taken by seamlessclone_hip_testing.h (SC_FLAG_LEGACY_PATHS, SC_FLAG_KEEP_FIELD, SC_FLAG_POISON_ARENA): do not reuse them */

#define SC_FLAG_FFT_FP64       (1 << 8)  /* SC_METHOD_FFT: the transforms in double instead of float32 (tables, LDS and the planes
                                            between the launches); at most 4096 unknowns per side.  No transform rounding is left:
                                            the result agrees with SC_METHOD_DST (both are the reference's float-table arithmetic
                                            with exact transforms)                                                          */

#define SC_FLAG_OPENCV_GREY_MASK (1 << 9) /* masks that are not 0 / 255: OpenCV's semantics -- the three erodes are minimum filters (a grey
                                            eroded mask) and the gradients are blended with the fractional weights M/255 and
                                            (255 - M)/255 (OpenCV 3.4.5 modules/photo, Cloning::computeDerivatives / normalClone).
                                            Default: the reference's -- it thresholds (seamlessClone_imp.cpp:917, sum == 255 * 9:
                                            every value below 255 erodes to 0) and so only ever blends with 0 / 1.  On 0 / 255 masks
                                            the two are bit-identical.  The BOUNDING BOX stays the reference's under this flag: all non-zero
                                            pixels (seamlessClone_imp.cpp:943, `mask != 0`), i.e. OpenCV's erode and blend weights on the
                                            reference's ROI; cv::seamlessClone itself takes the box of the pixels equal to 255 only, so for
                                            a feathered mask its ROI (and Dirichlet ring) is smaller than the one used here.
                                            PARITY UNPINNED: OpenCV's source is not part of the
                                            reference and none of its fixtures holds a grey mask; checked against a restatement
                                            of the published algorithm (oracle/).  Groups run one clone at a time with it.   */

#define SC_FLAG_FLOAT_L1       (1 << 10) /* multigrid: level 1's right-hand side and correction as float32 (default on the fast path:
                                            float16, see SC_FLAG_FLOAT_RHS).  Same fixed point, slightly different iterates.
                                            Implies SC_FLAG_FLOAT_FIELD                                                        */
#define SC_FLAG_FLOAT_FIELD    (1 << 11) /* multigrid: the field between the level-0 launches always as float32.  Default on the fast
                                            path (float16 right-hand side and level 1, output bytes from the last cycle): the first
                                            stores of a solve -- all but the one the judged cycle reads -- are 16-bit fixed point,
                                            code = trunc(64 u + 16384.5) in [0, 65535], i.e. [-256, 768) in steps of 1/64.  A clone's
                                            solution lies in [-255, 510], its 8-bit boundary values are exact, and a rounding of
                                            <= 1/128 two cycles before the output is gone by then (each cycle removes 90 % of any
                                            error).  Takes 2 bytes per unknown off four of the six field transfers between a
                                            solve's level-0 launches                                                           */

#define SC_FLAG_NO_STAGE_MARKS  (1 << 12) /* sc_hip_run_device(..., bSync = true) and the host-image call: record only the first and the last stage mark.  Every
                                            mark is an event in the stream with a ~5 us bubble behind it, so the per-stage timeline
                                            (ms_mask, ms_pre, ms_solve) costs a 2048^2 clone ~15 us; with this flag ms_device_total is the
                                            un-instrumented device time of the clone and the per-stage figures read 0 (all of it is booked
                                            under ms_post).  Results are unaffected                                              */

#define SC_FLAG_ROWS_RETURN    (1 << 13) /* host-image call, OPT-IN (round 5; the default of late round 4): a destination without row padding whose
                                            ROI covers most of its rows gets those ROWS back as one linear copy straight into the caller's image
                                            (0.05-0.1 ms faster at 2048^2) -- the pixels of those rows OUTSIDE the ROI are rewritten with the
                                            values they had when the call started, so nothing else may write them during the call (another
                                            thread cloning into a disjoint ROI of the same image would lose its result).  Default: the result
                                            comes back as the compact ROI through pinned staging and is spliced into the caller's rows -- only
                                            ROI bytes of the caller's image are ever written, as in the reference (seamlessClone_imp.cpp:470-483) */

/* ---- statistics of the last run */
typedef struct sc_run_info {
    int    x0, y0, W, H, ltx, lty;  /* patch offset, ROI size (ring included), ROI origin in body */
    int    sweeps;                  /* sweeps (or V-cycles) executed                        */
    int    converged;               /* 1 when tol reached (or tol<=0)                       */
    double rel_residual;            /* last evaluated ||r||/||lap|| (NaN if never evaluated) */
    float  ms_h2d, ms_mask, ms_pre, ms_solve, ms_post, ms_d2h; /* hipEvent times on the instance stream; the multigrid
                                   driver enqueues the post-process directly behind its last cycle, without a mark between
                                   them: ms_post is then 0 and ms_solve includes it.  sc_hip_run_device with
                                   bSync = false records no marks (each is an event in the stream) and reports 0 */
    float  ms_device_total;         /* mask + pre + solve + post                            */
    int    sweep_launches;          /* launches of the dominant sweep kernel in the last run */
    float  last_update;             /* MULTIGRID: max |coarse-grid correction| of the last checked cycle (grey levels) */
    size_t device_bytes;            /* arena bytes owned by the instance                    */
    int    method;                  /* enum sc_method that ran (what SC_METHOD_AUTO resolved to) */
    int    device;                  /* HIP device the instance runs on (create_instance's gpu_id)  */
    float  ms_call;                 /* my_seamlessclone_api_imp_run: hipEvent time of the whole call's stream work, first upload
                                       to last download (what the reference's bSync timing brackets, seamlessClone_imp.cu:310-344) */
    int    field_retry;             /* 1: the 16-bit fixed-point field of the multigrid fast path saturated during this clone (an
                                       iterate left [-256, 768): possible when the mask mixes patch and destination gradients into a
                                       non-conservative field) -- nothing was written, the clone was repeated on float32 fields */
    int    new_size;                /* 1: this run built per-size state (multigrid hierarchy, transform or correction tables) */
    int    group_members;           /* sc_hip_run_device_batch: members of the last set of launches the call shared (0: none were shared) */
    int    group_ragged;            /* ... 1: those members had DIFFERENT ROI sizes (a size class, round 5): W, H above are the class's largest */
} sc_run_info;

/* ---- the reference's four entry points ------------------------------------------------- */

/* seamlessclone_cuda.h:23-38 / seamlessClone_imp.cu:239-263.  Selects `gpu_id` (the
 * reference only prints its properties), creates the stream and the grow-only arena.
 * Returns NULL on failure. */
SC_API void *my_seamlessclone_api_imp_create_instance(int gpu_id);

/* seamlessclone_cuda.h:6-21 / seamlessClone_imp.cu:265-352.
 * face = patch (CV_8UC3), body = destination (CV_8UC3, modified in place), mask (CV_8UC1,
 * same size as face).  Host pointers (pageable or page-locked).  The call completes before it
 * returns whatever bSync says, because the result has to land in caller memory (the reference
 * is synchronous here as well: D2H + host splice, seamlessClone_imp.cpp:471-483).  bSync = true
 * does what the reference's does (seamlessClone_imp.cu:310-349): the call is timed with events on
 * the instance's stream and prints the reference's two lines on stdout,
 *     "Compute stage performance time= %.3f msec, patch size=%dx%d" and "total device memory used: %d";
 * the reference's Python binding passes false (SeamlessClone.cpp:63), its CLI true (seamlessClone_main.cu:91).
 * The same time is in sc_run_info.ms_call either way.  Returns SC_OK or a negative SC_ERR_*. */
SC_API int my_seamlessclone_api_imp_run(void *instance,
                                 const uint8_t *face, int face_cols, int face_rows, int face_step,
                                 uint8_t *body, int body_cols, int body_rows, int body_step,
                                 const uint8_t *mask, int mask_cols, int mask_rows, int mask_step,
                                 int centerX, int centerY, int gpu_id, bool bSync);

/* seamlessclone_cuda.h:40-55 / seamlessClone_imp.cu:354-363 */
SC_API void my_seamlessclone_api_imp_destroy(void *instance);

/* seamlessclone_cuda.h:57-61 / seamlessClone_imp.cu:365-370 */
SC_API void my_seamlessclone_api_imp_sync(void *instance);

/* ---- additions ------------------------------------------------------------------------- */

SC_API void sc_hip_default_opts(sc_solver_opts *opts);
SC_API int  sc_hip_set_solver(void *instance, const sc_solver_opts *opts);
SC_API int  sc_hip_get_solver(void *instance, sc_solver_opts *opts);
SC_API int  sc_hip_get_info(void *instance, sc_run_info *info);
SC_API const char *sc_hip_last_error(void *instance);
/* Clone mode of the instance's next runs (single, device-resident and batch): SC_NORMAL_CLONE (the default), SC_MIXED_CLONE or
 * SC_MONOCHROME_TRANSFER; anything else is SC_ERR_BAD_ARG.  sc_hip_set_solver leaves it alone.  A mode other than NORMAL together
 * with SC_FLAG_OPENCV_GREY_MASK is not supported: such a run (each job of such a batch) returns SC_ERR_BAD_ARG.
 * sc_hip_get_clone_mode returns the mode, or SC_ERR_BAD_ARG for a bad instance. */
SC_API int  sc_hip_set_clone_mode(void *instance, int mode);
SC_API int  sc_hip_get_clone_mode(void *instance);

/* ---- whole-image gradient edits: OpenCV 3.4.5's other "Seamless Cloning" functions.  The domain is the whole image: the unknowns
 * are rows 1..rows-2 and columns 1..cols-2, dst's one-pixel frame is src's, and the change made inside the mask spreads, decaying,
 * into the rest of the image.  The mask (8-bit, one channel, the image's size; never written) is eroded by a 7 x 7 minimum filter
 * that ignores pixels outside the image and weights the patch field by M / 255 and src's own gradient by (255 - M) / 255, grey
 * masks included.  Inside it, per channel, the gradient P = (gx, gy) of src becomes
 *   COLOR_CHANGE         (P m) k, k = blue_mul, green_mul, red_mul for channels 0, 1, 2
 *   ILLUMINATION_CHANGE  (Q alpha^beta) |Q|^-beta with Q = P m (0 where that is NaN)
 *   TEXTURE_FLATTENING   P m at Canny edges of src (L1 gradient, aperture kernel_size, thresholds swapped when low > high), else 0
 * and the Poisson problem is solved with the instance's solver options (method, flags); the clone mode, reference_warmup and
 * SC_FLAG_OPENCV_GREY_MASK do not apply.  An empty mask is valid: dst = src within the solve's rounding.  PARITY UNPINNED: checked
 * against a restatement of that arithmetic (tests/photo_edits_np.py), not against OpenCV.
 * SC_ERR_BAD_ARG: a bad op, a NULL pointer, a non-finite parameter the op uses, kernel_size not 3, 5 or 7.  SC_ERR_BAD_SIZE: an image
 * smaller than 3 x 3 or a row step smaller than its row.  Only the cols * 3 bytes of each dst row are written; dst may equal src.
 * sc_run_info: x0 = y0 = ltx = lty = 0, W x H = the image, the method, field_retry, and (host call, or bSync) the stage times:
 * ms_mask = erode + Canny.  Many images at once: sc_hip_edit_device_batch and sc_hip_pool_edit below. */
#define SC_EDIT_COLOR_CHANGE        1   /* cv::colorChange        */
#define SC_EDIT_ILLUMINATION_CHANGE 2   /* cv::illuminationChange */
#define SC_EDIT_TEXTURE_FLATTENING  3   /* cv::textureFlattening  */
typedef struct sc_edit_params {
    int   op;
    float red_mul, green_mul, blue_mul;     /* COLOR_CHANGE                   */
    float alpha, beta;                      /* ILLUMINATION_CHANGE            */
    float low_threshold, high_threshold;    /* TEXTURE_FLATTENING             */
    int   kernel_size;                      /* TEXTURE_FLATTENING: 3, 5 or 7  */
} sc_edit_params;
SC_API void sc_hip_default_edit_params(sc_edit_params *p, int op);   /* OpenCV's defaults */
SC_API int  sc_hip_edit(void *instance, const sc_edit_params *p,
                        const uint8_t *src, int cols, int rows, int src_step,
                        const uint8_t *mask, int mask_step,
                        uint8_t *dst, int dst_step);                 /* host images; dst may equal src */
SC_API int  sc_hip_edit_device(void *instance, const sc_edit_params *p,
                        const uint8_t *d_src, int cols, int rows, int src_step,
                        const uint8_t *d_mask, int mask_step,
                        uint8_t *d_dst, int dst_step, bool bSync);

/* Same as run(), but face/body/mask are DEVICE pointers on the instance's GPU (inputs
 * resident in HBM); body is updated in place on the device.  Asynchronous on the instance
 * stream unless bSync. */
SC_API int sc_hip_run_device(void *instance,
                      const uint8_t *d_face, int face_cols, int face_rows, int face_step,
                      uint8_t *d_body, int body_cols, int body_rows, int body_step,
                      const uint8_t *d_mask, int mask_cols, int mask_rows, int mask_step,
                      int centerX, int centerY, bool bSync);

/* plain device-memory helpers so non-HIP hosts (ctypes, cgo, JNI) can stage images */
SC_API void *sc_hip_malloc(void *instance, size_t bytes);
SC_API void  sc_hip_free(void *instance, void *dptr);
SC_API int   sc_hip_memcpy_h2d(void *instance, void *dptr, const void *hptr, size_t bytes);
SC_API int   sc_hip_memcpy_d2h(void *instance, void *hptr, const void *dptr, size_t bytes);
SC_API int   sc_hip_memcpy_d2d_async(void *instance, void *dst, const void *src, size_t bytes); /* on the instance stream */
SC_API int   sc_hip_device_count(void);
/* PCI address of HIP device `gpu_id` as "dddd:bb:dd.f" (what /sys/bus/pci/devices/ is keyed by: a host that pins its threads to
 * the cores local to a GPU reads <that directory>/local_cpulist).  Returns SC_OK, or SC_ERR_BAD_ARG / SC_ERR_HIP with buf[0] = 0. */
SC_API int   sc_hip_device_pci_bus_id(int gpu_id, char *buf, int len);
/* page-locked host memory for callers that want their images DMA-able in place (run() copies a page-locked image
 * whose row step equals the library's device pitch without staging; every other host image is packed first) */
SC_API void *sc_hip_host_alloc(void *instance, size_t bytes);
SC_API void  sc_hip_host_free(void *instance, void *hptr);

/* ---- native batch driver: K instances (HIP streams) on one GPU, one host thread each ----------
 * Clones are independent; several in flight hide one another's latency-bound phases.  Jobs are
 * pulled from a shared counter, each runs exactly once, sc_hip_pool_run returns when all are done. */
typedef struct sc_batch_job {
    const uint8_t *face; int face_cols, face_rows, face_step;
    uint8_t *body;       int body_cols, body_rows, body_step;
    const uint8_t *mask; int mask_cols, mask_rows, mask_step;
    int centerX, centerY;
    const uint8_t *body_restore;   /* device-resident batches only: if non-NULL, body is refreshed from this device image
                                      (body_step * body_rows bytes) as part of the clone: after the call's work body holds
                                      those bytes with the clone's result in the ROI interior.  A group copies only what
                                      its clone does not write and reads the ROI's pixels from this image, so it must stay
                                      valid and unchanged until the call's work has finished (the instance's sync) */
    int rc;                        /* out: SC_OK or SC_ERR_* of this job */
} sc_batch_job;
/* n device-resident clones on ONE instance.  Members whose ROIs have the same size (W x H; masks, positions and
 * images are free) are solved as one field of 3n channels: every solver launch is n times larger and there is one
 * set of launches for the group, which is what fills a 256-CU GPU with small and medium ROIs.  Results are the ones the
 * clones get one by one (channels never interact), except that the stop rule sees the group's largest correction, so
 * every member gets the cycle count of the slowest.  The group is launched on predicted bounding boxes (the masks'
 * interiors); a member whose box turns out different is left untouched by the group and repeated alone.
 * Round 5: the members of a call are PARTITIONED -- same-size members share launches as above; members of one SIZE CLASS
 * (different sizes whose solves are the same program: same hierarchy depth and bottom solve, widths and heights within 2x of
 * each other; default solver options) share them through a per-member geometry table the kernels read (csrc/sc_ragged.cpp),
 * each member with the bytes of its solo run; what fits neither (and a failing member) runs alone.  jobs[i].rc receives each
 * clone's code; the call is asynchronous like sc_hip_run_device(..., false): sync the instance before reading bodies. */
SC_API int   sc_hip_run_device_batch(void *instance, sc_batch_job *jobs, int n);
SC_API void *sc_hip_pool_create(int gpu_id, int streams);
SC_API void  sc_hip_pool_destroy(void *pool);
SC_API int   sc_hip_pool_size(void *pool);
SC_API void *sc_hip_pool_instance(void *pool, int k);          /* instance k, e.g. for sc_hip_get_info */
SC_API int   sc_hip_pool_set_solver(void *pool, const sc_solver_opts *opts);
SC_API int   sc_hip_pool_set_clone_mode(void *pool, int mode);  /* sc_hip_set_clone_mode on every instance of the pool (between batches) */
SC_API int   sc_hip_pool_run(void *pool, sc_batch_job *jobs, int n, int device_resident);
/* device-resident batches: every worker takes up to `group` jobs at a time -- the batch's jobs bucketed by ROI size: same-size
 * jobs and jobs of one size class -- and runs them through sc_hip_run_device_batch (default 1 = one clone per set of launches; at most 64).
 * SC_POOL_GROUP_AUTO: sixteen at least where the batch has them, more for small ROIs -- up to half the batch (two groups at a time
 * are what pays: more streams launching small kernels at once only contend) and 64, while a group's fields stay within what sixteen 2048 x 2048 members occupy (small clones are latency bound:
 * 64 clones of 120..190 pixels take 0.43 ms in two groups of 32, 0.64 in four of 16) */
#define SC_POOL_GROUP_AUTO 0
SC_API int   sc_hip_pool_set_group(void *pool, int group);

/* Host-only (needs no GPU): how sc_hip_run_device_batch / the pool would partition a batch whose members have these ROI sizes
 * (wh[2i], wh[2i+1]: width and height, ring included) under `opts` (NULL: the defaults), at most `cap` members per group (<= 0: no
 * limit): group_of[i] = the member's group, kind_of[i] (may be NULL) = 0 alone, 1 a same-size group, 2 a size class (different
 * sizes, the same solve: csrc/sc_ragged.cpp; the member's bytes are those of its solo run), 3 a size class on another hierarchy than
 * the member's solo run takes (a small ROI, or the leftover of a class moved onto the next deeper one: within one grey level of the
 * solo run).  Returns the number of groups, or SC_ERR_BAD_ARG. */
SC_API int sc_hip_plan_groups(const int *wh, int n, int cap, const sc_solver_opts *opts, int *group_of, int *kind_of);
/* ... and how sc_hip_pool_run would: a pool of `streams` workers with group size `group` (SC_POOL_GROUP_AUTO allowed), jobs handed
 * to the planner largest first */
SC_API int sc_hip_plan_groups_pool(const int *wh, int n, int group, int streams, const sc_solver_opts *opts, int *group_of, int *kind_of);

/* ---- batches of whole-image edits ---------------------------------------------------------------------------------------------
 * ONE op and ONE parameter set per call: every job of a call shares *p; each job has its own image, mask and destination (one mask
 * shared by every job is allowed).  Each job means what sc_hip_edit_device means on it, with the instance's solver options: the
 * whole image is the domain, dst's frame is src's, the caller's mask is never written.
 * Aliasing: a job's dst may equal its own src; no job's dst may overlap another job's src, mask or dst; jobs may read one src or mask.
 * Partitioning: jobs with the same cols x rows are solved as ONE field of 3n channels (erode, Canny, pre- and post-process one launch
 * per 16 members, one set of solver launches for the group); a job whose size no other job shares runs alone through the
 * single-image path.  Group members get the multigrid answer (SC_METHOD_AUTO resolves to it for a group), and the stop rule sees the
 * group's largest correction: a member equals its solo SC_METHOD_MULTIGRID run byte for byte when the cycle counts agree, and is within
 * one grey level of it otherwise.
 * Errors: a job that does not validate (the codes of sc_hip_edit_device) gets its own code in rc and is skipped, the others run; a group
 * that fails other than with SC_ERR_HIP runs its members alone.  The return value is the worst code (SC_ERR_NOT_CONVERGED only when
 * nothing worse happened).  A HIP error ends the call: every job that validated then reads SC_ERR_HIP, the ones already run included
 * (their work was on the failed stream).  A saturated 16-bit field repeats the whole group on float fields (sc_run_info.field_retry).
 * Asynchronous like sc_hip_run_device_batch (sync the instance before reading destinations), except that TEXTURE_FLATTENING waits on
 * the host once per batch of hysteresis launches, for the whole group at once.  sc_run_info afterwards: the last group's (group_members,
 * W x H = the image), or the last job's when no group was formed; no stage times. */
typedef struct sc_edit_job {
    const uint8_t *src;  int cols, rows, src_step;   /* 8-bit BGR */
    const uint8_t *mask; int mask_step;              /* 8-bit, one channel, cols x rows */
    uint8_t *dst;        int dst_step;               /* may equal src (in place) */
    int rc;                                          /* out: SC_OK or SC_ERR_* of this job */
} sc_edit_job;
SC_API int sc_hip_edit_device_batch(void *instance, const sc_edit_params *p, sc_edit_job *jobs, int n);
/* The pool's form.  device_resident: the jobs are bucketed by image size and cut into chunks of sc_hip_pool_set_group's size
 * (SC_POOL_GROUP_AUTO: the clone batches' rule, the image standing in for the ROI), largest images first; every worker takes a chunk at
 * a time through sc_hip_edit_device_batch (a chunk of one through sc_hip_edit_device).  Host images (device_resident = 0): one
 * sc_hip_edit per job on the worker's instance.  Returns when every job has completed: SC_OK, or the first failing job's code. */
SC_API int sc_hip_pool_edit(void *pool, const sc_edit_params *p, sc_edit_job *jobs, int n, int device_resident);
/* Host-only (needs no GPU): the chunks sc_hip_pool_edit would form for device-resident edits of these image sizes (wh[2i], wh[2i+1]) on
 * a pool of `streams` workers with group size `group` (SC_POOL_GROUP_AUTO allowed): group_of[i] = the job's chunk.  Returns the number
 * of chunks, or SC_ERR_BAD_ARG. */
SC_API int sc_hip_plan_edit_groups_pool(const int *wh, int n, int group, int streams, int *group_of);

/* ---- the Poisson solver on float32 images with caller guidance fields ------------------------------------------------------------
 * The problem (Perez et al.): the domain is the whole cols x rows rectangle, the unknowns are rows 1..rows-2, columns 1..cols-2, and
 * the call solves, per channel, the 5-point system the clone and edit paths solve:
 *     u(x-1,y) + u(x+1,y) + u(x,y-1) + u(x,y+1) - 4 u(x,y) = lap(x,y)       with u = boundary on the frame (Dirichlet).
 * SC_POISSON_GUIDANCE: lap(q) = (gx(q) - gx(q - x)) + (gy(q) - gy(q - y)), backward differences in float32, in this order (the edit
 * pre-process's formula).  Guidance made of forward differences of an image I, with I as the boundary, therefore gives back I.
 * SC_POISSON_LAPLACIAN: lap given directly (interior only; its frame is never read).
 * The answer is the exact system's: no float-table correction (that belongs to the reference's 8-bit answer; as with
 * SC_FLAG_EXACT_TABLES), and every field is float32 -- right-hand side, level 1, the field between level-0 launches (the 16-bit and
 * float16 forms of the clone path assume 8-bit data).  Nothing is clamped or rounded.
 * Solver options: the instance's sc_solver_opts apply except reference_warmup, the clone mode and SC_FLAG_OPENCV_GREY_MASK; p->tol
 * replaces update_tol for the call (in the data's units; <= 0: 1e-3), and a residual tol > 0 still stops on the residual.
 * SC_METHOD_AUTO resolves as for a single clone when n = 1 (whatever the channel count) and to SC_METHOD_MULTIGRID for n > 1.
 * The float32 floor: multigrid corrections settle at ~1e-8 x max|u| x sqrt(cols x rows), and the stop rule
 * fires once its predicted error is a tenth of tol -- a tol below ten times that floor ends with SC_ERR_NOT_CONVERGED after max_sweeps
 * cycles, the result then at the floor.  The default 1e-3 suits data of unit scale; 8-bit-range data at 1024^2 want ~0.1.
 * sc_run_info: method, cycles, converged, W x H = the image; stage times (ms_pre, ms_solve, ms_post) when bSync is set and for the
 * host call.  The instance's stored options are unchanged by the call.
 * Layout: ONE layout for every array of every job of a call.  Element (x, y, c) is at
 *     x * col_stride + y * row_stride + c * channel_stride   floats from the array's pointer.
 * Strides are positive and must nest: sorted by size (dimensions of extent 1 left out), each one exceeds the span of the smaller
 * ones, so no two elements share an offset.  HWC: (C, cols * C or more, 1); CHW: (1, cols or more, rows * row_stride or more);
 * RGBA-strided C = 3: (4, 4 * cols, 1).
 * Batches (sc_hip_poisson_device): all jobs have the layout's size and are solved as one field of n x channels planes, at most 192
 * planes per set of launches (floor(192 / channels) jobs per chunk).  Channels never interact: a member equals its solo
 * SC_METHOD_MULTIGRID run bit for bit when the cycle counts agree, and is within the stop rule's error otherwise.
 * Aliasing: a job's out may equal its own boundary; it must not overlap any other array of the call.  Inputs may be shared.
 * What a call writes: the cols x rows x channels elements of out the layout names (frame = boundary's, bit for bit).  Row padding,
 * unused channel slots (the 4th float of an RGBA-strided C = 3 layout) and memory outside the image are never written.
 * Codes: SC_ERR_BAD_ARG for a bad kind, a non-finite tol, channels outside 1..4, a stride <= 0 or strides that do not nest;
 * SC_ERR_BAD_SIZE for cols or rows < 3.  Per job (sc_poisson_job.rc; the job is skipped, the others run): SC_ERR_BAD_ARG for a NULL
 * pointer the kind needs or one that is not 4-byte aligned.  SC_ERR_NOT_CONVERGED: the budget ended first, the result is written.
 * The return value is the worst code, as in sc_hip_edit_device_batch; a HIP error marks every validated job SC_ERR_HIP.
 *
 * SC_POISSON_NEUMANN (or'ed into either kind): no boundary values are known.  All cols x rows pixels are unknowns, the stencil reflects
 * at the border, and the call solves per channel
 *     sum over the 2, 3 or 4 neighbours p of q inside the image of (u(p) - u(q)) = lap(q).
 * SC_POISSON_GUIDANCE: lap(q) = (a - b) + (c - d) in float32, a = gx(q) (0 in the last column), b = gx(q - x) (0 in column 0), c = gy(q)
 * (0 in the last row), d = gy(q - y) (0 in row 0): the normal equations of min sum (u(x+1,y) - u(x,y) - gx)^2 + (u(x,y+1) - u(x,y) - gy)^2.
 * Forward differences of an image give back the image up to a constant; gx's last column and gy's last row are never read.
 * SC_POISSON_LAPLACIAN: lap is read at EVERY pixel, frame included.  The system is solvable only for a lap of sum zero: the call
 * ignores lap's DC coefficient, i.e. it solves for lap - mean(lap).
 * The free constant: per channel mean(out) = mean(boundary) over the image's cols x rows elements (summed in double on the device);
 * boundary may be NULL: mean zero.  Nothing else of boundary is read.  out may equal boundary.
 * Solved directly by DCT-II transforms (the chirp convolution of SC_METHOD_FFT with a chirp of period 2n, exact eigenvalues in double,
 * the (0, 0) coefficient set to 0), in float32, or in double with SC_FLAG_FFT_FP64.  Methods: SC_METHOD_AUTO and SC_METHOD_FFT;
 * any other method: SC_ERR_BAD_ARG, nothing written (the multigrid and the relaxation solvers assume a zero ring on every level).
 * sc_run_info: method SC_METHOD_FFT, sweeps 1, converged 1; ms_pre = the boundary-mean reduction, ms_post ~ 0 (the last transform
 * launch stores into out).  tol is validated and otherwise unused.  Sizes: cols, rows >= 2; at most 8192 per side, 4096 with
 * SC_FLAG_FFT_FP64 (SC_ERR_BAD_SIZE beyond; sc_hip_poisson_check, which knows no instance, reports the 8192 limit).  Batches: one
 * field of n x channels planes in the same chunks; a member equals its solo run bit for bit, always.
 *
 * SC_POISSON_FREE_LEFT / _RIGHT / _TOP / _BOTTOM (or'ed into either kind): per-side free borders -- a region that touches the image
 * edge, a strip pinned at its two ends, a gradient field anchored on one side.  A side without its bit is a Dirichlet line: the whole
 * outermost row or column there, corners included, holds known values taken from boundary.  A side with its bit has no frame: its
 * outermost pixels are unknowns and the stencil lacks the neighbour beyond them (u(outside) = u(pixel)).  Unknowns per axis: pixels
 * less the axis's Dirichlet lines.  No bit: the Dirichlet call above, unchanged.  All four bits, with or without SC_POISSON_NEUMANN
 * (which stays the union with any of them): the Neumann call above, bit for bit.  The 14 combinations between:
 * SC_POISSON_GUIDANCE: lap(q) = (a - b) + (c - d) in float32, a = gx(q) (0 when q is in the last column and the right side is free),
 * b = gx(q - x) (0 when q is in column 0 and the left side is free), c and d likewise from gy with bottom and top: both formulas
 * above at the two extremes.  Forward differences of an image I, with I as boundary, give back I under every combination; gx's last
 * column and gy's last row are never read (along a non-periodic axis: see SC_POISSON_PERIODIC_* below).  SC_POISSON_LAPLACIAN: lap is
 * read at every unknown and nowhere else.  An unknown next to a Dirichlet line has that line's value subtracted from its right-hand side.
 * boundary: required as soon as one side is a Dirichlet line; only its Dirichlet lines are read (its interior and its lines on free
 * sides never).  The system is regular: no mean is taken, no constant is free.  out: boundary's values, bit for bit, on the Dirichlet
 * lines (corners where two meet included), the solution at every unknown; out may equal boundary.
 * Solved directly, each axis under the transform of its two ends: DST-I between two Dirichlet lines, DCT-II / III between two free
 * ends, and between a Dirichlet line and a free end the sine transform S[k][j] = sin(pi (2k+1) (j+1) / (2n+1)) (eigenvalues
 * 2 cos(pi (2k+1) / (2n+1)) - 2), all by the chirp convolution of SC_METHOD_FFT, the coefficients divided by the sum of the two
 * axes' eigenvalues in double; float32 transforms, or double with SC_FLAG_FFT_FP64.  Methods: SC_METHOD_AUTO (resolves to
 * SC_METHOD_FFT at every size and batch size) and SC_METHOD_FFT; any other method: SC_ERR_BAD_ARG, nothing written.  Sizes: cols,
 * rows >= 2, at least 1 and at most 8192 unknowns per axis, 4096 with SC_FLAG_FFT_FP64 (SC_ERR_BAD_SIZE beyond;
 * sc_hip_poisson_check reports the float32 limits).  tol is validated and otherwise unused.  sc_run_info and the stage times: the
 * Neumann call's, ms_pre and ms_post ~ 0.  Batches: the same chunks; a member equals its solo run bit for bit, always.
 * The lowest eigenvalue of an axis with one Dirichlet end is ~(pi / (2n+1))^2, a quarter of the Dirichlet axis's: long thin float32
 * problems pinned at one far end lose accuracy sooner than either other kind.
 *
 * SC_POISSON_PERIODIC_X / _Y (or'ed into either kind): an axis that wraps -- a 360-degree panorama (x), a tileable texture (both), any
 * field on a cylinder or torus.  A periodic axis has no Dirichlet line and no frame: all its pixels are unknowns, and the stencil's
 * neighbour beyond either end is the pixel at the other end (at length 2 the two neighbours are the same pixel, counted twice).  The
 * other axis keeps whatever its own two SC_POISSON_FREE_* bits say, or is periodic too: nine combinations beside the sixteen above.
 * SC_ERR_BAD_ARG, nothing written: SC_POISSON_PERIODIC_X with SC_POISSON_FREE_LEFT or _RIGHT, SC_POISSON_PERIODIC_Y with
 * SC_POISSON_FREE_TOP or _BOTTOM, either bit with SC_POISSON_NEUMANN or without a base kind.
 * SC_POISSON_GUIDANCE: lap(q) = (a - b) + (c - d) in float32 as above; along a periodic x, a = gx(q) at EVERY column -- in the last one
 * gx is the difference from the last pixel to the first -- and b = gx(q - x), which is gx of the last column when q is in column 0;
 * likewise gy along a periodic y.  So every column of gx is read under SC_POISSON_PERIODIC_X, every row of gy under _Y.  Wrapped
 * forward differences of an image I give back I: exactly, with I as boundary, where some side is a Dirichlet line, and up to the free
 * constant below where none is.  SC_POISSON_LAPLACIAN: lap is read at every unknown and nowhere else.
 * No Dirichlet line on either axis -- both periodic, or one periodic and the other free at both ends --: the unscreened system is
 * singular and behaves as the Neumann call does: lap's DC coefficient is ignored and per channel mean(out) = mean(boundary) over all
 * cols x rows elements (summed in double on the device); boundary may be NULL (mean zero), nothing else of it is read.  Otherwise
 * boundary is required and read on the remaining Dirichlet lines only, which span the whole periodic extent (with a periodic x the
 * top line is all cols pixels: there are no corners to share) and are copied to out bit for bit.
 * Solved directly like the free sides, a periodic axis under the discrete Hartley transform H[k][j] = cos(2 pi jk/n) + sin(2 pi jk/n)
 * (real and symmetric, H H = n I, eigenvalues 2 cos(2 pi k/n) - 2) by the same chirp convolution.  Methods, batches, aliasing, codes,
 * sc_run_info and stage times: the free sides' (singular: ms_pre = the boundary-mean reduction).  Sizes: 2 .. 8192 pixels along a
 * periodic axis, 4096 with SC_FLAG_FFT_FP64 (SC_ERR_BAD_SIZE outside; sc_hip_poisson_check reports the float32 limits). */
#define SC_POISSON_GUIDANCE  1   /* gx, gy given (gx read at columns 0..cols-2, gy at rows 0..rows-2; every column / row along a periodic axis) */
#define SC_POISSON_LAPLACIAN 2   /* lap given                                                          */
#define SC_POISSON_NEUMANN   (1 << 8)   /* or'ed into SC_POISSON_GUIDANCE / SC_POISSON_LAPLACIAN: reflecting border, no Dirichlet frame */
/* or'ed into either kind: that side has no Dirichlet line -- its outermost pixels are unknowns and the stencil reflects there.  All four
 * are SC_POISSON_NEUMANN.  (Bits 9..11 are not kinds.) */
#define SC_POISSON_FREE_LEFT   (1 << 12)   /* column 0        */
#define SC_POISSON_FREE_RIGHT  (1 << 13)   /* column cols - 1 */
#define SC_POISSON_FREE_TOP    (1 << 14)   /* row 0           */
#define SC_POISSON_FREE_BOTTOM (1 << 15)   /* row rows - 1    */
/* or'ed into either kind: that axis wraps.  (Bit 16 is not a kind.) */
#define SC_POISSON_PERIODIC_X  (1 << 17)   /* column cols-1 is column 0's left neighbour */
#define SC_POISSON_PERIODIC_Y  (1 << 18)   /* row rows-1 is row 0's upper neighbour      */
#define SC_POISSON_MAX_PLANES 192
typedef struct sc_poisson_layout {
    int cols, rows, channels;                            /* >= 3, >= 3 (SC_POISSON_NEUMANN: >= 2, <= 8192; SC_POISSON_FREE_*, SC_POISSON_PERIODIC_*: >= 2, unknowns per axis as above), 1..4 */
    long long col_stride, row_stride, channel_stride;    /* in floats                         */
} sc_poisson_layout;
typedef struct sc_poisson_params {
    int kind;                /* SC_POISSON_GUIDANCE or SC_POISSON_LAPLACIAN, alone or with SC_POISSON_NEUMANN, SC_POISSON_FREE_* or SC_POISSON_PERIODIC_* bits */
    float tol;               /* the multigrid stop rule's update_tol for this call, in the data's units; <= 0: 1e-3 */
} sc_poisson_params;
typedef struct sc_poisson_job {
    const float *gx, *gy;    /* SC_POISSON_GUIDANCE                                                           */
    const float *lap;        /* SC_POISSON_LAPLACIAN                                                          */
    const float *boundary;   /* its frame: the Dirichlet values; its interior: the initial guess of the iterative methods (SC_POISSON_NEUMANN: only its mean; may be NULL) */
    float *out;              /* every element the layout names is written; may equal boundary                  */
    int rc;                  /* out: SC_OK or SC_ERR_* of this job                                            */
} sc_poisson_job;
/* Host-only (needs no GPU): SC_OK, or the code a call with these parameters and this layout returns before it runs anything. */
SC_API int sc_hip_poisson_check(const sc_poisson_params *p, const sc_poisson_layout *l);
/* Device pointers.  Asynchronous unless bSync (sync the instance before reading out); bSync also records the stage times. */
SC_API int sc_hip_poisson_device(void *instance, const sc_poisson_params *p, const sc_poisson_layout *l, sc_poisson_job *jobs, int n,
                                 bool bSync);
/* One problem on host arrays: the span each array occupies under the layout (offsets 0 .. the largest) goes in and out through the
 * instance's pinned staging, and only the named elements of out are written.  Synchronous, like sc_hip_edit.  The arrays the kind
 * does not use may be NULL. */
SC_API int sc_hip_poisson(void *instance, const sc_poisson_params *p, const sc_poisson_layout *l, const float *gx, const float *gy,
                          const float *lap, const float *boundary, float *out);
/* ---- screened Poisson solves: the same solver with a data term -------------------------------------------------------------------
 * The problem: per channel,
 *     minimise   lambda sum (u - d)^2 + sum |grad u - g|^2       i.e.       (A - lambda) u = div g - lambda d,      lambda > 0,
 * A the 5-point operator of sc_hip_poisson under the same two boundary kinds: the solver of gradient-domain filtering (sharpen or
 * flatten gradients while staying close to the input), deblocking and reconstruction with a fidelity term.
 * kind: as sc_poisson_params.kind.  SC_POISSON_GUIDANCE forms lap = div g by the documented formula of the boundary kind, in the
 * same float32 order; SC_POISSON_LAPLACIAN takes it as given.  The right-hand side is lap - lambda * d in float32: one multiply
 * (lambda * d, rounded), then one subtract -- never a fused multiply-add.
 * Dirichlet (no SC_POISSON_NEUMANN): the unknowns are the interior, u = boundary on the frame.  data and lap are read on the interior
 * only, boundary on its frame only (its interior is never read: there is no iteration to start).  The frame of out is boundary's,
 * bit for bit.  boundary may be the data array itself.
 * SC_POISSON_NEUMANN: every pixel is an unknown, the stencil reflects at the border; data and lap (or the guidance) are read at every
 * pixel; boundary is not used and may be NULL.  The screened system is regular: there is no free constant, no mean is asked for,
 * lap's DC coefficient counts like any other (it is divided by -lambda).
 * Solved directly, always: DST-I transforms under a frame, DCT-II / DCT-III under SC_POISSON_NEUMANN (the chirp convolutions of
 * SC_METHOD_FFT), the coefficients divided by eigenvalue - lambda computed in double; float32 transforms, or double with
 * SC_FLAG_FFT_FP64.  Methods: SC_METHOD_AUTO (resolves to SC_METHOD_FFT at every size and batch size) and SC_METHOD_FFT; any other
 * method: SC_ERR_BAD_ARG, nothing written (the multigrid and relaxation kernels hold the unscreened diagonal).  Of the instance's other
 * options only SC_FLAG_FFT_FP64 matters.  Sizes: SC_POISSON_NEUMANN cols, rows in 2..8192 (4096 with SC_FLAG_FFT_FP64); under a
 * frame cols, rows >= 3 and at most 8192 unknowns per side, i.e. cols - 2, rows - 2 <= 8192 (4096 with SC_FLAG_FFT_FP64);
 * SC_ERR_BAD_SIZE beyond (sc_hip_screened_check, which knows no instance, reports the float32 limits).
 * Layout, batches (one field of n x channels planes, floor(192 / channels) jobs per chunk), what a call writes, the return value and
 * the per-job codes: sc_hip_poisson_device's.  A member equals its solo run bit for bit, always.  Aliasing: a job's out may equal
 * its own data or boundary; it must not overlap any other array of the call.  Inputs may be shared.
 * Codes: SC_ERR_BAD_ARG for a lambda that is not finite or is <= 0, a bad kind, channels outside 1..4, a stride <= 0 or strides that
 * do not nest; SC_ERR_BAD_SIZE as above.  Per job (the job is skipped, the others run): SC_ERR_BAD_ARG for a NULL or misaligned
 * pointer the kind needs -- data always, boundary under a frame.
 * sc_run_info: method SC_METHOD_FFT, sweeps 1, converged 1, W x H = the image; stage times when bSync is set and for the host call
 * (under a frame ms_pre = the pre-process, ms_post = the output launch; SC_POISSON_NEUMANN: both ~ 0, the transform launches read
 * and write the caller's arrays).  The instance's stored options are unchanged by the call.
 * SC_POISSON_FREE_* bits: the same per-side borders as in sc_hip_poisson, the denominators shifted by -lambda; data and lap (or the
 * guidance) are read at every unknown, boundary on its Dirichlet lines only and required if and only if some side is one; sizes, methods
 * and stage times as there.
 * SC_POISSON_PERIODIC_* bits: the same wrapping axes as in sc_hip_poisson.  The screened system is never singular: without any
 * Dirichlet line boundary is unused and may be NULL, and coefficient (0, 0) is divided by -lambda like any other. */
typedef struct sc_screened_params {
    int kind;                /* as sc_poisson_params.kind, SC_POISSON_NEUMANN included */
    float lambda;            /* the data term's weight: finite, > 0 */
} sc_screened_params;
typedef struct sc_screened_job {
    const float *gx, *gy;    /* SC_POISSON_GUIDANCE                                                           */
    const float *lap;        /* SC_POISSON_LAPLACIAN                                                          */
    const float *data;       /* d: read on the interior (SC_POISSON_NEUMANN: at every pixel)                  */
    const float *boundary;   /* its frame: the Dirichlet values, its interior is never read (SC_POISSON_NEUMANN: unused, may be NULL) */
    float *out;              /* every element the layout names is written; may equal data or boundary          */
    int rc;                  /* out: SC_OK or SC_ERR_* of this job                                            */
} sc_screened_job;
/* Host-only (needs no GPU): SC_OK, or the code a call with these parameters and this layout returns before it runs anything. */
SC_API int sc_hip_screened_check(const sc_screened_params *p, const sc_poisson_layout *l);
/* Device pointers.  Asynchronous unless bSync (sync the instance before reading out); bSync also records the stage times. */
SC_API int sc_hip_screened_device(void *instance, const sc_screened_params *p, const sc_poisson_layout *l, sc_screened_job *jobs, int n,
                                  bool bSync);
/* One problem on host arrays, as sc_hip_poisson: spans in and out through pinned staging, only the named elements of out written. */
SC_API int sc_hip_screened(void *instance, const sc_screened_params *p, const sc_poisson_layout *l, const float *gx, const float *gy,
                           const float *lap, const float *data, const float *boundary, float *out);
/* ---- weighted solves: a data term whose weight varies from pixel to pixel ---------------------------------------------------------
 * The problem: per channel,
 *     minimise   sum_q w(q) (u(q) - d(q))^2 + sum |grad u - g|^2       i.e.       (A - W) u = div g - W d,      W = diag(w), w >= 0,
 * A the 5-point operator of sc_hip_poisson under the same border kinds: scattered or scribbled constraints (w > 0 at a few pixels),
 * confidence-weighted reconstruction, soft regions of any shape (a large w pins u to d), the inner step of reweighted solves.
 * kind, layout, chunks of at most 192 planes, what a call writes, aliasing and the per-job codes: sc_hip_screened_device's.  weight is
 * read like data: at every unknown, under the call's layout, per channel; it must not overlap out.  The right-hand side is lap - w * d
 * in float32, one rounded multiply, then one subtract, as the screened call forms lap - lambda * d.  boundary is read on Dirichlet lines
 * only and copied to out bit for bit.
 * Solved by conjugate gradients on the device, preconditioned by the screened direct solve with the constant lambda-bar = precond_lambda,
 * or the mean of w over the unknowns of the call's chunk (a constant w converges in one iteration, random weights
 * over two decades in about ten, a half-plane of zero weight in tens).  The vectors are float32, every dot product is summed in double
 * in one fixed order: two runs of one call give the same bytes.  SC_FLAG_FFT_FP64: the preconditioner's transforms in double.
 * Methods: SC_METHOD_AUTO and SC_METHOD_FFT; sizes: the direct solves' limits, a Dirichlet frame on all four sides included.
 * Stop rule: ||r||_2 <= tol ||b||_2 on every plane of the chunk, r the iteration's own residual.  The norms of iteration k reach the
 * host SC_WEIGHTED_POLL iterations later (a pinned mailbox and an event per iteration, so the stream never waits for the host): a call
 * runs up to SC_WEIGHTED_POLL iterations past the one that met tol, and writes its last iterate.  SC_ERR_NOT_CONVERGED when max_iters
 * ends first: the last iterate is written -- of all iterates the one with the smallest error in the energy norm.
 * Host waits: one for the weights' statistics (their mean and validity, per chunk), the stop rule's reads, and one for the last
 * iteration's norms; the output launch behind them is asynchronous unless bSync.
 * Batches: every plane has its own alpha, beta and norms, but the stop is joint and the automatic lambda-bar is the chunk's: a member
 * agrees with its solo run to the stop rule's error, not bit for bit.
 * Codes: SC_ERR_BAD_ARG for a non-finite tol or precond_lambda, a method other than AUTO or FFT, a bad kind or layout (the screened
 * call's); per job SC_ERR_BAD_ARG for a NULL or misaligned pointer the kind needs (weight and data always), for a weight that is negative
 * or not finite anywhere in the job, and, in a call without any Dirichlet line, for a channel whose weights are all zero ("no data
 * weight and no Dirichlet line": the system is singular) -- nothing of such a job is written, the others run.
 * sc_run_info: method SC_METHOD_FFT, sweeps = iterations, converged, rel_residual = the worst plane's final ||r|| / ||b||, W x H = the
 * image (the last chunk's figures); ms_solve = ms_call = the call's stream time when bSync is set and for the host call. */
#define SC_WEIGHTED_POLL 4   /* iterations between an iteration and the host's read of its norms */
typedef struct sc_weighted_params {
    int   kind;              /* as sc_screened_params.kind: base kind | NEUMANN | FREE_* | PERIODIC_* */
    float tol;               /* stop when ||r||_2 <= tol * ||b||_2 on every plane; <= 0: 1e-5 */
    int   max_iters;         /* <= 0: 200 */
    float precond_lambda;    /* the constant of the preconditioner (A - lambda); <= 0: the mean of w over the unknowns of the call's chunk */
} sc_weighted_params;
typedef struct sc_weighted_job {
    const float *gx, *gy;    /* SC_POISSON_GUIDANCE */
    const float *lap;        /* SC_POISSON_LAPLACIAN */
    const float *data;       /* d: read at every unknown */
    const float *weight;     /* w >= 0: read at every unknown */
    const float *boundary;   /* its Dirichlet lines (no Dirichlet line on any side: unused, may be NULL) */
    float *out;              /* every element the layout names is written; may equal data or boundary */
    int rc;                  /* out: SC_OK or SC_ERR_* of this job */
} sc_weighted_job;
/* Host-only (needs no GPU): SC_OK, or the code a call with these parameters and this layout returns before it runs anything. */
SC_API int sc_hip_weighted_check(const sc_weighted_params *p, const sc_poisson_layout *l);
/* Device pointers.  bSync: waits for the stream and records the call's time. */
SC_API int sc_hip_weighted_device(void *instance, const sc_weighted_params *p, const sc_poisson_layout *l, sc_weighted_job *jobs, int n,
                                  bool bSync);
/* One problem on host arrays, as sc_hip_screened: spans in and out through pinned staging, only the named elements of out written. */
SC_API int sc_hip_weighted(void *instance, const sc_weighted_params *p, const sc_poisson_layout *l, const float *gx, const float *gy,
                           const float *lap, const float *data, const float *weight, const float *boundary, float *out);
/* ---- WLS solves: per-link smoothness weights on the gradient term -------------------------------------------------------------------
 * The problem: per channel,
 *     minimise   sum_p w(p) (u(p) - d(p))^2  +  sum_x-links sx (u(x+1,y) - u(x,y) - gx)^2  +  sum_y-links sy (u(x,y+1) - u(x,y) - gy)^2
 * i.e. at every unknown p
 *     sum_q s(p,q) (u(q) - u(p)) - w(p) u(p)  =  div(s g)(p) - w(p) d(p),
 *     div(s g)(x,y) = sx(x,y) gx(x,y) - sx(x-1,y) gx(x-1,y) + sy(x,y) gy(x,y) - sy(x,y-1) gy(x,y-1),
 * the sum over the neighbours q that exist under the call's border kind -- the weighted-least-squares operator of edge-preserving
 * smoothing and base / detail decomposition, colourisation and scribble propagation that stops at image edges, guided upsampling of
 * depth or flow, and the inner step of reweighted (robust, TV-like) gradient solves.  With every link 1 it is sc_hip_weighted's problem.
 * kind, layout, chunks of at most 192 planes, what a call writes, aliasing of out with data or boundary: sc_hip_weighted_device's.
 * Links: smooth_x(x,y) is the weight of the link between pixels (x,y) and (x+1,y), smooth_y(x,y) that of (x,y) - (x,y+1), both under
 * the call's layout, per channel, like weight.  A link is LIVE when at least one of its ends is an unknown.  Along a periodic axis the
 * element in the last column of smooth_x (last row of smooth_y) is the link from the last pixel to the first, as for gx / gy; otherwise
 * that element is not live.  A link between two pixels of one Dirichlet line is not live.  Elements that are not live are never
 * read.  A live link to a Dirichlet pixel q adds s to the diagonal at its unknown end and s * boundary(q) to the right-hand side.
 * Every live link must be finite and > 0 (a zero would cut the graph and can leave a part of it singular); weight >= 0 as in the
 * weighted call.  smooth_x, smooth_y and weight must not overlap out: a job in which the span of one of them under the layout (offsets
 * 0 .. the largest) shares a float with out's span is refused.
 * The right-hand side, in float32, in this order:  with SC_POISSON_LAPLACIAN lap is taken as div(s g), already weighted, and gx, gy
 * are unused; with SC_POISSON_GUIDANCE each product s * g is rounded on its own (never fused into the difference), the differences are
 * taken as sc_hip_poisson's reflecting and periodic kinds take them, (a - b) + (c - d) with a = sx(x,y) gx(x,y), b = sx(x-1,y) gx(x-1,y),
 * c = sy(x,y) gy(x,y), d = sy(x,y-1) gy(x,y-1), a term whose link does not exist counting 0 and column / row 0 of a periodic axis
 * taking the last column / row as its backward term.  Then - w * d: one rounded multiply, one subtract, as in the weighted call.  Then
 * the Dirichlet terms, each a rounded product s * boundary subtracted in turn: west, north, east, south.
 * Solved by the weighted call's conjugate gradients -- float32 vectors, every dot product summed in double in one fixed order (two runs
 * of one call give the same bytes), the stop rule ||r||_2 <= tol ||b||_2 on every plane of the chunk read SC_WEIGHTED_POLL iterations
 * late, SC_ERR_NOT_CONVERGED with the last iterate written when max_iters ends first -- preconditioned by M = s-bar (A - w-bar / s-bar),
 * A the constant-coefficient operator of the border kind through the direct solve: s-bar = precond_smooth, or the arithmetic mean of the
 * live links of the call's chunk; w-bar = precond_lambda, or the mean of w over its unknowns.  Constant links c and a constant weight
 * need no iteration; under a constant weight random links over two decades take about twenty and a contrast of 100 across image edges
 * about fifty; a data weight that varies as well adds to that (43 and 56 at 1024 x 1024 with w log-uniform over two decades), sparse
 * data weights can take a hundred or more (DESIGN.md sections 4 and 7).  SC_FLAG_FFT_FP64: the preconditioner's transforms in double.
 * Methods, sizes, batches (one joint stop, the chunk's s-bar and w-bar: a member agrees with its solo run to the stop rule's error, not
 * bit for bit), host waits and sc_run_info: the weighted call's.  rel_residual is the last iterate's: under strongly varying links the
 * residual of conjugate gradients is not monotone (the error in the energy norm is), so after the up to SC_WEIGHTED_POLL iterations
 * past the one that met tol it may lie somewhat above tol in a call that converged.
 * Codes: SC_ERR_BAD_ARG for a non-finite tol, precond_lambda or precond_smooth, a method other than AUTO or FFT, a bad kind or layout;
 * SC_ERR_BAD_SIZE as the weighted call.  Per job SC_ERR_BAD_ARG for a NULL or misaligned pointer the kind needs (data, weight, smooth_x
 * and smooth_y always), for smooth_x, smooth_y or weight overlapping out, for a weight that is negative or not finite, for a live link
 * that is not finite or not > 0 and, without any Dirichlet line, for a channel whose weights are all zero -- nothing of such a job is
 * written, the others run. */
typedef struct sc_wls_params {
    int   kind;              /* as sc_weighted_params.kind */
    float tol;               /* stop when ||r||_2 <= tol * ||b||_2 on every plane; <= 0: 1e-5 */
    int   max_iters;         /* <= 0: 400 */
    float precond_lambda;    /* w-bar of the preconditioner; <= 0: the mean of w over the unknowns of the call's chunk */
    float precond_smooth;    /* s-bar of the preconditioner; <= 0: the mean of the live links of the call's chunk */
} sc_wls_params;
typedef struct sc_wls_job {
    const float *gx, *gy;    /* SC_POISSON_GUIDANCE */
    const float *lap;        /* SC_POISSON_LAPLACIAN: div(s g), already weighted */
    const float *data;       /* d: read at every unknown */
    const float *weight;     /* w >= 0: read at every unknown */
    const float *smooth_x;   /* > 0: the link (x,y) - (x+1,y); live links only are read */
    const float *smooth_y;   /* > 0: the link (x,y) - (x,y+1); live links only are read */
    const float *boundary;   /* its Dirichlet lines (no Dirichlet line on any side: unused, may be NULL) */
    float *out;              /* every element the layout names is written; may equal data or boundary */
    int rc;                  /* out: SC_OK or SC_ERR_* of this job */
} sc_wls_job;
/* Host-only (needs no GPU): SC_OK, or the code a call with these parameters and this layout returns before it runs anything. */
SC_API int sc_hip_wls_check(const sc_wls_params *p, const sc_poisson_layout *l);
/* Device pointers.  bSync: waits for the stream and records the call's time. */
SC_API int sc_hip_wls_device(void *instance, const sc_wls_params *p, const sc_poisson_layout *l, sc_wls_job *jobs, int n, bool bSync);
/* One problem on host arrays, as sc_hip_weighted: spans in and out through pinned staging, only the named elements of out written. */
SC_API int sc_hip_wls(void *instance, const sc_wls_params *p, const sc_poisson_layout *l, const float *gx, const float *gy,
                      const float *lap, const float *data, const float *weight, const float *smooth_x, const float *smooth_y,
                      const float *boundary, float *out);
/* ---- robust solves: Lp penalties on the gradient and on the data term, by reweighting on the device -----------------------------------
 * The problem: per channel, with exponents 0 < p <= 2 on the gradient term and 0 < q <= 2 on the data term,
 *     minimise   sum_p w(p) phi_q(u(p) - d(p); eps_d)  +  sum_x-links c_x phi_p(u(x+1,y) - u(x,y) - gx; eps_g)
 *                                                      +  sum_y-links c_y phi_p(u(x,y+1) - u(x,y) - gy; eps_g),
 *     phi_r(t; eps) = (2 / r) (t^2 + eps^2)^(r/2)      (r = 2: t^2, eps is not used),
 * under every border kind of sc_hip_wls -- integrating gradient fields with gross outliers (photometric stereo, edited or thresholded
 * gradients), total-variation denoising (p = 1, q = 2: ROF; q = 1: TV-L1), robust fusion.  By default the penalty is anisotropic: one
 * residual per link; SC_ROBUST_ISOTROPIC and SC_ROBUST_JOINT_CHANNELS (below) couple the links of a pixel and of a job's channels.
 * With p < 1 (or q < 1) the energy is not convex and the call finds a local minimum, the one its quadratic start leads to.
 * Solved by iteratively reweighted least squares.  Round 0 is the quadratic problem with links c and weights w: sc_hip_wls's system,
 * set up and solved as that call does (without base links: with every link 1).  Round k >= 1 solves the WLS system with
 *     s_x = c_x rho_p(u_x - gx),   s_y = c_y rho_p(u_y - gy),   w' = w rho_q(u - d),      rho_r(t) = (t^2 + eps^2)^((r-2)/2),
 * taken at round k - 1's iterate (u beyond a Dirichlet line is boundary's value there; the link across a periodic seam wraps), started
 * from that iterate: r = b - L u, z = M^-1 r, p = z.  Conjugate gradients started there lower the round's quadratic surrogate at every
 * iterate, so a round lowers the energy even when its solve stops early.  rho in float32: r = 2: exactly 1, the base value passes through
 * without a multiply; r = 1: 1.0f / sqrtf(t * t + eps * eps), square and sum each rounded; any other r: powf(t * t + eps * eps, (r - 2) / 2).
 * The right-hand side of a round is sc_hip_wls's, in its order, from s and w'.  The preconditioner's s-bar and w-bar are each round's
 * own means.
 * With p = q = 2 no reweighting round runs and the call writes the bytes of sc_hip_wls with default parameters bar tol and max_iters
 * (links of 1.0f when the job has no base links).
 * Rounds: at most max_rounds after the quadratic one; the call stops earlier when in the last round no plane's energy fell by more
 * than round_tol times its energy (the rule needs two rounds' energies: rounds 0 and 1 always run).  Running out of rounds is SC_OK.
 * Host waits: the WLS call's per inner solve, and one more per round: the read of the sums of k_robust_setup (s-bar, w-bar, the energies).
 * The energy of the final iterate takes one more launch of that kernel and one more wait, also when p = q = 2.
 * Arrays, layout, chunks, aliasing and per-job codes: sc_hip_wls_device's; gx, gy are required (the base kind must be SC_POISSON_GUIDANCE:
 * the residual needs g itself).  smooth_x, smooth_y: the base links c, both or neither; in a device call all jobs carry them or none
 * does (the first job decides, a job that differs gets SC_ERR_BAD_ARG).  They and weight must be valid as in sc_hip_wls.
 * Codes: SC_ERR_BAD_ARG for an exponent outside (0, 2], an eps that is not finite or not > 0 where its exponent is not 2, a non-finite
 * tol or round_tol, a Laplacian base, exactly one of smooth_x / smooth_y; the others are the WLS call's.  SC_ERR_NOT_CONVERGED only when
 * an inner solve ran out of max_iters (the rounds go on from its last iterate; the last iterate is written).
 * sc_run_info: sweeps = the inner iterations of all rounds, converged = the round rule was met (always 1 when p = q = 2), rel_residual
 * = the last inner solve's; the rest as the WLS call.
 * Coupled gradient terms: two bits of sc_robust_params.kind (of that struct only: every other call refuses them with SC_ERR_BAD_ARG).
 * They couple the gradient term; the data term stays per pixel and per channel.  The owner of a link is its low end: pixel (x, y) owns
 * its x-link to (x+1, y) and its y-link to (x, y+1), along a periodic axis the last pixel the wrapped link; a pixel of a Dirichlet line
 * can own a live link; a dead link and a pixel without a live forward link contribute nothing.  With t = (u_hi - u_lo) - g of a live
 * link on channel k and a = c t^2 (c: the base link, 1 without), the gradient term is
 *     neither bit               sum_links c phi_p(t)                                             (as above, to the byte)
 *     SC_ROBUST_ISOTROPIC       sum_k sum_pixels psi_p(a_x + a_y)
 *     SC_ROBUST_JOINT_CHANNELS  sum_x-links psi_p(sum_k a_x) + sum_y-links psi_p(sum_k a_y)
 *     both (vectorial TV)       sum_pixels psi_p(sum_k (a_x + a_y)),          psi_p(M) = (2 / p) (M + eps^2)^(p/2):
 * the base links sit inside the magnitude M.  Round k >= 1 then solves the WLS system with s = c rho_p(M) on every link that shares M,
 * rho_p(M) = (M + eps^2)^((p-2)/2); psi_p is concave in M for p <= 2, so a round still lowers the energy.  In float32: t t rounded,
 * times c rounded (no base links: no multiply), a_x + a_y within a pixel, then the running sum over the channels 0 .. C - 1, Q = M +
 * eps eps, rho = 1.0f / sqrtf(Q) (p = 1) or powf(Q, (p - 2) / 2), s = c rho rounded; both ends of a link use the same bits.  The first
 * (quadratic) round is untouched.  With p_grad = 2 the bits change nothing (the bytes of the call without them); with one channel
 * SC_ROBUST_JOINT_CHANNELS changes nothing.  Under SC_ROBUST_JOINT_CHANNELS the round rule judges a job's energy (the sum over its
 * planes) instead of every plane's.  A chunk holds whole jobs: channels of different jobs never couple.  Each coupled round takes two
 * launches for its system (k_robust_rho, k_robust_setup_rho) and still one host wait.
 * Not offered: a robust term through the 8-bit entry points, a joint or isotropic data term. */
#define SC_ROBUST_ISOTROPIC       (1 << 20)   /* sc_robust_params.kind: one penalty per pixel over its two forward links */
#define SC_ROBUST_JOINT_CHANNELS  (1 << 21)   /* sc_robust_params.kind: one penalty over all channels of a job           */
typedef struct sc_robust_params {
    int   kind;              /* as sc_wls_params.kind; the base must be SC_POISSON_GUIDANCE; | SC_ROBUST_ISOTROPIC, SC_ROBUST_JOINT_CHANNELS */
    float p_grad, eps_grad;  /* 0 < p <= 2; eps > 0 and finite (unused when p == 2) */
    float p_data, eps_data;  /* likewise for the data term */
    int   max_rounds;        /* reweighting rounds after the quadratic solve; <= 0: 15 */
    float round_tol;         /* stop when no plane's (SC_ROBUST_JOINT_CHANNELS: no job's) energy fell by more than round_tol * its energy in the last round; 0: 1e-4; < 0: never stop early */
    float tol;               /* inner solves: ||r||_2 <= tol * ||b||_2 on every plane; <= 0: 1e-5 */
    int   max_iters;         /* per inner solve; <= 0: 400 */
} sc_robust_params;
typedef struct sc_robust_job {
    const float *gx, *gy;    /* the guidance: required */
    const float *data;       /* d: read at every unknown */
    const float *weight;     /* w >= 0: read at every unknown */
    const float *smooth_x;   /* the base links c > 0, live ones only are read; both NULL: all 1 */
    const float *smooth_y;
    const float *boundary;   /* its Dirichlet lines (no Dirichlet line on any side: unused, may be NULL) */
    float *out;              /* every element the layout names is written; may equal data or boundary */
    int rc;                  /* out: SC_OK or SC_ERR_* of this job */
} sc_robust_job;
/* Host-only (needs no GPU): SC_OK, or the code a call with these parameters and this layout returns before it runs anything. */
SC_API int sc_hip_robust_check(const sc_robust_params *p, const sc_poisson_layout *l);
/* Device pointers.  bSync: waits for the stream and records the call's time. */
SC_API int sc_hip_robust_device(void *instance, const sc_robust_params *p, const sc_poisson_layout *l, sc_robust_job *jobs, int n, bool bSync);
/* One problem on host arrays, as sc_hip_wls: spans in and out through pinned staging, only the named elements of out written. */
SC_API int sc_hip_robust(void *instance, const sc_robust_params *p, const sc_poisson_layout *l, const float *gx, const float *gy,
                         const float *data, const float *weight, const float *smooth_x, const float *smooth_y, const float *boundary,
                         float *out);
/* The last robust call's last chunk (sc_hip_robust*, sc_hip_region_robust*, sc_hip_volume_robust*, sc_hip_volume_coupled*,
 * sc_hip_volume_flow_robust*, sc_hip_volume_subflow_robust* or sc_hip_volume_flow_coupled*, whichever the instance ran last), round by round: returns the number of entries, rounds run + 1 (0: no robust call yet); fills the
 * first min(that, cap) of energy[k] = the energy, summed over the chunk's planes, of the iterate that round k produced, and iters[k] =
 * that round's inner iterations.  Either pointer may be NULL. */
SC_API int sc_hip_robust_trace(void *instance, double *energy, int *iters, int cap);
/* ---- region solves: known pixels, outside pixels, a domain of any shape -----------------------------------------------------------------
 * The problem: sc_hip_wls's, per channel, with one more array, state, under the call's layout (float32, per channel, read like weight).
 * Its values are exactly 0.0f, 1.0f or 2.0f:
 *     SC_REGION_UNKNOWN (0)   the pixel is solved for;
 *     SC_REGION_KNOWN   (1)   u = data there, exactly;
 *     SC_REGION_OUTSIDE (2)   the pixel is not part of the domain: every link to it does not exist (a natural border, as at a free side).
 * This is the region Omega of Poisson image editing in any shape (values fixed everywhere outside it), hard constraints at arbitrary
 * pixels (inpainting a hole from its rim, scribbles that hold exactly, depth or flow completion from valid samples) and domains with
 * holes or cuts (invalid depth, the outside of a segmentation).  state is consulted only at the pixels the border kind calls unknowns;
 * Dirichlet lines keep their meaning and are read from boundary.  Every border kind of sc_hip_wls is accepted.
 * Links: a link is LIVE IN THE REGION when it is live in the WLS sense, neither end is OUTSIDE and at least one end is an UNKNOWN
 * pixel.  KNOWN - KNOWN links and KNOWN - Dirichlet links are dead.  A link to a KNOWN pixel q acts as a link to a Dirichlet pixel: it
 * adds s to the diagonal of its unknown end and s * data(q) to the right-hand side.  smooth_x and smooth_y are both given or both NULL;
 * NULL: every link is 1 (the bytes of a call given arrays of 1.0f).
 * The data term: weight may be NULL: there is no data term, and data is then not read at UNKNOWN pixels (with every state 0 the
 * bytes of sc_hip_wls given a weight array of 0.0f).  In a device call the first job decides for weight and for the link arrays; a job
 * that differs gets SC_ERR_BAD_ARG.
 * The right-hand side at an UNKNOWN pixel, in float32, in this order: with SC_POISSON_LAPLACIAN lap is taken as given (read at UNKNOWN
 * pixels only); with SC_POISSON_GUIDANCE (a - b) + (c - d) of the separately rounded products s * g as in sc_hip_wls, the term of a link
 * that is not live in the region counting 0 and not read.  Then - w * d, one rounded multiply and one subtract (weight given).  Then
 * the Dirichlet lines' terms s * boundary: west, north, east, south.  Then the KNOWN neighbours' terms s * data(q): west, north, east,
 * south.  Each is a rounded product subtracted in turn.
 * What is read: state at every pixel the border kind calls an unknown; weight and lap at UNKNOWN pixels; a link weight and its g only
 * where the link is live in the region; data at UNKNOWN pixels when weight is given, and at KNOWN and OUTSIDE pixels always; boundary
 * on its Dirichlet lines.  Nothing else is read.
 * What is written: every element the layout names -- the solution at UNKNOWN pixels, data's bits at KNOWN and OUTSIDE pixels,
 * boundary's bits on the Dirichlet lines.  out may equal data or boundary.  state, weight and the link arrays must not overlap out
 * (sc_hip_wls's span rule).
 * Solved by the WLS call's conjugate gradients on the whole rectangle, unknowns and others alike: the set-up leaves every coefficient and
 * the right-hand side 0 at a pixel that is not UNKNOWN, which makes the iteration that of the UNKNOWN pixels alone, preconditioned by
 * M = s-bar (A - w-bar / s-bar), A the constant-coefficient operator of the border kind on the whole rectangle: s-bar = precond_smooth,
 * or the mean of the links live in the region over the call's chunk; w-bar = precond_lambda, or (the sum of w over the UNKNOWN pixels +
 * the sum of the UNKNOWN - KNOWN links) / (the number of UNKNOWN pixels) over the chunk.  The rectangle's solve does not know where the
 * constraints are: with unit links and zero guidance, scattered known pixels take about 30 iterations at any size, regions whose values
 * come from their rim alone about 1.5 times more per doubling of the side -- at 1024 x 1024 an ellipse of unknowns 123, a known frame
 * around an excluded blob 197, at 2048 x 2048 194 and 311 (DESIGN.md sections 4 and 7); raise max_iters for larger ones.
 * Stop rule, SC_WEIGHTED_POLL, SC_ERR_NOT_CONVERGED, chunks, batches (a member agrees with its solo run to the stop rule's error),
 * methods, sizes, host waits and sc_run_info: the WLS call's.  A plane without any UNKNOWN pixel is valid: it converges without an
 * iteration, data and boundary are copied.  Two runs of one call give the same bytes.  With every state 0 the call writes the bytes of
 * sc_hip_wls with the same parameters.
 * Codes: the WLS call's for parameters and layout.  Per job SC_ERR_BAD_ARG -- nothing of the job is written, the others run -- for a
 * state element that is not 0, 1 or 2 (NaN included); a weight that is negative or not finite or a link that is not finite or not > 0,
 * judged where it is read; a NULL or misaligned pointer the call needs (data and state always), exactly one of smooth_x / smooth_y,
 * a weight or link arrays where the first job has none (or the reverse), state, weight or a link array overlapping out; and, in a call
 * without any Dirichlet line, a channel with UNKNOWN pixels but no UNKNOWN - KNOWN link and no positive weight ("nothing pins the
 * channel").
 * NOT detected, the caller's responsibility: a connected component of UNKNOWN pixels that nothing pins (no KNOWN neighbour, no Dirichlet
 * line, no weight) while other components are pinned.  In the guidance form the system stays consistent and the call returns some
 * constant offset on that component; with SC_POISSON_LAPLACIAN it need not converge.
 * Not offered: region states through the 8-bit clone and edit entry points (robust penalties on a region: sc_hip_region_robust below). */
#define SC_REGION_UNKNOWN 0
#define SC_REGION_KNOWN   1
#define SC_REGION_OUTSIDE 2
typedef struct sc_region_params {
    int   kind;              /* as sc_wls_params.kind */
    float tol;               /* stop when ||r||_2 <= tol * ||b||_2 on every plane; <= 0: 1e-5 */
    int   max_iters;         /* <= 0: 400 */
    float precond_lambda;    /* w-bar of the preconditioner; <= 0: (sum of w + sum of UNKNOWN - KNOWN links) / UNKNOWN pixels of the chunk */
    float precond_smooth;    /* s-bar of the preconditioner; <= 0: the mean of the links live in the region of the chunk */
} sc_region_params;
typedef struct sc_region_job {
    const float *gx, *gy;    /* SC_POISSON_GUIDANCE: read at links live in the region */
    const float *lap;        /* SC_POISSON_LAPLACIAN: read at UNKNOWN pixels */
    const float *data;       /* the values at KNOWN pixels, copied at OUTSIDE ones; d of the data term at UNKNOWN ones when weight is given */
    const float *state;      /* SC_REGION_UNKNOWN / _KNOWN / _OUTSIDE as 0.0f / 1.0f / 2.0f */
    const float *weight;     /* w >= 0 at UNKNOWN pixels; NULL: no data term */
    const float *smooth_x;   /* > 0 where live in the region; both NULL: every link 1 */
    const float *smooth_y;
    const float *boundary;   /* its Dirichlet lines (no Dirichlet line on any side: unused, may be NULL) */
    float *out;              /* every element the layout names is written; may equal data or boundary */
    int rc;                  /* out: SC_OK or SC_ERR_* of this job */
} sc_region_job;
/* Host-only (needs no GPU): SC_OK, or the code a call with these parameters and this layout returns before it runs anything. */
SC_API int sc_hip_region_check(const sc_region_params *p, const sc_poisson_layout *l);
/* Device pointers.  bSync: waits for the stream and records the call's time. */
SC_API int sc_hip_region_device(void *instance, const sc_region_params *p, const sc_poisson_layout *l, sc_region_job *jobs, int n, bool bSync);
/* One problem on host arrays, as sc_hip_wls: spans in and out through pinned staging, only the named elements of out written. */
SC_API int sc_hip_region(void *instance, const sc_region_params *p, const sc_poisson_layout *l, const float *gx, const float *gy,
                         const float *lap, const float *data, const float *state, const float *weight, const float *smooth_x,
                         const float *smooth_y, const float *boundary, float *out);
/* ---- bounded solves: box constraints lower <= u <= upper on a region solve ---------------------------------------------------------------
 * The problem: sc_hip_region's, per channel, word for word -- the three states, the links live in the region, the data term, both forms
 * of the right-hand side, every border kind -- minimised under the constraint
 *     lower <= u <= upper   at every UNKNOWN pixel.
 * The bounds say nothing about KNOWN pixels, OUTSIDE pixels or Dirichlet lines.  A Poisson clone that stays inside the displayable
 * range, a height or depth field integrated from gradients that never goes negative, a matte or confidence map interpolated from
 * scribbles that stays in [0, 1], a membrane over an obstacle.  Clamping an unconstrained answer is not this: the constrained minimiser
 * spreads what the bound cuts off over the free pixels and differs from the clamped one everywhere.
 * Bounds: sc_bounded_params.lower / .upper are scalars; -INFINITY / +INFINITY mean no bound on that side.  sc_bounded_job.lower /
 * .upper, where not NULL, are arrays under the call's layout that replace the scalar for that job; they are read at UNKNOWN pixels
 * only.  In a device call the first job decides for each of the two arrays (as for weight); a job that differs gets SC_ERR_BAD_ARG.
 * The arrays fall under the span rule against out, as state does.
 * The method: the primal-dual active set method (Hintermueller, Ito, Kunisch 2002).  The region system is a symmetric M-matrix (links
 * > 0, weights >= 0), for which the method is monotone with one-sided bounds and ends after finitely many rounds.
 *   round 0   sc_hip_region's system, set-up and cold start, unchanged.
 *   the mark  after every solve one launch (k_bounded_mark) forms r = L u - b of the ORIGINAL system at every active pixel (the rule asks
 *             for it nowhere else), in float32:
 *             ((lw (uw - u) + le (ue - u)) + (ln (un - u) + ls (us - u))) - w (u - d) - the guidance term (lap, or (a - b) + (c - d)).
 *             Across a link it reads the bound at an active pixel, data at a KNOWN pixel, boundary on a Dirichlet line, and the iterate
 *             anywhere else; u of an active pixel is its bound.  r = - dE/du: at a minimiser r >= 0 on the upper bound, <= 0 on the lower.
 *   the rule  a free pixel with u > upper becomes upper-active, one with u < lower lower-active; an upper-active pixel stays while
 *             r > 0, a lower-active one while r < 0; every other pixel is free.  The launch writes the new set to the second of two
 *             set planes (the neighbours read the first) and per part the number of pixels whose set changed: doubles, no atomics,
 *             one host read.
 *   set-up    if any pixel of the chunk changed, a second launch (k_bounded_setup) builds the round's system: k_region_setup's planes
 *             with an active pixel treated as a KNOWN one whose value is its bound (its terms follow the KNOWN neighbours' in the
 *             right-hand side's order: west, north, east, south).  It puts the bound into the iterate at every pixel that is or was
 *             active, so a pixel released later starts from its bound, and sums what the preconditioner's w-bar is refreshed from: w
 *             over the free pixels, the links from a free pixel to a KNOWN or active one, the free pixels (a second host read; s-bar
 *             stays round 0's).  The conjugate gradients then start warm from the iterate.
 *   the end   no pixel of any job of the chunk changed: the iterate satisfies the KKT conditions to the inner tolerance.  When
 *             max_rounds solves have run and the set still changes, the last iterate is returned with sc_run_info.converged = 0 and
 *             SC_OK (the robust call's convention for rounds); SC_ERR_NOT_CONVERGED is kept for an inner solve that ran out of
 *             max_iters.  sc_run_info.sweeps is the total of the inner iterations.
 * Rounds: the contact set of a smooth obstacle problem (constant load, one bound) grows by one layer of pixels per round, so the
 * rounds grow with the side length there: 8 at 32 x 32, 13 at 64 x 64, 22 at 128 x 128 in float64, 94 at 512 x 512 on the device.
 * Bounds at the quartiles of a rough unconstrained answer take 3 to 8 rounds on the tests' inputs (up to 300 pixels a side), the same
 * as the float64 method.  Raise max_rounds for large smooth contact sets.  On megapixel inputs the set settles to a handful of
 * changing pixels within some 15 rounds and then a last pixel may alternate for long -- a 1024 x 1024 x 3 clone that overshoots by a
 * quarter of the range ended after 72 rounds, the same at 2048 x 2048 x 1 had one pixel alternating after 200:
 * with max_rounds = 30 such a call returns converged = 0, its answer in range and within the inner tolerance of the KKT conditions.
 * What is written: every element the layout names -- the bound's bits at active pixels; the iterate clamped into [lower, upper] at free
 * UNKNOWN pixels (after a converged stop the clamp changes nothing; after running out of rounds it still guarantees the range);
 * data's bits at KNOWN and OUTSIDE pixels; boundary's bits on the Dirichlet lines.  out may equal data or boundary.
 * Exact ties: (a) no finite bound anywhere (both scalars infinite, no arrays): the bytes of sc_hip_region, no extra launch, no extra
 * wait; (b) bounds that round 0's iterate already satisfies: the bytes of sc_hip_region after one mark launch, a trace of one entry;
 * (c) lower == upper: the bound's bits at every UNKNOWN pixel; (d) two runs of one call give the same bytes.
 * Codes: sc_hip_region_check's for parameters and layout, and SC_ERR_BAD_ARG for a scalar bound that is NaN or scalars with lower >
 * upper.  Per job SC_ERR_BAD_ARG -- nothing of the job is written, the others run -- for everything sc_hip_region refuses; a bound that
 * is NaN or lower > upper at an UNKNOWN pixel (at other pixels the bounds are not read); a bound array where the first job has none
 * (or the reverse), misaligned, or overlapping out.
 * Not offered: bounds together with robust penalties, on volumes, or through the 8-bit entry points; a tolerance rule for degenerate
 * pixels (u on its bound with r = 0) that alternate between the sets under inexact inner solves -- they show as converged = 0 with a
 * KKT violation at the inner tolerance's scale. */
typedef struct sc_bounded_params {
    int   kind;              /* as sc_region_params */
    float tol;
    int   max_iters;
    float precond_lambda;
    float precond_smooth;
    float lower, upper;      /* the bounds where a job gives no array; -INFINITY / +INFINITY: none on that side */
    int   max_rounds;        /* solves per chunk at the most; <= 0: 30 */
} sc_bounded_params;
typedef struct sc_bounded_job {
    const float *gx, *gy;    /* as sc_region_job */
    const float *lap;
    const float *data;
    const float *state;
    const float *weight;
    const float *smooth_x;
    const float *smooth_y;
    const float *boundary;
    const float *lower;      /* per-pixel bounds under the layout, read at UNKNOWN pixels; NULL: the scalar */
    const float *upper;
    float *out;              /* every element the layout names is written; may equal data or boundary */
    int rc;                  /* out: SC_OK or SC_ERR_* of this job */
} sc_bounded_job;
/* Host-only (needs no GPU): SC_OK, or the code a call with these parameters and this layout returns before it runs anything. */
SC_API int sc_hip_bounded_check(const sc_bounded_params *p, const sc_poisson_layout *l);
/* Device pointers.  bSync: waits for the stream and records the call's time. */
SC_API int sc_hip_bounded_device(void *instance, const sc_bounded_params *p, const sc_poisson_layout *l, sc_bounded_job *jobs, int n, bool bSync);
/* One problem on host arrays, as sc_hip_region: spans in and out through pinned staging, only the named elements of out written.
 * lower, upper: arrays, or NULL for the scalars. */
SC_API int sc_hip_bounded(void *instance, const sc_bounded_params *p, const sc_poisson_layout *l, const float *gx, const float *gy,
                          const float *lap, const float *data, const float *state, const float *weight, const float *smooth_x,
                          const float *smooth_y, const float *boundary, const float *lower, const float *upper, float *out);
/* The last bounded call's last chunk, round by round: entry k holds the pixels whose set changed in the mark behind solve k, the
 * pixels active after it, and solve k's inner iterations.  Returns the number of entries (fills at most cap); any pointer may be NULL. */
SC_API int sc_hip_bounded_trace(void *instance, int *changed, int *active, int *iters, int cap);
/* ---- robust region solves: Lp and TV penalties on a domain of any shape ------------------------------------------------------------------
 * sc_hip_region's domain with sc_hip_robust's penalties in place of the squares.  Per channel, with exponents 0 < p, q <= 2, the call
 * minimises over the UNKNOWN pixels
 *     sum w phi_q(u - d; eps_d)  +  sum_live x-links c_x phi_p(dx u - gx; eps_g)  +  sum_live y-links c_y phi_p(dy u - gy; eps_g),
 * phi, eps and the float32 forms of rho sc_hip_robust's; "live in the region", the three states, what is read and what is written
 * sc_hip_region's, word for word.  The value of u across a link is data's at a KNOWN pixel, boundary's on a Dirichlet line of the border
 * kind and the work plane's only at an UNKNOWN pixel.  Total-variation inpainting (the hole is filled so that edges run through it,
 * where sc_hip_region gives a membrane), robust integration of a gradient field on a valid-pixel mask (photometric-stereo normals,
 * depth from gradients: invalid pixels and outliers at once), robust interpolation from scattered hard samples, Poisson clones in the
 * exact mask shape that ignore a few wrong gradients.
 * The parameters are sc_robust_params themselves: exponents, eps, max_rounds, round_tol, tol and max_iters as in sc_hip_robust;
 * SC_ROBUST_ISOTROPIC and SC_ROBUST_JOINT_CHANNELS are accepted.  There is no lap (the base kind must be SC_POISSON_GUIDANCE).
 * weight NULL means no data term: p_data and eps_data are validated and unused, and data is not read at UNKNOWN pixels.  smooth_x,
 * smooth_y: the base links c, both or neither; NULL: every link is 1.  In a device call the first job decides for weight and for the
 * link arrays; a job that differs gets SC_ERR_BAD_ARG.
 * Coupled forms: sc_hip_robust's definitions restricted to the links live in the region.  The owner of a link is its low end, which may
 * be UNKNOWN, KNOWN or a pixel of a low Dirichlet line.  A dead link contributes nothing to a magnitude, and an owner without a live
 * link nothing to the energy.  Under SC_ROBUST_JOINT_CHANNELS the magnitude of a link sums the channels in which that link is live
 * (state is per channel).  The coupling changes nothing with p_grad = 2, or with the joint bit on one channel.
 * Rounds: round 0 is sc_hip_region's system with default precond_*, set up and cold-started as that call does.  Round k >= 1 is the
 * region system with s = c rho and w' = w rho_q taken at round k - 1's iterate, started warm from it.  Its right-hand side follows the
 * region section's order: the guidance products (a - b) + (c - d), then - w' d, then the Dirichlet lines' terms west, north, east,
 * south, then the KNOWN neighbours' terms west, north, east, south, each a rounded product.  Its diagonal is ((lw + le) + (ln + ls)) + w'.
 * Both ends of a link compute its weight with the same bits: t = (u_hi - u_lo) - g, then sc_hip_robust's rho and one rounded product
 * (the coupled forms: both ends read one rho).  The region section's zero condition -- right-hand side and coefficients 0 at every
 * pixel that is not UNKNOWN -- holds after every round.  The preconditioner's means are each round's own: s-bar the mean of the live s,
 * w-bar = (the sum of w' + the sum of the UNKNOWN - KNOWN links' s) / (the UNKNOWN pixels).  "Nothing pins the channel" and all other
 * per-job refusals are the region call's, made in round 0.  One launch (k_region_robust_setup; coupled forms: k_region_robust_rho and
 * k_region_robust_setup_rho) and one host read per round.
 * max_rounds, round_tol (a plane's energy; under SC_ROBUST_JOINT_CHANNELS a job's), SC_ERR_NOT_CONVERGED, methods, sizes (8192 unknowns
 * per side, 4096 with SC_FLAG_FFT_FP64), chunks, sc_run_info and the trace (sc_hip_robust_trace): sc_hip_robust's.
 * Ties, byte for byte on out with equal sweeps: (a) every state 0 with a weight array: the bytes of sc_hip_robust with the same
 * parameters, coupled bits included; (b) p_grad = p_data = 2: no round runs, the bytes of sc_hip_region (guidance base, default
 * precond_*, the same tol and max_iters); (c) link arrays of 1.0f: the bytes of NULL arrays; (d) every state 0 with weight NULL: the
 * bytes of the same call with a weight array of 0.0f; (e) two runs of one call give the same bytes.
 * Codes: everything sc_hip_region_check refuses for layout and kind; everything sc_hip_robust_check refuses for exponents, eps, tol,
 * round_tol and a Laplacian base.  Per job: the region call's refusals.
 * Not offered: the 8-bit clone and edit entry points, a joint or isotropic data term, continuation in p or eps. */
typedef struct sc_region_robust_job {   /* sc_region_job without lap */
    const float *gx, *gy;    /* read at links live in the region: required */
    const float *data;       /* the values at KNOWN pixels, copied at OUTSIDE ones; d of the data term at UNKNOWN ones when weight is given */
    const float *state;      /* SC_REGION_UNKNOWN / _KNOWN / _OUTSIDE as 0.0f / 1.0f / 2.0f */
    const float *weight;     /* w >= 0 at UNKNOWN pixels; NULL: no data term */
    const float *smooth_x;   /* the base links c > 0 where live in the region; both NULL: every base link 1 */
    const float *smooth_y;
    const float *boundary;   /* its Dirichlet lines (no Dirichlet line on any side: unused, may be NULL) */
    float *out;              /* every element the layout names is written; may equal data or boundary */
    int rc;                  /* out: SC_OK or SC_ERR_* of this job */
} sc_region_robust_job;
/* Host-only (needs no GPU): SC_OK, or the code a call with these parameters and this layout returns before it runs anything. */
SC_API int sc_hip_region_robust_check(const sc_robust_params *p, const sc_poisson_layout *l);
/* Device pointers.  bSync: waits for the stream and records the call's time. */
SC_API int sc_hip_region_robust_device(void *instance, const sc_robust_params *p, const sc_poisson_layout *l, sc_region_robust_job *jobs,
                                       int n, bool bSync);
/* One problem on host arrays, as sc_hip_region: spans in and out through pinned staging, only the named elements of out written. */
SC_API int sc_hip_region_robust(void *instance, const sc_robust_params *p, const sc_poisson_layout *l, const float *gx, const float *gy,
                                const float *data, const float *state, const float *weight, const float *smooth_x, const float *smooth_y,
                                const float *boundary, float *out);
/* ---- volume solves: region solves on frame stacks with temporal links ------------------------------------------------------------------
 * A stack of `frames` >= 2 images (video frames, CT or MRI slices, a depth stack) shares one sc_poisson_layout; in every array of a job
 * frame t begins frame_stride floats behind frame t - 1.  The unknown is u_t(q).  Per channel the call minimises
 *     sum_t [ sum_q w (u_t - d_t)^2 + sum |grad u_t - g_t|^2 ]  +  tau sum_{t < frames - 1} sum_q (u_{t+1}(q) - u_t(q) - gt_t(q))^2
 * over the pixels whose state is SC_REGION_UNKNOWN; u = data where state is SC_REGION_KNOWN; a link does not exist if either of its ends
 * is SC_REGION_OUTSIDE.  Within a frame this is sc_hip_region's problem with every spatial link 1: border kinds (all of them, periodic
 * axes included), links live in the region, KNOWN neighbours folded into the right-hand side.  A known keyframe is a frame of 1s:
 * flicker-free cloning, video inpainting, keyframe propagation, smoothing of a volume along its third axis.
 * Temporal links: the link between (q, t) and (q, t + 1) follows the spatial rule -- it is live when neither end is OUTSIDE and at
 * least one end is UNKNOWN.  Its weight is the constant tau.  A KNOWN temporal neighbour adds tau to the diagonal of its unknown end and
 * tau * data to the right-hand side.  The two ends of time are free: no frame lies before the first or after the last.  Pixels on the
 * border kind's Dirichlet lines are Dirichlet in every frame; they have no temporal links, as they have no spatial links among
 * themselves.  gt holds frames - 1 frames (gt_t at t * frame_stride) and may be NULL: zeros, plain temporal smoothness.
 * SC_POISSON_LAPLACIAN: lap is the complete right-hand side of the three-dimensional system at UNKNOWN pixels (before the Dirichlet and
 * KNOWN neighbours are folded in, as in sc_hip_region); gx, gy and gt are not read.
 * weight may be NULL (no data term; data is then not read at UNKNOWN pixels); data and state are required.  In a device call the first
 * volume decides for weight; a volume that differs gets SC_ERR_BAD_ARG.  gt is each volume's own choice.
 * The right-hand side at an UNKNOWN pixel, in float32, in this order:
 *   1. sc_hip_region's guidance sum for the frame, (a - b) + (c - d) of the products 1 * g, a link not live in the region counting 0
 *      and not read (SC_POISSON_LAPLACIAN: lap, and step 2 is left out);
 *   2. + (e - f): e the rounded product tau * gt_t(q) where the link to frame t + 1 is live, f the rounded product tau * gt_{t-1}(q)
 *      where the link to frame t - 1 is live; otherwise each counts 0 and is not read (gt NULL: both 0);
 *   3. - w * d, one rounded multiply and one subtract (weight given);
 *   4. the Dirichlet lines' terms 1 * boundary: west, north, east, south;
 *   5. the KNOWN spatial neighbours' terms 1 * data(q): west, north, east, south;
 *   6. the KNOWN temporal neighbours' terms tau * data: previous frame, then next frame;
 *   7. every product of 4 to 6 is rounded on its own and subtracted in turn.
 * What is read and written is sc_hip_region's, frame by frame: out gets the solution at UNKNOWN pixels, data's bits at KNOWN and
 * OUTSIDE pixels and boundary's bits on the Dirichlet lines of every frame; row padding, unused channel slots and the floats between
 * frames are never written.  gt is read only at live temporal links.  out may equal data or boundary; state and weight must not
 * overlap out (the span rule, the span being all frames').
 * Solved by conjugate gradients on one system per (volume, channel): the residual norm of the stop rule and the scalars of the
 * iteration are one per (volume, channel), summed over all its frames.  The preconditioner is M = A - w-bar + tau A_t on the whole
 * rectangle x frames, A the constant-coefficient operator of the border kind and A_t the free-ended second difference along the
 * frames; w-bar = precond_lambda, or (the sum of w over the UNKNOWN pixels + the sum of all UNKNOWN - KNOWN links, a spatial one 1 and
 * a temporal one tau) / (the number of UNKNOWN pixels) over the chunk.  M is inverted exactly: an orthonormal DCT-II along the frames,
 * one screened direct solve per mode k shifted by w-bar + tau (2 - 2 cos(pi k / frames)), the transposed transform.  With a constant
 * weight and every state 0 the first iterate is the answer.
 * Size: frames * channels <= SC_POISSON_MAX_PLANES, else SC_ERR_BAD_SIZE; a chunk holds floor(SC_POISSON_MAX_PLANES / (frames *
 * channels)) volumes.  Stop rule, SC_WEIGHTED_POLL, SC_ERR_NOT_CONVERGED, methods, SC_FLAG_FFT_FP64 limits, host waits and
 * sc_run_info: the region call's.  Two runs of one call give the same bytes.
 * Codes: SC_ERR_BAD_ARG for frames < 2, a frame_stride below the span of one frame under the layout (frames would overlap), tau that
 * is not finite or not > 0, and everything sc_hip_region_check refuses.  Per job SC_ERR_BAD_ARG -- nothing of the job is written, the
 * others run -- for every per-job refusal of the region call, with the pin check judged per channel over the whole volume and not per
 * frame: a channel whose middle frames hold no KNOWN pixel is fine when time links them to frames that do.  A channel is refused only
 * when the call has no Dirichlet line, the channel has UNKNOWN pixels, and the volume has no UNKNOWN - KNOWN link of either kind and
 * no positive weight.  Not detected, as in the region call: a connected component (through spatial and temporal links) that nothing
 * pins while others are pinned.
 * Not offered here: per-link spatial or temporal weights and periodic time (sc_hip_volume_wls has both), robust penalties
 * (sc_hip_volume_robust); anywhere: the 8-bit entry points. */
typedef struct sc_volume_params {
    int       kind;            /* as sc_region_params.kind */
    int       frames;          /* >= 2; frames * channels <= SC_POISSON_MAX_PLANES */
    long long frame_stride;    /* floats from a frame to the next in every array; at least the span of one frame under the layout */
    float     tau;             /* the temporal links' weight; finite, > 0 */
    float     tol;             /* stop when ||r||_2 <= tol * ||b||_2 on every (volume, channel); <= 0: 1e-5 */
    int       max_iters;       /* <= 0: 400 */
    float     precond_lambda;  /* w-bar of the preconditioner; <= 0: (sum of w + sum of UNKNOWN - KNOWN links) / UNKNOWN pixels of the chunk */
} sc_volume_params;
typedef struct sc_volume_job {
    const float *gx, *gy;    /* SC_POISSON_GUIDANCE: `frames` frames, read at links live in the region */
    const float *gt;         /* SC_POISSON_GUIDANCE: frames - 1 frames, read at live temporal links; NULL: zeros */
    const float *lap;        /* SC_POISSON_LAPLACIAN: read at UNKNOWN pixels */
    const float *data;       /* the values at KNOWN pixels, copied at OUTSIDE ones; d of the data term at UNKNOWN ones when weight is given */
    const float *state;      /* SC_REGION_UNKNOWN / _KNOWN / _OUTSIDE as 0.0f / 1.0f / 2.0f */
    const float *weight;     /* w >= 0 at UNKNOWN pixels; NULL: no data term */
    const float *boundary;   /* its Dirichlet lines in every frame (no Dirichlet line on any side: unused, may be NULL) */
    float *out;              /* every element the layout names in every frame is written; may equal data or boundary */
    int rc;                  /* out: SC_OK or SC_ERR_* of this job */
} sc_volume_job;
/* Host-only (needs no GPU): SC_OK, or the code a call with these parameters and this layout returns before it runs anything. */
SC_API int sc_hip_volume_check(const sc_volume_params *p, const sc_poisson_layout *l);
/* Device pointers, n volumes of the same shape.  bSync: waits for the stream and records the call's time. */
SC_API int sc_hip_volume_device(void *instance, const sc_volume_params *p, const sc_poisson_layout *l, sc_volume_job *jobs, int n, bool bSync);
/* One volume on host arrays, as sc_hip_region: spans in and out through pinned staging, only the named elements of out written. */
SC_API int sc_hip_volume(void *instance, const sc_volume_params *p, const sc_poisson_layout *l, const float *gx, const float *gy,
                         const float *gt, const float *lap, const float *data, const float *state, const float *weight,
                         const float *boundary, float *out);
/* ---- WLS volume solves: per-link weights in space and time, looping time ------------------------------------------------------------------
 * sc_hip_volume's problem with a weight on every link, as sc_hip_region has them within an image, and optionally periodic time.  Per
 * channel the call minimises
 *     sum_t [ sum_q w (u_t - d_t)^2 + sum sx (dx u_t - gx_t)^2 + sum sy (dy u_t - gy_t)^2 ]  +  sum_t sum_q lt (u_{t+1}(q) - u_t(q) - gt_t(q))^2
 * over the UNKNOWN pixels.  The temporal link lt is tau when smooth_t is NULL, else the float32 product tau * smooth_t, rounded once.
 * Edge-aware smoothing of video that does not flicker, scribble, colour or depth propagation that stops at edges in space and in time,
 * clones whose temporal coupling is switched down where the frames disagree, seamless loops.
 * States, the liveness of spatial and temporal links, Dirichlet lines, what is copied to out and what is never written: sc_hip_volume's.
 * smooth_x, smooth_y: `frames` frames, each stored at its link's low end as in sc_hip_region (the last pixel of a periodic axis holds the
 * wrapping link), read only at links live in the region; both given or both NULL: every spatial link 1.
 * smooth_t and gt: element (q, t) belongs to the link from frame t to frame t + 1.  With time_periodic = 0 both hold frames - 1 frames
 * and the two ends of time are free.  With time_periodic = 1 (frames >= 3) both hold `frames` frames, frame frames - 1 of them is the
 * link from the last frame to frame 0, and that link follows the same liveness rule as any other.  Each is read only at live temporal
 * links.  In a device call the first volume decides for weight, for smooth_x / smooth_y and for smooth_t (the two judged separately); a
 * volume that differs gets SC_ERR_BAD_ARG.  gt is each volume's own choice.
 * The right-hand side at an UNKNOWN pixel, in float32: the seven steps of sc_hip_volume, where
 *   1. each 1 * g is the rounded product s * g of the link's own weight (SC_POISSON_LAPLACIAN: lap, and step 2 is left out);
 *   2. e is the rounded product lt * gt of the link to the next frame, f that of the link to the previous frame, each with its own lt;
 *      under periodic time the previous frame of frame 0 is frame frames - 1 and the next frame of frame frames - 1 is frame 0;
 *   3. - w * d as there;
 *   4. the Dirichlet lines' terms s * boundary with their link's s: west, north, east, south;
 *   5. the KNOWN spatial neighbours' terms s * data(q) likewise;
 *   6. the KNOWN temporal neighbours' terms lt * data: previous frame, then next frame;
 *   7. every product of 4 to 6 is rounded on its own and subtracted in turn.
 * The diagonal is (((lw + le) + (ln + ls)) + (lb + lf)) + w over the live links west, east, north, south, back, forward.
 * What is read: sc_hip_volume's elements; a link weight only where its link is live.  A NaN at a dead link is fine.  weight, state and
 * the three link arrays must not overlap out (the span rule; a temporal array's span is its own frames').
 * Ties: with all three link arrays NULL and time_periodic = 0 the call writes the bytes of sc_hip_volume with the same parameters;
 * arrays of 1.0f give the bytes of NULL arrays.  Two runs of one call give the same bytes.
 * Solved as sc_hip_volume: conjugate gradients on one system per (volume, channel), preconditioned by
 *     M = s-bar A - w-bar + tau-bar A_t
 * on the whole rectangle x frames, exact for constant coefficients.  s-bar = precond_smooth, or the mean of the spatial links live in
 * the region over the chunk (exactly 1 without smooth_x or without such a link); tau-bar = precond_tau, or the mean of the live temporal
 * links lt (exactly tau without smooth_t or without such a link); w-bar = precond_lambda, or (the sum of w over the UNKNOWN pixels + the
 * sum of the UNKNOWN - KNOWN links' weights, spatial and temporal) / (the number of UNKNOWN pixels).  M is inverted by an orthonormal
 * table product along the frames, one screened direct solve per mode k shifted by (w-bar + tau-bar mu_k) / s-bar, and the transposed
 * product: with free time the DCT-II and mu_k = 2 - 2 cos(pi k / frames), with periodic time the Hartley table (cos + sin)(2 pi k t /
 * frames) / sqrt(frames) and mu_k = 2 - 2 cos(2 pi k / frames).  Measured on one MI355X with 1 in 30 pixels known: links
 * log-uniform over two decades 38 - 40 iterations, links over three to four decades 94 - 140 (raise max_iters for more contrast).
 * Size, chunks, stop rule, SC_WEIGHTED_POLL, SC_ERR_NOT_CONVERGED, methods, SC_FLAG_FFT_FP64 limits, host waits, sc_run_info:
 * sc_hip_volume's.
 * Codes: everything sc_hip_volume_check refuses, and SC_ERR_BAD_ARG for time_periodic that is not 0 or 1, frames < 3 with
 * time_periodic, precond_smooth or precond_tau that is not finite.  Per job SC_ERR_BAD_ARG -- nothing of the job is written, the others
 * run -- for every per-job refusal of sc_hip_volume; exactly one of smooth_x / smooth_y; link arrays where the first volume has none, or
 * the reverse; a link array overlapping out; a live link that is not finite or not > 0 (smooth_t as well as its product with tau),
 * judged only where it is read.  The pin check is sc_hip_volume's; an UNKNOWN - KNOWN link counts its own weight.
 * Not offered: the 8-bit entry points.  Motion-compensated temporal links: sc_hip_volume_flow below, with these parameters. */
typedef struct sc_volume_wls_params {
    int       kind;            /* as sc_volume_params.kind */
    int       frames;          /* >= 2 (>= 3 with time_periodic); frames * channels <= SC_POISSON_MAX_PLANES */
    long long frame_stride;    /* floats from a frame to the next in every array; at least the span of one frame under the layout */
    float     tau;             /* multiplies every temporal link; finite, > 0 */
    int       time_periodic;   /* 0: the ends of time are free; 1: frame frames - 1 is linked to frame 0 */
    float     tol;             /* stop when ||r||_2 <= tol * ||b||_2 on every (volume, channel); <= 0: 1e-5 */
    int       max_iters;       /* <= 0: 400 */
    float     precond_lambda;  /* w-bar of the preconditioner; <= 0: the chunk's mean */
    float     precond_smooth;  /* s-bar; <= 0: the mean of the spatial links live in the region of the chunk */
    float     precond_tau;     /* tau-bar; <= 0: the mean of the live temporal links of the chunk */
} sc_volume_wls_params;
typedef struct sc_volume_wls_job {
    const float *gx, *gy;    /* SC_POISSON_GUIDANCE: `frames` frames, read at links live in the region */
    const float *gt;         /* SC_POISSON_GUIDANCE: frames - 1 frames (time_periodic: frames), read at live temporal links; NULL: zeros */
    const float *lap;        /* SC_POISSON_LAPLACIAN: read at UNKNOWN pixels */
    const float *data;       /* the values at KNOWN pixels, copied at OUTSIDE ones; d of the data term at UNKNOWN ones when weight is given */
    const float *state;      /* SC_REGION_UNKNOWN / _KNOWN / _OUTSIDE as 0.0f / 1.0f / 2.0f */
    const float *weight;     /* w >= 0 at UNKNOWN pixels; NULL: no data term */
    const float *smooth_x;   /* `frames` frames, > 0 at links live in the region; both NULL: every spatial link 1 */
    const float *smooth_y;
    const float *smooth_t;   /* frames - 1 frames (time_periodic: frames), > 0 at live temporal links; NULL: every temporal link tau */
    const float *boundary;   /* its Dirichlet lines in every frame (no Dirichlet line on any side: unused, may be NULL) */
    float *out;              /* every element the layout names in every frame is written; may equal data or boundary */
    int rc;                  /* out: SC_OK or SC_ERR_* of this job */
} sc_volume_wls_job;
/* Host-only (needs no GPU): SC_OK, or the code a call with these parameters and this layout returns before it runs anything. */
SC_API int sc_hip_volume_wls_check(const sc_volume_wls_params *p, const sc_poisson_layout *l);
/* Device pointers, n volumes of the same shape.  bSync: waits for the stream and records the call's time. */
SC_API int sc_hip_volume_wls_device(void *instance, const sc_volume_wls_params *p, const sc_poisson_layout *l, sc_volume_wls_job *jobs, int n,
                                    bool bSync);
/* One volume on host arrays, as sc_hip_volume: spans in and out through pinned staging, only the named elements of out written. */
SC_API int sc_hip_volume_wls(void *instance, const sc_volume_wls_params *p, const sc_poisson_layout *l, const float *gx, const float *gy,
                             const float *gt, const float *lap, const float *data, const float *state, const float *weight,
                             const float *smooth_x, const float *smooth_y, const float *smooth_t, const float *boundary, float *out);
/* ---- flow volume solves: temporal links along a caller's motion field ----------------------------------------------------------------------
 * sc_hip_volume_wls's problem, word for word, except that a temporal link joins pixel p of frame t to pixel m_t(p) of frame t + 1, where
 * m_t follows a flow the caller supplies; the temporal term is
 *     sum_t sum_p lt(p) (u_{t+1}(m_t(p)) - u_t(p) - gt_t(p))^2
 * over the pixels p that hold a link.  On footage in which anything moves the straight link of sc_hip_volume_wls ties a pixel to another
 * surface point of the next frame and the solve smears along the motion; with the scene's flow the links follow the surface.  Cloning,
 * inpainting, propagation and smoothing of video with a moving camera or moving objects.  The parameters are sc_volume_wls_params,
 * unchanged.  smooth_t and gt stay stored at the link's source element (p, t).
 * flow_x, flow_y: float32, dense and without channel axis whatever the layout: element (x, y, t) at (t * rows + y) * cols + x; frames - 1
 * frames, with time_periodic `frames` of them, the last from frame frames - 1 onto frame 0.  Element (x, y, t) says that pixel (x, y) of
 * frame t is pixel (x + flow_x, y + flow_y) of frame t + 1.  Values are whole numbers (-0.0 is 0); a component that is not finite means
 * "no link": that is how a caller marks an occlusion.  A volume's channels share its flow.
 * The matching, per volume and pair of frames, without regard to state.  A pixel p of the work rectangle -- the border kind's unknowns:
 * a Dirichlet line is outside, it has no temporal links -- is a candidate when both components are finite, both have magnitude <= 1e6 (a
 * finite value beyond counts as leaving the rectangle) and its target lies inside the work rectangle; on a periodic axis the target wraps.
 * Among the candidates with the same target the one with the smallest y * nx + x in work-rectangle coordinates holds the link, the others
 * hold none.  So every pixel holds at most one link and at most one arrives at it, the system stays symmetric, and nothing depends on
 * the order in which anything ran.
 * Liveness, right-hand side, diagonal, pin check: sc_hip_volume_wls's rules on matched pairs.  A matched link is live when neither end
 * is OUTSIDE and at least one end is UNKNOWN.  In the seven steps "the link to the next frame" is the link this pixel holds and "the
 * link to the previous frame" the link that arrives at it, whose lt and gt are read at its source's element; a KNOWN temporal
 * neighbour's data is read at the partner pixel; the diagonal is (((lw + le) + (ln + ls)) + (lb + lf)) + w with lb the arriving link.
 * What is read: sc_hip_volume_wls's elements, with gt and smooth_t only at live matched links (a NaN at an unmatched or dead link is
 * fine), and the flow at every pixel of the work rectangle of every frame it holds, nowhere else.  The flow arrays must not overlap out.
 * Ties: flow arrays of zeros give the bytes and the iteration count of sc_hip_volume_wls; both arrays NULL runs sc_hip_volume_wls's
 * launches.  Two runs of one call give the same bytes: the matching's one atomic is an integer minimum.
 * Solved as sc_hip_volume_wls, with its preconditioner unchanged: M = s-bar A - w-bar + tau-bar A_t with straight time links and the
 * same means (tau-bar is exactly tau without smooth_t).  M is positive definite, so the iteration converges, but it is no longer exact
 * for constant coefficients: strong temporal coupling together with several pixels of motion is expensive.  Iterations of a float64
 * model at tol 1e-5 (all UNKNOWN, a data weight at 3 % of the pixels, free sides, 47 x 33 x 5 and 64 x 64 x 8):
 *     tau    zero flow   halves moving +-1 px   halves moving +-3 px   random +-3 px
 *     0.1       10            10 - 12                10 - 12              10 - 12
 *     1          8            17 - 18                43 - 46              25 - 26
 *     10         7           100 - 106              335 - 371            163 - 171
 * Raise max_iters there.  Size, chunks, stop rule, SC_WEIGHTED_POLL, SC_ERR_NOT_CONVERGED, methods, SC_FLAG_FFT_FP64 limits, host waits,
 * sc_run_info: sc_hip_volume_wls's.
 * Size: the link planes index a volume's unknowns with 32 bits, so (unknowns per frame) * frames must be below 2^31 - 1: a larger
 * volume -- 8192 x 8192 free-sided pixels take 31 frames, not 32 -- gets SC_ERR_BAD_SIZE from sc_hip_volume_flow_check and from a call
 * that carries a flow, before anything runs (without flow arrays the call is sc_hip_volume_wls and takes what that call takes).
 * Codes: everything sc_hip_volume_wls_check refuses, and SC_ERR_BAD_SIZE as above.  Per job SC_ERR_BAD_ARG -- nothing of the job is written, the others run -- for
 * every per-job refusal of sc_hip_volume_wls; exactly one of flow_x / flow_y; a flow where the first volume has none, or the reverse; a
 * flow array overlapping out; a finite flow value, where the flow is read, that is not a whole number.
 * Not offered: flow through sc_hip_volume or the 8-bit entry points (robust penalties along a flow: sc_hip_volume_flow_robust
 * below; the coupled forms along a flow: sc_hip_volume_flow_coupled); a preconditioner that transforms along the trajectories; an
 * estimator of the flow.  Sub-pixel flow and links of several pixels onto one: sc_hip_volume_subflow below, with these parameters and
 * jobs -- there a link is a bilinear stencil and no matching applies. */
typedef struct sc_volume_flow_job {     /* sc_volume_wls_job and the two flow arrays */
    const float *gx, *gy;    /* SC_POISSON_GUIDANCE: `frames` frames, read at links live in the region */
    const float *gt;         /* SC_POISSON_GUIDANCE: frames - 1 frames (time_periodic: frames), read at live matched links; NULL: zeros */
    const float *lap;        /* SC_POISSON_LAPLACIAN: read at UNKNOWN pixels */
    const float *data;       /* the values at KNOWN pixels, copied at OUTSIDE ones; d of the data term at UNKNOWN ones when weight is given */
    const float *state;      /* SC_REGION_UNKNOWN / _KNOWN / _OUTSIDE as 0.0f / 1.0f / 2.0f */
    const float *weight;     /* w >= 0 at UNKNOWN pixels; NULL: no data term */
    const float *smooth_x;   /* `frames` frames, > 0 at links live in the region; both NULL: every spatial link 1 */
    const float *smooth_y;
    const float *smooth_t;   /* frames - 1 frames (time_periodic: frames), > 0 at live matched links; NULL: every temporal link tau */
    const float *flow_x;     /* dense cols x rows x (frames - 1; time_periodic: frames), whole numbers; both NULL: straight links */
    const float *flow_y;
    const float *boundary;   /* its Dirichlet lines in every frame (no Dirichlet line on any side: unused, may be NULL) */
    float *out;              /* every element the layout names in every frame is written; may equal data or boundary */
    int rc;                  /* out: SC_OK or SC_ERR_* of this job */
} sc_volume_flow_job;
/* Host-only (needs no GPU): SC_OK, or the code a call with these parameters and this layout returns before it runs anything. */
SC_API int sc_hip_volume_flow_check(const sc_volume_wls_params *p, const sc_poisson_layout *l);
/* Device pointers, n volumes of the same shape.  bSync: waits for the stream and records the call's time. */
SC_API int sc_hip_volume_flow_device(void *instance, const sc_volume_wls_params *p, const sc_poisson_layout *l, sc_volume_flow_job *jobs, int n,
                                     bool bSync);
/* One volume on host arrays, as sc_hip_volume_wls: spans in and out through pinned staging, only the named elements of out written. */
SC_API int sc_hip_volume_flow(void *instance, const sc_volume_wls_params *p, const sc_poisson_layout *l, const float *gx, const float *gy,
                              const float *gt, const float *lap, const float *data, const float *state, const float *weight,
                              const float *smooth_x, const float *smooth_y, const float *smooth_t, const float *flow_x, const float *flow_y,
                              const float *boundary, float *out);
/* ---- sub-pixel flow volume solves: bilinear temporal links along a real-valued flow ----------------------------------------------------------
 * sc_hip_volume_flow's call with the flow's values taken as they are: every optical-flow estimator returns real-valued vectors, and on
 * a slow pan or a zoom a rounded flow is the straight link again for half the pixels.  A temporal link joins pixel p of frame t to the
 * bilinear interpolation of frame t + 1 at p + flow(p); the temporal term is
 *     sum_t sum_p lt(p) (sum_k b_k(p) u_{t+1}(q_k(p)) - u_t(p) - gt_t(p))^2
 * over the pixels p that hold a link.  The parameters are sc_volume_wls_params, the jobs sc_volume_flow_job, both unchanged; flow_x and
 * flow_y have sc_hip_volume_flow's layout, and smooth_t and gt stay stored at the link's source element (p, t).  Everything but the
 * temporal term is sc_hip_volume_wls's problem, word for word.
 * Taps.  Per component in float32: x0 = floorf(dx), ax = dx - x0 (one float32 subtraction: exact unless dx is a negative value within
 * 2^-25 of a whole number, where it rounds to 1 and the link is the whole-numbered one), y0 and ay likewise.  The tap columns are
 * x + (int)x0 and one more, the tap rows y + (int)y0 and one more, the four weights the float32 products (1 - ax)(1 - ay), ax (1 - ay),
 * (1 - ax) ay and ax ay, the taps in that order.  A tap whose weight is exactly 0 is no part of the link: a whole-numbered flow has one
 * tap, a flow that is fractional along one axis two; -0.0 is 0.
 * Candidates.  A pixel of the work rectangle (sc_hip_volume_flow's: a Dirichlet line is outside and carries no temporal links) whose
 * frame has a next frame -- or time is periodic -- is a candidate when both components are finite and at most 1e6 in magnitude.  A
 * periodic axis wraps each tap; elsewhere a link with any remaining tap outside the work rectangle is no link.  There is no matching:
 * every candidate holds its link, and any number of links may arrive at a pixel.  With B the matrix whose row p holds b_k(p) at the
 * taps and -1 at p, the temporal term of the system is B^T S B, S = diag(lt): symmetric by construction.
 * Liveness.  A link is dead when its source or any tap is OUTSIDE; it is live when it is not dead and at least one of its up to five
 * points is UNKNOWN.  KNOWN points enter the right-hand side with data's value times their coefficient (b_k at a tap, -1 at the
 * source).  The guidance form's temporal divergence is B^T S gt; the Laplacian form takes lap as it is and does not read gt.
 * What is read: sc_hip_volume_wls's elements, with gt and smooth_t only at the source of a live link (a NaN elsewhere is fine), and the
 * flow at every pixel of the work rectangle of every frame it holds, nowhere else.  The flow arrays must not overlap out.
 * Preconditioner: sc_hip_volume_wls's, unchanged, with straight time links.  tau-bar is the mean of lt over the live links (exactly tau
 * without smooth_t); in w-bar a temporal link's share is lt * (1 where its source is KNOWN, else the sum of b over its KNOWN taps) --
 * for a link of one tap sc_hip_volume_flow's "an UNKNOWN - KNOWN link counts its own weight".  The pin check is the volume call's over
 * these sums.  sc_hip_volume_flow's warning carries over: strong temporal coupling under motion costs iterations (a float64 model, all
 * UNKNOWN, a weight at 3 % of the pixels, 47 x 33 x 5, tol 1e-5: tau 0.1 / 1 / 10 take 11 / 16 / 65 iterations on a pan of (0.5, 0.5)
 * and 13 / 35 / 238 on one of (2.25, -0.75), against 10 / 9 / 8 on a zero flow).  Raise max_iters there.
 * Cost.  The arrivals at a pixel are summed by one lane in their fixed order, so an application of the operator takes time in proportion
 * to the longest row: about four arrivals per pixel under a smooth flow, but a flow that sends L pixels onto one point makes every
 * iteration wait for L dependent loads.  Mark such pixels as occluded (a component that is not finite) where that is what they are.
 * Determinism.  Two runs of one call give the same bytes: the operator and the right-hand side use no float atomics, and wherever the
 * arrivals at a pixel are summed the order is ascending (source index, tap).
 * Ties.  Both flow arrays NULL runs sc_hip_volume_wls's launches and gives its bytes.  No byte tie holds with sc_hip_volume_wls on a
 * flow of zeros, nor with sc_hip_volume_flow on a whole-numbered flow: the temporal operator is applied in product form, B^T (S (B u)),
 * which rounds differently from the assembled diagonal of those calls.  On a whole-numbered flow without collisions the two calls solve
 * the same system.
 * Size, chunks, stop rule, SC_WEIGHTED_POLL, SC_ERR_NOT_CONVERGED, methods, SC_FLAG_FFT_FP64 limits, host waits, sc_run_info:
 * sc_hip_volume_flow's, its 32-bit size rule included ((unknowns per frame) * frames below 2^31 - 1, else SC_ERR_BAD_SIZE).
 * Codes: sc_hip_volume_flow's without the refusal of a value that is not a whole number.
 * Robust penalties along a sub-pixel flow: sc_hip_volume_subflow_robust below.  Not offered: coupled penalties along a sub-pixel flow; a
 * preconditioner that transforms along the trajectories; the 8-bit entry points; an estimator of the flow. */
/* Host-only (needs no GPU): SC_OK, or the code a call with these parameters and this layout returns before it runs anything. */
SC_API int sc_hip_volume_subflow_check(const sc_volume_wls_params *p, const sc_poisson_layout *l);
/* Device pointers, n volumes of the same shape.  bSync: waits for the stream and records the call's time. */
SC_API int sc_hip_volume_subflow_device(void *instance, const sc_volume_wls_params *p, const sc_poisson_layout *l, sc_volume_flow_job *jobs, int n,
                                        bool bSync);
/* One volume on host arrays, as sc_hip_volume_flow: spans in and out through pinned staging, only the named elements of out written. */
SC_API int sc_hip_volume_subflow(void *instance, const sc_volume_wls_params *p, const sc_poisson_layout *l, const float *gx, const float *gy,
                                 const float *gt, const float *lap, const float *data, const float *state, const float *weight,
                                 const float *smooth_x, const float *smooth_y, const float *smooth_t, const float *flow_x, const float *flow_y,
                                 const float *boundary, float *out);
/* ---- robust volume solves: Lp penalties in space, time and data on frame stacks ---------------------------------------------------------
 * sc_hip_volume_wls's problem with sc_hip_robust's penalties in place of the squares.  Per channel, with exponents 0 < p, r, q <= 2, the
 * call minimises over the UNKNOWN pixels of all frames
 *     sum w phi_q(u - d; eps_d)  +  sum_live x-links c_x phi_p(dx u - gx; eps_g)  +  sum_live y-links c_y phi_p(dy u - gy; eps_g)
 *                                +  sum_live t-links c_t phi_r(u_{t+1} - u_t - gt; eps_t),
 * phi the robust call's penalty; c_x, c_y are smooth_x, smooth_y (NULL: 1) and c_t = lt, the float32 product tau * smooth_t rounded once
 * (NULL: tau), exactly as in sc_hip_volume_wls.  The value of u at a KNOWN pixel is data's, on a Dirichlet line of the border kind
 * boundary's.  Total-variation denoising of video that does not flicker (p = 1, r = 1 or 2, q = 2), integrating a video's gradient field
 * or a stack of edited gradients when some of them are grossly wrong (a bad flow vector, a shot cut, a specular frame), TV inpainting of
 * a moving hole, robust propagation from keyframes -- each on a domain of any shape.
 * States, the liveness of spatial and temporal links, periodic time, the arrays' lengths, what is read and what is written:
 * sc_hip_volume_wls's, word for word.  gt NULL means zeros: it is not read and the residual of a temporal link is the plain difference.
 * weight NULL means no data term: p_data and eps_data are validated and unused.  There is no lap: the residual of a link needs g itself
 * (the base kind must be SC_POISSON_GUIDANCE).
 * Solved by iteratively reweighted least squares, as sc_hip_robust.  Round 0 is sc_hip_volume_wls's system with the caller's arrays, set
 * up and cold-started as that call does.  Round k >= 1 is the same system with s = c rho(link residual) on every live link (rho_p on
 * the spatial, rho_r on the temporal ones) and w' = w rho_q(u - d), taken at round k - 1's iterate: each a rounded float32 product, and
 * with exponent 2 the base value passes through without a multiply (rho in float32: sc_hip_robust's).  Both ends of a link take its
 * residual as t = (u_hi - u_lo) - g with the same bits.  The right-hand side of round k is the seven steps of the WLS volume section in
 * that order with those links, its diagonal (((lw + le) + (ln + ls)) + (lb + lf)) + w'; its solve starts warm from the iterate.  The
 * preconditioner's means are each round's own: s-bar the mean of the live spatial s, tau-bar the mean of the live temporal s, w-bar =
 * (the sum of w' + the sum of the UNKNOWN - KNOWN links' s) / (the UNKNOWN pixels); the table along the frames and the modes' shifts
 * are rebuilt per round.  One launch (k_volume_robust_setup) and one host read per round, as in the robust call.
 * Rounds, max_rounds, round_tol (judged per plane: a channel's whole volume), SC_ERR_NOT_CONVERGED, sc_run_info and the trace
 * (sc_hip_robust_trace): sc_hip_robust's.  Size, chunks, methods, SC_FLAG_FFT_FP64 limits: sc_hip_volume's.
 * Ties: with p_grad = p_time = p_data = 2 no round runs and the call writes the bytes of sc_hip_volume_wls with default precond_* and the
 * same tol and max_iters.  Link arrays of 1.0f give the bytes of NULL arrays.  Two runs of one call give the same bytes.
 * Codes: everything sc_hip_volume_wls_check refuses; everything sc_hip_robust_check refuses for exponents, eps, tol, round_tol and a
 * Laplacian base; SC_ERR_BAD_ARG for SC_ROBUST_ISOTROPIC / SC_ROBUST_JOINT_CHANNELS in kind.  Per job: the WLS volume call's refusals;
 * the first volume decides for weight and for the link arrays.
 * Not offered here: the coupled forms -- kind refuses their bits; sc_hip_volume_coupled below takes a coupling of its own, time
 * included --, motion-compensated temporal links (sc_hip_volume_flow_robust below); anywhere: the 8-bit entry points.  A single image
 * with states and robust penalties is sc_hip_region_robust's, which also takes the coupled forms. */
typedef struct sc_volume_robust_params {
    int       kind;              /* as sc_volume_wls_params.kind; the base must be SC_POISSON_GUIDANCE */
    int       frames;            /* >= 2 (>= 3 with time_periodic); frames * channels <= SC_POISSON_MAX_PLANES */
    long long frame_stride;      /* floats from a frame to the next in every array; at least the span of one frame under the layout */
    float     tau;               /* multiplies every temporal base link; finite, > 0 */
    int       time_periodic;     /* 0: the ends of time are free; 1: frame frames - 1 is linked to frame 0 */
    float     p_grad, eps_grad;  /* spatial links:  0 < p <= 2; eps finite, > 0 (unused when p == 2) */
    float     p_time, eps_time;  /* temporal links: likewise */
    float     p_data, eps_data;  /* data term:      likewise */
    int       max_rounds;        /* reweighting rounds after the quadratic solve; <= 0: 15 */
    float     round_tol;         /* stop when no plane's energy fell by more than round_tol * its energy in the last round; 0: 1e-4; < 0: never stop early */
    float     tol;               /* inner solves: ||r||_2 <= tol * ||b||_2 on every (volume, channel); <= 0: 1e-5 */
    int       max_iters;         /* per inner solve; <= 0: 400 */
} sc_volume_robust_params;
typedef struct sc_volume_robust_job {   /* sc_volume_wls_job without lap */
    const float *gx, *gy;    /* `frames` frames, read at links live in the region: required */
    const float *gt;         /* frames - 1 frames (time_periodic: frames), read at live temporal links; NULL: zeros */
    const float *data;       /* the values at KNOWN pixels, copied at OUTSIDE ones; d of the data term at UNKNOWN ones when weight is given */
    const float *state;      /* SC_REGION_UNKNOWN / _KNOWN / _OUTSIDE as 0.0f / 1.0f / 2.0f */
    const float *weight;     /* w >= 0 at UNKNOWN pixels; NULL: no data term */
    const float *smooth_x;   /* the base links c > 0 at links live in the region; both NULL: every spatial base link 1 */
    const float *smooth_y;
    const float *smooth_t;   /* > 0 at live temporal links; NULL: every temporal base link tau */
    const float *boundary;   /* its Dirichlet lines in every frame (no Dirichlet line on any side: unused, may be NULL) */
    float *out;              /* every element the layout names in every frame is written; may equal data or boundary */
    int rc;                  /* out: SC_OK or SC_ERR_* of this job */
} sc_volume_robust_job;
/* Host-only (needs no GPU): SC_OK, or the code a call with these parameters and this layout returns before it runs anything. */
SC_API int sc_hip_volume_robust_check(const sc_volume_robust_params *p, const sc_poisson_layout *l);
/* Device pointers, n volumes of the same shape.  bSync: waits for the stream and records the call's time. */
SC_API int sc_hip_volume_robust_device(void *instance, const sc_volume_robust_params *p, const sc_poisson_layout *l, sc_volume_robust_job *jobs,
                                       int n, bool bSync);
/* One volume on host arrays, as sc_hip_volume_wls: spans in and out through pinned staging, only the named elements of out written. */
SC_API int sc_hip_volume_robust(void *instance, const sc_volume_robust_params *p, const sc_poisson_layout *l, const float *gx, const float *gy,
                                const float *gt, const float *data, const float *state, const float *weight, const float *smooth_x,
                                const float *smooth_y, const float *smooth_t, const float *boundary, float *out);
/* ---- robust flow volume solves: Lp penalties along a caller's motion field ------------------------------------------------------------------
 * sc_hip_volume_robust's problem, parameters and rounds, word for word, with every temporal link -- its weight lt = tau * smooth_t, its
 * guidance gt, its penalty phi_r -- on the matched link of sc_hip_volume_flow.  Per channel the call minimises over the UNKNOWN pixels
 *     sum w phi_q(u - d; eps_d)  +  sum_live x-links c_x phi_p(dx u - gx; eps_g)  +  sum_live y-links c_y phi_p(dy u - gy; eps_g)
 *                                +  sum_(matched live links i -> m(i)) c_t(i) phi_r(u(m(i)) - u(i) - gt(i); eps_t).
 * A wrong flow vector ties two surface points that disagree; under p_time = 1 such a link is down-weighted round by round where the
 * quadratic link of sc_hip_volume_flow smears across it.  Total-variation denoising of a panning shot that neither blurs along the
 * motion nor flickers, integrating a video's gradients with gt taken along the flow, robust propagation from keyframes.
 * The parameters are sc_volume_robust_params, unchanged; coupling bits in kind are refused as there.  flow_x, flow_y, the matching, the
 * liveness of a matched link, where lt and gt of a link are stored (at its source) and what is read: sc_hip_volume_flow's, word for
 * word -- gt and smooth_t only where a live matched link has its source, the flow at every pixel of the work rectangle of every frame
 * it holds and nowhere else.  The matching is built once per chunk and again when a volume leaves the chunk.
 * Rounds.  Round 0 is sc_hip_volume_flow's system with the caller's arrays and default precond_*, cold-started.  Round k >= 1 is that
 * system with s = c rho(link residual) on every live link and w' = w rho_q(u - d) at round k - 1's iterate, as in sc_hip_volume_robust;
 * the residual of a temporal link is t = (u(m(i)) - u(i)) - gt(i), computed by both of its ends with the same bits, so the system stays
 * symmetric.  One launch (k_volume_flow_robust_setup) and one host read per round.  The means are each round's own and a temporal link
 * is counted once, at its source.  The preconditioner keeps straight time links (sc_hip_volume_flow: what that costs): a temporal L1
 * penalty with a small eps_time raises the temporal weights by up to 1 / eps_time where the iterate is flat along the flow, which
 * together with several pixels of motion is the expensive regime of that section's table.  Raise eps_time or max_iters there.
 * Ties: flow arrays of zeros give the bytes, the rounds and the inner iteration counts of sc_hip_volume_robust; both arrays NULL (in
 * every volume) runs sc_hip_volume_robust's launches; p_grad = p_time = p_data = 2 gives the bytes of sc_hip_volume_flow with default
 * precond_*; link arrays of 1.0f give the bytes of NULL arrays.  Two runs of one call give the same bytes.
 * Trace, rounds, max_rounds, round_tol, SC_ERR_NOT_CONVERGED, sc_run_info: sc_hip_volume_robust's.  Size: sc_hip_volume_flow's 32-bit rule.
 * Codes: everything sc_hip_volume_robust_check refuses, then SC_ERR_BAD_SIZE as sc_hip_volume_flow_check.  Per job SC_ERR_BAD_ARG --
 * nothing of the job is written, the others run -- for every per-job refusal of sc_hip_volume_robust; exactly one of flow_x / flow_y; a
 * flow where the first volume has none, or the reverse; a flow array overlapping out; a finite flow value, where the flow is read,
 * that is not a whole number.
 * Not offered: a preconditioner along the trajectories, the 8-bit entry points.  A real-valued flow: sc_hip_volume_subflow_robust below,
 * with these jobs.  The coupled forms along a flow: sc_hip_volume_flow_coupled below, with these jobs. */
typedef struct sc_volume_flow_robust_job {   /* sc_volume_robust_job and the two flow arrays, as sc_volume_flow_job has them */
    const float *gx, *gy;    /* `frames` frames, read at links live in the region: required */
    const float *gt;         /* frames - 1 frames (time_periodic: frames), read at live matched links; NULL: zeros */
    const float *data;       /* the values at KNOWN pixels, copied at OUTSIDE ones; d of the data term at UNKNOWN ones when weight is given */
    const float *state;      /* SC_REGION_UNKNOWN / _KNOWN / _OUTSIDE as 0.0f / 1.0f / 2.0f */
    const float *weight;     /* w >= 0 at UNKNOWN pixels; NULL: no data term */
    const float *smooth_x;   /* the base links c > 0 at links live in the region; both NULL: every spatial base link 1 */
    const float *smooth_y;
    const float *smooth_t;   /* > 0 at live matched links; NULL: every temporal base link tau */
    const float *flow_x;     /* dense cols x rows x (frames - 1; time_periodic: frames), whole numbers; both NULL: straight links */
    const float *flow_y;
    const float *boundary;   /* its Dirichlet lines in every frame (no Dirichlet line on any side: unused, may be NULL) */
    float *out;              /* every element the layout names in every frame is written; may equal data or boundary */
    int rc;                  /* out: SC_OK or SC_ERR_* of this job */
} sc_volume_flow_robust_job;
/* Host-only (needs no GPU): SC_OK, or the code a call with these parameters and this layout returns before it runs anything. */
SC_API int sc_hip_volume_flow_robust_check(const sc_volume_robust_params *p, const sc_poisson_layout *l);
/* Device pointers, n volumes of the same shape.  bSync: waits for the stream and records the call's time. */
SC_API int sc_hip_volume_flow_robust_device(void *instance, const sc_volume_robust_params *p, const sc_poisson_layout *l,
                                            sc_volume_flow_robust_job *jobs, int n, bool bSync);
/* One volume on host arrays, the arrays of sc_hip_volume_robust in its order with flow_x, flow_y behind smooth_t -- before boundary
 * and out, the place sc_hip_volume_flow and both flow job structs give them, not directly in front of out. */
SC_API int sc_hip_volume_flow_robust(void *instance, const sc_volume_robust_params *p, const sc_poisson_layout *l, const float *gx,
                                     const float *gy, const float *gt, const float *data, const float *state, const float *weight,
                                     const float *smooth_x, const float *smooth_y, const float *smooth_t, const float *flow_x,
                                     const float *flow_y, const float *boundary, float *out);
/* ---- robust sub-pixel flow volume solves: Lp penalties on bilinear temporal links -----------------------------------------------------------
 * sc_hip_volume_robust's problem, parameters and rounds with every temporal link -- its weight c_t = tau * smooth_t, its guidance gt, its
 * penalty phi_r -- on the bilinear link of sc_hip_volume_subflow: the flow's values are taken as they are.  Per channel the call
 * minimises over the UNKNOWN pixels of all frames
 *     sum w phi_q(u - d; eps_d)  +  sum_live x-links c_x phi_p(dx u - gx; eps_g)  +  sum_live y-links c_y phi_p(dy u - gy; eps_g)
 *                                +  sum_(live links p) c_t(p) phi_r(sum_k b_k(p) u~(q_k(p)) - u~(p) - gt(p); eps_t),
 * u~ = u at an UNKNOWN pixel and data at a KNOWN one.  The call for a caller whose flow comes from an estimator -- real-valued, and
 * wrong in places: the flow is not rounded, and under p_time = 1 a link along a wrong vector is down-weighted round by round.
 * The parameters are sc_volume_robust_params, the jobs sc_volume_flow_robust_job, both unchanged; coupling bits in kind are refused.
 * The taps (q_k, b_k), the candidates, the liveness of a link, where smooth_t and gt of a link are stored (at its source) and what is
 * read: sc_hip_volume_subflow's, word for word -- no whole-number refusal, no matching, any number of links may arrive at a pixel.
 * Rounds.  Round 0 is sc_hip_volume_subflow's system with the caller's arrays and default precond_*, cold-started.  Round k >= 1 is that
 * system with three replacements at round k - 1's iterate: the weight of the link p holds is robust_link's s = c_t(p) rho_r(t), t =
 * (hi - u~(p)) - gt(p) with hi = sum_k b_k u~(q_k) accumulated in float32 in tap order (r = 2: c_t(p) in every round); the spatial links
 * and w' are sc_hip_volume_robust's; the right-hand side's temporal part is B^T S g' with that S.  A link's weight is stored once, at its
 * source, and both the source's and the taps' rows of the operator read it there: symmetric by construction.  Two launches
 * (k_subflow_robust_sigma, k_subflow_robust_setup) and one host read per round; the transposed links are built once per chunk and
 * again when a volume leaves it.  The means are each round's own: tau-bar the mean of the links' weights, a link's share of w-bar its
 * weight times (1 where its source is KNOWN, else the sum of b over its KNOWN taps).  The preconditioner keeps straight time links:
 * sc_hip_volume_subflow's and sc_hip_volume_flow_robust's warnings both hold -- a temporal L1 penalty with a small eps_time under a flow
 * that moves pixels is the expensive regime.  Raise eps_time or max_iters there.
 * Ties: both arrays NULL (in every volume) runs sc_hip_volume_robust itself; p_grad = p_time = p_data = 2 gives the bytes of
 * sc_hip_volume_subflow with default precond_*; link arrays of 1.0f give the bytes of NULL arrays; two runs of one call give the same
 * bytes, whatever arrives where.  No byte tie holds with sc_hip_volume_flow_robust on a whole-numbered flow (the product form rounds
 * differently); without collisions the two calls run the same rounds.
 * Trace, rounds, max_rounds, round_tol, SC_ERR_NOT_CONVERGED, sc_run_info: sc_hip_volume_robust's.  Size: sc_hip_volume_flow's 32-bit rule.
 * Codes: everything sc_hip_volume_robust_check refuses, then SC_ERR_BAD_SIZE as sc_hip_volume_subflow_check.  Per job SC_ERR_BAD_ARG --
 * nothing of the job is written, the others run -- for every per-job refusal of sc_hip_volume_robust; exactly one of flow_x / flow_y; a
 * flow where the first volume has none, or the reverse; a flow array overlapping out.
 * Not offered: coupled penalties along a sub-pixel flow, a preconditioner along the trajectories, the 8-bit entry points. */
/* Host-only (needs no GPU): SC_OK, or the code a call with these parameters and this layout returns before it runs anything. */
SC_API int sc_hip_volume_subflow_robust_check(const sc_volume_robust_params *p, const sc_poisson_layout *l);
/* Device pointers, n volumes of the same shape (flow_x, flow_y: real values).  bSync: waits for the stream and records the call's time. */
SC_API int sc_hip_volume_subflow_robust_device(void *instance, const sc_volume_robust_params *p, const sc_poisson_layout *l,
                                               sc_volume_flow_robust_job *jobs, int n, bool bSync);
/* One volume on host arrays, the arrays of sc_hip_volume_flow_robust in its order. */
SC_API int sc_hip_volume_subflow_robust(void *instance, const sc_volume_robust_params *p, const sc_poisson_layout *l, const float *gx,
                                        const float *gy, const float *gt, const float *data, const float *state, const float *weight,
                                        const float *smooth_x, const float *smooth_y, const float *smooth_t, const float *flow_x,
                                        const float *flow_y, const float *boundary, float *out);
/* ---- coupled volume solves: isotropic, space-time and joint-channel total variation on frame stacks ---------------------------------------
 * sc_hip_volume_robust with one penalty over several links, as SC_ROBUST_ISOTROPIC and SC_ROBUST_JOINT_CHANNELS couple them on single
 * images (sc_hip_robust, sc_hip_region_robust) -- and a volume's third axis, which those two bits cannot describe.  The parameters and
 * the jobs are sc_hip_volume_robust's, unchanged; the coupling comes beside them (p->kind carries no coupling bits here either):
 *     SC_VOLUME_COUPLE_SPACE     one penalty per pixel over its x- and its y-link: per frame the isotropic total variation (p_grad = 1),
 *                                ROF as usually meant -- discs stay discs where the anisotropic form makes them diamonds;
 *     SC_VOLUME_COUPLE_TIME      ... and its forward temporal link in the same magnitude: the space-time total variation, which
 *                                penalises a moving edge once, as one surface.  Comes with SPACE; p_time = p_grad, eps_time = eps_grad;
 *     SC_VOLUME_COUPLE_CHANNELS  every magnitude sums over the channels of a volume: the vectorial total variation, no colour fringes.
 * Owners and magnitudes.  The owner of a link is its low end, as in sc_hip_region_robust: the last pixel of a periodic axis owns the
 * wrapping link, the earlier frame a temporal link, frame frames - 1 the wrapping temporal link.  A pixel of a low Dirichlet line owns
 * only its one spatial link into the domain, which forms a magnitude of its own; it owns no temporal link (a Dirichlet pixel's temporal
 * neighbour is a Dirichlet pixel: the link is never live).  For a live link t = (u_hi - u_lo) - g and a = c t^2, c = smooth_x or smooth_y
 * (NULL: 1, no multiply) or lt = tau * smooth_t rounded once (NULL: tau).  A dead link adds nothing to a magnitude; an owner with no
 * live link adds nothing to the energy.  With psi_e(M; eps) = (2 / e) (M + eps^2)^(e/2), the gradient-plus-time term of the energy is
 *     0                         sc_hip_volume_robust's, to the byte
 *     SPACE                     sum_k sum_pixels psi_p(a_x + a_y; eps_g)  +  sum_k sum_t-links c_t phi_r(t_t; eps_t)
 *     SPACE | TIME              sum_k sum_pixels psi_p((a_x + a_y) + a_t; eps_g)
 *     CHANNELS                  sum_x-links psi_p(sum_k a_x)  +  sum_y-links psi_p(sum_k a_y)  +  sum_t-links psi_r(sum_k a_t; eps_t)
 *     SPACE | CHANNELS          sum_pixels psi_p(sum_k (a_x + a_y))  +  sum_t-links psi_r(sum_k a_t; eps_t)
 *     SPACE | TIME | CHANNELS   sum_pixels psi_p(sum_k ((a_x + a_y) + a_t))
 * The data term stays per pixel and per channel.  Under CHANNELS a magnitude sums only the channels in which that link is live (state
 * is per channel).  TIME without SPACE is SC_ERR_BAD_ARG, and so are unknown bits; TIME with p_time != p_grad or eps_time != eps_grad
 * (compared as floats) is SC_ERR_BAD_ARG: there is one penalty.
 * Float32 order, as in the robust sections: t t is rounded, then multiplied by c and rounded; within a pixel the sum is (a_x + a_y) + a_t;
 * then the running sum over channels 0 .. C - 1; Q = M + eps eps; rho = 1.0f / sqrtf(Q) for exponent 1, powf(Q, (e - 2) / 2) otherwise;
 * s = c rho, one rounded product.  A magnitude whose exponent is 2 gives rho exactly 1: the base value passes through without a
 * multiply, and its links' energy is booked link by link, c t^2.  Both ends of a link read the same rho bits.
 * Rounds.  Round 0 is sc_hip_volume_wls's system, untouched.  Round k >= 1 is the WLS volume system with s = c rho(M) on every link
 * that shares M and w' = w rho_q(u - d).  The right-hand side, the diagonal, the warm start and each round's means (s-bar, tau-bar,
 * w-bar) follow sc_hip_volume_robust word for word, and the region family's zero condition holds after every round.  Two launches per
 * coupled round (k_volume_robust_rho: rho of every owner's magnitudes and the gradient-and-time energy; k_volume_robust_setup_rho: the
 * system with s read from them) and still one host read.  The rho planes live in the instance's arena: per volume and channel (under
 * CHANNELS: per volume) frames * (the frame's pixels, rounded up to 64) floats for each component -- one under SPACE | TIME, two under
 * SPACE, three otherwise, a component whose exponent is 2 not stored; where the arena cannot grow the call returns SC_ERR_HIP.
 * Effective coupling.  SPACE and TIME change nothing when p_grad = 2; CHANNELS changes nothing on one channel or when p_grad = p_time = 2.
 * A call whose effective coupling is 0 runs the uncoupled launch and writes the bytes of sc_hip_volume_robust.
 * Under CHANNELS the round rule judges a volume's energy, the sum over its channels; otherwise a plane's.  sc_hip_robust_trace reports
 * this call too.  max_rounds, round_tol, SC_ERR_NOT_CONVERGED, sc_run_info, sizes, chunks (a chunk holds whole volumes), methods and
 * SC_FLAG_FFT_FP64 limits: sc_hip_volume_robust's.
 * Codes: everything sc_hip_volume_robust_check refuses, coupling bits in kind included; the two refusals of a coupling above.  Per
 * job: the robust volume call's refusals.
 * Not offered: a coupled data term, a separate s-bar for x and y, bounds on volumes, the 8-bit entry points.  Motion-compensated
 * temporal links under a coupling: sc_hip_volume_flow_coupled below, with these parameters and this coupling. */
#define SC_VOLUME_COUPLE_SPACE    1   /* one penalty per pixel over its x- and y-link (per frame isotropic TV)          */
#define SC_VOLUME_COUPLE_TIME     2   /* ... and its forward temporal link in the same magnitude (space-time TV)       */
#define SC_VOLUME_COUPLE_CHANNELS 4   /* every magnitude sums over the channels of a volume (vectorial TV)            */
/* Host-only (needs no GPU): SC_OK, or the code a call with these parameters, this coupling and this layout returns before it runs anything. */
SC_API int sc_hip_volume_coupled_check(const sc_volume_robust_params *p, int coupling, const sc_poisson_layout *l);
/* Device pointers, n volumes of the same shape.  bSync: waits for the stream and records the call's time. */
SC_API int sc_hip_volume_coupled_device(void *instance, const sc_volume_robust_params *p, int coupling, const sc_poisson_layout *l,
                                        sc_volume_robust_job *jobs, int n, bool bSync);
/* One volume on host arrays, the arrays of sc_hip_volume_robust in its order. */
SC_API int sc_hip_volume_coupled(void *instance, const sc_volume_robust_params *p, int coupling, const sc_poisson_layout *l, const float *gx,
                                 const float *gy, const float *gt, const float *data, const float *state, const float *weight,
                                 const float *smooth_x, const float *smooth_y, const float *smooth_t, const float *boundary, float *out);
/* ---- coupled flow volume solves: isotropic, space-time and joint-channel total variation along a caller's motion field --------------------
 * sc_hip_volume_coupled with every temporal link along a flow: the video total-variation solve when something moves -- isotropic in
 * space, so that discs stay discs; vectorial, so that there are no colour fringes; and its temporal term compares a surface point
 * with itself in the next frame.  The parameters are sc_volume_robust_params, the coupling SC_VOLUME_COUPLE_*, the job
 * sc_volume_flow_robust_job, all unchanged.
 * Problem.  sc_hip_volume_coupled's energy table, word for word, in which every temporal link is the matched live link i -> m(i) of
 * sc_hip_volume_flow; its base weight lt = tau * smooth_t and its gt are stored at its source i.  flow_x, flow_y, the matching, the
 * liveness of a matched link and what is read: sc_hip_volume_flow's, word for word.
 * Owners and magnitudes.  The owner of a temporal link is its source, the pixel that holds it (not "the earlier frame": under periodic
 * time and under a flow the target's frame is in the link); spatial owners are sc_hip_volume_coupled's.  Under SPACE | TIME a pixel's
 * magnitude is (a_x + a_y) + a_t with a_t that of the link the pixel holds; a pixel that holds no live link -- occluded (NaN), the
 * loser of a collision's claim, its target off the rectangle, or a dead end -- has a_t add nothing.  A link that arrives at a pixel
 * plays no part in that pixel's magnitude.  Under CHANNELS a magnitude sums the channels in which that link is live: the matching is
 * per volume, liveness per channel.  TIME without CHANNELS or SPACE | TIME leaves the temporal link its uncoupled penalty c_t phi_r,
 * exactly as in sc_hip_volume_coupled.
 * Float32 order: sc_hip_volume_coupled's -- t t rounded, then times c rounded; (a_x + a_y) + a_t; then the running sum over channels
 * 0 .. C - 1.  The residual of a temporal link is t = (u(m(i)) - u(i)) - gt(i), computed on the same operands by whoever needs it.  Both
 * ends of every link read the same rho bits from the rho planes, so the system stays symmetric: a temporal link's rho is written once,
 * by its source, at the source's element, and the pixel it arrives at reads it there, through the matching's backward index.
 * Rounds.  Round 0 is sc_hip_volume_flow's system with the caller's arrays and default precond_*, cold-started.  Round k >= 1 is as in
 * sc_hip_volume_coupled, with the means counted as sc_hip_volume_flow_robust counts them: a temporal link once, at its source.  Two
 * launches (k_volume_flow_robust_rho, k_volume_flow_robust_setup_rho) and one host read per coupled round; the matching is built once
 * per chunk and again when a volume leaves the chunk.  The rho planes: sc_hip_volume_coupled's.
 * Effective coupling: sc_hip_volume_coupled's rule.  A call whose effective coupling is 0 runs k_volume_flow_robust_setup and writes the
 * bytes of sc_hip_volume_flow_robust.
 * The preconditioner keeps straight time links (sc_hip_volume_flow: what that costs): a temporal or space-time L1 penalty with a small
 * eps raises the temporal weights by up to 1 / eps where the iterate is flat along the flow, which together with several pixels of
 * motion is the expensive regime of that section's table.  Raise eps or max_iters there.
 * Ties, to the byte (the first two also in the trace's rounds and inner iteration counts): flow arrays of zeros (-0.0f among them)
 * give sc_hip_volume_coupled's result; both flow arrays NULL in every volume runs sc_hip_volume_coupled's launches; every exponent 2
 * gives the bytes of sc_hip_volume_flow with default precond_*; link arrays of 1.0f give the bytes of NULL arrays; two runs give the
 * same bytes.
 * Trace (sc_hip_robust_trace reports this call too), round rule, max_rounds, round_tol, SC_ERR_NOT_CONVERGED, sc_run_info, chunks,
 * methods, SC_FLAG_FFT_FP64 limits: sc_hip_volume_coupled's.  Size: sc_hip_volume_flow's 32-bit rule.
 * Codes: everything sc_hip_volume_coupled_check refuses, then SC_ERR_BAD_SIZE as sc_hip_volume_flow_check gives it.  Per job:
 * sc_hip_volume_flow_robust's refusals.
 * Not offered: a coupled data term, sub-pixel flow, a preconditioner along the trajectories, the 8-bit entry points. */
/* Host-only (needs no GPU): SC_OK, or the code a call with these parameters, this coupling and this layout returns before it runs anything. */
SC_API int sc_hip_volume_flow_coupled_check(const sc_volume_robust_params *p, int coupling, const sc_poisson_layout *l);
/* Device pointers, n volumes of the same shape.  bSync: waits for the stream and records the call's time. */
SC_API int sc_hip_volume_flow_coupled_device(void *instance, const sc_volume_robust_params *p, int coupling, const sc_poisson_layout *l,
                                             sc_volume_flow_robust_job *jobs, int n, bool bSync);
/* One volume on host arrays, the arrays of sc_hip_volume_flow_robust in its order. */
SC_API int sc_hip_volume_flow_coupled(void *instance, const sc_volume_robust_params *p, int coupling, const sc_poisson_layout *l, const float *gx,
                                      const float *gy, const float *gt, const float *data, const float *state, const float *weight,
                                      const float *smooth_x, const float *smooth_y, const float *smooth_t, const float *flow_x,
                                      const float *flow_y, const float *boundary, float *out);
/* Host-only: what decides a ROI size's class: out = { eligible, levels, level held by k_mg_tail (THE class key, beside the 2x spread),
 * operand padding x, y of the level solved directly, mode-block padding x, y of the correction, its column tiles, its row splits,
 * 1000 * nx + ny of the level solved directly, solo_differs (1: a small ROI whose level 1 a solo clone solves directly -- inside a
 * class it runs the general hierarchy and comes out within one grey level of its solo run instead of with its bytes), conditional
 * (1: the float tables' lowest modes are off by more than 4 % at this size; such members form classes of their own, in which the
 * judged cycle's measured update decides the output's form for the whole group) } */
SC_API int sc_hip_plan_size(int W, int H, const sc_solver_opts *opts, int out[12]);
/* Host-only: plans and per-size host tables (the float-table correction's ratio table, its part maps) are pure functions of the ROI
 * size and memoised process-wide on first use -- 5-20 us of host arithmetic per NEW size, paid inside the first batch call that meets
 * it.  A caller that knows its sizes ahead (a set of patch templates, the boxes of the previous frame) moves that out of its latency
 * path: prepares wh[2i], wh[2i+1] (ring included) under `opts` (NULL: the defaults); returns how many of them can join a size class.
 * sc_hip_plan_cache_clear forgets everything memoised (tests and measurements). */
SC_API int sc_hip_plan_prepare(const int *wh, int n, const sc_solver_opts *opts);
SC_API void sc_hip_plan_cache_clear(void);

/* Host-only (needs no GPU): 1 when the reference's float32 eigenvalue tables are singular for an ROI of w x h unknowns --
 * (float)(2 cos(PI/(n+1))) is exactly 2.0f in both directions (n >= ~12 870), so the reference's denominator
 * filter_X[0] + filter_Y[0] - 4 (seamlessClone_imp.cpp:1651-1653) is zero and its result undefined.  For such ROIs the
 * default path and SC_METHOD_DST return the exact system's solution (as SC_FLAG_EXACT_TABLES does). */
SC_API int sc_hip_reference_tables_singular(int w, int h);

#ifdef __cplusplus
}
#endif
#endif /* SEAMLESSCLONE_HIP_H */
