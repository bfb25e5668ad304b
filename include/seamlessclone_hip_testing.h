/*
 * seamlessclone_hip_testing.h -- the test and measurement surface of libseamlessclone_hip.so (MI355X / gfx950).
 *
 * Not part of the drop-in boundary: an integrator includes seamlessclone_hip.h only.  What is declared here serves the
 * parity tests, bench.py and the tools: the flags that run superseded launch forms or debugging aids, the stage-level
 * hooks that drive one kernel at a time, the microbenchmarks and the host-only self test.  The symbols come from the
 * same library.
 */
#ifndef SEAMLESSCLONE_HIP_TESTING_H
#define SEAMLESSCLONE_HIP_TESTING_H

#include "seamlessclone_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- sc_solver_opts.flags bits for tests and measurements (the drop-in header leaves bits 6, 7 and 14 to them) */
#define SC_FLAG_LEGACY_PATHS   (1 << 6)  /* run the superseded launch forms named in sc_solver_opts.legacy_paths (round 5: one switch for the
                                            A/B scaffolding of decisions that are made; rounds 2-4 had a public flag for each):           */
#define SC_LEGACY_SEPARATE_RESTRICT 1    /*   float-table correction: the hat-weighted cell sums of the field come from a pass of their own
                                            over it (k_lm_restrict); default: the level-0 multigrid launch that writes the field leaves them
                                            behind.  Same cells, another order of the additions (differences at float rounding level)     */
#define SC_LEGACY_BOTTOM_F32   2         /*   multigrid: the bottom kernel's direct solve as float32 SIMD inner products with every operand
                                            staged in LDS (k_mg_bottom, rounds 1-3) on the hierarchy of those rounds.  Default since round 4
                                            where the bottom's first level has at most 96 unknowns per side: four products on the matrix
                                            cores in float32 (v_mfma_f32_32x32x2_f32: k_mg_bottom_mm).  Same arithmetic up to the order of
                                            the additions                                                                               */
#define SC_LEGACY_SEPARATE_TAIL 4        /*   multigrid: the level above the bottom and the bottom as the three launches of rounds 1-3
                                            (pre-smoothing + residual + restriction, direct solve, prolongation + post-smoothing).  Default
                                            since round 4 where that level has at most 127 unknowns per side: ONE launch, the level in
                                            registers (k_mg_tail).  Same arithmetic per point                                            */
#define SC_LEGACY_UNPACKED_TILES 8        /*   multigrid, coarse levels: every column tile in a workgroup of its own.  Default: where the last
                                            column tile of a level needs at most half a wave, one workgroup serves that tile of several
                                            planes (sc_hip_coarse_tile_plan).  Same values, bit for bit                                   */
#define SC_LEGACY_SPLICE_LAUNCH 16        /*   multigrid, same-size groups: the judged cycle always leaves its bytes planar and a splice launch
                                            (k_splice_planar_group) interleaves them into the destinations.  Default: from
                                            members x level-0 tiles = SC_OUT3_MIN_TILES on (sc_instance.h) one workgroup of the judged launch
                                            serves the three channels of a member's tile and writes the interleaved bytes itself
                                            (k_cycle0 with C0_OUT3).  Same bytes                                                         */
#define SC_FORCE_INTERLEAVED_OUT 32      /*   ... and that form wherever it exists (a same-size group of up to 16 members on the default
                                            path), whatever the threshold says: tests and A/B runs                                       */
#define SC_LEGACY_U0_PLANES     64        /*   multigrid, same-size groups: the pre-process always stores the destination's 8-bit ROI values as
                                            float16 planes and the first level-0 launch reads those.  Default: from members x level-0 tiles =
                                            SC_IN3_MIN_TILES on (sc_instance.h) the pre-process stores no initial field and one workgroup of
                                            the first launch serves the three channels of a member's tile from the destination's own bytes
                                            (k_cycle0 with C0_IN3).  Same values, same bytes                                              */
#define SC_FORCE_U0_BYTES       128       /*   ... and that form wherever it exists (a same-size group of up to 16 members on the default
                                            path), whatever the threshold says: tests and A/B runs                                       */
#define SC_FLAG_KEEP_FIELD     (1 << 7)  /* sc_hip_run*: keep the solution field on the device (sc_hip_field_store,
                                            _residual, _finish after a run): the last multigrid cycle writes the field
                                            and a post-process launch reads it.  Default: that cycle writes the output
                                            bytes itself and no final field exists (those hooks then fail with
                                            SC_ERR_BAD_ARG); the float-table node correction it adds is the one of the
                                            iterate one cycle earlier (difference at most 0.05 grey levels in the worst case the stop rule admits,
                                            0.001-0.003 measured; ROIs where
                                            that bound does not hold take this flag's path by themselves)        */

#define SC_FLAG_POISON_ARENA   (1 << 14) /* testing: every device block the arena hands out -- or hands out AGAIN -- WITHOUT zeroing it (fields,
                                            level planes, image staging: "written before they are read") is filled with 0xFF bytes first -- NaN as float32 and
                                            float16 -- which is what RECYCLED device memory may hold (fresh memory reads as zero and hides a
                                            read of something never written).  Results must not change (tests/test_gpu_round5.py)            */

/* ---- stage-level hooks (parity tests drive each kernel through these) ------------------- */

/* mask stage only (seamlessClone_imp.cpp:978-1071): geo = {x0,y0,W,H,ltx,lty}; M_out
 * receives the 3x eroded ROI mask, dense W*H bytes (may be NULL). */
SC_API int sc_hip_mask_stage(void *instance, const uint8_t *mask, int mask_cols, int mask_rows, int mask_step,
                      int centerX, int centerY, int geo[6], uint8_t *M_out, size_t M_capacity);

/* mask stage + fused pre-process (seamlessClone_imp.cpp:1920-2018): downloads the dst-ROI
 * field B and the un-folded RHS lap, planar [3][H][W] float32, channel = BGR index. */
SC_API int sc_hip_build_rhs(void *instance,
                     const uint8_t *face, int face_cols, int face_rows, int face_step,
                     const uint8_t *body, int body_cols, int body_rows, int body_step,
                     const uint8_t *mask, int mask_cols, int mask_rows, int mask_step,
                     int centerX, int centerY, int geo[6], float *B_out, float *lap_out, size_t plane_capacity);

/* The front end of n device-resident clones WHERE THE CALLER'S BYTES LIE: face / body / mask of every job are device pointers with the
 * caller's own base and step, handed to the launches as the clone calls hand them.  Runs the scan, the erode and the pre-process and
 * nothing else -- no solve, no output launch, nothing is written to body -- through the functions the clone calls run:
 *   form 0  solo: the scan, the erode (grey: the minimum filter), the pre-process without a scan, one member after the other
 *   form 1  predicted: member i is launched on the rectangle guess[4 i ..] = {x0, x1, y0, y1}; no erode launch, the scan rides in the
 *           pre-process launch as extra workgroup rows and its tiles erode the mask themselves.  M, B and lap belong to the guessed box,
 *           the rectangle to the true one
 *   form 2  group: the scans, the erodes and the tiles of all members as one launch each; every member has the fields' size
 *   form 3  size class: as form 2, the fields take the largest W and H and every member carries its own
 * storage: bit 0 the right-hand side as float16, bit 1 the initial field as float16, bit 2 no initial field stored (groups; B stays
 * untouched); SC_ERR_BAD_ARG for a word no launcher instantiates (0, 1, 3; 7 for groups).  The instance's clone mode and
 * SC_FLAG_OPENCV_GREY_MASK (form 0, storage 0) apply as in a run.
 * Per member i: rect_dev / rect_host [4 i ..] the raw rectangle the scan left in device memory / in the pinned mailbox, geo[6 i ..] =
 * {x0, y0, W, H, ltx, lty} (zeros where jobs[i].rc says the rectangle gives no usable ROI -- the rectangle is still returned), and at
 * member strides of `capacity` pixels: M_out the eroded mask, dense W x H bytes, B_out / lap_out dense [3][H][W] float32 (float16
 * expanded).  M_out, B_out and lap_out may be NULL; all three NULL in forms 0, 2 and 3: the scan alone (a group's masks may then differ
 * in size). */
SC_API int sc_hip_front_end_device(void *instance, sc_batch_job *jobs, int n, int form, int storage, const int *guess, int *rect_dev,
                                   int *rect_host, int *geo, uint8_t *M_out, float *B_out, float *lap_out, size_t capacity);

/* whole-image edit (sc_hip_edit) up to its right-hand side: M_out receives the eroded mask (dense cols * rows bytes), lap_out the
 * un-folded right-hand side, planar [3][rows][cols] float32 (0 on the frame).  Either may be NULL. */
SC_API int sc_hip_edit_rhs(void *instance, const sc_edit_params *p, const uint8_t *src, int cols, int rows, int src_step,
                           const uint8_t *mask, int mask_step, uint8_t *M_out, float *lap_out, size_t plane_capacity);
/* the Canny detector of SC_EDIT_TEXTURE_FLATTENING on a host image: classes_out = the map after non-maximum suppression (0 none,
 * 1 weak, 2 strong), edges_out = the edge map after hysteresis (255 edge, 0 not), dense cols * rows bytes each (either may be NULL);
 * counts[0] = hysteresis launches, counts[1] = mailbox reads (may be NULL).  sc_hip_edit_counts: the same two counts of the last
 * edit (0 unless it was a texture flattening). */
SC_API int sc_hip_canny(void *instance, const uint8_t *src, int cols, int rows, int src_step, float low_threshold,
                        float high_threshold, int kernel_size, uint8_t *classes_out, uint8_t *edges_out, int counts[2]);
SC_API int sc_hip_edit_counts(void *instance, int counts[2]);

/* solver-only hooks on caller-supplied fields, planar [C][H][W] float32 (ring included). */
SC_API int sc_hip_field_load(void *instance, int W, int H, int C, const float *U, const float *lap);
SC_API int sc_hip_field_sweep(void *instance, int method, int sweeps, float omega, int sweeps_per_launch);
SC_API int sc_hip_field_residual(void *instance, double out[2] /* sum r^2, sum lap^2 */);
SC_API int sc_hip_field_solve(void *instance);                      /* run the configured solver on the loaded field */
SC_API int sc_hip_field_shape(void *instance, int whc[3]);   /* W, H, C of the fields currently on the device */
SC_API int sc_hip_field_store(void *instance, float *U_out, size_t capacity_floats);

/* post-process alone (seamlessClone_imp.cpp:2078-2103 and the host splice :470-483) on the field currently on the
 * device (sc_hip_field_load, or what a solve left): clamp to [0,255], truncate, interleave the interior of the
 * 3-channel field into the host image `body` with the ROI origin at (ltx, lty). */
SC_API int sc_hip_field_finish(void *instance, uint8_t *body, int body_cols, int body_rows, int body_step, int ltx, int lty);
/* float-table correction alone on the field currently on the device: the result becomes
 * result + correction, i.e. the exact solution of the 5-point system turns into what the reference's float32
 * eigenvalue tables give (seamlessClone_imp.cpp:596-599, :1651-1653). */
SC_API int sc_hip_field_lowmode(void *instance);

/* microbenchmark hook used by bench.py: runs `launches` launches of the sweep kernel
 * (method, sweeps_per_launch) on the loaded field and returns the mean launch time measured
 * with hipEvents on the instance stream. */
SC_API int sc_hip_field_time_sweeps(void *instance, int method, int launches, int sweeps_per_launch, float omega,
                             float *ms_per_launch);

/* isolated timing of the fused level-0 multigrid cycle kernel on the state left by the last
 * MULTIGRID run (values are discarded; bench.py roofline) */
SC_API int sc_hip_time_cycle0(void *instance, int launches, float *ms_per_launch);
/* ... and of the other three level-0 launches a fast-path solve is made of, each under a second symbol of its own:
 * form 0 = the full cycle (as sc_hip_time_cycle0), 1 = the full cycle before the judged one (16-bit field in, float out, leaves the
 * float-table correction's cell shares), 2 = the judged cycle (two sweeps, output bytes), 3 = the first launch of a solve (two
 * sweeps from the float16 initial field, no prolongation).  SC_ERR_BAD_ARG unless the last run was a default multigrid solve. */
SC_API int sc_hip_time_cycle0_form(void *instance, int form, int launches, float *ms_per_launch);
/* measurement: the launch-bound part of a multigrid cycle (levels 2 .. bottom .. 2 of the hierarchy the last multigrid run left,
 * `*launches` dependent launches) `reps` times as plain launches and as replays of ONE captured HIP graph: ms per pass of each */
SC_API int sc_hip_time_coarse_chain(void *instance, int reps, float *ms_eager, float *ms_graph, int *launches);
/* measurement: the shader clock at the eleven phase boundaries of ONE k_mg_tail launch (the level above the bottom and the bottom in one
 * launch, the default; SC_LEGACY_SEPARATE_TAIL runs three) on the hierarchy the last multigrid run left: entry | right-hand side loaded | pre-smoothing | residual +
 * restriction | the four products of the direct solve | prolongation | post-smoothing | stores issued.  SC_ERR_BAD_ARG unless that
 * hierarchy runs its bottom this way. */
SC_API int sc_hip_time_tail_phases(void *instance, unsigned long long *cycles11);

/* host-only self test (needs no GPU): the parked-thread row copier of the host path and the tridiagonal
 * eigen-solver behind the direct bottom solve (residual of T V = V L for level operators with an irregular
 * last interval).  Returns 0, or the number of the check that failed. */
SC_API int sc_hip_selftest_host(void);

/* host only (needs no GPU, launches nothing): the instantiation k_cycle0<T, .., PRO, .., TAG> (csrc/sc_cycle0.hip; TAG: the C0_* bits of
 * csrc/sc_common.h) the level-0 multigrid launcher picks for facts[13] = sweeps, prolong, f_half, u_half, q16_in, q16_out, final_cycle (u_half + 2: the initial field
 * is read from the members' destination bytes instead, in_bytes),
 * out_bytes (+ 2: as interleaved bytes into the members' destinations, out_interleaved), composed, l1_half, timing, bands (pointer given), rag (size class).  form[3] receives T, PRO, TAG; returns 0, or -1: no such
 * form, nothing would be launched.  facts == NULL: form receives entry `index` of the table of instantiated forms, its length is returned. */
SC_API int sc_hip_cycle0_form(const int *facts, int index, int form[3]);

/* Who wrote the output bytes of the judged multigrid cycles that left bytes on this instance since this was last asked (asking clears
 * it): bit 0 a splice launch behind planar bytes, bit 1 the judged launch itself, interleaved (k_cycle0 with C0_OUT3: same-size groups,
 * see SC_LEGACY_SPLICE_LAUNCH).  SC_ERR_BAD_ARG for a bad handle. */
SC_API int sc_hip_bytes_writer(void *instance);
/* Where the first level-0 launches of the fused multigrid solves on this instance read their initial field since this was last asked
 * (asking clears it): bit 0 the float16 planes the pre-process stored, bit 1 the members' destination bytes (k_cycle0 with C0_IN3,
 * see SC_LEGACY_U0_PLANES), bit 2 float16 planes that a safety-net launch filled because the pre-process had stored none and the
 * solve had no bytes form.  SC_ERR_BAD_ARG for a bad handle. */
SC_API int sc_hip_u0_reader(void *instance);
/* Host only, nothing is launched: what the 64 lanes of a wave whose lane 0 serves column xw fetch of the interleaved ROI row of W
 * pixels at `row` for that form, by the rule the kernel runs (csrc/sc_u0_bytes.h), read from host memory here.
 * out[64][16], per lane = { offset of the first of four dwords from `row`, re-alignment shift, bit k set: dword k was read (the others
 * count as 0), 1: the wave takes the unguarded 16-byte load, then per channel 0, 1, 2 the four values of columns xw + 4 lane .. + 3
 * (clamped as the kernel clamps) }. */
SC_API int sc_hip_u0_bytes_fetch(const uint8_t *row, int W, int xw, int *out);

/* Host only, nothing is launched: the column tiling of a coarse-level multigrid launch and what the lanes of its workgroups serve.
 * facts = { W, H, C (field width and height, ring included; planes), useful width, halo (columns a tile owns; halo columns per side: 232, 12
 * for the way down, 248, 4 for the way up), rows a tile owns, size class (0 / 1), unpacked (1: SC_LEGACY_UNPACKED_TILES), first workgroup,
 * number of workgroups n (0: the plan only) }.
 * plan = { full column tiles (one plane per workgroup), lanes per slot of a packed workgroup, planes per packed workgroup K (1: nothing
 * packed), workgroups of the launch }, then 130 ints for each of the n workgroups from `first workgroup` on (logical numbers): its row
 * tile, its lanes per slot (64: a full tile; lane l is lane l % that of its slot, and a halo lane where that is below halo / 4 or among
 * the last halo / 4), and per lane its plane (>= C: an empty slot) and first column.  Returns 0, SC_ERR_BAD_ARG for facts outside their
 * ranges. */
SC_API int sc_hip_coarse_tile_plan(const int *facts, int *plan);

/* Host only, nothing is launched: the tiling of a level-0 multigrid launch (csrc/sc_cycle0.hip: k_cycle0) on a W x H field (ring
 * included) by the functions its launcher evaluates and, per wave, what the kernel's wave-uniform `inner` test answers -- a restatement of
 * the kernel's lines beside them (csrc/sc_cycle0.hip: cycle0_inner_fail), on the level sizes of the library's own ladder.
 * facts = { W, H, sweeps of the launch (2: first launch, judged cycle; 4: full cycle), prolong (0 / 1), composed (0 / 1: it prolongs from
 * the composed level 1) }.
 * plan = { column tiles nbx, row tiles nby, columns a tile owns, rows a tile owns, halo columns hx, halo rows hy, waves per tile, rows
 * per wave, levels of the ladder, first level of the bottom under the default options, the default tail level (0: none), 1: the default
 * schedule composes level 1, unknowns of level 1 in x and y, unknowns of level 2 in x and y (0: no such level) }, then -- where
 * capacity allows more than these SC_CYCLE0_PLAN_HEAD ints -- one int per wave, (row tile * nbx + column tile) * waves per tile + wave:
 * 0 the wave takes the mask-free forms, else the first condition that fails: 1 xw >= 4, 2 xw + 255 <= W - 2, 3 y0 >= 1,
 * 4 y0 + R - 1 <= H - 2, and of a launch that prolongs 5 level 1's last column, 6 its first row, 7 its last row, composed 8 level 2's
 * last column, 9 its last row (xw = column tile * columns owned - hx, y0 = row tile * rows owned - hy + wave * R).
 * Returns 0; SC_ERR_BAD_ARG for facts outside their ranges, a ladder without the levels asked of it, or too little capacity for the waves. */
#define SC_CYCLE0_PLAN_HEAD 16
SC_API int sc_hip_cycle0_plan(const int *facts, int *plan, int capacity);

/* Host only, nothing is launched: the tiling of the work planes a conjugate-gradient call (sc_hip_weighted, _wls, _robust, _region,
 * _volume, _volume_wls) would run with on images of cols x rows pixels under the border word `kind` (a base kind with its SC_POISSON_NEUMANN,
 * SC_POISSON_FREE_* or SC_POISSON_PERIODIC_* bits, as the calls take it); frames: a volume call's (its frames' unknowns stacked along
 * y), 1: not a volume.  The functions the calls themselves ask (csrc/sc_pcg.h: PcgOperator::work_geo).
 * plan = { nx, ny (the unknowns of a work plane), x0, y0 (the first unknown's pixel), cg (column groups of 256 columns), bands, rows
 * (per band; cg * bands partial sums per plane), eparts (segments of the element-wise launches), egroups (float4 groups of a plane),
 * stride (floats between planes) }.  Returns 0, or the code the calls' checks give this kind and size. */
SC_API int sc_hip_pcg_plan(int cols, int rows, int kind, int frames, long long plan[10]);

/* Host only, nothing is launched: the level-0 launches of a fused multigrid solve (csrc/sc_multigrid.cpp: fused_next, the function the solve
 * itself asks) for facts[12] = pre, post (1 or 2), budget (max_sweeps, 1..64), tol > 0, out_wanted (the splice is armed, no tol, no
 * SC_FLAG_KEEP_FIELD, V(2,2)), q16 (the field starts as 16-bit fixed point), u_half (the initial field is float16), level 1 composed,
 * SC_LEGACY_SEPARATE_RESTRICT, the early node correction's kind (0 nothing to add, 1 allowed, 2 not, 3 allowed if the judged update is
 * small), bytes form instantiated, small (more than 3 planes or fewer than 3 << 18 pixels) -- and for what the read-back behind each
 * judged launch shows: verdicts[k] = 0 accept, 1 reject, 2 an update the stop rule accepts but the early condition does not (an accept
 * where that condition does not apply), 3 the saturation word (an accept unless q16); the last entry repeats, none = accept.
 * rows receives SC_FUSED_ROW ints per launch -- kind (1 first launch, 2 full cycle, 3 full cycle before the judged one, 4 judged cycle
 * leaving bytes, 5 judged cycle leaving its field, 6 catch-up), sweeps, prolong, final_cycle, out_bytes, u_half, q16_in, q16_out,
 * composed, bands (sweeps the bands buffer it receives is sized for, 0: none), lm (carries the early node correction), nodes (a node
 * correction is computed from its result: 1 on the main stream, 2 on the second, 3 there is nothing to add, 0 no), judged (the stop rule
 * reads its maxima), coarse_first (levels 1 .. bottom run in front of it), sat (it is given the saturation word), bands asked (sweeps the
 * bands buffer asked for in front of it is sized for), early kind asked in front of it, cycles completed in front of it -- and behind the
 * last row sc_run_info's sweeps and sweep_launches and the solve's code (0, SC_ERR_NOT_CONVERGED, 1: repeated on float fields).
 * Returns the number of launches, SC_ERR_BAD_ARG for facts outside their ranges or fewer than SC_FUSED_ROW * launches + 3 ints of capacity. */
#define SC_FUSED_ROW 18
SC_API int sc_hip_fused_schedule(const int *facts, const int *verdicts, int nverdicts, int *rows, int capacity);

/* Host only, nothing is launched: the byte spans [begin, end) that sc_hip_run_device_batch copies from sc_batch_job.body_restore for a
 * grouped member whose ROI interior the clone writes -- the image's step x rows bytes without the interior (byte columns
 * [3 (ltx + 1), 3 (ltx + W - 1)) of rows lty + 1 .. lty + H - 2) of the W x H ROI at (ltx, lty).  spans receives begin, end per span in
 * ascending order.  Returns their number; SC_ERR_BAD_ARG for a ROI outside the image or more spans than `capacity`. */
SC_API int sc_hip_restore_spans(long long step, int rows, int ltx, int lty, int W, int H, long long *spans, int capacity);

#ifdef __cplusplus
}
#endif
#endif /* SEAMLESSCLONE_HIP_TESTING_H */
