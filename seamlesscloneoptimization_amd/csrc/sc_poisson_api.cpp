// sc_poisson_api.cpp -- the Poisson solver on float32 images with caller guidance fields (sc_hip_poisson_check, sc_hip_poisson_device,
// sc_hip_poisson), and the front end it shares with the screened and the weighted call (sc_screened_api.cpp, sc_weighted_api.cpp):
// family_validate, direct_instance_check, float_job_validate, float_stage and poisson_download here, float_intake and run_chunks in
// sc_instance.h.
//
// A call: validation -> per chunk of at most SC_POISSON_MAX_PLANES planes: setup_fields(W, H, C m) -> pre-process (U0 = boundary,
// F = lap; sc_poisson.hip) -> the drivers' shared solve step (solve_step, with no output target: spec_post stays disarmed) -> output
// launch (interior from the solution field, frame from boundary).  The solve runs under per-call options: the exact system
// (SC_FLAG_EXACT_TABLES: no float-table correction, which belongs to the reference's 8-bit answer), all fields float32 (the float16
// right-hand side and level 1 and the 16-bit field between level-0 launches assume 8-bit data), update_tol = the call's tol.  The
// instance's stored options and solve state (CallScope) are restored on every way out.
//
// SC_POISSON_NEUMANN and SC_POISSON_FREE_* on one to three sides: no fields, no pre-process or output launch -- per chunk
// direct_jobs_solve (sc_fft.hip) works straight between the jobs' arrays: three transform launches, each axis under the transform of
// its two ends, the Dirichlet lines of out written by the last one; in front of them the boundary-mean reduction of a Neumann call.
// SC_POISSON_PERIODIC_X / _Y: the same path -- a periodic axis is one more axis kind of those launches; without a Dirichlet line on the
// other axis either, the call is singular like the Neumann one and has its reduction.
//
// The screened call (sc_screened_api.cpp) runs through the same poisson_run with PoissonCall::lam > 0: the jobs carry their data
// term, the solve is the direct one (SC_METHOD_FFT) with its denominators shifted by -lam.
#include "sc_instance.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

using namespace sc;

namespace sc {

// host-only: the call's code for these parameters and this layout (SC_OK: it may run); `why` gets the reason
int poisson_validate(const sc_poisson_params *p, const sc_poisson_layout *l, const char **why)
{
    const char *dummy;
    if (!why) why = &dummy;
    *why = "";
    if (!p || !l) { *why = "null pointer"; return SC_ERR_BAD_ARG; }
    const int free = poisson_free_sides(p->kind), per = poisson_periodic(p->kind), base = poisson_base(p->kind);
    const bool neumann = free == 15;
    if (base != SC_POISSON_GUIDANCE && base != SC_POISSON_LAPLACIAN) {
        *why = "kind must be SC_POISSON_GUIDANCE or SC_POISSON_LAPLACIAN, alone or with SC_POISSON_NEUMANN, SC_POISSON_FREE_* or SC_POISSON_PERIODIC_* bits";
        return SC_ERR_BAD_ARG;
    }
    if (per && (p->kind & SC_POISSON_NEUMANN)) { *why = "SC_POISSON_PERIODIC_* with SC_POISSON_NEUMANN: an axis wraps or reflects, not both"; return SC_ERR_BAD_ARG; }
    if (((per & 1) && (free & 3)) || ((per & 2) && (free & 12))) {
        *why = "a periodic axis has no free side: SC_POISSON_PERIODIC_X excludes SC_POISSON_FREE_LEFT / _RIGHT, SC_POISSON_PERIODIC_Y excludes _TOP / _BOTTOM";
        return SC_ERR_BAD_ARG;
    }
    if (!std::isfinite(p->tol)) { *why = "tol must be finite"; return SC_ERR_BAD_ARG; }
    if (l->channels < 1 || l->channels > 4) { *why = "channels must be 1..4"; return SC_ERR_BAD_ARG; }
    if (l->col_stride <= 0 || l->row_stride <= 0 || l->channel_stride <= 0) { *why = "strides must be positive"; return SC_ERR_BAD_ARG; }
    if (free || per) {
        if (l->cols < 2 || l->rows < 2) {
            *why = neumann ? "SC_POISSON_NEUMANN: the image must be at least 2 x 2" : per ? "periodic axes: the image must be at least 2 x 2" : "free sides: the image must be at least 2 x 2";
            return SC_ERR_BAD_SIZE;
        }
        const MixedGeo mg = poisson_mixed_geo(free, l->cols, l->rows, per);       // (all four sides free: every pixel an unknown)
        if (mg.nx < 1 || mg.ny < 1) {
            *why = per ? "periodic axes: at least 1 unknown along the other axis (3 pixels between two Dirichlet lines)"
                       : "free sides: at least 1 unknown per axis (3 pixels between two Dirichlet lines)";
            return SC_ERR_BAD_SIZE;
        }
        if (!fft_supported(mg.nx, mg.ny, false)) {
            *why = neumann ? "SC_POISSON_NEUMANN: the image must be at most 8192 x 8192"
                 : per ? "periodic axes: at most 8192 unknowns (pixels less the axis's Dirichlet lines) per axis"
                           : "free sides: at most 8192 unknowns (pixels less the axis's Dirichlet lines) per axis";
            return SC_ERR_BAD_SIZE;
        }
    } else {
        if (l->cols < 3 || l->rows < 3) { *why = "the image must be at least 3 x 3"; return SC_ERR_BAD_SIZE; }
        if (l->cols > 65536 || l->rows > 65536) { *why = "the image must be at most 65536 x 65536"; return SC_ERR_BAD_SIZE; }
    }
    // the strides must nest: sorted by size, each exceeds the span of the smaller ones (dimensions of extent 1 take no part)
    struct Dim { unsigned __int128 s, n; } d[3] = { { (unsigned __int128)l->col_stride, (unsigned)l->cols },
                                                     { (unsigned __int128)l->row_stride, (unsigned)l->rows },
                                                     { (unsigned __int128)l->channel_stride, (unsigned)l->channels } };
    std::sort(d, d + 3, [](const Dim &a, const Dim &b) { return a.s < b.s; });
    unsigned __int128 span = 0;
    for (const Dim &k : d) {
        if (k.n < 2) continue;
        if (k.s <= span) { *why = "the layout's strides overlap (they must nest: each exceeds the span of the smaller ones)"; return SC_ERR_BAD_ARG; }
        span += k.s * (k.n - 1);
    }
    if (span >= ((unsigned __int128)1 << 60)) { *why = "the layout spans more than 2^60 floats"; return SC_ERR_BAD_ARG; }
    return SC_OK;
}

// floats from an array's pointer to one past its last element under the layout
size_t poisson_span(const sc_poisson_layout *l)
{
    return (size_t)((l->cols - 1) * l->col_stride + (l->rows - 1) * l->row_stride + (l->channels - 1) * l->channel_stride) + 1;
}

static bool aligned4(const void *p) { return ((uintptr_t)p & 3u) == 0; }

int family_validate(const int *kind, const sc_poisson_layout *l, const char *own, const char *limit_why, const char **why)
{
    const char *dummy;
    if (!why) why = &dummy;
    *why = "";
    if (!kind || !l) { *why = "null pointer"; return SC_ERR_BAD_ARG; }
    if (own) { *why = own; return SC_ERR_BAD_ARG; }
    const sc_poisson_params pp{ *kind, 0.f };
    const int rc = poisson_validate(&pp, l, why);       // kind, channels, strides; the direct calls' side limits; at least 3 x 3 under a frame
    if (rc) return rc;
    if (!poisson_direct(*kind) && !fft_supported(l->cols - 2, l->rows - 2, false)) { *why = limit_why; return SC_ERR_BAD_SIZE; }
    return SC_OK;
}

int direct_instance_check(Instance *I, int kind, const sc_poisson_layout *l, const char *method_why, const char *fp64_why)
{
    if (I->opts.method != SC_METHOD_AUTO && I->opts.method != SC_METHOD_FFT) { I->err = method_why; return SC_ERR_BAD_ARG; }
    const MixedGeo mg = poisson_mixed_geo(poisson_free_sides(kind), l->cols, l->rows, poisson_periodic(kind));
    if ((I->opts.flags & SC_FLAG_FFT_FP64) && !fft_supported(mg.nx, mg.ny, true)) { I->err = fp64_why; return SC_ERR_BAD_SIZE; }
    return SC_OK;
}

// (a job without a Dirichlet line on any side -- the Neumann call, a periodic axis beside a periodic or free-free one -- needs no
// boundary: out is then checked in its place)
int float_job_validate(int kind, int carries, const FloatArrays &a, const char **why, size_t span, size_t tspan, size_t fspan)
{
    if (a.refuse) { *why = a.refuse; return SC_ERR_BAD_ARG; }
    if ((carries & FLOAT_DATA) && !a.data) { *why = "null data pointer"; return SC_ERR_BAD_ARG; }
    if ((carries & FLOAT_WEIGHT) && !a.weight) { *why = "null weight pointer"; return SC_ERR_BAD_ARG; }
    const bool guidance = poisson_base(kind) == SC_POISSON_GUIDANCE;
    const float *b = poisson_no_dirichlet(kind) && (carries || !a.boundary) ? a.out : a.boundary;
    const float *need[6] = { a.data, a.weight, b, a.out, guidance ? a.gx : a.lap, guidance ? a.gy : a.lap };
    for (int i = 0; i < 6; ++i) {
        const float *q = need[i];
        if (i < 2 && !(carries & (i ? FLOAT_WEIGHT : FLOAT_DATA))) continue;      // not this family's
        if (!q) { *why = "null array pointer"; return SC_ERR_BAD_ARG; }
        if (!aligned4(q)) { *why = "array pointer not 4-byte aligned"; return SC_ERR_BAD_ARG; }
    }
    if (carries & FLOAT_SMOOTH) {
        for (const float *q : { a.smooth_x, a.smooth_y }) {
            if (!q) { *why = "null smooth_x or smooth_y pointer"; return SC_ERR_BAD_ARG; }
            if (!aligned4(q)) { *why = "array pointer not 4-byte aligned"; return SC_ERR_BAD_ARG; }
        }
    }
    if (carries & FLOAT_STATE) {
        if (!a.state) { *why = "null state pointer"; return SC_ERR_BAD_ARG; }
        if (!aligned4(a.state)) { *why = "array pointer not 4-byte aligned"; return SC_ERR_BAD_ARG; }
    }
    if ((carries & FLOAT_GT) && a.gt && !aligned4(a.gt)) { *why = "array pointer not 4-byte aligned"; return SC_ERR_BAD_ARG; }
    if (carries & FLOAT_SMOOTH_T) {
        if (!a.smooth_t) { *why = "null smooth_t pointer"; return SC_ERR_BAD_ARG; }
        if (!aligned4(a.smooth_t)) { *why = "array pointer not 4-byte aligned"; return SC_ERR_BAD_ARG; }
    }
    if (carries & FLOAT_LOWER) {
        if (!a.lower) { *why = "null lower pointer"; return SC_ERR_BAD_ARG; }
        if (!aligned4(a.lower)) { *why = "array pointer not 4-byte aligned"; return SC_ERR_BAD_ARG; }
    }
    if (carries & FLOAT_UPPER) {
        if (!a.upper) { *why = "null upper pointer"; return SC_ERR_BAD_ARG; }
        if (!aligned4(a.upper)) { *why = "array pointer not 4-byte aligned"; return SC_ERR_BAD_ARG; }
    }
    if (span && (carries & (FLOAT_SMOOTH | FLOAT_STATE))) {
        const uintptr_t o = (uintptr_t)a.out, bytes = span * sizeof(float);
        auto overlaps = [&](const float *q) { return (uintptr_t)q < o + bytes && o < (uintptr_t)q + bytes; };
        for (const float *q : { carries & FLOAT_WEIGHT ? a.weight : nullptr, carries & FLOAT_SMOOTH ? a.smooth_x : nullptr,
                                carries & FLOAT_SMOOTH ? a.smooth_y : nullptr })
            if (q && overlaps(q)) { *why = "weight, smooth_x or smooth_y overlaps out"; return SC_ERR_BAD_ARG; }
        if ((carries & FLOAT_STATE) && overlaps(a.state)) { *why = "state overlaps out"; return SC_ERR_BAD_ARG; }
        for (const float *q : { carries & FLOAT_LOWER ? a.lower : nullptr, carries & FLOAT_UPPER ? a.upper : nullptr })
            if (q && overlaps(q)) { *why = "lower or upper overlaps out"; return SC_ERR_BAD_ARG; }
    }
    if (carries & FLOAT_FLOW) {
        for (const float *q : { a.flow_x, a.flow_y }) {
            if (!q) { *why = "null flow_x or flow_y pointer"; return SC_ERR_BAD_ARG; }
            if (!aligned4(q)) { *why = "array pointer not 4-byte aligned"; return SC_ERR_BAD_ARG; }
            const uintptr_t o = (uintptr_t)a.out, f = (uintptr_t)q;          // (their own length: dense, no channel axis)
            if (span && fspan && f < o + span * sizeof(float) && o < f + fspan * sizeof(float)) { *why = "flow_x or flow_y overlaps out"; return SC_ERR_BAD_ARG; }
        }
    }
    if (span && tspan && (carries & FLOAT_SMOOTH_T)) {          // (its own length: the call's temporal frames)
        const uintptr_t o = (uintptr_t)a.out, q = (uintptr_t)a.smooth_t;
        if (q < o + span * sizeof(float) && o < q + tspan * sizeof(float)) { *why = "smooth_t overlaps out"; return SC_ERR_BAD_ARG; }
    }
    return SC_OK;
}

PoissonJobDev float_dev_job(int kind, int carries, const FloatArrays &a)
{
    PoissonJobDev j{ a.gx, a.gy, a.lap, carries && poisson_no_dirichlet(kind) ? nullptr : a.boundary, a.out };
    if (carries & FLOAT_DATA) j.d = a.data;
    return j;
}

int float_stage(Instance *I, const sc_poisson_layout *l, int kind, int carries, const FloatArrays &a, FloatStaged &s, int frames, long long frame_stride,
                int tframes, size_t flow_floats)
{
    const size_t bytes = (poisson_span(l) + (size_t)(frames - 1) * (size_t)frame_stride) * sizeof(float), slot = (bytes + 255) / 256 * 256;
    const bool guidance = poisson_base(kind) == SC_POISSON_GUIDANCE;
    const float *data = carries & FLOAT_DATA ? a.data : nullptr, *weight = carries & FLOAT_WEIGHT ? a.weight : nullptr;
    // (the Poisson call keeps a boundary without a Dirichlet line: it gives the mean)
    const float *boundary = carries && poisson_no_dirichlet(kind) ? nullptr : a.boundary;
    const bool own_b = boundary && boundary != data, in_place = (data && a.out == data) || (boundary && a.out == boundary);
    const bool smooth = (carries & FLOAT_SMOOTH) != 0, state = (carries & FLOAT_STATE) != 0, gt = (carries & FLOAT_GT) && guidance && a.gt;
    const bool smooth_t = (carries & FLOAT_SMOOTH_T) != 0, lower = (carries & FLOAT_LOWER) != 0, upper = (carries & FLOAT_UPPER) != 0;
    const bool flow = (carries & FLOAT_FLOW) != 0;
    const int slots = (guidance ? 2 : 1) + (data ? 1 : 0) + (weight ? 1 : 0) + (own_b ? 1 : 0) + (in_place ? 0 : 1) + (smooth ? 2 : 0) + (state ? 1 : 0) + (gt ? 1 : 0) +
                      (smooth_t ? 1 : 0) + (lower ? 1 : 0) + (upper ? 1 : 0) + (flow ? 2 : 0);
    int rc, at = 0;
    if ((rc = ensure(I, I->d_pois, slot * slots, false))) return rc;
    auto next = [&](bool wanted) { return wanted ? (float *)((uint8_t *)I->d_pois.p + slot * at++) : nullptr; };
    auto upload = [&](DevBuf &stage, float *d, const float *h) {
        return d ? upload_rows(I, stage, d, bytes, (const uint8_t *)h, bytes, bytes, 1) : SC_OK;
    };
    float *d_in0 = next(true), *d_in1 = next(guidance), *d_d = next(data != nullptr), *d_w = next(weight != nullptr);
    float *d_b = own_b ? next(true) : (boundary ? d_d : nullptr);
    float *d_out = !in_place ? next(true) : (data && a.out == data ? d_d : d_b);
    float *d_sx = next(smooth), *d_sy = next(smooth), *d_state = next(state), *d_gt = next(gt), *d_smt = next(smooth_t);
    float *d_lo = next(lower), *d_hi = next(upper), *d_fx = next(flow), *d_fy = next(flow);
    SC_HIP(I, hipEventRecord(I->ev_k0, I->stream));
    if ((rc = upload(I->h_face, d_in0, guidance ? a.gx : a.lap))) return rc;
    if ((rc = upload(I->h_body, d_in1, a.gy))) return rc;
    if ((rc = upload(I->h_in, d_d, data))) return rc;
    if ((rc = upload(I->h_out, d_w, weight))) return rc;      // (h_out: free until the download)
    if ((rc = upload(I->h_mask, own_b ? d_b : nullptr, boundary))) return rc;
    s.job = float_dev_job(kind, carries, FloatArrays{ guidance ? d_in0 : nullptr, d_in1, guidance ? nullptr : d_in0, d_d, d_w, d_b, d_out });
    if ((rc = upload(I->h_sx, d_sx, a.smooth_x))) return rc;      // (pinned blocks of their own: the uploads stay back to back)
    if ((rc = upload(I->h_sy, d_sy, a.smooth_y))) return rc;
    if ((rc = upload(I->h_state, d_state, a.state))) return rc;
    // the temporal arrays: tframes frames (0: one less than the others)
    const size_t tbytes = (poisson_span(l) + (size_t)((tframes > 0 ? tframes : frames - 1) - 1) * (size_t)frame_stride) * sizeof(float);
    if (d_gt && (rc = upload_rows(I, I->h_gt, d_gt, tbytes, (const uint8_t *)a.gt, tbytes, tbytes, 1))) return rc;
    if (d_smt && (rc = upload_rows(I, I->h_smt, d_smt, tbytes, (const uint8_t *)a.smooth_t, tbytes, tbytes, 1))) return rc;
    if ((rc = upload(I->h_lo, d_lo, a.lower))) return rc;
    if ((rc = upload(I->h_hi, d_hi, a.upper))) return rc;
    const size_t fbytes = flow_floats * sizeof(float);
    if (flow && fbytes > slot) { I->err = "a flow array is longer than the call's arrays"; return SC_ERR_BAD_ARG; }
    if (d_fx && (rc = upload_rows(I, I->h_fx, d_fx, fbytes, (const uint8_t *)a.flow_x, fbytes, fbytes, 1))) return rc;
    if (d_fy && (rc = upload_rows(I, I->h_fy, d_fy, fbytes, (const uint8_t *)a.flow_y, fbytes, fbytes, 1))) return rc;
    s.side = SideArrays{ d_w, d_sx, d_sy, d_state, d_gt, d_smt, d_lo, d_hi };      // (an array the call does not carry has no slot: NULL)
    s.side.fx = d_fx;
    s.side.fy = d_fy;
    return SC_OK;
}

} // namespace sc

namespace {

// The call's effective options, the instance's own restored on every way out (the rest of the call's state: CallScope).
struct PoissonScope {
    Instance *I;
    sc_solver_opts saved;
    PoissonScope(Instance *I_, const PoissonCall &p, int n_valid) : I(I_), saved(I_->opts)
    {
        sc_solver_opts &o = I->opts;
        o.flags = (o.flags | SC_FLAG_EXACT_TABLES | SC_FLAG_FLOAT_RHS | SC_FLAG_FLOAT_U0 | SC_FLAG_FLOAT_L1 | SC_FLAG_FLOAT_FIELD) &
                  ~SC_FLAG_OPENCV_GREY_MASK;
        o.update_tol = p.tol > 0.f ? p.tol : 1e-3f;
        o.reference_warmup = 0;
        if (o.method == SC_METHOD_AUTO && n_valid > 1) o.method = SC_METHOD_MULTIGRID;     // a batch: the cycles, as the edit batches
        I->auto_as_single = n_valid == 1;           // one problem: AUTO decides as for a single clone, whatever its channel count
        if (p.lam > 0.f) {                          // a screened call: the direct solve at any size, its denominators shifted
            o.method = SC_METHOD_FFT;
            I->screen_lambda = p.lam;
        }
    }
    ~PoissonScope() { I->opts = saved; }
};

// One chunk of m same-size problems as one field of C m planes.  Marks: 0 start, 5 pre-process done, 6 solve done, 7 output done.
int poisson_chunk(Instance *I, int kind, const PoissonGeo &g, const PoissonJobDev *jobs, int m, float lam)
{
    int rc;
    if ((rc = setup_fields(I, g.W, g.H, g.C * m))) return rc;
    I->guard = RectGuard();
    stage_mark(I, 0);
    const bool lap = kind == SC_POISSON_LAPLACIAN;
    const int solve_rc = solve_step(I, SolveTarget(), [&]() -> int {      // float32 right-hand side and initial field (FLOAT_RHS | FLOAT_U0)
        if (m == 1) launch_poisson_pre(g, lap, jobs[0], I->U0, I->F, I->stream, lam);
        else launch_poisson_pre_group(g, lap, jobs, m, I->U0, I->F, I->stream, lam);
        SC_HIP(I, hipGetLastError());
        stage_mark(I, 5);
        return SC_OK;
    });
    if (solve_rc != SC_OK && solve_rc != SC_ERR_NOT_CONVERGED) return solve_rc;
    stage_mark(I, 6);
    if (m == 1) launch_poisson_out(g, jobs[0], result(I), I->stream);
    else launch_poisson_out_group(g, jobs, m, result(I), I->stream);
    SC_HIP(I, hipGetLastError());
    stage_mark(I, 7);
    return solve_rc;
}

// The same for a call with free sides or periodic axes (kind: poisson_norm_kind's; all four free: the Neumann call): no fields; marks 5
// (a singular call's reduction done) and 6 (transforms done) come from direct_jobs_solve, 7 = 6 (the output is the last transform launch's store).
int free_sides_chunk(Instance *I, int kind, const PoissonGeo &g, const PoissonJobDev *jobs, int m, float lam)
{
    stage_mark(I, 0);
    const MixedGeo mg = poisson_mixed_geo(poisson_free_sides(kind), g.W, g.H, poisson_periodic(kind));
    const int rc = direct_jobs_solve(I, g, mg, poisson_base(kind) == SC_POISSON_LAPLACIAN, jobs, m, (I->opts.flags & SC_FLAG_FFT_FP64) != 0, lam);
    if (rc) return rc;
    stage_mark(I, 7);
    return SC_OK;
}

// the instance's word on a call of this kind (poisson_norm_kind's) before anything runs: with free sides, the methods that serve it
// and the limit of its transforms' precision
int poisson_instance_check(Instance *I, int kind, const sc_poisson_layout *l)
{
    const int free = poisson_free_sides(kind), per = poisson_periodic(kind);
    if (!free && !per) return SC_OK;
    return direct_instance_check(I, kind, l,
                 per ? "periodic axes (SC_POISSON_PERIODIC_*) are solved by SC_METHOD_AUTO and SC_METHOD_FFT only (the multigrid and the relaxation solvers assume a zero ring on every level)"
               : free == 15 ? "SC_POISSON_NEUMANN is solved by SC_METHOD_AUTO and SC_METHOD_FFT only (the multigrid and the relaxation solvers know Dirichlet problems)"
                            : "free sides (SC_POISSON_FREE_*) are solved by SC_METHOD_AUTO and SC_METHOD_FFT only (the multigrid and the relaxation solvers assume a zero ring on every level)",
                 per ? "periodic axes with SC_FLAG_FFT_FP64: at most 4096 unknowns per axis"
               : free == 15 ? "SC_POISSON_NEUMANN with SC_FLAG_FFT_FP64: the image must be at most 4096 x 4096"
                            : "free sides with SC_FLAG_FFT_FP64: at most 4096 unknowns per axis");
}

void add_timing(Instance *I, float t[4])
{
    t[0] += ev_ms(I->ev[0], I->ev[5]);
    t[1] += ev_ms(I->ev[5], I->ev[6]);
    t[2] += ev_ms(I->ev[6], I->ev[7]);
    t[3] += ev_ms(I->ev[0], I->ev[7]);
}

} // namespace

namespace sc {

void poisson_set_timing(Instance *I, const float t[4])
{
    I->info.ms_mask = 0.f;
    I->info.ms_pre = t[0]; I->info.ms_solve = t[1]; I->info.ms_post = t[2];
    I->info.ms_device_total = t[0] + t[1] + t[2];
    I->info.ms_call = t[3];
}

// The nv validated jobs of a call (their device arrays in dj, where each one's code goes in rcs) through chunks of at most
// SC_POISSON_MAX_PLANES planes.  timed: stage marks, a wait per chunk, the stage times summed into t.  Codes as
// sc_hip_edit_device_batch: the worst; a HIP error marks every job.
int poisson_run(Instance *I, const PoissonCall &p, const sc_poisson_layout *l, const PoissonJobDev *dj, int *const *rcs, int nv,
                bool timed, float t[4])
{
    CallScope call{ I };
    PoissonScope scope(I, p, nv);
    const PoissonGeo g{ l->cols, l->rows, l->channels, l->col_stride, l->row_stride, l->channel_stride };
    Geo geo{ 0, 0, g.W, g.H, 0, 0 };
    fill_info_geo(I, geo);
    I->stage_marks = timed;
    I->marks_ends_only = false;
    return run_chunks(I, g.C, rcs, nv, [&](int i0, int m) -> int {
        const int rc = poisson_direct(p.kind) ? free_sides_chunk(I, p.kind, g, dj + i0, m, p.lam) : poisson_chunk(I, p.kind, g, dj + i0, m, p.lam);
        if (rc != SC_OK && rc != SC_ERR_NOT_CONVERGED) return rc;
        if (timed) {
            SC_HIP(I, hipStreamSynchronize(I->stream));
            add_timing(I, t);
        }
        for (int k = 0; k < m; ++k) *rcs[i0 + k] = rc;
        return rc;
    });
}

} // namespace sc

extern "C" {

int sc_hip_poisson_check(const sc_poisson_params *p, const sc_poisson_layout *l)
{
    return poisson_validate(p, l, nullptr);
}

int sc_hip_poisson_device(void *inst, const sc_poisson_params *p, const sc_poisson_layout *l, sc_poisson_job *jobs, int n, bool bSync)
{
    Instance *I;
    int rc = begin_call(inst, I);
    if (rc) return rc;
    const char *why = "";
    if ((rc = poisson_validate(p, l, &why))) { I->err = why; return rc; }
    const int kind = poisson_norm_kind(p->kind);
    if ((rc = poisson_instance_check(I, kind, l))) return rc;
    FloatJobs v;
    const int worst = float_intake(I, kind, 0, jobs, n, [](const sc_poisson_job &j) {
        return FloatArrays{ j.gx, j.gy, j.lap, nullptr, nullptr, j.boundary, j.out }; }, v);
    if (v.rcs.empty()) return worst;
    float t[4] = { 0.f, 0.f, 0.f, 0.f };
    I->info.ms_h2d = I->info.ms_d2h = 0.f;
    rc = poisson_run(I, PoissonCall{ kind, p->tol, 0.f }, l, v.dj.data(), v.rcs.data(), (int)v.rcs.size(), bSync, t);
    if (rc != SC_OK && rc != SC_ERR_NOT_CONVERGED) return rc;
    poisson_set_timing(I, t);       // (zeros without bSync)
    return worst == SC_OK ? rc : worst;
}

int sc_hip_poisson(void *inst, const sc_poisson_params *p, const sc_poisson_layout *l, const float *gx, const float *gy,
                   const float *lap, const float *boundary, float *out)
{
    Instance *I;
    int rc = begin_call(inst, I);
    if (rc) return rc;
    const char *why = "";
    if ((rc = poisson_validate(p, l, &why))) { I->err = why; return rc; }
    const int kind = poisson_norm_kind(p->kind);
    if ((rc = poisson_instance_check(I, kind, l))) return rc;
    const FloatArrays a{ gx, gy, lap, nullptr, nullptr, boundary, out };
    if ((rc = float_job_validate(kind, 0, a, &why))) { I->err = why; return rc; }
    FloatStaged s;
    if ((rc = float_stage(I, l, kind, 0, a, s))) return rc;
    int job_rc = SC_OK, *const job_rcs[1] = { &job_rc };
    float t[4] = { 0.f, 0.f, 0.f, 0.f };
    rc = poisson_run(I, PoissonCall{ kind, p->tol, 0.f }, l, &s.job, job_rcs, 1, true, t);
    if (rc != SC_OK && rc != SC_ERR_NOT_CONVERGED) return rc;
    return poisson_download(I, l, s.job.out, out, t, rc);
}

} // extern "C"

namespace sc {

// The host call's way back: out's span into pinned staging, then only the elements the layout names into the caller's array; the
// call's times.  Returns rc_solve.
int poisson_download(Instance *I, const sc_poisson_layout *l, const float *d_out, float *out, const float t[4], int rc_solve, int frames, long long frame_stride)
{
    const size_t span = poisson_span(l) + (size_t)(frames - 1) * (size_t)frame_stride, bytes = span * sizeof(float);
    int rc;
    if ((rc = ensure_pinned(I, I->h_out, bytes))) return rc;
    SC_HIP(I, hipMemcpyAsync(I->h_out.p, d_out, bytes, hipMemcpyDeviceToHost, I->stream));
    SC_HIP(I, hipEventRecord(I->ev_k1, I->stream));
    SC_HIP(I, hipStreamSynchronize(I->stream));
    const float *h = (const float *)I->h_out.p;
    const int W = l->cols, H = l->rows, Cn = l->channels;
    if (span == (size_t)W * H * Cn * frames) {
        copy_rows(I, (uint8_t *)out, bytes, (const uint8_t *)h, bytes, bytes, 1);     // dense: every float of the span is named
    } else {
        for (int f = 0; f < frames; ++f)
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x)
                    for (int c = 0; c < Cn; ++c) {
                        const size_t o = (size_t)f * (size_t)frame_stride + (size_t)(x * l->col_stride + y * l->row_stride + c * l->channel_stride);
                        out[o] = h[o];
                    }
    }
    poisson_set_timing(I, t);
    I->info.ms_h2d = ev_ms(I->ev_k0, I->ev[0]);
    I->info.ms_d2h = ev_ms(I->ev[7], I->ev_k1);
    I->info.ms_call = ev_ms(I->ev_k0, I->ev_k1);
    return rc_solve;
}

} // namespace sc
