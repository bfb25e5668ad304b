// sc_hooks.cpp -- the test and measurement hooks of include/seamlessclone_hip_testing.h: the host-only self test, the stage hooks
// (mask stage, right-hand side), the solver hooks on caller-supplied fields and the kernel timings bench.py reads.  No clone path
// calls into this file.
#include "sc_pcg.h"
#include "sc_u0_bytes.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

using namespace sc;

// A multigrid clone leaves its right-hand side as float16 inside F's buffer; the diagnostic hooks below read
// float.  Expand through the field that does not hold the result and copy back (not on any hot path).
static int float_rhs(Instance *I)
{
    if (!I->f_half) return SC_OK;
    SC_HIP(I, hipSetDevice(I->gpu));
    Field scratch = I->result_in_U1 ? I->U0 : I->U1;
    const size_t n = I->F.plane * (size_t)I->F.C;
    launch_half_to_float(I->F.p, scratch.p, n, I->stream);
    SC_HIP(I, hipGetLastError());
    SC_HIP(I, hipMemcpyAsync(I->F.p, scratch.p, n * sizeof(float), hipMemcpyDeviceToDevice, I->stream));
    I->f_half = false;
    return SC_OK;
}

// Measurement hook (sc_hip_time_coarse_chain): the launch-bound part of a cycle -- levels 2 .. bottom .. 2: seven dependent launches
// for a 2048^2 clone, 2 % of the unknowns -- run `reps` times back to back on the hierarchy the last multigrid solve left, (a) as
// plain launches and (b) captured once into a HIP graph and replayed.  hipEvents on the instance's stream around each batch.
// Values are discarded (level 2's right-hand side is whatever the last cycle left there).
static int mg_time_coarse_chain(Instance *I, int reps, float *ms_eager, float *ms_graph, int *launches)
{
    if (I->mg.size() < 4 || I->mg_bottom < 3 || !mg_composes_level1(I)) { I->err = "time_coarse_chain: run a multigrid clone of at least ~500^2 first"; return SC_ERR_BAD_ARG; }
    const int pre = mg_params(I->opts).pre, post = mg_params(I->opts).post;
    int rc;
    if ((rc = fd_wait(I))) return rc;
    *launches = (int)(2 * (I->mg_bottom - 2) + 1) - (tail_serves(I, I->mg_bottom - 1) ? 2 : 0);
    if ((rc = vcycle(I, 2, pre, post))) return rc;                       // warm
    SC_HIP(I, hipEventRecord(I->ev_k0, I->stream));
    for (int i = 0; i < reps; ++i) if ((rc = vcycle(I, 2, pre, post))) return rc;
    SC_HIP(I, hipEventRecord(I->ev_k1, I->stream));
    SC_HIP(I, hipStreamSynchronize(I->stream));
    float ms = 0.f;
    SC_HIP(I, hipEventElapsedTime(&ms, I->ev_k0, I->ev_k1));
    *ms_eager = ms / (float)reps;
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    SC_HIP(I, hipStreamBeginCapture(I->stream, hipStreamCaptureModeThreadLocal));
    rc = vcycle(I, 2, pre, post);
    hipError_t e = hipStreamEndCapture(I->stream, &graph);
    if (rc || e != hipSuccess || !graph) { if (graph) (void)hipGraphDestroy(graph); return rc ? rc : hip_fail(I, e, "hipStreamEndCapture"); }
    e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    if (e != hipSuccess) { (void)hipGraphDestroy(graph); return hip_fail(I, e, "hipGraphInstantiate"); }
    (void)hipGraphLaunch(exec, I->stream);                                 // warm (uploads the executable graph)
    SC_HIP(I, hipEventRecord(I->ev_k0, I->stream));
    for (int i = 0; i < reps; ++i) (void)hipGraphLaunch(exec, I->stream);
    SC_HIP(I, hipEventRecord(I->ev_k1, I->stream));
    e = hipStreamSynchronize(I->stream);
    (void)hipGraphExecDestroy(exec);
    (void)hipGraphDestroy(graph);
    if (e != hipSuccess) return hip_fail(I, e, "hipStreamSynchronize");
    SC_HIP(I, hipEventElapsedTime(&ms, I->ev_k0, I->ev_k1));
    *ms_graph = ms / (float)reps;
    return SC_OK;
}

// Measurement hook (sc_hip_time_tail_phases): one k_mg_tail launch on the hierarchy the last multigrid solve left, with the shader
// clock of channel 0's first thread at its eleven phase boundaries: entry | right-hand side in registers | pre-smoothing done |
// residual + restriction done (level B's right-hand side in LDS) | products 1, 2, 3, 4 | prolongation + edge exchange |
// post-smoothing | stores issued.  Differences are cycles of the shader clock.
static int mg_time_tail_phases(Instance *I, unsigned long long *out11)
{
    if (I->mg.size() < 4 || I->mg_bottom < 3 || !tail_serves(I, I->mg_bottom - 1)) { I->err = "time_tail_phases: the last run was not a multigrid solve whose bottom runs as k_mg_tail"; return SC_ERR_BAD_ARG; }
    const int pre = mg_params(I->opts).pre, post = mg_params(I->opts).post;
    unsigned long long *d = nullptr;
    SC_HIP(I, hipMalloc(&d, 11 * sizeof(unsigned long long)));
    bool done = false;
    int rc = run_tail(I, I->mg_bottom - 1, pre, post, done);             // warm
    if (!rc) rc = run_tail(I, I->mg_bottom - 1, pre, post, done, d);
    hipError_t e = hipStreamSynchronize(I->stream);
    if (!rc && e == hipSuccess && done) e = hipMemcpy(out11, d, 11 * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (rc) return rc;
    if (e != hipSuccess) return hip_fail(I, e, "time_tail_phases");
    return done ? SC_OK : SC_ERR_BAD_ARG;
}

// A step of the default fast-path solve's schedule (sc_multigrid.cpp: V(2,2), output bytes wanted, the early node correction allowed),
// by kind: the launches the timing hooks below repeat are the solve's own.
static FusedStep default_step(int kind, bool q16, bool composed)
{
    FusedSchedule S{ FusedFacts{ 2, 2, mg_params(sc_solver_opts{}).budget, false, true, q16, q16, composed, false, true } };
    for (;;) {
        FusedStep s = fused_next(S, VERDICT_REJECT);
        if (s.ask_early) fused_early(S, s, 1);
        if (s.kind == kind || s.kind == FUSED_DONE) return s;
    }
}

// ---- the front end where the caller's bytes lie (sc_hip_front_end_device)
namespace {

struct FrontOut { uint8_t *M; float *B, *lap; size_t cap; };

// W x H of plane c of `src` (the fields' pitch and plane size) into plane c of member k's dense [3][H][W] block of `out`
int front_planes(Instance *I, const Field &f, const float *src, int k, int W, int H, float *out, size_t cap)
{
    int rc;
    for (int c = 0; c < 3; ++c)
        if ((rc = download_rows(I, I->h_out, (uint8_t *)(out + 3 * cap * k + (size_t)c * W * H), (size_t)W * sizeof(float),
                                src + (size_t)(3 * k + c) * f.plane, (size_t)f.pitch * sizeof(float), (size_t)W * sizeof(float), H))) return rc;
    return SC_OK;
}

// what the launches left for members 0 .. n-1 (first: the caller's index of member 0) of the instance's fields and d_M (mplane bytes per
// member), to the host: float16 fields are expanded through U1, which no front-end launch writes
int front_download(Instance *I, int first, int n, const Geo *geo, size_t mplane, bool f_half, bool u_half, bool no_u0, const FrontOut &o)
{
    int rc;
    const size_t elems = I->F.plane * (size_t)I->F.C;
    if (o.M)
        for (int k = 0; k < n; ++k)
            if ((rc = download_rows(I, I->h_out, o.M + o.cap * (first + k), geo[k].W, (const uint8_t *)I->d_M.p + mplane * k, I->mpitch, geo[k].W, geo[k].H))) return rc;
    if (o.lap) {
        if (f_half) { launch_half_to_float(I->F.p, I->U1.p, elems, I->stream); SC_HIP(I, hipGetLastError()); }
        for (int k = 0; k < n; ++k)
            if ((rc = front_planes(I, I->F, f_half ? I->U1.p : I->F.p, k, geo[k].W, geo[k].H, o.lap + 3 * o.cap * first, o.cap))) return rc;
    }
    if (o.B && !no_u0) {
        if (u_half) { launch_half_to_float(I->U0.p, I->U1.p, elems, I->stream); SC_HIP(I, hipGetLastError()); }
        for (int k = 0; k < n; ++k)
            if ((rc = front_planes(I, I->U0, u_half ? I->U1.p : I->U0.p, k, geo[k].W, geo[k].H, o.B + 3 * o.cap * first, o.cap))) return rc;
    }
    return SC_OK;
}

void front_geo(const Geo &g, int *out) { out[0] = g.x0; out[1] = g.y0; out[2] = g.W; out[3] = g.H; out[4] = g.ltx; out[5] = g.lty; }

} // namespace

extern "C" {

int sc_hip_selftest_host(void)
{
    // 1: row copier -- strided copy of an awkward shape through the parked helpers, twice (reuse of the pool)
    {
        RowCopier rc(5);
        const int rows = 1237, rb = 3001, sp = 3100, dp = 3072;
        std::vector<uint8_t> src((size_t)rows * sp), dst((size_t)rows * dp, 0);
        for (size_t i = 0; i < src.size(); ++i) src[i] = (uint8_t)(i * 2654435761u >> 24);
        for (int rep = 0; rep < 2; ++rep) {
            std::fill(dst.begin(), dst.end(), 0);
            const int per = 17, parts = (rows + per - 1) / per;
            rc.parallel(parts, [&](int i) {
                for (int y = i * per; y < std::min(rows, (i + 1) * per); ++y) memcpy(&dst[(size_t)y * dp], &src[(size_t)y * sp], rb);
            });
            for (int y = 0; y < rows; ++y) {
                if (memcmp(&dst[(size_t)y * dp], &src[(size_t)y * sp], rb) != 0) return 1;
                for (int x = rb; x < dp; ++x) if (dst[(size_t)y * dp + x]) return 1;
            }
        }
        int hits = 0;
        rc.parallel(1, [&](int) { ++hits; });              // single part runs inline
        rc.parallel(0, [&](int) { ++hits; });
        if (hits != 1) return 1;
    }
    // 2: eigen-decomposition of the 1-D level operators (the QL reference), 4: the closed form the device builds from against it
    if (!(sc::fd_selftest_error() < 1e-11)) return 2;
    if (!(sc::fd_closed_selftest_error() < 1e-10)) return 4;
    // 3: which parts of a level-0 launch make up each cell row of the float-table correction (sc_lowmode.hip)
    if (sc::lowmode_part_map_selftest() != 0) return 3;
    // 5: the pruned search for the correction's largest ratio (plan_size) against the full table's maximum, over sizes of every kind
    //    (square, elongated, the 2100s and 3000s where one size in ten crosses the 4 % line)
    {
        std::vector<float> R(256 * 256);
        const int ws[] = { 46, 98, 154, 300, 511, 640, 1000, 1027, 1100, 1555, 2046, 2051, 2105, 2118, 2135, 2400, 3118, 3328, 3468, 4096, 6000, 9000 };
        for (int w : ws)
            for (int dh = -7; dh <= 7; ++dh) {
                for (int h : { w + 3 * dh, w / 3 + dh + 40 }) {
                    if (h < 4) continue;
                    const int Kx = sc::lowmode_count(w), Ky = sc::lowmode_count(h), Kxp = (Kx + 31) / 32 * 32;
                    double pruned = -1.0, full = -2.0;
                    const bool a = sc::lowmode_ratio(w, h, Kx, Ky, Kxp, nullptr, pruned), b = sc::lowmode_ratio(w, h, Kx, Ky, Kxp, R.data(), full);
                    if (a != b || pruned != full) return 5;
                }
            }
    }
    return 0;
}

// ---------------------------------------------------------------- stage-level hooks

int sc_hip_mask_stage(void *p, const uint8_t *mask, int mc, int mr, int ms, int cx, int cy, int geo[6], uint8_t *M_out,
                      size_t M_capacity)
{
    Instance *I = get(p);
    if (!I || !mask || !geo) return SC_ERR_BAD_ARG;
    I->err.clear();
    SC_HIP(I, hipSetDevice(I->gpu));
    if (mc <= 0 || mr <= 0 || ms < mc) return SC_ERR_BAD_SIZE;
    int rc;
    const int dms = round_up(mc, 256);
    if ((rc = ensure(I, I->d_mask, (size_t)dms * mr))) return rc;
    if ((rc = upload_rows(I, I->h_mask, I->d_mask.p, dms, mask, ms, mc, mr))) return rc;
    Geo g;
    if ((rc = device_bbox(I, (const uint8_t *)I->d_mask.p, mc, mr, dms, cx, cy, g))) return rc;
    fill_info_geo(I, g);
    geo[0] = g.x0; geo[1] = g.y0; geo[2] = g.W; geo[3] = g.H; geo[4] = g.ltx; geo[5] = g.lty;
    I->mpitch = round_up(g.W, 64);
    if ((rc = ensure(I, I->d_M, (size_t)I->mpitch * g.H, false))) return rc;
    erode_mask(I, (const uint8_t *)I->d_mask.p, dms, mr, g);
    SC_HIP(I, hipGetLastError());
    if (M_out) {
        if (M_capacity < (size_t)g.W * g.H) return SC_ERR_BAD_SIZE;
        if ((rc = download_rows(I, I->h_out, M_out, g.W, I->d_M.p, I->mpitch, g.W, g.H))) return rc;
    }
    SC_HIP(I, hipStreamSynchronize(I->stream));
    return SC_OK;
}

// planar float field -> dense [C][H][W] host array.  The planes of a field are contiguous (plane = pitch * H), so the
// whole field is C * H rows at one pitch.
static int download_field(Instance *I, const Field &f, float *out)
{
    return download_rows(I, I->h_out, (uint8_t *)out, (size_t)f.W * sizeof(float), f.p, (size_t)f.pitch * sizeof(float),
                         (size_t)f.W * sizeof(float), f.C * f.H);
}

int sc_hip_build_rhs(void *p, const uint8_t *face, int fc, int fr, int fs, const uint8_t *body, int bc, int br, int bs,
                     const uint8_t *mask, int mc, int mr, int ms, int cx, int cy, int geo[6], float *B_out,
                     float *lap_out, size_t plane_capacity)
{
    Instance *I = get(p);
    if (!I || !geo) return SC_ERR_BAD_ARG;
    I->err.clear();
    SC_HIP(I, hipSetDevice(I->gpu));
    int rc = validate_images(I, face, fc, fr, fs, body, bc, br, bs, mask, mc, mr, ms);
    if (rc) return rc;
    if ((rc = sc_hip_mask_stage(p, mask, mc, mr, ms, cx, cy, geo, nullptr, 0))) return rc;
    Geo g{ geo[0], geo[1], geo[2], geo[3], geo[4], geo[5] };
    if ((rc = check_roi(I, g, bc, br))) return rc;
    if (plane_capacity < (size_t)g.W * g.H) return SC_ERR_BAD_SIZE;
    const int dfs = round_up(3 * g.W, 256);
    if ((rc = ensure(I, I->d_face, (size_t)dfs * g.H))) return rc;
    if ((rc = ensure(I, I->d_body_roi, (size_t)dfs * g.H))) return rc;
    if ((rc = upload_rows(I, I->h_face, I->d_face.p, dfs, face + (size_t)g.y0 * fs + 3 * g.x0, fs, 3 * (size_t)g.W, g.H))) return rc;
    if ((rc = upload_rows(I, I->h_body, I->d_body_roi.p, dfs, body + (size_t)g.lty * bs + 3 * g.ltx, bs, 3 * (size_t)g.W, g.H))) return rc;
    if ((rc = setup_fields(I, g.W, g.H, 3))) return rc;
    launch_preprocess((const uint8_t *)I->d_body_roi.p, dfs, (const uint8_t *)I->d_face.p, dfs,
                      (const uint8_t *)I->d_M.p, I->mpitch, I->U0, I->U1, I->F, I->stream, false, false, (I->opts.flags & SC_FLAG_OPENCV_GREY_MASK) != 0,
                      nullptr, I->clone_mode);
    SC_HIP(I, hipGetLastError());
    if (B_out && (rc = download_field(I, I->U0, B_out))) return rc;
    if (lap_out && (rc = download_field(I, I->F, lap_out))) return rc;
    SC_HIP(I, hipStreamSynchronize(I->stream));
    return SC_OK;
}

int sc_hip_front_end_device(void *p, sc_batch_job *jobs, int n, int form, int storage, const int *guess, int *rect_dev, int *rect_host,
                                       int *geo_out, uint8_t *M_out, float *B_out, float *lap_out, size_t capacity)
{
    Instance *I = get(p);
    if (!I || !jobs || n < 1 || form < 0 || form > 3 || !rect_dev || !rect_host || !geo_out || (form == 1 && !guess)) return SC_ERR_BAD_ARG;
    I->err.clear();
    SC_HIP(I, hipSetDevice(I->gpu));
    const bool f_half = (storage & 1) != 0, u_half = (storage & 2) != 0, no_u0 = (storage & 4) != 0;
    const bool grey = (I->opts.flags & SC_FLAG_OPENCV_GREY_MASK) != 0;
    // the storage words the launchers instantiate: float, float16 right-hand side, both float16, and for a group both without the initial field
    if (storage != 0 && storage != 1 && storage != 3 && !(storage == 7 && form >= 2)) { I->err = "front_end: no launch form stores the fields that way"; return SC_ERR_BAD_ARG; }
    if (grey && (form != 0 || storage != 0)) { I->err = "front_end: grey masks run solo on float fields"; return SC_ERR_BAD_ARG; }
    const bool fields = M_out || B_out || lap_out;
    const FrontOut out{ M_out, B_out, lap_out, capacity };
    int rc;
    for (int i = 0; i < n; ++i) {
        sc_batch_job &j = jobs[i];
        if ((rc = validate_images(I, j.face, j.face_cols, j.face_rows, j.face_step, j.body, j.body_cols, j.body_rows, j.body_step, j.mask, j.mask_cols,
                                  j.mask_rows, j.mask_step))) return rc;
        j.rc = SC_OK;
    }
    std::fill(geo_out, geo_out + 6 * (size_t)n, 0);
    I->stage_marks = false;
    I->guard = RectGuard();
    if (form <= 1) {
        for (int i = 0; i < n; ++i) {
            sc_batch_job &j = jobs[i];
            Geo g{};
            auto rects = [&]() -> int {      // behind the scan: the rectangle it left, device copy and pinned mailbox
                SC_HIP(I, hipMemcpyAsync(rect_dev + 4 * i, I->d_rect, 4 * sizeof(int), hipMemcpyDeviceToHost, I->stream));
                SC_HIP(I, hipStreamSynchronize(I->stream));
                memcpy(rect_host + 4 * i, I->h_rect + 4, 4 * sizeof(int));
                return SC_OK;
            };
            if (form == 1) {
                if ((rc = geo_from_rect(I, guess + 4 * i, j.centerX, j.centerY, g)) || (rc = check_roi(I, g, j.body_cols, j.body_rows))) return rc;
                if ((rc = bbox_enqueue(I, j.mask, j.mask_cols, j.mask_rows, j.mask_step, &g))) return rc;
            } else {
                if ((rc = bbox_enqueue(I, j.mask, j.mask_cols, j.mask_rows, j.mask_step))) return rc;
                if ((rc = rects())) return rc;
                if (!(j.rc = geo_from_rect(I, I->h_rect + 4, j.centerX, j.centerY, g))) j.rc = check_roi(I, g, j.body_cols, j.body_rows);
                if (j.rc || !fields) { if (!j.rc) front_geo(g, geo_out + 6 * i); continue; }
            }
            if (capacity < (size_t)g.W * g.H) return SC_ERR_BAD_SIZE;
            I->mpitch = round_up(g.W, 64);
            if ((rc = ensure(I, I->d_M, (size_t)I->mpitch * g.H, false))) return rc;
            if ((rc = setup_fields(I, g.W, g.H, 3))) return rc;
            if (!I->erode_done) erode_mask(I, j.mask, j.mask_step, j.mask_rows, g);
            I->erode_done = false;
            I->f_half = f_half; I->u_half = u_half;
            launch_clone_preprocess(I, roi_at(j.body, j.body_step, g.ltx, g.lty), j.body_step, roi_at(j.face, j.face_step, g.x0, g.y0), j.face_step);
            SC_HIP(I, hipGetLastError());
            if (form == 1 && (rc = rects())) return rc;
            front_geo(g, geo_out + 6 * i);
            if ((rc = front_download(I, i, 1, &g, 0, f_half, u_half, false, out))) return rc;
        }
        SC_HIP(I, hipStreamSynchronize(I->stream));
        return SC_OK;
    }
    // --- a group: the scans of all members, then their erodes and tiles as one launch each
    if ((rc = ensure(I, I->d_rects, (size_t)n * GROUP_RS * sizeof(int))) || (rc = ensure_pinned(I, I->h_rects, (size_t)n * 2 * GROUP_RS * sizeof(int)))) return rc;
    int *h_dev = (int *)I->h_rects.p, *h_out = h_dev + GROUP_RS * n, *d_r = (int *)I->d_rects.p;
    {
        const std::vector<MaskJob> mj = group_scan_jobs(jobs, n, std::vector<char>(n, 1), d_r, h_out);
        if ((rc = ensure(I, I->d_bbox_parts, sizeof(int) * mask_bbox_group_parts(mj.data(), n)))) return rc;
        launch_mask_bbox_group(mj.data(), n, I->stream, (int *)I->d_bbox_parts.p);
    }
    SC_HIP(I, hipGetLastError());
    SC_HIP(I, hipMemcpyAsync(h_dev, d_r, (size_t)n * GROUP_RS * sizeof(int), hipMemcpyDeviceToHost, I->stream));
    SC_HIP(I, hipStreamSynchronize(I->stream));
    std::vector<Geo> geo(n);
    int worst = SC_OK;
    Geo g0{};
    for (int i = 0; i < n; ++i) {
        sc_batch_job &j = jobs[i];
        memcpy(rect_dev + 4 * i, h_dev + GROUP_RS * i, 4 * sizeof(int));
        memcpy(rect_host + 4 * i, h_out + GROUP_RS * i, 4 * sizeof(int));
        if (!(j.rc = geo_from_rect(I, h_out + GROUP_RS * i, j.centerX, j.centerY, geo[i]))) j.rc = check_roi(I, geo[i], j.body_cols, j.body_rows);
        worst = worse(worst, j.rc);
        if (j.rc) continue;
        front_geo(geo[i], geo_out + 6 * i);
        if (form == 2 && i > 0 && (geo[i].W != geo[0].W || geo[i].H != geo[0].H)) worst = worse(worst, SC_ERR_BAD_SIZE);
        g0.W = std::max(g0.W, geo[i].W); g0.H = std::max(g0.H, geo[i].H);
    }
    if (!fields) return SC_OK;
    if (worst) return worst;
    if (capacity < (size_t)g0.W * g0.H) return SC_ERR_BAD_SIZE;
    I->mpitch = round_up(g0.W, 64);
    const size_t mplane = (size_t)I->mpitch * g0.H;
    if ((rc = ensure(I, I->d_M, mplane * n, false))) return rc;
    if ((rc = setup_fields(I, g0.W, g0.H, 3 * n))) return rc;
    std::vector<int> idx(n);
    for (int i = 0; i < n; ++i) idx[i] = i;
    std::vector<MaskJob> mj;
    std::vector<ImageJob> ij;
    group_member_jobs(I, jobs, idx, geo, nullptr, d_r, form == 3, std::vector<char>(n, 0), mplane, mj, ij);
    launch_mask_erode3_group(mj.data(), n, I->stream);
    I->erode_done = false;
    I->f_half = f_half; I->u_half = u_half; I->u0_bytes = no_u0;
    launch_preprocess_group(ij.data(), n, I->mpitch, I->U0, I->F, I->stream, I->f_half, I->u_half, I->clone_mode, !I->u0_bytes);
    SC_HIP(I, hipGetLastError());
    if ((rc = front_download(I, 0, n, geo.data(), mplane, f_half, u_half, no_u0, out))) return rc;
    SC_HIP(I, hipStreamSynchronize(I->stream));
    I->u0_bytes = false;
    return SC_OK;
}

// the image and the mask of an edit hook to the device (d_face, d_mask at their padded pitches)
static int edit_upload(Instance *I, const uint8_t *src, int cols, int rows, int ss, const uint8_t *mask, int ms, int &dps, int &dms)
{
    int rc;
    dps = round_up(3 * cols, 256);
    dms = round_up(cols, 256);
    if ((rc = ensure(I, I->d_face, (size_t)dps * rows + 64, false))) return rc;
    if ((rc = upload_rows(I, I->h_face, I->d_face.p, dps, src, ss, 3 * (size_t)cols, rows))) return rc;
    if (mask) {
        if ((rc = ensure(I, I->d_mask, (size_t)dms * rows + 64, false))) return rc;
        if ((rc = upload_rows(I, I->h_mask, I->d_mask.p, dms, mask, ms, cols, rows))) return rc;
    }
    return SC_OK;
}

int sc_hip_edit_rhs(void *p, const sc_edit_params *ep, const uint8_t *src, int cols, int rows, int ss, const uint8_t *mask, int ms,
                    uint8_t *M_out, float *lap_out, size_t plane_capacity)
{
    Instance *I = get(p);
    if (!I) return SC_ERR_BAD_ARG;
    I->err.clear();
    SC_HIP(I, hipSetDevice(I->gpu));
    int rc = edit_validate(I, ep, src, cols, rows, ss, mask, ms, src, 3 * cols);
    if (rc) return rc;
    if (plane_capacity < (size_t)cols * rows) return SC_ERR_BAD_SIZE;
    int dps, dms;
    if ((rc = edit_upload(I, src, cols, rows, ss, mask, ms, dps, dms))) return rc;
    if ((rc = setup_fields(I, cols, rows, 3))) return rc;
    if ((rc = edit_stage(I, ep, (const uint8_t *)I->d_face.p, cols, rows, dps, (const uint8_t *)I->d_mask.p, dms))) return rc;
    edit_preprocess(I, ep, (const uint8_t *)I->d_face.p, dps);
    SC_HIP(I, hipGetLastError());
    if (M_out && (rc = download_rows(I, I->h_out, M_out, cols, I->d_M.p, I->mpitch, cols, rows))) return rc;
    if (lap_out && (rc = download_field(I, I->F, lap_out))) return rc;
    SC_HIP(I, hipStreamSynchronize(I->stream));
    return SC_OK;
}

int sc_hip_canny(void *p, const uint8_t *src, int cols, int rows, int ss, float low, float high, int aperture, uint8_t *classes_out,
                 uint8_t *edges_out, int counts[2])
{
    Instance *I = get(p);
    if (!I || !src) return SC_ERR_BAD_ARG;
    I->err.clear();
    SC_HIP(I, hipSetDevice(I->gpu));
    if (!std::isfinite(low) || !std::isfinite(high) || (aperture != 3 && aperture != 5 && aperture != 7)) return SC_ERR_BAD_ARG;
    if (cols < 1 || rows < 1 || ss < 3 * cols) return SC_ERR_BAD_SIZE;
    int rc, dps, dms;
    if ((rc = edit_upload(I, src, cols, rows, ss, nullptr, 0, dps, dms))) return rc;
    I->mpitch = round_up(cols, 64);
    if ((rc = canny_stage(I, (const uint8_t *)I->d_face.p, cols, rows, dps, low, high, aperture, classes_out))) return rc;
    if (edges_out) {
        if ((rc = download_rows(I, I->h_out, edges_out, cols, I->d_edge.p, I->mpitch, cols, rows))) return rc;
        for (size_t i = 0; i < (size_t)cols * rows; ++i) edges_out[i] = edges_out[i] == 2 ? 255 : 0;
    }
    if (counts) { counts[0] = I->hyst_launches; counts[1] = I->hyst_reads; }
    SC_HIP(I, hipStreamSynchronize(I->stream));
    return SC_OK;
}

int sc_hip_edit_counts(void *p, int counts[2])
{
    Instance *I = get(p);
    if (!I || !counts) return SC_ERR_BAD_ARG;
    counts[0] = I->hyst_launches; counts[1] = I->hyst_reads;
    return SC_OK;
}

int sc_hip_bytes_writer(void *p)
{
    Instance *I = get(p);
    if (!I) return SC_ERR_BAD_ARG;
    const int w = I->bytes_writer;
    I->bytes_writer = 0;
    return w;
}

int sc_hip_u0_reader(void *p)
{
    Instance *I = get(p);
    if (!I) return SC_ERR_BAD_ARG;
    const int w = I->u0_reader;
    I->u0_reader = 0;
    return w;
}

int sc_hip_u0_bytes_fetch(const uint8_t *row, int W, int xw, int *out)
{
    if (!row || !out || W < 1) return SC_ERR_BAD_ARG;
    const bool whole = u0_wave_unguarded(xw, W);
    for (int lane = 0; lane < 64; ++lane, out += 16) {
        const int xc = u0_clamp_x(xw + 4 * lane, W);
        int shift;
        const int q = u0_first_dword(row, xc, shift);
        unsigned fetched = 15u, ch[3];
        const U0Quad v = whole ? u0_fetch_unguarded(row, q) : u0_fetch_guarded(row, W, q, fetched);
        u0_channels(v, shift, ch);
        out[0] = q; out[1] = shift; out[2] = (int)fetched; out[3] = whole ? 1 : 0;
        for (int c = 0; c < 3; ++c) {
            float f[4];
            u0_values(ch[c], xc, W, f);
            for (int k = 0; k < 4; ++k) out[4 + 4 * c + k] = (int)f[k];
        }
    }
    return SC_OK;
}

int sc_hip_field_load(void *p, int W, int H, int C, const float *U, const float *lap)
{
    Instance *I = get(p);
    if (I) field_moved(I);
    if (I) I->out_direct = false;
    if (!I || !U || !lap) return SC_ERR_BAD_ARG;
    I->err.clear();
    SC_HIP(I, hipSetDevice(I->gpu));
    if (W < 1 || H < 1 || C < 1 || C > 16) return SC_ERR_BAD_SIZE;
    int rc;
    if ((rc = setup_fields(I, W, H, C))) return rc;
    // deterministic pads
    SC_HIP(I, hipMemsetAsync(I->d_U0.p, 0, I->U0.bytes(), I->stream));
    SC_HIP(I, hipMemsetAsync(I->d_U1.p, 0, I->U1.bytes(), I->stream));
    SC_HIP(I, hipMemsetAsync(I->d_F.p, 0, I->F.bytes(), I->stream));
    const size_t wb = (size_t)W * sizeof(float), pb = (size_t)I->U0.pitch * sizeof(float);
    // a field's planes are contiguous: C * H rows at one pitch, one packed upload each (separate staging buffers)
    if ((rc = upload_rows(I, I->h_face, I->U0.p, pb, (const uint8_t *)U, wb, wb, C * H))) return rc;
    if ((rc = upload_rows(I, I->h_body, I->F.p, pb, (const uint8_t *)lap, wb, wb, C * H))) return rc;
    SC_HIP(I, hipMemcpyAsync(I->U1.p, I->U0.p, pb * (size_t)(C * H - 1) + wb, hipMemcpyDeviceToDevice, I->stream));
    SC_HIP(I, hipStreamSynchronize(I->stream));
    return SC_OK;
}

int sc_hip_field_sweep(void *p, int method, int sweeps, float omega, int spl)
{
    Instance *I = get(p);
    if (I && I->out_direct) { I->err = "the last clone kept no solution field (set SC_FLAG_KEEP_FIELD to keep it)"; return SC_ERR_BAD_ARG; }
    if (I && I->f_half) { int frc = float_rhs(I); if (frc) return frc; }
    if (!I || !I->F.p) return SC_ERR_BAD_ARG;
    SC_HIP(I, hipSetDevice(I->gpu));
    I->info.sweep_launches = 0;
    int rc = run_sweeps(I, method, sweeps, omega, spl);
    if (rc) return rc;
    SC_HIP(I, hipStreamSynchronize(I->stream));
    return SC_OK;
}

int sc_hip_field_residual(void *p, double out[2])
{
    Instance *I = get(p);
    if (I && I->out_direct) { I->err = "the last clone kept no solution field (set SC_FLAG_KEEP_FIELD to keep it)"; return SC_ERR_BAD_ARG; }
    if (I && I->f_half) { int frc = float_rhs(I); if (frc) return frc; }
    if (!I || !I->F.p || !out) return SC_ERR_BAD_ARG;
    SC_HIP(I, hipSetDevice(I->gpu));
    return eval_residual(I, out);
}

int sc_hip_field_solve(void *p)
{
    Instance *I = get(p);
    if (I && I->f_half) { int frc = float_rhs(I); if (frc) return frc; }
    if (!I || !I->F.p) return SC_ERR_BAD_ARG;
    SC_HIP(I, hipSetDevice(I->gpu));
    I->info.sweep_launches = 0;
    int rc = solve(I);
    hipError_t e = hipStreamSynchronize(I->stream);
    if (e != hipSuccess) return hip_fail(I, e, "hipStreamSynchronize");
    return rc;
}

int sc_hip_field_shape(void *p, int whc[3])
{
    Instance *I = get(p);
    if (!I || !I->F.p || !whc) return SC_ERR_BAD_ARG;
    whc[0] = I->F.W; whc[1] = I->F.H; whc[2] = I->F.C;
    return SC_OK;
}

int sc_hip_field_store(void *p, float *U_out, size_t capacity_floats)
{
    Instance *I = get(p);
    if (I && I->out_direct) { I->err = "the last clone kept no solution field (set SC_FLAG_KEEP_FIELD to keep it)"; return SC_ERR_BAD_ARG; }
    if (!I || !I->F.p || !U_out) return SC_ERR_BAD_ARG;
    if (capacity_floats < (size_t)I->F.W * I->F.H * I->F.C) { I->err = "field_store: buffer too small"; return SC_ERR_BAD_SIZE; }
    SC_HIP(I, hipSetDevice(I->gpu));
    int rc = download_field(I, result(I), U_out);
    if (rc) return rc;
    SC_HIP(I, hipStreamSynchronize(I->stream));
    return SC_OK;
}

int sc_hip_field_finish(void *p, uint8_t *body, int bc, int br, int bs, int ltx, int lty)
{
    Instance *I = get(p);
    if (I && I->out_direct) { I->err = "the last clone kept no solution field (set SC_FLAG_KEEP_FIELD to keep it)"; return SC_ERR_BAD_ARG; }
    if (!I || !I->F.p || !body) return SC_ERR_BAD_ARG;
    I->err.clear();
    SC_HIP(I, hipSetDevice(I->gpu));
    const Field &U = result(I);
    if (U.C != 3) { I->err = "field_finish: needs a 3-channel field"; return SC_ERR_BAD_SIZE; }
    if (bc <= 0 || br <= 0 || bs < 3 * bc) return SC_ERR_BAD_SIZE;
    Geo g{ 0, 0, U.W, U.H, ltx, lty };
    int rc;
    if ((rc = check_roi(I, g, bc, br))) return rc;
    const int dfs = round_up(3 * g.W, 256);
    if ((rc = ensure(I, I->d_body_roi, (size_t)dfs * g.H))) return rc;
    uint8_t *roi = body + (size_t)lty * bs + 3 * ltx;
    if ((rc = upload_rows(I, I->h_body, I->d_body_roi.p, dfs, roi, bs, 3 * (size_t)g.W, g.H))) return rc;
    launch_postprocess(U, (uint8_t *)I->d_body_roi.p, dfs, I->stream);
    SC_HIP(I, hipGetLastError());
    return download_rows(I, I->h_out, roi, bs, I->d_body_roi.p, dfs, 3 * (size_t)g.W, g.H);
}

int sc_hip_field_lowmode(void *p)
{
    Instance *I = get(p);
    if (I && I->out_direct) { I->err = "the last clone kept no solution field (set SC_FLAG_KEEP_FIELD to keep it)"; return SC_ERR_BAD_ARG; }
    if (I && I->f_half) { int frc = float_rhs(I); if (frc) return frc; }
    if (!I || !I->F.p) return SC_ERR_BAD_ARG;
    SC_HIP(I, hipSetDevice(I->gpu));
    Field &U = result(I), &O = I->result_in_U1 ? I->U0 : I->U1;
    // the partner buffer receives the interior; give it the ring as well so it is a complete field
    SC_HIP(I, hipMemcpyAsync(O.p, U.p, U.bytes(), hipMemcpyDeviceToDevice, I->stream));
    int rc = lowmode_correct(I, U, O);
    if (rc) return rc;
    I->result_in_U1 = !I->result_in_U1;
    SC_HIP(I, hipStreamSynchronize(I->stream));
    return SC_OK;
}

int sc_hip_field_time_sweeps(void *p, int method, int launches, int spl, float omega, float *ms_per_launch)
{
    Instance *I = get(p);
    if (I) field_moved(I);
    if (I && I->f_half) { int frc = float_rhs(I); if (frc) return frc; }
    if (!I || !I->F.p || !ms_per_launch || launches < 1) return SC_ERR_BAD_ARG;
    SC_HIP(I, hipSetDevice(I->gpu));
    int d = fused_depth(method, spl);
    if (method == SC_METHOD_JACOBI && (d == 5 || d == 7)) d -= 1;   // instantiated depths: 1-4, 6, 8
    const int per = d > 0 ? d : 1;                      // sweeps one "launch group" performs
    I->bench_tag = true;                                // same code under a second symbol (see k_jacobi)
    int rc = run_sweeps(I, method, per, omega, spl);    // warm-up
    if (rc) { I->bench_tag = false; return rc; }
    I->info.sweep_launches = 0;
    SC_HIP(I, hipEventRecord(I->ev_k0, I->stream));
    rc = run_sweeps(I, method, launches * per, omega, spl);
    I->bench_tag = false;
    if (rc) return rc;
    SC_HIP(I, hipEventRecord(I->ev_k1, I->stream));
    SC_HIP(I, hipStreamSynchronize(I->stream));
    const int n = I->info.sweep_launches > 0 ? I->info.sweep_launches : 1;
    *ms_per_launch = ev_ms(I->ev_k0, I->ev_k1) / (float)n;
    return SC_OK;
}

// Isolated timing of the level-0 cycle kernel (prolongation + 4 red-black sweeps + residual +
// restriction) on the fields and hierarchy the last MULTIGRID run left on the device.  The values
// it produces are discarded; only the launch duration matters (bench.py roofline).
int sc_hip_time_cycle0(void *p, int launches, float *ms_per_launch)
{
    Instance *I = get(p);
    if (I) field_moved(I);
    if (!I || !ms_per_launch || launches < 1) return SC_ERR_BAD_ARG;
    if (!I->F.p || I->mg.size() < 2 || !I->mg_partial.p) { I->err = "time_cycle0: run a multigrid clone first"; return SC_ERR_BAD_ARG; }
    SC_HIP(I, hipSetDevice(I->gpu));
    const bool comp = mg_composes_level1(I);          // time the form the clone itself runs
    const bool l1_half = comp && I->mg_l1_half;
    const FusedStep full = default_step(FUSED_FULL, l1_half && I->mg_q16_last, comp);
    auto once = [&]() {
        Cycle0Launch d = step_launch(level0_launch(I, comp), full);
        d.timing = true; d.partial = (float *)I->mg_partial.p;
        d.rag = nullptr;        // (a class's fields under the plain form: the class's dimensions)
        d.l1_half = l1_half;
        launch_cycle0(d);
        I->result_in_U1 = !I->result_in_U1;
    };
    once();
    SC_HIP(I, hipEventRecord(I->ev_k0, I->stream));
    for (int i = 0; i < launches; ++i) once();
    SC_HIP(I, hipEventRecord(I->ev_k1, I->stream));
    SC_HIP(I, hipGetLastError());
    SC_HIP(I, hipStreamSynchronize(I->stream));
    *ms_per_launch = ev_ms(I->ev_k0, I->ev_k1) / (float)launches;
    return SC_OK;
}

int sc_hip_time_cycle0_form(void *p, int form, int launches, float *ms_per_launch)
{
    if (form == 0) return sc_hip_time_cycle0(p, launches, ms_per_launch);
    Instance *I = get(p);
    if (I) field_moved(I);
    if (!I || !ms_per_launch || launches < 1 || form < 1 || form > 3) return SC_ERR_BAD_ARG;
    if (!I->F.p || I->mg.size() < 3 || !I->mg_partial.p || !mg_composes_level1(I) || !I->mg_l1_half || !I->mg_q16_last || !I->f_half) {
        I->err = "time_cycle0_form: run a default multigrid clone first";
        return SC_ERR_BAD_ARG;
    }
    SC_HIP(I, hipSetDevice(I->gpu));
    float4 *bands = form == 1 ? lowmode_bands_buffer(I, 4) : nullptr;
    LmNodes lm;
    if (form == 2 && I->lm.CN.p && !I->lm.singular) { lm.CN = (const float *)I->lm.CN.p; lm.ny = I->lm.ny; lm.npitch = I->lm.npitch; }
    // the other three launches of a fast-path solve -- the full cycle before the judged one (16-bit field in, float out, leaves the correction's
    // cell shares), the judged cycle writing output bytes, the first launch (float16 initial field in, 16-bit field out, no prolongation) -- as
    // that solve's schedule says them, under their second symbols
    const FusedStep s = default_step(form == 1 ? FUSED_BEFORE_JUDGED : form == 2 ? FUSED_JUDGED_BYTES : FUSED_FIRST, true, true);
    Cycle0Launch d = step_launch(level0_launch(I, s.composed), s);
    d.timing = true; d.partial = (float *)I->mg_partial.p; d.rag = nullptr;
    if (s.bands) d.bands = bands;
    if (s.lm) d.lm = lm;
    // values are discarded: every form reads the fields in the format it expects (whatever bits they hold) and writes the partner
    auto once = [&]() { return launch_cycle0(d); };
    if (once() < 0) { I->err = "time_cycle0_form: form not instantiated"; return SC_ERR_BAD_ARG; }
    SC_HIP(I, hipEventRecord(I->ev_k0, I->stream));
    for (int i = 0; i < launches; ++i) once();
    SC_HIP(I, hipEventRecord(I->ev_k1, I->stream));
    SC_HIP(I, hipGetLastError());
    SC_HIP(I, hipStreamSynchronize(I->stream));
    lowmode_bands_written(I, nullptr);
    *ms_per_launch = ev_ms(I->ev_k0, I->ev_k1) / (float)launches;
    return SC_OK;
}

int sc_hip_coarse_tile_plan(const int *facts, int *plan)
{
    if (!facts || !plan) return SC_ERR_BAD_ARG;
    const int W = facts[0], H = facts[1], C = facts[2], uw = facts[3], hx = facts[4], rows = facts[5], first = facts[8], n = facts[9];
    if (W < 1 || H < 1 || C < 1 || hx < 4 || hx % 4 || uw != 256 - 2 * hx || rows < 1 || first < 0 || n < 0) return SC_ERR_BAD_ARG;
    const TilePlan tp = coarse_tile_plan(W, H, C, uw, hx, rows, facts[6] != 0, facts[7] == 0);
    if ((long)first + n > tp.blocks) return SC_ERR_BAD_ARG;
    plan[0] = tp.full; plan[1] = tp.lps; plan[2] = tp.K; plan[3] = tp.blocks;
    for (int k = 0; k < n; ++k) {
        int *o = plan + 4 + 130 * (size_t)k;
        for (int lane = 0; lane < 64; ++lane) {
            const TileLane tl = coarse_tile_lane(tp, C, uw, hx, first + k, lane);
            o[0] = tl.by; o[1] = tl.lps; o[2 + 2 * lane] = tl.c; o[3 + 2 * lane] = tl.x;
        }
    }
    return SC_OK;
}

int sc_hip_cycle0_plan(const int *facts, int *plan, int capacity)
{
    if (!facts || !plan || capacity < SC_CYCLE0_PLAN_HEAD) return SC_ERR_BAD_ARG;
    const int W = facts[0], H = facts[1], sweeps = facts[2];
    const bool prolong = facts[3] != 0, composed = facts[4] != 0;
    if (W < 3 || H < 3 || W > 65536 || H > 65536) return SC_ERR_BAD_ARG;
    std::vector<MGGeom> g;
    mg_plan_levels(W, H, g);                                  // build_levels' ladder
    const int nl = (int)g.size();
    if ((prolong && nl < 2) || (composed && nl < 3)) return SC_ERR_BAD_ARG;
    const size_t bottom = mg_plan_bottom(g, true);            // ... and its default bottom
    int *const verdicts = capacity > SC_CYCLE0_PLAN_HEAD ? plan + SC_CYCLE0_PLAN_HEAD : nullptr;
    if (cycle0_plan(W, H, sweeps, prolong, composed, g[0].x.nc, g[0].y.nc, nl > 1 ? g[1].x.nc : 0, nl > 1 ? g[1].y.nc : 0, plan, verdicts,
                    capacity - SC_CYCLE0_PLAN_HEAD) < 0) return SC_ERR_BAD_ARG;
    plan[8] = nl; plan[9] = (int)bottom; plan[10] = (int)mg_default_tail_level(g);
    plan[11] = mg_ladder_composes((size_t)nl, bottom);         // mg_composes_level1 under the default options
    plan[12] = g[0].x.nc; plan[13] = g[0].y.nc; plan[14] = nl > 1 ? g[1].x.nc : 0; plan[15] = nl > 1 ? g[1].y.nc : 0;
    return SC_OK;
}

int sc_hip_pcg_plan(int cols, int rows, int kind, int frames, long long plan[10])
{
    if (!plan || frames < 1 || frames > SC_POISSON_MAX_PLANES) return SC_ERR_BAD_ARG;
    const sc_poisson_layout l{ cols, rows, 1, 1, (long long)cols, (long long)cols * rows };
    const int rc = family_validate(&kind, &l, nullptr, "at most 8192 unknowns (pixels - 2) per side", nullptr);
    if (rc) return rc;
    const int k = poisson_norm_kind(kind);
    const MixedGeo mg = poisson_mixed_geo(poisson_free_sides(k), cols, rows, poisson_periodic(k));      // pcg_chunk_begin's
    const PcgGeo wg = frames > 1 ? volume_work_geo(mg, frames) : pcg_geo(mg);                            // PcgOperator::work_geo's two forms
    const long long out[10] = { wg.nx, wg.ny, wg.x0, wg.y0, wg.cg, wg.bands, wg.rows, wg.eparts, wg.egroups, wg.stride };
    std::copy(out, out + 10, plan);
    return SC_OK;
}

int sc_hip_cycle0_form(const int *facts, int index, int form[3])
{
    if (!form) return SC_ERR_BAD_ARG;
    int T = 0, TAG = 0, rc;
    bool PRO = false;
    if (facts) {
        static float4 some_bands;
        static const RagMember some_class{};
        Cycle0Launch d;
        d.sweeps = facts[0]; d.prolong = facts[1]; d.f_half = facts[2]; d.u_half = (facts[3] & 1) != 0; d.in_bytes = (facts[3] & 2) != 0; d.q16_in = facts[4]; d.q16_out = facts[5];
        d.final_cycle = facts[6]; d.out_bytes = (facts[7] & 1) != 0; d.out_interleaved = (facts[7] & 2) != 0; d.composed = facts[8]; d.l1_half = facts[9]; d.timing = facts[10];
        d.bands = facts[11] ? &some_bands : nullptr; d.rag = facts[12] ? &some_class : nullptr;
        rc = cycle0_form(d, T, PRO, TAG) ? 0 : -1;
    } else if ((rc = cycle0_form_at(index, T, PRO, TAG)) <= index || index < 0) {
        return rc;
    }
    if (rc >= 0) { form[0] = T; form[1] = PRO; form[2] = TAG; }
    return rc;
}

int sc_hip_fused_schedule(const int *facts, const int *verdicts, int nverdicts, int *rows, int capacity)
{
    if (!facts || !rows || nverdicts < 0 || (nverdicts > 0 && !verdicts)) return SC_ERR_BAD_ARG;
    const int pre = facts[0], post = facts[1], budget = facts[2], early_kind = facts[9];
    if (pre < 1 || pre > 2 || post < 1 || post > 2 || budget < 1 || budget > 64 || early_kind < 0 || early_kind > 3) return SC_ERR_BAD_ARG;
    const bool bytes_form = facts[10] != 0;
    FusedSchedule S{ FusedFacts{ pre, post, budget, facts[3] != 0, facts[4] != 0, facts[5] != 0, facts[6] != 0, facts[7] != 0, facts[8] != 0, facts[11] != 0 } };
    int n = 0, used = 0, verdict = VERDICT_NONE;
    for (;;) {
        FusedStep s = fused_next(S, verdict);
        if (s.kind == FUSED_DONE) break;
        if (s.ask_early) fused_early(S, s, early_kind);
        if (capacity < SC_FUSED_ROW * (n + 1) + 3) return SC_ERR_BAD_ARG;
        const int row[SC_FUSED_ROW] = { s.kind, s.sweeps, s.prolong, s.final_cycle, s.out_bytes, s.u_half, s.q16_in, s.q16_out, s.composed, s.bands, s.lm,
                                        s.nodes, s.judged, s.coarse_first, s.sat, s.bands_sweeps, s.ask_early, S.cyc };
        std::memcpy(rows + SC_FUSED_ROW * n++, row, sizeof(row));
        verdict = VERDICT_NONE;
        if (!s.judged) continue;
        if (s.out_bytes && !bytes_form) { verdict = VERDICT_NO_FORM; continue; }
        // what the read-back showed, as the driver reads it: the early condition applies to conditional bytes only, the saturation word to a 16-bit solve
        verdict = nverdicts ? verdicts[std::min(used++, nverdicts - 1)] : VERDICT_ACCEPT;
        if (verdict < VERDICT_ACCEPT || verdict > VERDICT_SATURATED) return SC_ERR_BAD_ARG;
        if (verdict == VERDICT_REJECT_EARLY && !(s.out_bytes && S.early_cond)) verdict = VERDICT_ACCEPT;
        if (verdict == VERDICT_SATURATED && !S.f.q16) verdict = VERDICT_ACCEPT;
    }
    if (capacity < SC_FUSED_ROW * n + 3) return SC_ERR_BAD_ARG;
    rows[SC_FUSED_ROW * n] = S.cyc; rows[SC_FUSED_ROW * n + 1] = S.sweep_launches; rows[SC_FUSED_ROW * n + 2] = S.result;
    return n;
}

int sc_hip_time_coarse_chain(void *p, int reps, float *ms_eager, float *ms_graph, int *launches)
{
    Instance *I = get(p);
    if (!I || reps < 1 || !ms_eager || !ms_graph || !launches) return SC_ERR_BAD_ARG;
    SC_HIP(I, hipSetDevice(I->gpu));
    return mg_time_coarse_chain(I, reps, ms_eager, ms_graph, launches);
}

int sc_hip_time_tail_phases(void *p, unsigned long long *cycles11)
{
    Instance *I = get(p);
    if (!I || !cycles11) return SC_ERR_BAD_ARG;
    SC_HIP(I, hipSetDevice(I->gpu));
    return mg_time_tail_phases(I, cycles11);
}

} // extern "C"
