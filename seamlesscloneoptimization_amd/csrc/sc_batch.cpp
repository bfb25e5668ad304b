// sc_batch.cpp -- the batch path: n device-resident clones on one instance (sc_hip_run_device_batch), partitioned into same-size
// groups and size classes (sc_ragged.cpp), and the host-only planner exports (sc_hip_plan_*) that show how a batch would be split.
#include "sc_instance.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

using namespace sc;

namespace sc {

// The frame of a destination (sc_common.h, FrameSpans): what splice_block and postprocess_block leave alone -- the ROI's ring, everything
// around the ROI, row padding, the bytes behind the last pixel of a row.  The interior they write is the byte columns
// [3 (ltx + 1), 3 (ltx + W - 1)) of rows lty + 1 .. lty + H - 2; the bytes from the end of one interior row's interior to the start of
// the next one's are contiguous in memory, so the H - 2 interior rows leave H - 3 runs between them.  The ROI lies inside the image
// (check_roi) and 3 * cols <= step, so every run has at least six bytes and the tail ends at the image's last byte.
FrameSpans frame_spans(size_t step, int rows, int ltx, int lty, int W, int H)
{
    FrameSpans f{};
    f.bytes = step * (size_t)rows;
    f.head_end = f.tail_begin = f.bytes;
    if (W < 3 || H < 3) return f;          // no interior: nothing the clone writes
    const size_t c0 = 3 * (size_t)(ltx + 1), c1 = 3 * (size_t)(ltx + W - 1), top = (size_t)(lty + 1) * step;
    f.head_end = top + c0;
    f.mid_first = top + c1; f.mid_len = step - (c1 - c0); f.stride = step; f.mids = H - 3;
    f.tail_begin = top + (size_t)(H - 3) * step + c1;
    return f;
}

std::vector<MaskJob> group_scan_jobs(const sc_batch_job *jobs, int n, const std::vector<char> &usable, int *d_r, int *h_out)
{
    std::vector<MaskJob> mj;
    mj.reserve(n);
    for (int i = 0; i < n; ++i) {
        if (!usable[i]) continue;
        MaskJob m{};
        m.mask = jobs[i].mask; m.mw = jobs[i].mask_cols; m.mh = jobs[i].mask_rows; m.mstep = jobs[i].mask_step;
        m.rect = d_r + GROUP_RS * i; m.rect_host = h_out + GROUP_RS * i;
        mj.push_back(m);
    }
    return mj;
}

void group_member_jobs(Instance *I, const sc_batch_job *jobs, const std::vector<int> &idx, const std::vector<Geo> &geo, const int *guess, int *d_r,
                       bool size_class, const std::vector<char> &frame, size_t mplane, std::vector<MaskJob> &mj, std::vector<ImageJob> &ij)
{
    const int n = (int)idx.size();
    mj.assign(n, MaskJob{});
    ij.assign(n, ImageJob{});
    for (int k = 0; k < n; ++k) {
        const int i = idx[k];
        const sc_batch_job &j = jobs[i];
        mj[k].mask = j.mask; mj[k].mw = j.mask_cols; mj[k].mh = j.mask_rows; mj[k].mstep = j.mask_step;
        mj[k].rect = d_r + GROUP_RS * i;
        mj[k].g = geo[i]; mj[k].M = (uint8_t *)I->d_M.p + mplane * k; mj[k].mpitch = I->mpitch;
        ij[k].face_org = roi_at(j.face, j.face_step, geo[i].x0, geo[i].y0); ij[k].fstep = j.face_step;
        ij[k].body_org = roi_at(j.body, j.body_step, geo[i].ltx, geo[i].lty);
        ij[k].body_src = frame[i] ? roi_at(j.body_restore, j.body_step, geo[i].ltx, geo[i].lty) : ij[k].body_org; ij[k].bstep = j.body_step;
        ij[k].M = (const uint8_t *)I->d_M.p + mplane * k;
        ij[k].d_rect = guess ? d_r + GROUP_RS * i : nullptr;
        if (guess) { ij[k].rx0 = guess[4 * i]; ij[k].rx1 = guess[4 * i + 1]; ij[k].ry0 = guess[4 * i + 2]; ij[k].ry1 = guess[4 * i + 3]; }
        if (size_class) { ij[k].W = geo[i].W; ij[k].H = geo[i].H; }
    }
}

} // namespace sc

// ---- n device-resident clones through ONE set of launches ------------------------------------------------------
// The solver treats the channels of a field as independent planes, so n clones whose ROIs have the same size are one
// field of 3n channels: every multigrid launch is n times larger (the coarse levels stop being launch-latency bound,
// the level-1 grid fills whole rounds of workgroup slots) and there are 27 solver launches for the group instead of
// 27 n.  Masks, positions and images are per clone (bounding box, erode, pre- and post-process each go out as one launch
// for the group, blockIdx.z = member); the stop rule sees the largest correction of the group.
// Round 5: the members of a call are PARTITIONED by ROI size -- every sub-group of two or more same-size members shares one
// set of launches, the rest run alone -- instead of the whole call falling back to one clone at a time as soon as one member
// differs (a batch of real clones has a mask box per face / frame).  A failing member, the reference's warm-up option and
// OpenCV's grey-mask semantics still run one after the other through sc_hip_run_device.
namespace {

struct RagScope {      // leaves the size-class mode on every way out
    Instance *I;
    ~RagScope() { rag_end(I); }
};

// members idx[0..n) of `jobs` as one field of 3n channels: all with the same ROI size (plans == nullptr), or a SIZE CLASS (sc_ragged.cpp:
// plans[k] = member idx[k]'s plan; the fields take the class's largest width and height).  guess: the predicted rectangles the
// members were launched on (nullptr: their boxes are the device's), d_r: the device rectangles of ALL members of the call.
// frame[i]: only the frame of member i's destination was restored (sc_hip_run_device_batch), so its destination pixels are READ from
// body_restore; its output is written to body as ever.  Such a member's interior holds stale bytes until it is SPLICED, and a code of
// SC_OK or SC_ERR_NOT_CONVERGED from here says an output launch over every member's interior is in the stream:
//  - the accepted bytes form in mg_solve_fused, which then sets spec_post.done (VERDICT_ACCEPT): the judged launch itself where it writes
//    the members' interleaved bytes (k_cycle0 with C0_OUT3: every interior pixel of every member, the same guards as the splice), else
//    launch_splice_planar_group behind it;
//  - write_output: mg_solve_fused's behind a judged cycle that leaves its field (spec_post.done), else the line behind solve_step below
//    (every other solver, a budget that ran out, a rejected bytes form);
//  - the saturation retry inside solve_step: the first attempt's output launches carried the solve's AbortFlag and wrote nothing, the
//    pre-process runs again -- from body_src, the pristine pixels -- and the second attempt ends in one of the two lines above.
// What is left is the member's own guard (a predicted box the device did not find): the caller compares and restores.
int run_group_members(Instance *I, sc_batch_job *jobs, const std::vector<int> &idx, const std::vector<Geo> &geo, const int *guess, int *d_r,
                      const std::vector<SizePlan> *plans, const std::vector<char> &frame)
{
    const int n = (int)idx.size();
    Geo g0 = geo[idx[0]];
    if (plans) for (int k = 1; k < n; ++k) { g0.W = std::max(g0.W, geo[idx[k]].W); g0.H = std::max(g0.H, geo[idx[k]].H); }
    int rc;
    I->mpitch = round_up(g0.W, 64);
    const size_t mplane = (size_t)I->mpitch * g0.H;
    if ((rc = ensure(I, I->d_M, mplane * n, false))) return rc;
    if ((rc = setup_fields(I, g0.W, g0.H, 3 * n))) return rc;
    RagScope scope{ I };
    CallScope call{ I };
    std::vector<MaskJob> mj;
    std::vector<ImageJob> ij;
    group_member_jobs(I, jobs, idx, geo, guess, d_r, plans != nullptr, frame, mplane, mj, ij);
    // (a size class: the members' table goes up FIRST -- 9 us of host time, a 3-us copy in front of the erode -- so that the other
    //  streams' builds, which wait for it, run beside the erode and the pre-process)
    if (plans && (rc = rag_begin_table(I, *plans))) return rc;
    bool builds_done = false;
    launch_mask_erode3_group(mj.data(), n, I->stream);
    I->erode_done = false;
    // --- one solve for the group, results spliced per clone
    I->guard = RectGuard();
    const SolveTarget to{ nullptr, 0, &ij };
    const int solve_rc = solve_step(I, to, [&]() -> int {
        launch_preprocess_group(ij.data(), n, I->mpitch, I->U0, I->F, I->stream, I->f_half, I->u_half, I->clone_mode, !I->u0_bytes);
        SC_HIP(I, hipGetLastError());
        // a size class: the launches that build its per-call state (rag_begin_builds: 12 us of host time) go in HERE, while the device
        // erodes and pre-processes -- neither reads the table (member sizes travel in the ImageJobs); with all of rag_begin in front of
        // the erode the device idled for as long (16 x 320^2: the first level-0 launch started 119 us into the call, now ~80)
        if (plans && !builds_done) {
            if ((rc = rag_begin_builds(I))) return rc;
            builds_done = true;
        }
        return SC_OK;
    });
    if (solve_rc != SC_OK && solve_rc != SC_ERR_NOT_CONVERGED) return solve_rc;
    if (!I->spec_post.done && (rc = write_output(I, to))) return rc;
    for (int k = 0; k < n; ++k) jobs[idx[k]].rc = solve_rc;
    SC_HIP(I, hipGetLastError());
    fill_info_geo(I, g0);
    I->info.group_members = n; I->info.group_ragged = plans ? 1 : 0;
    return solve_rc;
}

// the planner exports' group_of / kind_of (sc_hip_plan_groups) for `groups`; plan i is the caller's member order[i] (nullptr: i)
int report_groups(const std::vector<std::vector<int>> &groups, const std::vector<SizePlan> &plans, const int *order, int *group_of, int *kind_of)
{
    for (size_t g = 0; g < groups.size(); ++g) {
        bool uniform = true;
        for (int i : groups[g]) uniform = uniform && plans[i].W == plans[groups[g][0]].W && plans[i].H == plans[groups[g][0]].H;
        for (int i : groups[g]) {
            const int m = order ? order[i] : i;
            group_of[m] = (int)g;
            if (kind_of) kind_of[m] = groups[g].size() < 2 ? 0 : uniform ? 1 : plans[i].solo_differs ? 3 : 2;
        }
    }
    return (int)groups.size();
}

} // namespace

extern "C" {

int sc_hip_run_device_batch(void *p, sc_batch_job *jobs, int n)
{
    if (!jobs || n <= 0) return SC_ERR_BAD_ARG;
    Instance *I;
    int rc = begin_call(p, I);
    if (rc) return rc;
    auto alone = [&](int i) -> int {
        sc_batch_job &j = jobs[i];
        j.rc = sc_hip_run_device(p, j.face, j.face_cols, j.face_rows, j.face_step, j.body, j.body_cols, j.body_rows, j.body_step,
                                 j.mask, j.mask_cols, j.mask_rows, j.mask_step, j.centerX, j.centerY, false);
        return j.rc;
    };
    auto one_by_one = [&]() -> int {
        int worst = SC_OK;
        for (int i = 0; i < n; ++i) worst = worse(worst, alone(i));
        return worst;
    };
    // Refresh the destinations that ask for it: one launch per 16 (k_copy_group); odd alignments take the runtime's copy.  frame[i]:
    // only the frame of member i's destination (frame_spans) -- its clone writes the rest.  The calls that group nothing restore
    // everything at once; a call that may group restores behind the host's decision on who is grouped (below).
    std::vector<char> frame(n, 0);
    std::vector<Geo> geo(n);
    auto restore = [&]() -> int {
        CopyJobs cj{};
        int cn = 0;
        auto flush = [&]() { if (cn) { launch_copy_group(cj, cn, I->stream); cn = 0; } };
        for (int i = 0; i < n; ++i) {
            const sc_batch_job &j = jobs[i];
            if (!j.body_restore) continue;
            const size_t bytes = (size_t)j.body_step * j.body_rows;
            if ((((uintptr_t)j.body | (uintptr_t)j.body_restore) & 15) != 0) {
                SC_HIP(I, hipMemcpyAsync(j.body, j.body_restore, bytes, hipMemcpyDeviceToDevice, I->stream));
                continue;
            }
            cj.dst[cn] = j.body; cj.src[cn] = j.body_restore; cj.bytes[cn] = bytes;
            cj.frame[cn] = frame[i] ? frame_spans((size_t)j.body_step, j.body_rows, geo[i].ltx, geo[i].lty, geo[i].W, geo[i].H) : FrameSpans{};
            if (++cn == CopyJobs::MAX) flush();
        }
        flush();
        SC_HIP(I, hipGetLastError());
        return SC_OK;
    };
    // the interior ROWS of a member whose frame alone was restored and that was not spliced: with them its destination is the restore
    // source again, byte for byte
    auto restore_rows = [&](int i) -> int {
        const sc_batch_job &j = jobs[i];
        const size_t at = (size_t)(geo[i].lty + 1) * j.body_step, end = std::min((size_t)(geo[i].lty + geo[i].H - 1) * j.body_step, (size_t)j.body_step * j.body_rows);
        frame[i] = 0;
        SC_HIP(I, hipMemcpyAsync(j.body + at, j.body_restore + at, end - at, hipMemcpyDeviceToDevice, I->stream));
        return SC_OK;
    };
    if (n == 1 || I->opts.reference_warmup || (I->opts.flags & SC_FLAG_OPENCV_GREY_MASK)) return (rc = restore()) ? rc : one_by_one();
    // members whose images do not even validate run alone (and report their own error); the others are candidates for a group
    std::vector<char> usable(n, 1);
    int nusable = 0;
    for (int i = 0; i < n; ++i) {
        const sc_batch_job &j = jobs[i];
        if (validate_images(I, j.face, j.face_cols, j.face_rows, j.face_step, j.body, j.body_cols, j.body_rows, j.body_step,
                            j.mask, j.mask_cols, j.mask_rows, j.mask_step) != SC_OK) usable[i] = 0;
        else ++nusable;
    }
    I->err.clear();
    if (nusable < 2) return (rc = restore()) ? rc : one_by_one();
    I->stage_marks = false;
    // --- bounding boxes of all masks, one read-back
    constexpr int RS = GROUP_RS;
    if ((rc = ensure(I, I->d_rects, (size_t)n * RS * sizeof(int))) || (rc = ensure_pinned(I, I->h_rects, (size_t)n * 2 * RS * sizeof(int)))) {
        restore();
        return rc;
    }
    // (the fold launch writes every usable member's rectangle to d_r AND into the pinned h_out: no seeds to upload, nothing to read back)
    int *h_out = (int *)I->h_rects.p + RS * n, *d_r = (int *)I->d_rects.p;
    {
        std::vector<MaskJob> mj = group_scan_jobs(jobs, n, usable, d_r, h_out);
        if ((rc = ensure(I, I->d_bbox_parts, sizeof(int) * mask_bbox_group_parts(mj.data(), (int)mj.size())))) {
            restore();
            return rc;
        }
        launch_mask_bbox_group(mj.data(), (int)mj.size(), I->stream, (int *)I->d_bbox_parts.p);
    }
    SC_HIP(I, hipGetLastError());
    if (!I->ev_rects) SC_HIP(I, hipEventCreateWithFlags(&I->ev_rects, hipEventDisableTiming));
    SC_HIP(I, hipEventRecord(I->ev_rects, I->stream));
    // Like a single clone (predict_rect), the members are launched on PREDICTED bounding boxes -- the interior of every mask,
    // which is what a mask that touches its four inner borders gives -- while the scans' answers are in flight: no host
    // wait in front of the erodes.  Every member's splice carries its guess and writes nothing unless the device found
    // that box; the host compares when the answers are in (they are by the time the solver has waited for its stop rule)
    // and repeats the members that were guessed wrong, one by one on their true boxes.
    std::vector<int> guess(4 * (size_t)n);
    bool speculative = !(I->opts.flags & SC_FLAG_NO_SPECULATE) && I->group_spec_cooldown == 0;
    if (I->group_spec_cooldown > 0) --I->group_spec_cooldown;
    std::vector<char> grouped(n, 0);          // the member's geometry is known (or predicted) and fits its destination
    if (speculative) {
        for (int i = 0; i < n; ++i) {
            if (!usable[i]) continue;
            int *r = &guess[4 * i];
            r[0] = 1; r[1] = jobs[i].mask_cols - 2; r[2] = 1; r[3] = jobs[i].mask_rows - 2;
            // (a member whose guess does not fit -- a mask narrower than three pixels, a box that leaves the destination -- runs alone on its true box)
            grouped[i] = jobs[i].mask_cols >= 3 && jobs[i].mask_rows >= 3 && geo_from_rect(I, r, jobs[i].centerX, jobs[i].centerY, geo[i]) == SC_OK &&
                         check_roi(I, geo[i], jobs[i].body_cols, jobs[i].body_rows) == SC_OK;
        }
    } else {
        SC_HIP(I, hipStreamSynchronize(I->stream));
        for (int i = 0; i < n; ++i) {
            if (!usable[i]) continue;
            grouped[i] = geo_from_rect(I, h_out + RS * i, jobs[i].centerX, jobs[i].centerY, geo[i]) == SC_OK &&
                         check_roi(I, geo[i], jobs[i].body_cols, jobs[i].body_rows) == SC_OK;
        }
    }
    I->err.clear();
    // --- partition (first-come order inside a sub-group and between them): same-size members share one set of launches as they
    //     are, members of one size class (sc_ragged.cpp: different sizes, the same solve) through the per-member table
    std::vector<int> cand;
    std::vector<SizePlan> plans;
    bool one_size = true;
    for (int i = 0; i < n; ++i) {
        if (!grouped[i]) continue;
        if (!cand.empty() && (geo[i].W != geo[cand[0]].W || geo[i].H != geo[cand[0]].H)) one_size = false;
        cand.push_back(i);
    }
    std::vector<std::vector<int>> parts;          // indices into cand / plans
    if (one_size && cand.size() >= 2) {
        // every member has the same ROI size (a benchmark's batch, a tiled image): one field of 3n channels as in rounds 2-4, and
        // nothing to plan -- sixteen memo look-ups per call and thirty-two in the pool were 0.5 % of the 2048^2 step
        parts.emplace_back(cand.size());
        for (size_t k = 0; k < cand.size(); ++k) parts[0][k] = (int)k;
        plans.resize(cand.size());
    } else {
        plans.resize(cand.size());
        for (size_t k = 0; k < cand.size(); ++k) plan_size(I->opts, geo[cand[k]].W, geo[cand[k]].H, plans[k]);
        plan_groups(plans, n, parts);
    }
    std::vector<int> singles;
    for (int i = 0; i < n; ++i) if (!grouped[i]) singles.push_back(i);
    for (const auto &pq : parts) if (pq.size() < 2) { singles.push_back(cand[pq[0]]); grouped[cand[pq[0]]] = 0; }
    // --- the restore, now that the host knows who is grouped.  A member that is launched on its predicted box in a part of two or more
    //     gets its frame only: the group reads its ROI from body_restore and writes the interior.  Both pointers must take the kernel's
    //     16-byte copies, and no other job of the call may share the destination (its restore or its clone would meet this one's stale
    //     interior).  Everyone else -- no prediction, alone, misaligned, shared -- gets the whole image as before.
    if (speculative)
        for (int i = 0; i < n; ++i) {
            const sc_batch_job &j = jobs[i];
            if (!grouped[i] || !j.body_restore || j.body_restore == j.body || geo[i].W < 3 || geo[i].H < 3 || (((uintptr_t)j.body | (uintptr_t)j.body_restore) & 15) != 0) continue;
            bool shared = false;
            for (int k = 0; k < n && !shared; ++k) shared = k != i && jobs[k].body == j.body;
            frame[i] = !shared;
        }
    if ((rc = restore())) return rc;
    int worst = SC_OK;
    sc_run_info keep{};
    bool have_group = false;
    for (const auto &pq : parts) {
        if (pq.size() < 2) continue;
        std::vector<int> q(pq.size());
        std::vector<SizePlan> qp;
        bool uniform = true;
        for (size_t k = 0; k < pq.size(); ++k) {
            q[k] = cand[pq[k]];
            uniform = uniform && geo[q[k]].W == geo[q[0]].W && geo[q[k]].H == geo[q[0]].H;
        }
        if (!uniform) for (int k : pq) qp.push_back(plans[k]);
        rc = run_group_members(I, jobs, q, geo, speculative ? guess.data() : nullptr, d_r, uniform ? nullptr : &qp, frame);
        if (rc != SC_OK && rc != SC_ERR_NOT_CONVERGED) {
            // nothing of this part or of the ones behind it was spliced.  A HIP error: nothing more can be trusted on this stream
            if (rc != SC_ERR_HIP && hipEventSynchronize(I->ev_rects) == hipSuccess)
                for (int i = 0; i < n; ++i)
                    if (frame[i] == 1 || (frame[i] == 2 && memcmp(&guess[4 * i], h_out + RS * i, 4 * sizeof(int)) != 0)) (void)restore_rows(i);
            return rc;
        }
        for (int i : q) frame[i] = frame[i] ? 2 : 0;          // spliced, if the device found the predicted box
        worst = worse(worst, rc);
        keep = I->info; have_group = true;
    }
    SC_HIP(I, hipEventRecord(I->ev_k1, I->stream));
    I->info.ms_h2d = I->info.ms_mask = I->info.ms_pre = I->info.ms_solve = I->info.ms_post = I->info.ms_d2h = I->info.ms_device_total = 0.f;
    if (have_group) keep = I->info;
    if (speculative && have_group) {
        SC_HIP(I, hipEventSynchronize(I->ev_rects));       // long since passed when the solver has waited for its stop rule
        for (int i = 0; i < n; ++i)
            if (grouped[i] && memcmp(&guess[4 * i], h_out + RS * i, 4 * sizeof(int)) != 0) {
                I->group_spec_cooldown = 8;
                if (frame[i] && (rc = restore_rows(i))) return rc;   // (its interior was not even restored)
                singles.push_back(i);                          // its destination was not touched: repeat it alone on its true box
            }
    }
    for (int i : singles) worst = worse(worst, alone(i));
    if (have_group) I->info = keep;                            // the statistics of the (last) group, not of a straggler
    return worst;
}

int sc_hip_plan_size(int W, int H, const sc_solver_opts *opts, int out[12])
{
    if (!out) return SC_ERR_BAD_ARG;
    sc_solver_opts o;
    if (opts) o = *opts; else sc_hip_default_opts(&o);
    SizePlan p;
    plan_size(o, W, H, p);
    const int v[12] = { p.ok ? 1 : 0, p.nl, p.tail, p.npx, p.npy, p.Kxp, p.Kyp, p.nxt, p.nrs, (p.t && p.tail > 0) ? p.t->g[p.tail].x.nc * 1000 + p.t->g[p.tail].y.nc : 0,
                        p.solo_differs ? 1 : 0, p.conditional ? 1 : 0 };
    memcpy(out, v, sizeof(v));
    return SC_OK;
}

int sc_hip_plan_groups(const int *wh, int n, int cap, const sc_solver_opts *opts, int *group_of, int *kind_of)
{
    if (!wh || n < 1 || !group_of) return SC_ERR_BAD_ARG;
    sc_solver_opts o;
    if (opts) o = *opts; else sc_hip_default_opts(&o);
    std::vector<SizePlan> plans(n);
    for (int i = 0; i < n; ++i) plan_size(o, wh[2 * i], wh[2 * i + 1], plans[i]);
    std::vector<std::vector<int>> groups;
    plan_groups(plans, cap > 0 ? cap : n, groups);
    return report_groups(groups, plans, nullptr, group_of, kind_of);
}

int sc_hip_plan_groups_pool(const int *wh, int n, int group, int streams, const sc_solver_opts *opts, int *group_of, int *kind_of)
{
    if (!wh || n < 1 || !group_of || group < 0 || group > 64 || streams < 1) return SC_ERR_BAD_ARG;
    sc_solver_opts o;
    if (opts) o = *opts; else sc_hip_default_opts(&o);
    // as sc_hip_pool_run: largest first, then the planner under the pool's caps
    std::vector<int> order(n);
    for (int i = 0; i < n; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return (long)(wh[2 * x] + 2) * (wh[2 * x + 1] + 2) > (long)(wh[2 * y] + 2) * (wh[2 * y + 1] + 2); });
    std::vector<SizePlan> plans(n);
    for (int i = 0; i < n; ++i) plan_size(o, wh[2 * order[i]], wh[2 * order[i] + 1], plans[i]);
    int cap, cap_max;
    long budget;
    pool_group_caps(group, n, streams, cap, cap_max, budget);
    std::vector<std::vector<int>> groups;
    plan_groups(plans, cap, groups, cap_max, budget);
    return report_groups(groups, plans, order.data(), group_of, kind_of);
}

int sc_hip_plan_prepare(const int *wh, int n, const sc_solver_opts *opts)
{
    if (!wh || n < 1) return SC_ERR_BAD_ARG;
    sc_solver_opts o;
    if (opts) o = *opts; else sc_hip_default_opts(&o);
    int eligible = 0;
    for (int i = 0; i < n; ++i) {
        SizePlan p;
        if (plan_size(o, wh[2 * i], wh[2 * i + 1], p)) ++eligible;
    }
    return eligible;
}

void sc_hip_plan_cache_clear(void) { plan_cache_clear(); }

int sc_hip_restore_spans(long long step, int rows, int ltx, int lty, int W, int H, long long *spans, int capacity)
{
    if (!spans || step < 3 || rows < 1 || ltx < 0 || lty < 0 || W < 1 || H < 1 || 3 * ((long long)ltx + W) > step || lty + H > rows) return SC_ERR_BAD_ARG;
    const FrameSpans f = frame_spans((size_t)step, rows, ltx, lty, W, H);
    int k = 0;
    auto put = [&](size_t a, size_t b) {
        if (a >= b) return;
        if (k < capacity) { spans[2 * k] = (long long)a; spans[2 * k + 1] = (long long)b; }
        ++k;
    };
    put(0, f.head_end);
    for (int r = 0; r < f.mids; ++r) put(f.mid_first + (size_t)r * f.stride, f.mid_first + (size_t)r * f.stride + f.mid_len);
    put(f.tail_begin, f.bytes);
    return k <= capacity ? k : SC_ERR_BAD_ARG;
}

int sc_hip_reference_tables_singular(int w, int h)
{
    if (w < 1 || h < 1) return 0;
    const double PIf = (double)3.14159265358979323846f;           // seamlessClone_imp.h:17
    const float fx0 = (float)(2.0 * std::cos(PIf / (w + 1.0))), fy0 = (float)(2.0 * std::cos(PIf / (h + 1.0)));
    return ((fx0 + fy0) - 4.0f < 0.0f) ? 0 : 1;
}

} // extern "C"
