// sanitize_main.cpp -- host-side sanitizer run of libseamlessclone_hip's C++ (make sanitize; tests/test_host.py).
//
// GPU AddressSanitizer is not available on the pool this library is developed on, the host side is: 3 000 lines of C++ with a
// parked-thread row copier (sc_hostcopy.cpp), pool workers pulling chunks from a shared counter (sc_pool.cpp), memoised size plans
// behind mutexes (sc_ragged.cpp), LRU bookkeeping and level geometry.  This program is the library's host code -- every source,
// compiled for the host only, with -fsanitize=address,undefined or -fsanitize=thread -- driven through the entry points that need
// no GPU:
//   1. sc_hip_selftest_host: the row copier across its helper threads, both eigen-solvers, the part maps;
//   2. the planner from several threads at once (plan cache hits, misses and evictions), against a single-threaded reference;
//   3. the pool's hand-out of jobs against stub instances (sc_pool.cpp compiled with its instance calls renamed to the stubs
//      below): groups formed, every job run exactly once, per-job codes copied back, several batches on one pool;
//   4. the same for batches of whole-image edits (sc_hip_pool_edit): chunks of one image size, every job exactly once, codes back,
//      and a chunk whose batch call fails with SC_ERR_HIP (after writing SC_OK into its members) reported as failed, job and pool.
//   5. sc_hip_poisson_check over valid and invalid layouts (the overlap test's 128-bit arithmetic at extreme strides included).
//   6. sc_hip_screened_check: lambda, the kinds and the side limits of each boundary kind.
//   7. sc_hip_weighted_check: tol, precond_lambda, the kinds, the side limits and the layouts (the chunk driver behind it starts with a
//      launch, so it is not reachable here); sc_hip_wls_check beside it on the same cases, precond_smooth like precond_lambda, and
//      sc_hip_robust_check: the same verdicts on a guidance base, its own on a Laplacian base, a bad exponent, a bad eps; the coupling
//      bits (SC_ROBUST_ISOTROPIC, SC_ROBUST_JOINT_CHANNELS) change none of its verdicts and are refused by every other check;
//      sc_hip_volume_check: the same verdicts for two frames a frame's span apart, then frames, the plane limit, frame_stride and tau.
//      sc_hip_volume_wls_check: the volume call's verdicts under free and periodic time, then time_periodic, precond_smooth, precond_tau;
//      sc_hip_volume_flow_check beside it: the flow call takes the same parameters and gives the same verdicts.
//      sc_hip_region_robust_check: the robust call's verdicts (the region call's on a guidance base), the coupling bits accepted, then every
//      exponent, every eps, round_tol and tol.
//      sc_hip_bounded_check: the region call's verdicts under any valid pair of scalar bounds, then lower > upper and a NaN bound.
//      sc_hip_volume_robust_check: the WLS volume call's verdicts on a guidance base, then every exponent, every eps, round_tol, the coupling
//      bits, a Laplacian base and the WLS volume call's own refusals; sc_hip_volume_flow_robust_check and
//      sc_hip_volume_subflow_robust_check beside every one of these calls: the same parameters, the same verdicts.
//      sc_hip_volume_coupled_check: every legal coupling accepted, TIME alone and unknown bits refused, unequal p or eps under TIME
//      refused, the coupling bits in kind still refused; sc_hip_volume_flow_coupled_check beside every one of these calls: the same
//      parameters and coupling, the same verdicts.
//   8. sc_hip_fused_schedule: the schedule of a fused multigrid solve's level-0 launches over a few hundred facts and verdict lists.
//   9. sc_hip_restore_spans: a frame-only restore's byte spans applied to heap buffers of exactly the image's size.
//  10. a job's side arrays (SideArrays; sc_instance.h, sc_pcg.h): for_side_tables fills every family's table, 20 jobs as 16 + 4, each
//      slot with exactly its table's members of the matching record; float_intake pairs every array of a job it takes in with that job
//      and stores NULL for what the call does not carry.
//  11. sc_hip_pcg_plan: the work planes' tiling over a walk of sizes, borders and frame counts, its invariants, its refusals.
// Exit code 0 = clean (a sanitizer report aborts with its own).
#include "../../include/seamlessclone_hip_testing.h"
#include "sc_pcg.h"
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <thread>
#include <vector>

// ---- stub instances for the pool (sc_pool.cpp is compiled with -Dmy_seamlessclone_api_imp_create_instance=stub_create ...)
namespace {
struct StubInst { int gpu; std::atomic<long> calls{ 0 }; sc_solver_opts opts; int clone_mode = SC_NORMAL_CLONE; };
std::atomic<long> g_jobs_run{ 0 };
}
extern "C" {
void *stub_create(int gpu) { StubInst *s = new StubInst(); s->gpu = gpu; sc_hip_default_opts(&s->opts); return s; }
void stub_destroy(void *p) { delete (StubInst *)p; }
void stub_sync(void *) {}
int stub_set_solver(void *p, const sc_solver_opts *o) { ((StubInst *)p)->opts = *o; return SC_OK; }
int stub_get_solver(void *p, sc_solver_opts *o) { *o = ((StubInst *)p)->opts; return SC_OK; }
int stub_set_clone_mode(void *p, int mode)
{
    if (mode < SC_NORMAL_CLONE || mode > SC_MONOCHROME_TRANSFER) return SC_ERR_BAD_ARG;
    ((StubInst *)p)->clone_mode = mode;
    return SC_OK;
}
int stub_memcpy_d2d_async(void *, void *, const void *, size_t) { return SC_OK; }
int stub_run_device(void *p, const uint8_t *, int, int, int, uint8_t *body, int, int, int, const uint8_t *, int, int, int, int, int, bool)
{
    ((StubInst *)p)->calls++;
    g_jobs_run++;
    *(volatile uint8_t *)body += 1;          // every job owns its body byte: a job handed out twice shows as 2 (and as a race under TSan)
    return SC_OK;
}
int stub_run(void *p, const uint8_t *f, int fc, int fr, int fs, uint8_t *body, int bc, int br, int bs, const uint8_t *m, int mc, int mr, int ms, int cx, int cy, int, bool)
{
    return stub_run_device(p, f, fc, fr, fs, body, bc, br, bs, m, mc, mr, ms, cx, cy, false);
}
std::atomic<long> g_edit_mixed{ 0 };      // an edit chunk with more than one image size
int stub_edit_device(void *p, const sc_edit_params *, const uint8_t *, int, int, int, const uint8_t *, int, uint8_t *dst, int, bool)
{
    ((StubInst *)p)->calls++;
    g_jobs_run++;
    *(volatile uint8_t *)dst += 1;
    return SC_OK;
}
int stub_edit(void *p, const sc_edit_params *e, const uint8_t *s, int c, int r, int ss, const uint8_t *m, int ms, uint8_t *dst, int ds)
{
    return stub_edit_device(p, e, s, c, r, ss, m, ms, dst, ds, false);
}
constexpr int FAILING_COLS = 777;          // a chunk of this width: the batch call writes SC_OK into every member, then fails with a HIP error
int stub_edit_device_batch(void *p, const sc_edit_params *, sc_edit_job *jobs, int n)
{
    ((StubInst *)p)->calls++;
    for (int i = 0; i < n; ++i) {
        if (jobs[i].cols != jobs[0].cols || jobs[i].rows != jobs[0].rows) g_edit_mixed++;
        g_jobs_run++; *(volatile uint8_t *)jobs[i].dst += 1; jobs[i].rc = SC_OK;
    }
    return jobs[0].cols == FAILING_COLS ? SC_ERR_HIP : SC_OK;
}
int stub_run_device_batch(void *p, sc_batch_job *jobs, int n)
{
    ((StubInst *)p)->calls++;
    for (int i = 0; i < n; ++i) { g_jobs_run++; *(volatile uint8_t *)jobs[i].body += 1; jobs[i].rc = SC_OK; }
    return SC_OK;
}
}

// the compiler's registration hooks for device code: there is none in this build
extern "C" {
void **__hipRegisterFatBinary(const void *) { static void *h = nullptr; return &h; }
void __hipUnregisterFatBinary(void **) {}
void __hipRegisterFunction(void **, const void *, char *, const char *, unsigned, void *, void *, void *, void *, int *) {}
void __hipRegisterVar(void **, void *, char *, const char *, int, size_t, int, int) {}
void __hipRegisterManagedVar(void *, void *, void *, const char *, size_t, unsigned) {}
void __hipRegisterSurface(void **, void *, char *, char *, int, int) {}
void __hipRegisterTexture(void **, void *, char *, char *, int, int, int) {}
}

// 10: the pointer that stands for array `which` (0 .. 5: w, sx, sy, st, gt, smt; 6 ..: a PoissonJobDev's or a public job's others) of job k; never read
static const float *fake(int k, int which) { return (const float *)(uintptr_t)(0x10000 * (k + 1) + 0x100 * (which + 1)); }
// m jobs through Table's tables: the callback sees them in order, Table::MAX at a time; in every slot the job is job k's and each member
// the table has (members(t): its arrays in w, sx, sy, st, gt, smt order, nullptr for one it lacks) is record k's; the rest of a table is zeros
template <class Table, class Members> static bool tables_ok(const sc::PoissonJobDev *jobs, const sc::SideArrays *sides, int m, Members members)
{
    int calls = 0, seen = 0;
    bool ok = true;
    sc::for_side_tables<Table>(jobs, sides, m, [&](const Table &t, int i0, int cnt) {
        ok = ok && i0 == seen && cnt == std::min(m - i0, (int)Table::MAX);
        const auto mem = members(t);
        const float *const *const *has = mem.a;
        for (int i = 0; i < (int)Table::MAX; ++i) {
            const int k = i0 + i;
            const bool used = i < cnt;
            for (int a = 0; a < 6; ++a) ok = ok && (!has[a] || has[a][i] == (used ? fake(k, a) : nullptr));
            ok = ok && t.j[i].gx == (used ? fake(k, 6) : nullptr) && t.j[i].out == (used ? (float *)fake(k, 7) : nullptr) && t.j[i].d == (used ? fake(k, 8) : nullptr);
        }
        seen += cnt;
        ++calls;
    });
    return ok && seen == m && calls == (m + (int)Table::MAX - 1) / (int)Table::MAX;
}

static int fail(const char *what) { fprintf(stderr, "sanitize_main: %s\n", what); return 1; }

int main()
{
    // 1
    if (sc_hip_selftest_host() != 0) return fail("sc_hip_selftest_host");
    // 2: the planner, concurrently
    {
        const int N = 96, T = 6, ROUNDS = 40;
        std::vector<int> wh(2 * N);
        unsigned s = 12345u;
        auto rnd = [&](int lo, int hi) { s = s * 1664525u + 1013904223u; return lo + (int)((s >> 8) % (unsigned)(hi - lo + 1)); };
        for (int i = 0; i < N; ++i) { wh[2 * i] = rnd(90, 2300); wh[2 * i + 1] = rnd(90, 2300); }
        for (int i = 0; i < N; i += 3) { wh[2 * i] = 1000 + i; wh[2 * i + 1] = 1040 - i; }      // a size class among them
        std::vector<int> ref_g(N), ref_k(N);
        const int ref_n = sc_hip_plan_groups(wh.data(), N, 16, nullptr, ref_g.data(), ref_k.data());
        if (ref_n < 1) return fail("plan_groups");
        std::atomic<int> bad{ 0 };
        std::vector<std::thread> th;
        for (int t = 0; t < T; ++t)
            th.emplace_back([&, t]() {
                std::vector<int> g(N), k(N), other(2 * 700);
                unsigned q = 777u * (t + 1);
                for (int r = 0; r < ROUNDS; ++r) {
                    if (sc_hip_plan_groups(wh.data(), N, 16, nullptr, g.data(), k.data()) != ref_n || g != ref_g || k != ref_k) bad++;
                    for (int i = 0; i < 700; ++i) { q = q * 1664525u + 1013904223u; other[2 * i] = 100 + (int)((q >> 9) % 3000u); other[2 * i + 1] = 100 + (int)((q >> 3) % 3000u); }
                    std::vector<int> og(700);
                    if (sc_hip_plan_groups(other.data(), 700, 0, nullptr, og.data(), nullptr) < 1) bad++;      // misses, evictions
                    int out[12];
                    if (sc_hip_plan_size(1000 + r, 1000 + t, nullptr, out) != SC_OK) bad++;
                }
            });
        for (std::thread &x : th) x.join();
        if (bad.load()) return fail("the planner gave different answers under concurrency");
    }
    // 3: the pool's hand-out
    for (int streams : { 1, 3, 8 })
        for (int group : { 1, 4, 16 }) {
            void *pool = sc_hip_pool_create(0, streams);
            if (!pool) return fail("pool_create (stub instances)");
            if (sc_hip_pool_set_group(pool, group) != SC_OK) return fail("pool_set_group");
            if (sc_hip_pool_set_clone_mode(pool, 0) != SC_ERR_BAD_ARG) return fail("pool_set_clone_mode took mode 0");
            if (sc_hip_pool_set_clone_mode(pool, SC_MIXED_CLONE) != SC_OK) return fail("pool_set_clone_mode");
            for (int k = 0; k < sc_hip_pool_size(pool); ++k)
                if (((StubInst *)sc_hip_pool_instance(pool, k))->clone_mode != SC_MIXED_CLONE) return fail("pool_set_clone_mode missed an instance");
            for (int batch = 0; batch < 5; ++batch) {
                const int n = 1 + 37 * batch;
                std::vector<uint8_t> bodies(n, 0);
                std::vector<sc_batch_job> jobs(n);
                unsigned s = 99u + batch;
                for (int i = 0; i < n; ++i) {
                    memset(&jobs[i], 0, sizeof(jobs[i]));
                    s = s * 1664525u + 1013904223u;
                    const int w = (i % 5 == 0) ? 1002 : 1000 + (int)((s >> 10) % 90u), h = 1000 + (int)((s >> 17) % 90u);
                    jobs[i].face = jobs[i].mask = &bodies[i]; jobs[i].body = &bodies[i];
                    jobs[i].face_cols = jobs[i].mask_cols = w; jobs[i].face_rows = jobs[i].mask_rows = h;
                    jobs[i].face_step = 3 * w; jobs[i].mask_step = w; jobs[i].body_cols = 4000; jobs[i].body_rows = 4000; jobs[i].body_step = 12000;
                    jobs[i].centerX = jobs[i].centerY = 2000;
                    jobs[i].rc = -12345;
                }
                const long before = g_jobs_run.load();
                for (int device_resident : { 1, 0 }) {
                    if (sc_hip_pool_run(pool, jobs.data(), n, device_resident) != SC_OK) return fail("pool_run");
                    for (int i = 0; i < n; ++i) if (jobs[i].rc != SC_OK) return fail("a job's code was not copied back");
                }
                if (g_jobs_run.load() - before != 2L * n) return fail("jobs run != jobs given");
                for (int i = 0; i < n; ++i) if (bodies[i] != 2) return fail("a job was handed out twice or never");
            }
            sc_hip_pool_destroy(pool);
        }
    // 4: edit batches through the pool
    for (int streams : { 1, 3 })
        for (int group : { 1, 4, SC_POOL_GROUP_AUTO }) {
            void *pool = sc_hip_pool_create(0, streams);
            if (!pool) return fail("pool_create (stub instances)");
            if (sc_hip_pool_set_group(pool, group) != SC_OK) return fail("pool_set_group");
            sc_edit_params ep;
            sc_hip_default_edit_params(&ep, SC_EDIT_COLOR_CHANGE);
            for (int batch = 0; batch < 4; ++batch) {
                const int n = 1 + 29 * batch;
                std::vector<uint8_t> dsts(n, 0);
                std::vector<sc_edit_job> jobs(n);
                std::vector<int> wh(2 * n), group_of(n);
                for (int i = 0; i < n; ++i) {
                    memset(&jobs[i], 0, sizeof(jobs[i]));
                    const int w = (i % 3 == 0) ? 640 : (i % 7 == 0) ? 1000 + i : 320, h = (i % 3 == 0) ? 360 : 200;
                    jobs[i].src = jobs[i].mask = &dsts[i]; jobs[i].dst = &dsts[i];
                    jobs[i].cols = w; jobs[i].rows = h; jobs[i].src_step = jobs[i].dst_step = 3 * w; jobs[i].mask_step = w;
                    jobs[i].rc = -12345;
                    wh[2 * i] = w; wh[2 * i + 1] = h;
                }
                const int chunks = sc_hip_plan_edit_groups_pool(wh.data(), n, group, streams, group_of.data());
                if (chunks < 1 || chunks > n) return fail("plan_edit_groups_pool");
                for (int i = 0; i < n; ++i)
                    for (int k = 0; k < n; ++k)
                        if (group_of[i] == group_of[k] && (wh[2 * i] != wh[2 * k] || wh[2 * i + 1] != wh[2 * k + 1])) return fail("an edit chunk mixes sizes");
                const long before = g_jobs_run.load();
                for (int device_resident : { 1, 0 }) {
                    if (sc_hip_pool_edit(pool, &ep, jobs.data(), n, device_resident) != SC_OK) return fail("pool_edit");
                    for (int i = 0; i < n; ++i) if (jobs[i].rc != SC_OK) return fail("an edit job's code was not copied back");
                }
                if (g_jobs_run.load() - before != 2L * n) return fail("edit jobs run != jobs given");
                for (int i = 0; i < n; ++i) if (dsts[i] != 2) return fail("an edit job was handed out twice or never");
            }
            sc_hip_pool_destroy(pool);
        }
    if (g_edit_mixed.load()) return fail("the pool handed one edit batch call several image sizes");
    // 4b: a batch call that fails with a HIP error after its members' codes read SC_OK
    {
        void *pool = sc_hip_pool_create(0, 2);
        if (!pool) return fail("pool_create (stub instances)");
        if (sc_hip_pool_set_group(pool, 4) != SC_OK) return fail("pool_set_group");
        sc_edit_params ep;
        sc_hip_default_edit_params(&ep, SC_EDIT_COLOR_CHANGE);
        const int n = 11;
        std::vector<uint8_t> dsts(n, 0);
        std::vector<sc_edit_job> jobs(n);
        for (int i = 0; i < n; ++i) {
            memset(&jobs[i], 0, sizeof(jobs[i]));
            const int w = (i % 3 == 0) ? FAILING_COLS : 320;
            jobs[i].src = jobs[i].mask = &dsts[i]; jobs[i].dst = &dsts[i];
            jobs[i].cols = w; jobs[i].rows = 200; jobs[i].src_step = jobs[i].dst_step = 3 * w; jobs[i].mask_step = w;
            jobs[i].rc = -12345;
        }
        if (sc_hip_pool_edit(pool, &ep, jobs.data(), n, 1) != SC_ERR_HIP) return fail("pool_edit hid a failed batch call");
        for (int i = 0; i < n; ++i)
            if (jobs[i].rc != (jobs[i].cols == FAILING_COLS ? SC_ERR_HIP : SC_OK)) return fail("a job of a failed batch call reads as done");
        sc_hip_pool_destroy(pool);
    }
    // 5: the Poisson call's validation
    {
        struct Case { int kind; float tol; int w, h, c; long long cs, rs, chs; int want; };
        const long long big = 1LL << 62;
        const Case cases[] = {
            { SC_POISSON_GUIDANCE, 0.f, 640, 480, 3, 3, 3 * 640, 1, SC_OK },                 // HWC
            { SC_POISSON_LAPLACIAN, 1e-2f, 640, 480, 3, 1, 640, 640 * 480, SC_OK },          // CHW
            { SC_POISSON_GUIDANCE, 0.f, 640, 480, 3, 4, 4 * 640, 1, SC_OK },                 // RGBA-strided C = 3
            { SC_POISSON_GUIDANCE, 0.f, 33, 7, 1, 1, 40, 1, SC_OK },                         // padded rows, C = 1 (channel stride free)
            { SC_POISSON_GUIDANCE, 0.f, 640, 480, 3, 2, 3 * 640, 1, SC_ERR_BAD_ARG },        // x and c overlap
            { SC_POISSON_GUIDANCE, 0.f, 640, 480, 3, 1, 640, 640, SC_ERR_BAD_ARG },          // rows and planes overlap
            { SC_POISSON_GUIDANCE, 0.f, 640, 480, 3, 3, 0, 1, SC_ERR_BAD_ARG },
            { SC_POISSON_GUIDANCE, 0.f, 640, 480, 0, 3, 3 * 640, 1, SC_ERR_BAD_ARG },
            { SC_POISSON_GUIDANCE, 0.f, 640, 480, 5, 5, 5 * 640, 1, SC_ERR_BAD_ARG },
            { SC_POISSON_GUIDANCE, 0.f, 2, 480, 3, 3, 6, 1, SC_ERR_BAD_SIZE },
            { 3, 0.f, 640, 480, 3, 3, 3 * 640, 1, SC_ERR_BAD_ARG },
            { SC_POISSON_GUIDANCE, NAN, 640, 480, 3, 3, 3 * 640, 1, SC_ERR_BAD_ARG },
            { SC_POISSON_GUIDANCE, 0.f, 65536, 65536, 4, big / 4, big / 2, 1, SC_ERR_BAD_ARG },   // spans beyond 2^60 floats
            { SC_POISSON_GUIDANCE, 0.f, 640, 480, 4, big, big, big, SC_ERR_BAD_ARG },
            // SC_POISSON_NEUMANN: 2 x 2 up to 8192 per side, a base kind required
            { SC_POISSON_GUIDANCE | SC_POISSON_NEUMANN, 0.f, 2, 2, 1, 1, 2, 4, SC_OK },
            { SC_POISSON_LAPLACIAN | SC_POISSON_NEUMANN, 0.f, 8192, 8, 3, 3, 3 * 8192, 1, SC_OK },
            { SC_POISSON_GUIDANCE | SC_POISSON_NEUMANN, 0.f, 1, 40, 1, 1, 1, 40, SC_ERR_BAD_SIZE },
            { SC_POISSON_LAPLACIAN | SC_POISSON_NEUMANN, 0.f, 40, 1, 1, 1, 40, 40, SC_ERR_BAD_SIZE },
            { SC_POISSON_GUIDANCE | SC_POISSON_NEUMANN, 0.f, 8193, 8, 1, 1, 8193, 8 * 8193, SC_ERR_BAD_SIZE },
            { SC_POISSON_GUIDANCE | SC_POISSON_NEUMANN, 0.f, 8, 8193, 1, 1, 8, 8 * 8193, SC_ERR_BAD_SIZE },
            { SC_POISSON_NEUMANN, 0.f, 640, 480, 1, 1, 640, 640 * 480, SC_ERR_BAD_ARG },
            { SC_POISSON_NEUMANN | 3, 0.f, 640, 480, 1, 1, 640, 640 * 480, SC_ERR_BAD_ARG },
            { (1 << 9) | SC_POISSON_GUIDANCE, 0.f, 640, 480, 1, 1, 640, 640 * 480, SC_ERR_BAD_ARG },
            // SC_POISSON_FREE_*: any combination on a base kind; per axis 1 .. 8192 unknowns = pixels less its Dirichlet lines
            { SC_POISSON_GUIDANCE | SC_POISSON_FREE_LEFT, 0.f, 640, 480, 3, 3, 3 * 640, 1, SC_OK },
            { SC_POISSON_LAPLACIAN | SC_POISSON_FREE_TOP | SC_POISSON_FREE_BOTTOM, 0.f, 640, 480, 3, 1, 640, 640 * 480, SC_OK },
            { SC_POISSON_GUIDANCE | SC_POISSON_FREE_LEFT | SC_POISSON_FREE_RIGHT | SC_POISSON_FREE_TOP, 0.f, 2, 2, 1, 1, 2, 4, SC_OK },
            { SC_POISSON_GUIDANCE | SC_POISSON_FREE_LEFT | SC_POISSON_FREE_RIGHT | SC_POISSON_FREE_TOP | SC_POISSON_FREE_BOTTOM, 0.f, 2, 2, 1, 1, 2, 4, SC_OK },
            { SC_POISSON_GUIDANCE | SC_POISSON_NEUMANN | SC_POISSON_FREE_LEFT, 0.f, 2, 2, 1, 1, 2, 4, SC_OK },      // the union: all four
            { SC_POISSON_GUIDANCE | SC_POISSON_FREE_RIGHT, 0.f, 2, 3, 1, 1, 2, 6, SC_OK },                           // 1 x 1 unknowns
            { SC_POISSON_GUIDANCE | SC_POISSON_FREE_RIGHT, 0.f, 2, 2, 1, 1, 2, 4, SC_ERR_BAD_SIZE },                 // no unknown between top and bottom
            { SC_POISSON_GUIDANCE | SC_POISSON_FREE_TOP, 0.f, 2, 8, 1, 1, 2, 16, SC_ERR_BAD_SIZE },                  // none between left and right
            { SC_POISSON_GUIDANCE | SC_POISSON_FREE_TOP, 0.f, 8, 1, 1, 1, 8, 8, SC_ERR_BAD_SIZE },
            { SC_POISSON_GUIDANCE | SC_POISSON_FREE_LEFT, 0.f, 8193, 8, 1, 1, 8193, 8 * 8193, SC_OK },               // 8192 unknowns beside one Dirichlet line
            { SC_POISSON_GUIDANCE | SC_POISSON_FREE_LEFT, 0.f, 8194, 8, 1, 1, 8194, 8 * 8194, SC_ERR_BAD_SIZE },
            { SC_POISSON_GUIDANCE | SC_POISSON_FREE_LEFT, 0.f, 8, 8194, 1, 1, 8, 8 * 8194, SC_OK },                  // ... between two
            { SC_POISSON_GUIDANCE | SC_POISSON_FREE_LEFT, 0.f, 8, 8195, 1, 1, 8, 8 * 8195, SC_ERR_BAD_SIZE },
            { SC_POISSON_LAPLACIAN | SC_POISSON_FREE_LEFT | SC_POISSON_FREE_RIGHT, 0.f, 8192, 8, 1, 1, 8192, 8 * 8192, SC_OK },   // ... beside none
            { SC_POISSON_LAPLACIAN | SC_POISSON_FREE_LEFT | SC_POISSON_FREE_RIGHT, 0.f, 8193, 8, 1, 1, 8193, 8 * 8193, SC_ERR_BAD_SIZE },
            { SC_POISSON_FREE_LEFT, 0.f, 640, 480, 1, 1, 640, 640 * 480, SC_ERR_BAD_ARG },                           // no base kind
            { SC_POISSON_FREE_LEFT | 3, 0.f, 640, 480, 1, 1, 640, 640 * 480, SC_ERR_BAD_ARG },
            { (1 << 9) | SC_POISSON_GUIDANCE | SC_POISSON_FREE_LEFT, 0.f, 640, 480, 1, 1, 640, 640 * 480, SC_ERR_BAD_ARG },
            { (1 << 11) | SC_POISSON_GUIDANCE, 0.f, 640, 480, 1, 1, 640, 640 * 480, SC_ERR_BAD_ARG },
            { (1 << 16) | SC_POISSON_GUIDANCE, 0.f, 640, 480, 1, 1, 640, 640 * 480, SC_ERR_BAD_ARG },
            // SC_POISSON_PERIODIC_*: 2 .. 8192 pixels along a periodic axis, the other axis under its own rules; no free side on a periodic
            // axis, no SC_POISSON_NEUMANN, a base kind required
            { SC_POISSON_GUIDANCE | SC_POISSON_PERIODIC_X, 0.f, 640, 480, 3, 3, 3 * 640, 1, SC_OK },
            { SC_POISSON_LAPLACIAN | SC_POISSON_PERIODIC_Y, 0.f, 640, 480, 3, 1, 640, 640 * 480, SC_OK },
            { SC_POISSON_GUIDANCE | SC_POISSON_PERIODIC_X | SC_POISSON_PERIODIC_Y, 0.f, 2, 2, 1, 1, 2, 4, SC_OK },
            { SC_POISSON_GUIDANCE | SC_POISSON_PERIODIC_X | SC_POISSON_FREE_TOP | SC_POISSON_FREE_BOTTOM, 0.f, 2, 2, 1, 1, 2, 4, SC_OK },
            { SC_POISSON_GUIDANCE | SC_POISSON_PERIODIC_Y | SC_POISSON_FREE_LEFT, 0.f, 2, 2, 1, 1, 2, 4, SC_OK },
            { SC_POISSON_GUIDANCE | SC_POISSON_PERIODIC_X, 0.f, 2, 3, 1, 1, 2, 6, SC_OK },                               // 2 x 1 unknowns
            { SC_POISSON_GUIDANCE | SC_POISSON_PERIODIC_X, 0.f, 2, 2, 1, 1, 2, 4, SC_ERR_BAD_SIZE },                     // no unknown between top and bottom
            { SC_POISSON_GUIDANCE | SC_POISSON_PERIODIC_X, 0.f, 1, 40, 1, 1, 1, 40, SC_ERR_BAD_SIZE },                   // length 1
            { SC_POISSON_LAPLACIAN | SC_POISSON_PERIODIC_Y, 0.f, 40, 1, 1, 1, 40, 40, SC_ERR_BAD_SIZE },
            { SC_POISSON_GUIDANCE | SC_POISSON_PERIODIC_X | SC_POISSON_PERIODIC_Y, 0.f, 1, 1, 1, 1, 1, 1, SC_ERR_BAD_SIZE },
            { SC_POISSON_GUIDANCE | SC_POISSON_PERIODIC_X, 0.f, 8192, 8, 1, 1, 8192, 8 * 8192, SC_OK },
            { SC_POISSON_GUIDANCE | SC_POISSON_PERIODIC_X, 0.f, 8193, 8, 1, 1, 8193, 8 * 8193, SC_ERR_BAD_SIZE },
            { SC_POISSON_GUIDANCE | SC_POISSON_PERIODIC_Y, 0.f, 8, 8192, 1, 1, 8, 8 * 8192, SC_OK },
            { SC_POISSON_GUIDANCE | SC_POISSON_PERIODIC_Y, 0.f, 8, 8193, 1, 1, 8, 8 * 8193, SC_ERR_BAD_SIZE },
            { SC_POISSON_GUIDANCE | SC_POISSON_PERIODIC_X, 0.f, 8, 8194, 1, 1, 8, 8 * 8194, SC_OK },                     // the other axis between two Dirichlet lines
            { SC_POISSON_GUIDANCE | SC_POISSON_PERIODIC_X, 0.f, 8, 8195, 1, 1, 8, 8 * 8195, SC_ERR_BAD_SIZE },
            { SC_POISSON_GUIDANCE | SC_POISSON_PERIODIC_X | SC_POISSON_FREE_LEFT, 0.f, 640, 480, 1, 1, 640, 640 * 480, SC_ERR_BAD_ARG },
            { SC_POISSON_GUIDANCE | SC_POISSON_PERIODIC_X | SC_POISSON_FREE_RIGHT, 0.f, 640, 480, 1, 1, 640, 640 * 480, SC_ERR_BAD_ARG },
            { SC_POISSON_GUIDANCE | SC_POISSON_PERIODIC_Y | SC_POISSON_FREE_TOP, 0.f, 640, 480, 1, 1, 640, 640 * 480, SC_ERR_BAD_ARG },
            { SC_POISSON_GUIDANCE | SC_POISSON_PERIODIC_Y | SC_POISSON_FREE_BOTTOM, 0.f, 640, 480, 1, 1, 640, 640 * 480, SC_ERR_BAD_ARG },
            { SC_POISSON_GUIDANCE | SC_POISSON_PERIODIC_X | SC_POISSON_NEUMANN, 0.f, 640, 480, 1, 1, 640, 640 * 480, SC_ERR_BAD_ARG },
            { SC_POISSON_LAPLACIAN | SC_POISSON_PERIODIC_Y | SC_POISSON_NEUMANN, 0.f, 640, 480, 1, 1, 640, 640 * 480, SC_ERR_BAD_ARG },
            { SC_POISSON_PERIODIC_X, 0.f, 640, 480, 1, 1, 640, 640 * 480, SC_ERR_BAD_ARG },                             // no base kind
            { SC_POISSON_PERIODIC_X | SC_POISSON_PERIODIC_Y | 3, 0.f, 640, 480, 1, 1, 640, 640 * 480, SC_ERR_BAD_ARG },
            { (1 << 16) | SC_POISSON_GUIDANCE | SC_POISSON_PERIODIC_X, 0.f, 640, 480, 1, 1, 640, 640 * 480, SC_ERR_BAD_ARG },
            { (1 << 19) | SC_POISSON_GUIDANCE | SC_POISSON_PERIODIC_Y, 0.f, 640, 480, 1, 1, 640, 640 * 480, SC_ERR_BAD_ARG },
        };
        for (const Case &k : cases) {
            sc_poisson_params p{ k.kind, k.tol };
            sc_poisson_layout l{ k.w, k.h, k.c, k.cs, k.rs, k.chs };
            if (sc_hip_poisson_check(&p, &l) != k.want) return fail("poisson_check");
        }
        sc_poisson_params p{ SC_POISSON_GUIDANCE, 0.f };
        if (sc_hip_poisson_check(nullptr, nullptr) != SC_ERR_BAD_ARG || sc_hip_poisson_check(&p, nullptr) != SC_ERR_BAD_ARG) return fail("poisson_check (null)");
    }
    // 6: the screened call's validation (lambda, the kinds, the direct solves' side limits of each boundary kind)
    {
        struct Case { int kind; float lambda; int w, h, c; long long cs, rs, chs; int want; };
        const float nan = std::nanf(""), inf = HUGE_VALF;
        const int N = SC_POISSON_NEUMANN, G = SC_POISSON_GUIDANCE, Lp = SC_POISSON_LAPLACIAN;
        const Case cases[] = {
            { G, 0.5f, 640, 480, 3, 3, 1920, 1, SC_OK },
            { Lp | N, 1e-3f, 640, 480, 3, 1, 640, 640 * 480, SC_OK },
            { G, 0.f, 640, 480, 3, 3, 1920, 1, SC_ERR_BAD_ARG },
            { G | N, -1.f, 640, 480, 3, 3, 1920, 1, SC_ERR_BAD_ARG },
            { G, nan, 640, 480, 3, 3, 1920, 1, SC_ERR_BAD_ARG },
            { Lp, inf, 640, 480, 3, 3, 1920, 1, SC_ERR_BAD_ARG },
            { 0, 1.f, 640, 480, 3, 3, 1920, 1, SC_ERR_BAD_ARG },
            { N, 1.f, 640, 480, 3, 3, 1920, 1, SC_ERR_BAD_ARG },
            { G, 1.f, 640, 480, 3, 2, 1920, 1, SC_ERR_BAD_ARG },          // x and c overlap
            { G | N, 1.f, 2, 2, 1, 1, 2, 4, SC_OK },
            { G | N, 1.f, 8192, 2, 1, 1, 8192, 16384, SC_OK },
            { G | N, 1.f, 8193, 2, 1, 1, 8193, 16386, SC_ERR_BAD_SIZE },
            { G, 1.f, 2, 8, 1, 1, 2, 16, SC_ERR_BAD_SIZE },
            { G, 1.f, 3, 3, 1, 1, 3, 9, SC_OK },
            { G, 1.f, 8194, 3, 1, 1, 8194, 3 * 8194, SC_OK },               // 8192 unknowns per side
            { Lp, 1.f, 3, 8195, 1, 1, 3, 3 * 8195, SC_ERR_BAD_SIZE },
            // SC_POISSON_FREE_*
            { G | SC_POISSON_FREE_LEFT, 1.f, 640, 480, 3, 3, 1920, 1, SC_OK },
            { Lp | SC_POISSON_FREE_TOP | SC_POISSON_FREE_RIGHT, 1e-3f, 2, 2, 1, 1, 2, 4, SC_OK },
            { G | SC_POISSON_FREE_LEFT | SC_POISSON_FREE_RIGHT | SC_POISSON_FREE_TOP | SC_POISSON_FREE_BOTTOM, 1.f, 2, 2, 1, 1, 2, 4, SC_OK },
            { G | SC_POISSON_FREE_BOTTOM, 1.f, 3, 8193, 1, 1, 3, 3 * 8193, SC_OK },
            { G | SC_POISSON_FREE_BOTTOM, 1.f, 3, 8194, 1, 1, 3, 3 * 8194, SC_ERR_BAD_SIZE },
            { G | SC_POISSON_FREE_BOTTOM, 1.f, 2, 8, 1, 1, 2, 16, SC_ERR_BAD_SIZE },
            { G | SC_POISSON_FREE_BOTTOM, 0.f, 640, 480, 3, 3, 1920, 1, SC_ERR_BAD_ARG },
            { (1 << 9) | G | SC_POISSON_FREE_BOTTOM, 1.f, 640, 480, 3, 3, 1920, 1, SC_ERR_BAD_ARG },
            // SC_POISSON_PERIODIC_*
            { G | SC_POISSON_PERIODIC_X, 1.f, 640, 480, 3, 3, 1920, 1, SC_OK },
            { Lp | SC_POISSON_PERIODIC_X | SC_POISSON_PERIODIC_Y, 1e-3f, 2, 2, 1, 1, 2, 4, SC_OK },
            { G | SC_POISSON_PERIODIC_Y | SC_POISSON_FREE_LEFT | SC_POISSON_FREE_RIGHT, 1.f, 2, 2, 1, 1, 2, 4, SC_OK },
            { G | SC_POISSON_PERIODIC_Y, 1.f, 3, 8192, 1, 1, 3, 3 * 8192, SC_OK },
            { G | SC_POISSON_PERIODIC_Y, 1.f, 3, 8193, 1, 1, 3, 3 * 8193, SC_ERR_BAD_SIZE },
            { G | SC_POISSON_PERIODIC_Y, 1.f, 3, 1, 1, 1, 3, 3, SC_ERR_BAD_SIZE },
            { G | SC_POISSON_PERIODIC_X, 1.f, 1, 8, 1, 1, 1, 8, SC_ERR_BAD_SIZE },
            { G | SC_POISSON_PERIODIC_X | SC_POISSON_FREE_RIGHT, 1.f, 640, 480, 3, 3, 1920, 1, SC_ERR_BAD_ARG },
            { G | SC_POISSON_PERIODIC_Y | SC_POISSON_FREE_TOP, 1.f, 640, 480, 3, 3, 1920, 1, SC_ERR_BAD_ARG },
            { G | SC_POISSON_PERIODIC_X | N, 1.f, 640, 480, 3, 3, 1920, 1, SC_ERR_BAD_ARG },
            { SC_POISSON_PERIODIC_X, 1.f, 640, 480, 3, 3, 1920, 1, SC_ERR_BAD_ARG },
            { G | SC_POISSON_PERIODIC_X, 0.f, 640, 480, 3, 3, 1920, 1, SC_ERR_BAD_ARG },
            { (1 << 16) | G | SC_POISSON_PERIODIC_X, 1.f, 640, 480, 3, 3, 1920, 1, SC_ERR_BAD_ARG },
        };
        for (const Case &k : cases) {
            sc_screened_params p{ k.kind, k.lambda };
            sc_poisson_layout l{ k.w, k.h, k.c, k.cs, k.rs, k.chs };
            if (sc_hip_screened_check(&p, &l) != k.want) return fail("screened_check");
        }
        sc_screened_params p{ SC_POISSON_GUIDANCE, 1.f };
        if (sc_hip_screened_check(nullptr, nullptr) != SC_ERR_BAD_ARG || sc_hip_screened_check(&p, nullptr) != SC_ERR_BAD_ARG) return fail("screened_check (null)");
    }
    // 7: the weighted call's validation
    {
        struct Case { int kind; float tol; int iters; float plam; int w, h, c; long long cs, rs, chs; int want; };
        const float nan = std::nanf(""), inf = HUGE_VALF;
        const int G = SC_POISSON_GUIDANCE, Lp = SC_POISSON_LAPLACIAN, N = SC_POISSON_NEUMANN;
        const Case cases[] = {
            { G, 0.f, 0, 0.f, 640, 480, 3, 3, 1920, 1, SC_OK },
            { Lp | N, 1e-6f, 50, 0.5f, 640, 480, 3, 3, 1920, 1, SC_OK },
            { Lp | N, -1.f, -5, -1.f, 2, 2, 1, 1, 2, 4, SC_OK },
            { Lp | SC_POISSON_PERIODIC_X | SC_POISSON_PERIODIC_Y, 0.f, 0, 0.f, 2, 2, 4, 4, 8, 1, SC_OK },
            { Lp | SC_POISSON_FREE_LEFT | SC_POISSON_FREE_TOP, 0.f, 0, 0.f, 2, 2, 1, 1, 2, 4, SC_OK },
            { Lp | N, nan, 0, 0.f, 640, 480, 3, 3, 1920, 1, SC_ERR_BAD_ARG },
            { Lp | N, inf, 0, 0.f, 640, 480, 3, 3, 1920, 1, SC_ERR_BAD_ARG },
            { Lp | N, 0.f, 0, nan, 640, 480, 3, 3, 1920, 1, SC_ERR_BAD_ARG },
            { Lp | N, 0.f, 0, -inf, 640, 480, 3, 3, 1920, 1, SC_ERR_BAD_ARG },
            { 0, 0.f, 0, 0.f, 640, 480, 3, 3, 1920, 1, SC_ERR_BAD_ARG },
            { Lp | N | SC_POISSON_PERIODIC_X, 0.f, 0, 0.f, 640, 480, 3, 3, 1920, 1, SC_ERR_BAD_ARG },
            { Lp | SC_POISSON_PERIODIC_Y | SC_POISSON_FREE_TOP, 0.f, 0, 0.f, 640, 480, 3, 3, 1920, 1, SC_ERR_BAD_ARG },
            { Lp, 0.f, 0, 0.f, 2, 7, 1, 1, 2, 14, SC_ERR_BAD_SIZE },
            { Lp, 0.f, 0, 0.f, 8194, 3, 1, 1, 8194, 24582, SC_OK },
            { Lp, 0.f, 0, 0.f, 8195, 3, 1, 1, 8195, 24585, SC_ERR_BAD_SIZE },
            { Lp | N, 0.f, 0, 0.f, 8193, 2, 1, 1, 8193, 16386, SC_ERR_BAD_SIZE },
            { Lp | N, 0.f, 0, 0.f, 640, 480, 3, 3, 1919, 1, SC_ERR_BAD_ARG },
            { Lp | N, 0.f, 0, 0.f, 640, 480, 5, 5, 3200, 1, SC_ERR_BAD_ARG },
            { Lp | N, 0.f, 0, 0.f, 640, 480, 3, 1LL << 58, 1LL << 59, 1, SC_ERR_BAD_ARG },
        };
        for (const Case &k : cases) {
            sc_weighted_params p{ k.kind, k.tol, k.iters, k.plam };
            sc_poisson_layout l{ k.w, k.h, k.c, k.cs, k.rs, k.chs };
            if (sc_hip_weighted_check(&p, &l) != k.want) return fail("weighted_check");
            sc_wls_params q{ k.kind, k.tol, k.iters, k.plam, 0.f };
            if (sc_hip_wls_check(&q, &l) != k.want) return fail("wls_check");
            q.precond_smooth = k.plam;          // (the same values make the same verdicts)
            if (sc_hip_wls_check(&q, &l) != k.want) return fail("wls_check (precond_smooth)");
            sc_region_params rg{ k.kind, k.tol, k.iters, k.plam, 0.f };          // the region call: the WLS call's verdicts
            if (sc_hip_region_check(&rg, &l) != k.want) return fail("region_check");
            rg.precond_smooth = k.plam;
            if (sc_hip_region_check(&rg, &l) != k.want) return fail("region_check (precond_smooth)");
            // the bounded call: the region call's verdicts whatever valid bounds it carries, then its own refusals of the scalars
            struct Pair { float lo, hi; };
            for (const Pair b : { Pair{ -inf, inf }, Pair{ 0.f, 1.f }, Pair{ 0.25f, 0.25f }, Pair{ -inf, 0.f } }) {
                sc_bounded_params bp{ k.kind, k.tol, k.iters, k.plam, 0.f, b.lo, b.hi, 7 };
                if (sc_hip_bounded_check(&bp, &l) != k.want) return fail("bounded_check");
            }
            if (k.want == SC_OK) {
                for (const Pair b : { Pair{ 1.f, 0.f }, Pair{ nan, 1.f }, Pair{ 0.f, nan }, Pair{ inf, -inf } }) {
                    sc_bounded_params bp{ k.kind, k.tol, k.iters, k.plam, 0.f, b.lo, b.hi, 0 };
                    if (sc_hip_bounded_check(&bp, &l) != SC_ERR_BAD_ARG) return fail("bounded_check (bounds)");
                }
                sc_bounded_params bp{ k.kind, k.tol, k.iters, k.plam, 0.f, 0.f, 1.f, 0 };
                if (sc_hip_bounded_check(nullptr, &l) != SC_ERR_BAD_ARG || sc_hip_bounded_check(&bp, nullptr) != SC_ERR_BAD_ARG) return fail("bounded_check (null)");
            }
            // the volume call: the region call's verdicts for two frames a frame's span apart, then its own refusals
            const long long span = k.want == SC_OK ? (k.w - 1) * k.cs + (k.h - 1) * k.rs + (k.c - 1) * k.chs + 1 : 1LL << 40;
            sc_volume_params vp{ k.kind, 2, span, 1.f, k.tol, k.iters, k.plam };
            if (sc_hip_volume_check(&vp, &l) != k.want) return fail("volume_check");
            vp.kind = k.kind | SC_ROBUST_ISOTROPIC;
            if (sc_hip_volume_check(&vp, &l) != SC_ERR_BAD_ARG) return fail("volume_check (coupling bits)");
            vp.kind = k.kind;
            if (k.want == SC_OK) {
                vp.frames = 1;
                if (sc_hip_volume_check(&vp, &l) != SC_ERR_BAD_ARG) return fail("volume_check (frames < 2)");
                vp.frames = SC_POISSON_MAX_PLANES / k.c;
                if (sc_hip_volume_check(&vp, &l) != SC_OK) return fail("volume_check (the plane limit)");
                vp.frames = SC_POISSON_MAX_PLANES / k.c + 1;
                if (sc_hip_volume_check(&vp, &l) != SC_ERR_BAD_SIZE) return fail("volume_check (beyond the plane limit)");
                vp.frames = 2; vp.frame_stride = span - 1;
                if (sc_hip_volume_check(&vp, &l) != SC_ERR_BAD_ARG) return fail("volume_check (frame_stride)");
                vp.frame_stride = span;
                for (float tau : { 0.f, -1.f, nan, inf }) {
                    vp.tau = tau;
                    if (sc_hip_volume_check(&vp, &l) != SC_ERR_BAD_ARG) return fail("volume_check (tau)");
                }
            }
            // the WLS volume call: the volume call's verdicts on the same cases under either kind of time, then its own refusals
            for (int tp = 0; tp < 2; ++tp) {
                const int fr = tp ? 3 : 2;
                sc_volume_wls_params wp{ k.kind, fr, span, 1.f, tp, k.tol, k.iters, k.plam, 0.f, 0.f };
                if (sc_hip_volume_wls_check(&wp, &l) != k.want) return fail("volume_wls_check");
                if (sc_hip_volume_flow_check(&wp, &l) != k.want) return fail("volume_flow_check");          // (the same parameters, the same verdicts)
                wp.precond_smooth = wp.precond_tau = k.plam;          // (the same values make the same verdicts)
                if (sc_hip_volume_wls_check(&wp, &l) != k.want) return fail("volume_wls_check (precond_smooth, precond_tau)");
                wp.precond_smooth = wp.precond_tau = 0.f;
                wp.kind = k.kind | SC_ROBUST_ISOTROPIC;
                if (sc_hip_volume_wls_check(&wp, &l) != SC_ERR_BAD_ARG) return fail("volume_wls_check (coupling bits)");
                wp.kind = k.kind;
                if (k.want != SC_OK) continue;
                wp.frames = tp ? 2 : 1;
                if (sc_hip_volume_wls_check(&wp, &l) != SC_ERR_BAD_ARG) return fail("volume_wls_check (too few frames)");
                wp.frames = SC_POISSON_MAX_PLANES / k.c;
                if (sc_hip_volume_wls_check(&wp, &l) != SC_OK) return fail("volume_wls_check (the plane limit)");
                wp.frames = SC_POISSON_MAX_PLANES / k.c + 1;
                if (sc_hip_volume_wls_check(&wp, &l) != SC_ERR_BAD_SIZE) return fail("volume_wls_check (beyond the plane limit)");
                wp.frames = fr; wp.frame_stride = span - 1;
                if (sc_hip_volume_wls_check(&wp, &l) != SC_ERR_BAD_ARG) return fail("volume_wls_check (frame_stride)");
                wp.frame_stride = span;
                for (float tau : { 0.f, -1.f, nan, inf }) {
                    wp.tau = tau;
                    if (sc_hip_volume_wls_check(&wp, &l) != SC_ERR_BAD_ARG) return fail("volume_wls_check (tau)");
                }
                wp.tau = 1.f;
                for (float v : { nan, inf, -inf }) {
                    wp.precond_smooth = v;
                    if (sc_hip_volume_wls_check(&wp, &l) != SC_ERR_BAD_ARG) return fail("volume_wls_check (precond_smooth)");
                    wp.precond_smooth = 0.f; wp.precond_tau = v;
                    if (sc_hip_volume_wls_check(&wp, &l) != SC_ERR_BAD_ARG) return fail("volume_wls_check (precond_tau)");
                    wp.precond_tau = 0.f;
                }
                for (int bad : { 2, -1 }) {
                    wp.time_periodic = bad;
                    if (sc_hip_volume_wls_check(&wp, &l) != SC_ERR_BAD_ARG) return fail("volume_wls_check (time_periodic)");
                }
            }
            const bool lap_base = (k.kind & 3) == SC_POISSON_LAPLACIAN;
            // the robust volume call: the WLS volume call's verdict on a guidance base under either kind of time, a refusal on a Laplacian
            // one; then the robust call's refusals -- every exponent, every eps, round_tol --, the coupling bits and the WLS volume call's own
            for (int tp = 0; tp < 2; ++tp) {
                const int fr = tp ? 3 : 2;
                const sc_volume_robust_params good{ k.kind, fr, span, 1.f, tp, 1.f, 1e-3f, 1.f, 1e-3f, 2.f, 0.f, 0, 0.f, k.tol, k.iters };
                sc_volume_robust_params vr = good;
                // sc_hip_volume_flow_robust_check and sc_hip_volume_subflow_robust_check beside every call: the same parameters, the same
                // verdicts (these sizes lie far below the links' 32-bit limit); a verdict that differs is no code at all
                auto robust_checks = [](const sc_volume_robust_params *vp, const sc_poisson_layout *vl) {
                    const int v = sc_hip_volume_robust_check(vp, vl);
                    return sc_hip_volume_flow_robust_check(vp, vl) == v && sc_hip_volume_subflow_robust_check(vp, vl) == v ? v : -1000;
                };
                const int verdict = robust_checks(&vr, &l);
                if (lap_base ? verdict == SC_OK : verdict != k.want) return fail("volume_robust_check");
                if (lap_base || k.want != SC_OK) continue;
                for (float bad : { 0.f, -1.f, 2.5f, nan }) {
                    vr = good; vr.p_grad = bad;
                    if (robust_checks(&vr, &l) != SC_ERR_BAD_ARG) return fail("volume_robust_check (p_grad)");
                    vr = good; vr.p_time = bad;
                    if (robust_checks(&vr, &l) != SC_ERR_BAD_ARG) return fail("volume_robust_check (p_time)");
                    vr = good; vr.p_data = bad;
                    if (robust_checks(&vr, &l) != SC_ERR_BAD_ARG) return fail("volume_robust_check (p_data)");
                }
                for (float bad : { 0.f, -1.f, nan, inf }) {
                    vr = good; vr.eps_grad = bad;
                    if (robust_checks(&vr, &l) != SC_ERR_BAD_ARG) return fail("volume_robust_check (eps_grad)");
                    vr = good; vr.eps_time = bad;
                    if (robust_checks(&vr, &l) != SC_ERR_BAD_ARG) return fail("volume_robust_check (eps_time)");
                    vr = good; vr.p_data = 1.f; vr.eps_data = bad;
                    if (robust_checks(&vr, &l) != SC_ERR_BAD_ARG) return fail("volume_robust_check (eps_data)");
                    vr = good; vr.eps_data = bad;          // (an exponent of 2 does not look at its eps)
                    if (robust_checks(&vr, &l) != SC_OK) return fail("volume_robust_check (eps_data unused)");
                }
                vr = good; vr.round_tol = nan;
                if (robust_checks(&vr, &l) != SC_ERR_BAD_ARG) return fail("volume_robust_check (round_tol)");
                vr = good; vr.round_tol = -1.f;
                if (robust_checks(&vr, &l) != SC_OK) return fail("volume_robust_check (round_tol < 0)");
                for (int bits : { SC_ROBUST_ISOTROPIC, SC_ROBUST_JOINT_CHANNELS, SC_ROBUST_ISOTROPIC | SC_ROBUST_JOINT_CHANNELS }) {
                    vr = good; vr.kind = k.kind | bits;
                    if (robust_checks(&vr, &l) != SC_ERR_BAD_ARG) return fail("volume_robust_check (coupling bits)");
                }
                vr = good; vr.frames = tp ? 2 : 1;
                if (robust_checks(&vr, &l) != SC_ERR_BAD_ARG) return fail("volume_robust_check (too few frames)");
                vr = good; vr.frames = SC_POISSON_MAX_PLANES / k.c + 1;
                if (robust_checks(&vr, &l) != SC_ERR_BAD_SIZE) return fail("volume_robust_check (beyond the plane limit)");
                vr = good; vr.frame_stride = span - 1;
                if (robust_checks(&vr, &l) != SC_ERR_BAD_ARG) return fail("volume_robust_check (frame_stride)");
                vr = good; vr.tau = nan;
                if (robust_checks(&vr, &l) != SC_ERR_BAD_ARG) return fail("volume_robust_check (tau)");
                vr = good; vr.time_periodic = 2;
                if (robust_checks(&vr, &l) != SC_ERR_BAD_ARG) return fail("volume_robust_check (time_periodic)");
                vr = good; vr.tol = inf;
                if (robust_checks(&vr, &l) != SC_ERR_BAD_ARG) return fail("volume_robust_check (tol)");
                // the coupled volume call: every legal coupling (and none) accepted, TIME alone and unknown bits refused, unequal p or eps
                // under TIME refused (not without it), the coupling bits in kind still refused, the robust volume call's own refusals kept
                const int S = SC_VOLUME_COUPLE_SPACE, T = SC_VOLUME_COUPLE_TIME, J = SC_VOLUME_COUPLE_CHANNELS;
                // sc_hip_volume_flow_coupled_check beside every call, as above: the same parameters and coupling, the same verdicts
                auto coupled_checks = [](const sc_volume_robust_params *vp, int cpl, const sc_poisson_layout *vl) {
                    const int v = sc_hip_volume_coupled_check(vp, cpl, vl);
                    return sc_hip_volume_flow_coupled_check(vp, cpl, vl) == v ? v : -1000;
                };
                for (int cpl : { 0, S, S | T, J, S | J, S | T | J }) {
                    vr = good;
                    if (coupled_checks(&vr, cpl, &l) != SC_OK) return fail("volume_coupled_check (a legal coupling)");
                    vr.kind = k.kind | SC_ROBUST_ISOTROPIC;
                    if (coupled_checks(&vr, cpl, &l) != SC_ERR_BAD_ARG) return fail("volume_coupled_check (coupling bits in kind)");
                    vr = good; vr.p_data = 2.5f;
                    if (coupled_checks(&vr, cpl, &l) != SC_ERR_BAD_ARG) return fail("volume_coupled_check (p_data)");
                    vr = good; vr.frame_stride = span - 1;
                    if (coupled_checks(&vr, cpl, &l) != SC_ERR_BAD_ARG) return fail("volume_coupled_check (frame_stride)");
                    vr = good; vr.p_time = 1.5f;
                    if (coupled_checks(&vr, cpl, &l) != ((cpl & T) ? SC_ERR_BAD_ARG : SC_OK)) return fail("volume_coupled_check (p_time != p_grad)");
                    vr = good; vr.eps_time = 2e-3f;
                    if (coupled_checks(&vr, cpl, &l) != ((cpl & T) ? SC_ERR_BAD_ARG : SC_OK)) return fail("volume_coupled_check (eps_time != eps_grad)");
                }
                vr = good;
                for (int cpl : { T, T | J, 8, S | 8, -1, 1 << 20 })
                    if (coupled_checks(&vr, cpl, &l) != SC_ERR_BAD_ARG) return fail("volume_coupled_check (an illegal coupling)");
            }
            // the robust call: the WLS call's verdict on a guidance base, SC_ERR_BAD_ARG on a Laplacian one and on a bad exponent or eps
            sc_robust_params r{ k.kind, 1.f, 1e-3f, 2.f, 0.f, 0, 0.f, k.tol, k.iters };
            const int got = sc_hip_robust_check(&r, &l);
            if (lap_base ? got != SC_ERR_BAD_ARG : got != k.want) return fail("robust_check");
            r.p_grad = 2.5f;
            if (sc_hip_robust_check(&r, &l) != SC_ERR_BAD_ARG) return fail("robust_check (p_grad)");
            r.p_grad = 1.f; r.eps_grad = 0.f;
            if (sc_hip_robust_check(&r, &l) != SC_ERR_BAD_ARG) return fail("robust_check (eps_grad)");
            // the robust region call: the robust call's verdicts -- the region call's on a guidance base --, then every exponent, every eps,
            // round_tol and tol
            {
                const sc_robust_params good{ k.kind, 1.f, 1e-3f, 2.f, 0.f, 0, 0.f, k.tol, k.iters };
                sc_robust_params rr = good;
                if (sc_hip_region_robust_check(&rr, &l) != got) return fail("region_robust_check");
                rg.kind = k.kind;
                if (!lap_base && sc_hip_region_check(&rg, &l) != got) return fail("region_robust_check (the region call's verdict)");
                if (!lap_base && got == SC_OK) {
                    for (float bad : { 0.f, -1.f, 2.5f, nan }) {
                        rr = good; rr.p_grad = bad;
                        if (sc_hip_region_robust_check(&rr, &l) != SC_ERR_BAD_ARG) return fail("region_robust_check (p_grad)");
                        rr = good; rr.p_data = bad;
                        if (sc_hip_region_robust_check(&rr, &l) != SC_ERR_BAD_ARG) return fail("region_robust_check (p_data)");
                    }
                    for (float bad : { 0.f, -1.f, nan, inf }) {
                        rr = good; rr.eps_grad = bad;
                        if (sc_hip_region_robust_check(&rr, &l) != SC_ERR_BAD_ARG) return fail("region_robust_check (eps_grad)");
                        rr = good; rr.p_data = 1.f; rr.eps_data = bad;
                        if (sc_hip_region_robust_check(&rr, &l) != SC_ERR_BAD_ARG) return fail("region_robust_check (eps_data)");
                        rr = good; rr.eps_data = bad;          // (an exponent of 2 does not look at its eps)
                        if (sc_hip_region_robust_check(&rr, &l) != SC_OK) return fail("region_robust_check (eps_data unused)");
                    }
                    rr = good; rr.round_tol = nan;
                    if (sc_hip_region_robust_check(&rr, &l) != SC_ERR_BAD_ARG) return fail("region_robust_check (round_tol)");
                    rr = good; rr.round_tol = -1.f;
                    if (sc_hip_region_robust_check(&rr, &l) != SC_OK) return fail("region_robust_check (round_tol < 0)");
                    rr = good; rr.tol = inf;
                    if (sc_hip_region_robust_check(&rr, &l) != SC_ERR_BAD_ARG) return fail("region_robust_check (tol)");
                }
                if (sc_hip_region_robust_check(nullptr, &l) != SC_ERR_BAD_ARG || sc_hip_region_robust_check(&good, nullptr) != SC_ERR_BAD_ARG)
                    return fail("region_robust_check (null)");
            }
            // the coupling bits: the robust calls' verdicts do not change with them, every other family refuses them
            r.eps_grad = 1e-3f;
            for (int bits : { SC_ROBUST_ISOTROPIC, SC_ROBUST_JOINT_CHANNELS, SC_ROBUST_ISOTROPIC | SC_ROBUST_JOINT_CHANNELS }) {
                r.kind = k.kind | bits;
                if (sc_hip_robust_check(&r, &l) != got) return fail("robust_check (coupling bits)");
                if (sc_hip_region_robust_check(&r, &l) != got) return fail("region_robust_check (coupling bits)");
                p.kind = q.kind = k.kind | bits;
                if (sc_hip_weighted_check(&p, &l) != SC_ERR_BAD_ARG || sc_hip_wls_check(&q, &l) != SC_ERR_BAD_ARG) return fail("weighted_check / wls_check (coupling bits)");
                rg.kind = k.kind | bits;
                if (sc_hip_region_check(&rg, &l) != SC_ERR_BAD_ARG) return fail("region_check (coupling bits)");
                sc_poisson_params pp{ k.kind | bits, 0.f };
                sc_screened_params sp{ k.kind | bits, 1.f };
                if (sc_hip_poisson_check(&pp, &l) != SC_ERR_BAD_ARG || sc_hip_screened_check(&sp, &l) != SC_ERR_BAD_ARG) return fail("poisson_check / screened_check (coupling bits)");
            }
        }
        sc_weighted_params p{ SC_POISSON_GUIDANCE, 0.f, 0, 0.f };
        if (sc_hip_weighted_check(nullptr, nullptr) != SC_ERR_BAD_ARG || sc_hip_weighted_check(&p, nullptr) != SC_ERR_BAD_ARG) return fail("weighted_check (null)");
    }
    // 8: the schedule of a fused multigrid solve over a few hundred inputs: every row a launch that exists, the counts those of the rows
    {
        std::vector<int> rows(SC_FUSED_ROW * (3 * 6 + 2) + 3);
        unsigned s = 4242u;
        for (int i = 0; i < 600; ++i) {
            int facts[12], verdicts[4];
            for (int k = 0; k < 12; ++k) { s = s * 1664525u + 1013904223u; facts[k] = (int)((s >> 13) & 1u); }
            facts[0] += 1; facts[1] += 1; facts[2] = 1 + i % 6; facts[9] = (i / 6) % 4;
            for (int k = 0; k < 4; ++k) { s = s * 1664525u + 1013904223u; verdicts[k] = (int)((s >> 11) & 3u); }
            const int n = sc_hip_fused_schedule(facts, verdicts, i % 5, rows.data(), (int)rows.size());
            if (n < 1 || n > 3 * facts[2] + 1) return fail("fused_schedule: launches");
            int launches = 0;
            for (int r = 0; r < n; ++r) {
                const int *row = &rows[SC_FUSED_ROW * (size_t)r];
                if (row[0] < 1 || row[0] > 6 || row[1] < 1 || row[1] > 4 || row[17] < 0 || row[17] >= facts[2]) return fail("fused_schedule: a row");
                launches += row[0] != 4;
            }
            const int *tail = &rows[SC_FUSED_ROW * (size_t)n];
            if (tail[0] < 1 || tail[0] > facts[2] || tail[1] < launches || tail[1] > n) return fail("fused_schedule: counts");
            if (sc_hip_fused_schedule(facts, verdicts, i % 5, rows.data(), SC_FUSED_ROW * n + 2) != SC_ERR_BAD_ARG) return fail("fused_schedule wrote past its capacity");
        }
        int facts[12] = { 2, 2, 0, 0, 1, 1, 1, 1, 0, 1, 1, 1 };
        if (sc_hip_fused_schedule(facts, nullptr, 0, rows.data(), (int)rows.size()) != SC_ERR_BAD_ARG) return fail("fused_schedule took budget 0");
        if (sc_hip_fused_schedule(nullptr, nullptr, 0, rows.data(), (int)rows.size()) != SC_ERR_BAD_ARG) return fail("fused_schedule (null)");
    }
    // 9: the spans of a frame-only restore, applied as copies between heap blocks of exactly step x rows bytes (a span that leaves the
    //    image is the sanitizer's to report); the interior stays untouched, a capacity one short is refused
    {
        for (int i = 0; i < 400; ++i) {
            const int W = 1 + i % 9, H = 1 + (i / 9) % 8, ltx = i % 5, lty = (i / 5) % 3, cols = ltx + W + i % 3, rows = lty + H + (i / 3) % 2;
            const long long step = 3 * cols + i % 4;
            std::vector<long long> sp(2 * (size_t)(H + 1));
            const int n = sc_hip_restore_spans(step, rows, ltx, lty, W, H, sp.data(), H + 1);
            if (n < 1 || n > std::max(1, H - 1)) return fail("restore_spans: count");
            std::vector<uint8_t> src((size_t)step * rows, 1), dst((size_t)step * rows, 0);
            for (int k = 0; k < n; ++k) memcpy(dst.data() + sp[2 * k], src.data() + sp[2 * k], (size_t)(sp[2 * k + 1] - sp[2 * k]));
            for (int y = 0; y < rows; ++y)
                for (long long x = 0; x < step; ++x) {
                    const bool inside = y > lty && y < lty + H - 1 && x >= 3 * (ltx + 1) && x < 3 * (ltx + W - 1);
                    if (dst[(size_t)y * step + x] != (inside ? 0 : 1)) return fail("restore_spans: a byte");
                }
            if (sc_hip_restore_spans(step, rows, ltx, lty, W, H, sp.data(), n - 1) != SC_ERR_BAD_ARG) return fail("restore_spans wrote past its capacity");
        }
        long long sp[4];
        if (sc_hip_restore_spans(30, 4, 8, 0, 5, 3, sp, 2) != SC_ERR_BAD_ARG || sc_hip_restore_spans(30, 4, 0, 0, 5, 3, nullptr, 2) != SC_ERR_BAD_ARG) return fail("restore_spans (bad geometry)");
    }
    // 10: a job's side arrays from the record to the kernels' tables, and from the public jobs to the record
    {
        using namespace sc;
        const int m = 20;
        std::vector<PoissonJobDev> jobs(m);
        std::vector<SideArrays> sides(m);
        for (int k = 0; k < m; ++k) {
            jobs[k] = PoissonJobDev{ fake(k, 6), nullptr, nullptr, nullptr, (float *)fake(k, 7), fake(k, 8) };
            sides[k] = SideArrays{ fake(k, 0), fake(k, 1), fake(k, 2), fake(k, 3), fake(k, 4), fake(k, 5) };
        }
        struct Members { const float *const *a[6]; };
        if (!tables_ok<VolumeJobs>(jobs.data(), sides.data(), m, [](const VolumeJobs &t) { return Members{ { t.w, t.sx, t.sy, t.st, t.gt, t.smt } }; })) return fail("for_side_tables<VolumeJobs>");
        if (!tables_ok<RegionJobs>(jobs.data(), sides.data(), m, [](const RegionJobs &t) { return Members{ { t.w, t.sx, t.sy, t.st, nullptr, nullptr } }; })) return fail("for_side_tables<RegionJobs>");
        if (!tables_ok<WlsJobs>(jobs.data(), sides.data(), m, [](const WlsJobs &t) { return Members{ { t.w, t.sx, t.sy, nullptr, nullptr, nullptr } }; })) return fail("for_side_tables<WlsJobs>");
        if (!tables_ok<WeightedJobs>(jobs.data(), sides.data(), m, [](const WeightedJobs &t) { return Members{ { t.w, nullptr, nullptr, nullptr, nullptr, nullptr } }; })) return fail("for_side_tables<WeightedJobs>");

        // the intake: job 1 without state and job 3 with an unaligned smooth_t are refused; what stays is paired job by job
        const int all = FLOAT_DATA | FLOAT_WEIGHT | FLOAT_SMOOTH | FLOAT_STATE | FLOAT_GT | FLOAT_SMOOTH_T;
        auto arrays_of = [](const sc_volume_wls_job &j) {
            FloatArrays a{ j.gx, j.gy, j.lap, j.data, j.weight, j.boundary, j.out, j.smooth_x, j.smooth_y, j.state };
            a.gt = j.gt;
            a.smooth_t = j.smooth_t;
            return a;
        };
        for (int pass = 0; pass < 2; ++pass) {
            const bool links = pass == 0;
            const int carries = links ? all : all & ~(FLOAT_SMOOTH | FLOAT_SMOOTH_T);
            sc_volume_wls_job pub[5];
            for (int k = 0; k < 5; ++k) {
                pub[k] = sc_volume_wls_job{ fake(k, 6), fake(k, 9), fake(k, 4), nullptr, fake(k, 8), k == 1 ? nullptr : fake(k, 3), fake(k, 0),
                                            links ? fake(k, 1) : nullptr, links ? fake(k, 2) : nullptr,
                                            !links ? nullptr : k == 3 ? (const float *)((uintptr_t)fake(k, 5) + 2) : fake(k, 5), fake(k, 10),
                                            (float *)fake(k, 7), 12345 };
            }
            Instance inst;
            FloatJobs v;
            const int rc = float_intake(&inst, SC_POISSON_GUIDANCE, carries, pub, 5, arrays_of, v);
            const std::vector<int> stay = links ? std::vector<int>{ 0, 2, 4 } : std::vector<int>{ 0, 2, 3, 4 };
            if (rc != SC_ERR_BAD_ARG || inst.err != "null state pointer") return fail("float_intake: the worst code and the first reason");
            if (v.dj.size() != stay.size() || v.side.size() != stay.size() || v.rcs.size() != stay.size()) return fail("float_intake: how many jobs stay");
            if (pub[1].rc != SC_ERR_BAD_ARG || (links && pub[3].rc != SC_ERR_BAD_ARG)) return fail("float_intake: a refused job's code");
            for (size_t i = 0; i < stay.size(); ++i) {
                const int k = stay[i];
                const SideArrays &a = v.side[i];
                if (v.rcs[i] != &pub[k].rc || pub[k].rc != SC_ERR_HIP) return fail("float_intake: where a job's code goes");
                if (v.dj[i].gx != fake(k, 6) || v.dj[i].gy != fake(k, 9) || v.dj[i].b != fake(k, 10) || v.dj[i].out != (float *)fake(k, 7) || v.dj[i].d != fake(k, 8))
                    return fail("float_intake: a job's own arrays");
                if (a.w != fake(k, 0) || a.st != fake(k, 3) || a.gt != fake(k, 4)) return fail("float_intake: w, st or gt of another job");
                if (links ? (a.sx != fake(k, 1) || a.sy != fake(k, 2) || a.smt != fake(k, 5)) : (a.sx || a.sy || a.smt))
                    return fail("float_intake: sx, sy or smt of another job, or not NULL where the call carries none");
            }
        }
        // ... and an array the call does not carry is NULL in the record whatever the job brings (the entries refuse such a job before)
        {
            sc_volume_wls_job one{ fake(0, 6), fake(0, 9), fake(0, 4), nullptr, fake(0, 8), fake(0, 3), fake(0, 0), fake(0, 1), fake(0, 2), fake(0, 5), fake(0, 10),
                                   (float *)fake(0, 7), 0 };
            Instance inst;
            FloatJobs v;
            if (float_intake(&inst, SC_POISSON_GUIDANCE, FLOAT_DATA | FLOAT_STATE, &one, 1, arrays_of, v) != SC_OK || v.side.size() != 1) return fail("float_intake (a plain region call)");
            const SideArrays &a = v.side[0];
            if (a.w || a.sx || a.sy || a.gt || a.smt || a.st != fake(0, 3)) return fail("float_intake: an array the call does not carry must be NULL");
        }
    }
    // 11: the conjugate-gradient families' tiling: every part and segment has a slot, no band is empty, the bands cover the rows
    {
        const int kinds[] = { SC_POISSON_LAPLACIAN, SC_POISSON_LAPLACIAN | SC_POISSON_NEUMANN, SC_POISSON_GUIDANCE | SC_POISSON_FREE_LEFT | SC_POISSON_FREE_TOP,
                              SC_POISSON_GUIDANCE | SC_POISSON_PERIODIC_X, SC_POISSON_LAPLACIAN | SC_POISSON_PERIODIC_X | SC_POISSON_PERIODIC_Y };
        for (int kind : kinds)
            for (int frames : { 1, 2, 17, 64, SC_POISSON_MAX_PLANES })
                for (int cols = 3; cols <= 2105; cols += (cols < 20 ? 1 : 83))
                    for (int rows = 3; rows <= 2205; rows += (rows < 70 ? 1 : 61)) {
                        long long p[10];
                        if (sc_hip_pcg_plan(cols, rows, kind, frames, p) != SC_OK) return fail("pcg_plan");
                        const long long nx = p[0], ny = p[1], cg = p[4], bands = p[5], rows_per = p[6], eparts = p[7], egroups = p[8], stride = p[9];
                        if (nx < 1 || nx > cols || ny < 1 || ny > (long long)rows * frames || ny % frames) return fail("pcg_plan: the unknown block");
                        if (cg != (nx + 255) / 256 || cg * bands > sc::PCG_PARTS || bands * rows_per < ny || (bands - 1) * rows_per >= ny) return fail("pcg_plan: the bands");
                        if (eparts < 1 || eparts > sc::PCG_PARTS || egroups != (nx * ny + 3) / 4 || eparts * ((egroups + eparts - 1) / eparts) < egroups) return fail("pcg_plan: the segments");
                        if (stride % 64 || stride < nx * ny) return fail("pcg_plan: the stride");
                    }
        long long p[10];
        if (sc_hip_pcg_plan(2, 7, SC_POISSON_LAPLACIAN, 1, p) != SC_ERR_BAD_SIZE || sc_hip_pcg_plan(33, 47, SC_POISSON_NEUMANN, 1, p) != SC_ERR_BAD_ARG ||
            sc_hip_pcg_plan(33, 47, SC_POISSON_LAPLACIAN, 0, p) != SC_ERR_BAD_ARG || sc_hip_pcg_plan(33, 47, SC_POISSON_LAPLACIAN, SC_POISSON_MAX_PLANES + 1, p) != SC_ERR_BAD_ARG ||
            sc_hip_pcg_plan(33, 47, SC_POISSON_LAPLACIAN, 1, nullptr) != SC_ERR_BAD_ARG) return fail("pcg_plan (refusals)");
    }
    // 12: the first level-0 launch that reads a group's destination bytes (sc_u0_bytes.h): the row sits in an allocation that ends 3
    // bytes behind it and starts 4 + its misalignment before it -- the farthest the rule may read -- so a fetch beyond is this program's to find
    {
        std::vector<int> out(64 * 16);
        for (int W = 3; W <= 600; ++W)
            for (int al = 0; al < 4; ++al) {
                const size_t lead = 4 + (size_t)al;
                std::unique_ptr<uint8_t[]> buf(new uint8_t[lead + 3 * (size_t)W + 3]);
                uint8_t *base = buf.get();
                if (((uintptr_t)base & 3) != 0) return fail("u0_bytes: allocation alignment");
                uint8_t *row = base + lead;
                for (size_t i = 0; i < lead + 3 * (size_t)W + 3; ++i) base[i] = (uint8_t)(i * 37u + (unsigned)W);
                const int nbx = (W + 231) / 232;
                for (int bx : { 0, nbx / 2, nbx - 1 }) {
                    const int xw = bx * 232 - 12;
                    if (sc_hip_u0_bytes_fetch(row, W, xw, out.data()) != SC_OK) return fail("u0_bytes_fetch");
                    for (int lane = 0; lane < 64; ++lane) {
                        const int *o = &out[16 * lane];
                        const int x = std::min(std::max(xw + 4 * lane, 0), W);
                        for (int k = 0; k < 4; ++k) {
                            if ((o[2] >> k & 1) && !(o[0] + 4 * k + 3 >= 0 && o[0] + 4 * k < 3 * W)) return fail("u0_bytes: a dword outside the row was read");
                            for (int ci = 0; ci < 3; ++ci)
                                if (o[4 + 4 * ci + k] != (x + k < W ? (int)row[3 * (x + k) + ci] : 0)) return fail("u0_bytes: value");
                        }
                    }
                }
            }
    }
    printf("sanitize_main: clean\n");
    return 0;
}
