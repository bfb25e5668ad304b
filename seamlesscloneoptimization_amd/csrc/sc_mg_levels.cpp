// sc_mg_levels.cpp -- the multigrid hierarchy: the ladder of level geometries of a ROI (arbitrary sizes coarsen by letting the LAST
// grid interval of each level differ from the others, MGDim, so the Dirichlet ring never moves), the level planes of one clone or of a
// size class, the choice of the bottom and of the level solved directly.  sc_multigrid.cpp runs the cycles on what is built here.
#include "sc_instance.h"
#include <algorithm>
#include <cmath>

namespace sc {

static void coarsen_1d(int n, double a, int &nc, double &ac)
{
    if (n % 2 == 1) { nc = (n - 1) / 2; ac = (1.0 + a) / 2.0; }       // boundary stays (1+a)/2 coarse cells away
    else if (a >= 1.0) { nc = n / 2; ac = a / 2.0; }                   // keep the last point
    else { nc = n / 2 - 1; ac = 1.0 + a / 2.0; }                       // drop it: gap would fall below 1/2
}

MGDim make_dim(int n, double a, int nc)
{
    MGDim d;
    d.n = n; d.nc = nc; d.alpha = (float)a;
    d.cw_last = (float)(2.0 / (1.0 + a));
    d.d_last = (float)(2.0 / a);
    const int tail = n - 2 * nc;          // 0, 1 or 2 fine points beyond the last coarse point
    const double D = n + a - 2.0 * nc;    // their distance budget to the boundary
    d.tw1 = tail >= 1 ? (float)(1.0 - 1.0 / D) : 0.f;
    d.tw2 = tail >= 2 ? (float)(1.0 - 2.0 / D) : 0.f;
    d.inv_last = (float)(1.0 / (1.5 + (double)d.tw1 + (double)d.tw2));
    return d;
}

static Field level_field(void *p, int W, int H, int C)
{
    Field f;
    f.p = (float *)p; f.W = W; f.H = H; f.C = C;
    // at least two pad columns behind the ring: the level-0 kernel reads three coarse columns starting at an even column <= nc
    // (k_cycle0's prolongation), and must find them where it expects them, not shifted by an address clamp
    f.pitch = round_up(W + 2, 64);
    f.plane = (size_t)f.pitch * H;
    return f;
}

// LDS floats level l needs inside the bottom kernel: U and F planes, odd row pitch
int bottom_pitch(const MGLevel &L) { return (L.g.x.n + 2) | 1; }
static long bottom_floats(const MGGeom &g) { return 2L * ((g.x.n + 2) | 1) * (g.y.n + 2); }
static long bottom_floats(const MGLevel &L) { return bottom_floats(L.g); }

// first level handled by the fused bottom kernel: the first l >= 1 from which all remaining
// levels fit the LDS budget together (never level 0: it runs the exact kernels)
static size_t bottom_start(const std::vector<MGGeom> &g)
{
    for (size_t l = 1; l < g.size(); ++l) {
        if (g.size() - l > (size_t)MG_BOTTOM_MAX_LEVELS) continue;
        long tot = 0;
        for (size_t k = l; k < g.size(); ++k) tot += bottom_floats(g[k]);
        if (tot * (long)sizeof(float) <= (long)MG_BOTTOM_LDS_BYTES) return l;
    }
    return g.size();
}

// Chooses the bottom level solved directly and has its matrices built ON THE DEVICE from the closed-form eigenpairs of the
// level's two 1-D operators (sc_fd_closed.h, k_fd_build) -- no host eigen-solve, no staging copy, no wait.  The build runs on
// the instance's second stream, beside the first launches of the clone that needs it; run_bottom() makes the main stream
// wait for it.  (Rounds 1-3 ran the implicit-QL solve of sc_fd_selftest.cpp on the host for every new ROI size: 0.1-0.3 ms per direction at
// n = 63, as long as the clone itself; it now only serves sc_hip_selftest_host as the reference the closed form is checked
// against.)  I->fd_level = -1 when nothing fits.
static int build_fd(Instance *I)
{
    I->fd_level = -1;
    if ((I->opts.flags & SC_FLAG_VCYCLE_BOTTOM) || I->mg_bottom >= I->mg.size()) return SC_OK;
    long planes = 0;
    I->fd_mm = false;
    for (size_t l = I->mg_bottom; l < I->mg.size(); ++l) {
        const MGLevel &L = I->mg[l];
        planes += bottom_floats(L);
        const int nx = L.g.x.n, ny = L.g.y.n, nxp = round_up(nx, 4), nyp = round_up(ny, 4);
        const int dmax = I->opts.mg_direct_max > 0 ? std::min(I->opts.mg_direct_max, 128) : SC_MG_DIRECT_MAX_DEFAULT;
        if (nx > dmax || ny > dmax) continue;
        // the bottom's first level on the matrix cores (k_mg_bottom_mm): up to 96 unknowns per side, no LDS budget to meet
        const bool mm = l == I->mg_bottom && nx <= 96 && ny <= 96 && !legacy_path(I->opts, SC_LEGACY_BOTTOM_F32);
        if (!mm && (planes + fd_lds_floats(nxp, nyp)) * (long)sizeof(float) > (long)MG_BOTTOM_LDS_BYTES) continue;
        const long nf = (fd_mat_floats(nxp, nyp) + 15) & ~15L;          // the matrix-core operands behind the float matrices, 64-byte aligned
        const int NPX = round_up(nx, 32), NPY = round_up(ny, 32);
        int rc;
        // a build nobody waited for (a solve that never reached its bottom): order it in front of whatever follows on the main stream --
        // ensure() below waits for that stream before it frees
        if ((rc = fd_wait(I))) return rc;
        if ((rc = ensure(I, I->mg_fd, sizeof(float) * (size_t)nf + (mm ? (size_t)fd_mm_bytes(NPX, NPY) : 0)))) return rc;
        // everything that read the previous matrices has been enqueued on the main stream: the build starts behind it
        SC_HIP(I, hipEventRecord(I->ev_fd_fork, I->stream));
        SC_HIP(I, hipStreamWaitEvent(I->aux, I->ev_fd_fork, 0));
        launch_fd_build((float *)I->mg_fd.p, L.g, nxp, nyp, I->aux, mm ? (unsigned char *)((float *)I->mg_fd.p + nf) : nullptr, NPX, NPY);
        SC_HIP(I, hipGetLastError());
        SC_HIP(I, hipEventRecord(I->ev_fd, I->aux));
        I->fd_pending = true;
        I->fd_level = (int)(l - I->mg_bottom);
        I->fd_nxp = nxp; I->fd_nyp = nyp;
        I->fd_mm = mm; I->fd_npx = NPX; I->fd_npy = NPY; I->fd_mm_off = (size_t)nf;
        return SC_OK;
    }
    return SC_OK;
}

// The ladder of levels of a W x H field (ring included): the geometry of every level (and of its transfer to the next coarser one).
// Host arithmetic only; the size-class planner (sc_ragged.cpp) runs it per member.
void mg_plan_levels(int W, int H, std::vector<MGGeom> &g)
{
    struct L1 { int nx, ny; double ax, ay; };
    std::vector<L1> ls;
    ls.push_back({ W - 2, H - 2, 1.0, 1.0 });
    while (std::min(ls.back().nx, ls.back().ny) > 3) {
        L1 c;
        coarsen_1d(ls.back().nx, ls.back().ax, c.nx, c.ax);
        coarsen_1d(ls.back().ny, ls.back().ay, c.ny, c.ay);
        if (c.nx < 1 || c.ny < 1) break;
        ls.push_back(c);
    }
    const size_t nl = ls.size();
    g.resize(nl);
    for (size_t l = 0; l < nl; ++l) {
        const int ncx = (l + 1 < nl) ? ls[l + 1].nx : 0, ncy = (l + 1 < nl) ? ls[l + 1].ny : 0;
        g[l].x = make_dim(ls[l].nx, ls[l].ax, ncx);
        g[l].y = make_dim(ls[l].ny, ls[l].ay, ncy);
    }
}

// The default hierarchy's deepest launched level (see build_levels): the first level >= 2 with at most 127 unknowns per side, held in
// registers by k_mg_tail with the level below it solved directly in the same launch; 0: this ladder ends differently (its level 1
// is solved directly -- at most 64 unknowns per side: 10-13 us per solve for a group of sixteen, against ~24 for a level-1 launch plus
// k_mg_tail; up to 96 until late in round 5, but the 96-wide solve takes 31-34 us (ROIs of 131..194 pixels: measured on groups of
// 16, tools/class_timeline.sh) --, or no such level exists)
size_t mg_default_tail_level(const std::vector<MGGeom> &g)
{
    const size_t nl = g.size();
    size_t a = 0;
    for (size_t l = 2; l + 1 < nl && !a; ++l)
        if (g[l].x.n <= 127 && g[l].y.n <= 127) a = l;
    const bool level1_direct = nl > 1 && g[1].x.n <= 64 && g[1].y.n <= 64;
    return (a && !(a == 2 && level1_direct)) ? a : 0;
}

// The first level the bottom of the cycle handles on the ladder g: the LDS-fit rule (bottom_start), and under the default rule (see
// build_levels) the level below the tail level, or the first level the matrix-core solve fits where level 1 does not fit it already.
size_t mg_plan_bottom(const std::vector<MGGeom> &g, bool default_rule)
{
    const size_t nl = g.size();
    size_t b = bottom_start(g);
    if (default_rule) {
        const size_t a = mg_default_tail_level(g);
        const bool level1_direct = nl > 1 && g[1].x.n <= 96 && g[1].y.n <= 96;
        if (a) b = a + 1;
        else if (!level1_direct)
            for (size_t l = 1; l < nl; ++l)
                if (g[l].x.n <= 96 && g[l].y.n <= 96) { b = l; break; }
    }
    return b;
}

// The ladder's part of mg_composes_level1 (sc_multigrid.cpp): a launched level 1 with a level 2 below it.
bool mg_ladder_composes(size_t levels, size_t bottom) { return levels >= 3 && bottom >= 2; }

// The three planes of level l (>= 1, geometry in I->mg[l].g) for C channels: their buffers, the Fields over them, and those of
// U, F, T (bits 0, 1, 2 of `zero`) queued in zj to be zeroed by the launch that zeroes every plane (a full queue goes out on
// `zero_on`; the caller launches what is left).
static int level_planes(Instance *I, size_t l, int C, unsigned zero, ZeroJobs &zj, hipStream_t zero_on)
{
    MGLevel &L = I->mg[l];
    const int Wl = L.g.x.n + 2, Hl = L.g.y.n + 2;
    Field proto = level_field(nullptr, Wl, Hl, C);
    for (int k = 0; k < 3; ++k) {
        int rc = ensure(I, I->mg_bufs[3 * l + k], proto.bytes() + 4096, false);      // (zeroed by the caller's launch; buffers are 4096 bytes larger than the field)
        if (rc) return rc;
    }
    L.U = level_field(I->mg_bufs[3 * l + 0].p, Wl, Hl, C);
    L.F = level_field(I->mg_bufs[3 * l + 1].p, Wl, Hl, C);
    L.T = level_field(I->mg_bufs[3 * l + 2].p, Wl, Hl, C);
    const Field *const planes[3] = { &L.U, &L.F, &L.T };
    for (int k = 0; k < 3; ++k) {
        if (!((zero >> k) & 1u)) continue;
        if (zj.count == ZeroJobs::MAX) { launch_zero_multi(zj, zero_on); zj.count = 0; }
        zj.p[zj.count] = planes[k]->p; zj.n16[zj.count] = (planes[k]->bytes() + 15) / 16; ++zj.count;
    }
    return SC_OK;
}

int build_levels(Instance *I)
{
    if (I->rag.dev) {          // a size class: rag_begin_builds built the hierarchy (mg_build_levels_rag)
        if (!I->rag.levels_built || I->mg.empty()) { I->err = "size class: hierarchy missing"; return SC_ERR_BAD_ARG; }
        return SC_OK;
    }
    const int W = I->F.W, H = I->F.H, C = I->F.C;
    if (!I->mg.empty() && I->mg[0].F.p == I->F.p && I->mg[0].F.W == W && I->mg[0].F.H == H && I->mg[0].F.C == C)
        return SC_OK;
    I->info.new_size = 1;
    I->mg.clear();
    std::vector<MGGeom> plan;
    mg_plan_levels(W, H, plan);
    const size_t nl = plan.size();
    if (I->mg_bufs.size() < 3 * nl) I->mg_bufs.resize(3 * nl);
    I->mg.resize(nl);
    ZeroJobs zj{};
    for (size_t l = 0; l < nl; ++l) {
        MGLevel &L = I->mg[l];
        L.g = plan[l];
        const double rho = 0.5 * (std::cos(M_PI / (L.g.x.n + 1.0)) + std::cos(M_PI / (L.g.y.n + 1.0)));
        L.omega = (float)(2.0 / (1.0 + std::sqrt(std::max(0.0, 1.0 - rho * rho))));
        if (l == 0) continue; // level 0 aliases the instance fields, bound per cycle
        // rings and pads of F/U must be zero; ensure() zero-fills fresh memory, but a reused
        // larger buffer may hold stale data from another ROI size: every plane of every level in ONE launch below
        // (24-36 memsets were 70-100 us of launches in front of the first clone at a new size)
        int rc = level_planes(I, l, C, 1 | 2 | 4, zj, I->stream);
        if (rc) return rc;
    }
    launch_zero_multi(zj, I->stream);
    SC_HIP(I, hipGetLastError());
    I->mg[0].F = I->F;
    const bool default_rule = !(I->opts.flags & SC_FLAG_VCYCLE_BOTTOM) && !legacy_path(I->opts, SC_LEGACY_BOTTOM_F32) && I->opts.mg_direct_max <= 0;
    I->mg_bottom = mg_plan_bottom(plan, default_rule);
    // Default hierarchy since round 4: the deepest launched level ("A") is the first one (>= 2) with at most 127 unknowns per side --
    // k_mg_tail holds it in registers -- and the level below it ("B", at most 63 per side) is the one solved directly, on the matrix
    // cores, inside the same launch.  The LDS-fit rule above chose the bottom in rounds 1-3; where it landed on a level with 97 .. ~190
    // unknowns on a side (ROIs like 2090 x 1632, 2500 x 1300, 3540^2: no matrix-core solve, an LDS-resident V-cycle inside
    // k_mg_bottom instead) a cycle cost 60 us more than at the sizes next to it (0.55 against 0.38 ms for one clone).  Kept: a ROI
    // whose level 1 fits the matrix-core solve at 64 (solved there; at 65..96 only where the ladder has no level for k_mg_tail),
    // the flags that ask for the older bottoms.
    // (mg_plan_bottom above: the rule itself, which sc_hip_cycle0_plan answers from as well)
    I->mg_l1_half = false;        // fresh planes: all zero in either format
    return build_fd(I);
}

// The hierarchy of a SIZE CLASS (RagState, sc_instance.h): level planes at the class's strides -- the largest width and height any
// member has on that level --, every plane zeroed (a member's ring and what lies beyond it must be zero, and the slot may have held a
// larger member a call ago), the members' bottom matrices by one launch on the second stream.  The per-member geometries are in the
// table on the device; I->mg[l].g holds the class's MAXIMA (grid sizes and the launchers' shape tests read those).
// Called from rag_begin_builds: the zeroing goes to `zero_on` (the instance's second stream, which the main stream joins in front of its
// first coarse-level launch, mg_solve) -- the caller has ordered that stream behind everything that read the planes before.
int mg_build_levels_rag(Instance *I, hipStream_t zero_on)
{
    RagState &R = I->rag;
    R.levels_built = false;
    const int C = I->F.C, n = R.n;
    const size_t nl = (size_t)R.nl;
    I->info.new_size = 1;
    I->mg.clear();
    if (I->mg_bufs.size() < 3 * nl) I->mg_bufs.resize(3 * nl);
    I->mg.resize(nl);
    ZeroJobs zj{};
    for (size_t l = 0; l < nl; ++l) {
        MGLevel &L = I->mg[l];
        L.g = R.host[0].g[l];
        for (int i = 1; i < n; ++i) {
            const MGGeom &g = R.host[i].g[l];
            L.g.x.n = std::max(L.g.x.n, g.x.n); L.g.x.nc = std::max(L.g.x.nc, g.x.nc);
            L.g.y.n = std::max(L.g.y.n, g.y.n); L.g.y.nc = std::max(L.g.y.nc, g.y.nc);
        }
        L.omega = 1.f;
        if (l == 0) continue;
        // What must be zero: a member's ring and everything beyond it in the planes a finer level interpolates FROM -- U and its
        // ping-pong partner T (the launches write a member's own extent only, and the slot may have held a larger member a call
        // ago).  Right-hand sides are read under the interior masks only: F needs nothing.
        int rc = level_planes(I, l, C, 1 | 4, zj, zero_on);
        if (rc) return rc;
    }
    launch_zero_multi(zj, zero_on);
    SC_HIP(I, hipGetLastError());
    I->mg[0].F = I->F;
    I->mg_bottom = (size_t)R.tail + 1;
    I->mg_l1_half = true;      // a class runs the fast path (plan_size): float16 level 1, and its planes are all zero -- valid in either format, nothing to re-zero in mg_solve
    // the class's bottom: every member's level below `tail` solved directly on the matrix cores inside k_mg_tail, operands padded
    // alike; the matrices are being built on the third stream since rag_begin_builds (run_tail waits for them)
    I->fd_level = 0; I->fd_mm = true; I->fd_npx = R.npx; I->fd_npy = R.npy; I->fd_nxp = I->fd_nyp = 0; I->fd_mm_off = 0;
    R.levels_built = true;
    return SC_OK;
}

} // namespace sc
