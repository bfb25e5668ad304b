"""The quantities the volume GPU tests hold the library to, their bounds and their inputs (tests/test_gpu_volume.py), after the pattern of
tests/region_bounds.py with the operator of tests/volume_np.py:

    ERR  max |u - solve_exact| / max |solve_exact|      both maxima over the UNKNOWN pixels of all frames
    RES  max |L u - b| / max |b|                         likewise; b the library's float32 right-hand side, the rest in float64

Bounds:  measured <= max(FACTOR x the same quantity for volume_np.pcg_f32 on the same input, FLOOR).  pcg_f32 is the same iteration with
the same preconditioner, start and stop rule, so both stop somewhere below tol; the library runs up to SC_WEIGHTED_POLL iterations longer,
adds its sums in another order and transforms by chirp convolutions where the restatement uses pocketfft.  The four constants come from
one MI355X run of tools/volume_probe.py --lengths over a length walk and the tests' own inputs (DESIGN.md section 4 holds the table,
profiles/volume_lengths.txt the record), by wls_bounds' rule: each factor is the worst ratio to the restatement, times 2, rounded up to
one digit; each floor twice the worst absolute value among the inputs where the restatement needed no iteration at all.
Iterations:  sweeps <= 2 x pcg_f32's count + SC_WEIGHTED_POLL, both from the reference iteration."""
import functools

import numpy as np

import direct_np
import volume_np
import weighted_bounds as wb

POLL = wb.POLL
RES_FACTOR, RES_FLOOR = 2.0, 2.9e-6             # measured: worst ratio 1.00 (periodic x 2 x 7, 2 frames, keyframes: one unknown), worst value without an iteration 1.42e-6 (neumann 2 x 7, 5 frames, tau 10, every state 0)
ERR_FACTOR, ERR_FLOOR = 6.0, 2.1e-6             # measured: worst ratio 2.55 (neumann 2 x 7, 3 frames, tau 0.1, split, sparse), worst value without an iteration 1.04e-6 (neumann 2 x 7, 5 frames, tau 10, every state 0)

BORDERS = wb.BORDERS
SIZES = [(47, 33), (9, 300), (7, 2), (5, 16)]  # rows x columns; 300 columns cross the 256-column group
FRAMES = [2, 3, 5, 8]
CHANNELS = [1, 3]
TAUS = [0.1, 1.0, 10.0]
PATTERNS = ["all", "keyframes", "hole", "scatter", "split"]
WEIGHTS = [None, "constant", "sparse"]         # None: no data term
FORMS = ["gt", "guidance", "lap"]              # guidance with gt, guidance without it, the whole right-hand side as lap
MAX_ITERS = 400                                # sc_volume_params' default


def matrix():
    """the inputs of the GPU tests' walk (and of tools/volume_probe.py): (border, H, W, C, T, tau, pattern, wkind, form).  Every border x
    size twice (a frame around 2 x 7 pixels leaves no unknown and is left out), the other axes rotating so that every value of each meets
    every border and every size class; tests/test_volume_host.py checks that every value of every axis occurs."""
    out = []
    for bi, (border, _, _) in enumerate(BORDERS):
        for si, (H, W) in enumerate(SIZES):
            if border == "frame" and min(H, W) < 3:
                continue
            for j in range(2):
                i = 2 * (bi * len(SIZES) + si) + j
                out.append((border, H, W, CHANNELS[(bi + si + j) % 2], FRAMES[(bi + 2 * si + j) % 4], TAUS[(i + bi) % 3], PATTERNS[(i + si) % 5],
                            WEIGHTS[(i // 2 + j) % 3], FORMS[(i + bi + j) % 3]))
    return out


def pattern_state(pattern, T, H, W, C, rng):
    y, x = np.mgrid[0:H, 0:W]
    st = np.zeros((T, H, W, C), np.float32)
    for c in range(C):
        for t in range(T):
            f = st[t, :, :, c]
            if pattern == "all":              # every pixel unknown
                pass
            elif pattern == "keyframes":      # the first and the last frame known, nothing pinned in between
                f[...] = 1 if t in (0, T - 1) else 0
            elif pattern == "hole":           # UNKNOWN inside an ellipse that moves across the frames, KNOWN around it
                cy, cx = (H - 1) / 2 + 0.3 * c, (W - 1) * (t + 1) / (T + 1) - 0.4 * c
                f[...] = np.where(((y - cy) / max(0.3 * H, 0.8)) ** 2 + ((x - cx) / max(0.25 * W, 0.8)) ** 2 <= 1.0, 0, 1)
            elif pattern == "scatter":        # about 1 in 30 KNOWN around an excluded tube
                f[...] = rng.random((H, W)) < 1 / 30
                by, bx, r = 0.3 * H + c, 0.65 * W - c, 0.18 * min(H, W)
                f[(y - by) ** 2 + (x - bx) ** 2 <= r * r] = 2
            elif pattern == "split":          # an OUTSIDE frame cuts the volume in two, a few KNOWN pixels on each side
                if t == T // 2:
                    f[...] = 2
                else:
                    f[rng.random((H, W)) < 1 / 12] = 1
            else:
                raise ValueError(pattern)
    return st


def states(pattern, sides, periodic, T, H, W, C, weight=None, seed=0):
    """state, float32 T x H x W x C, of one pattern under these borders, mended as region_bounds.states does: every channel has an
    UNKNOWN pixel inside the borders (else the centre pixel of its first frame that is not OUTSIDE becomes one), and every UNKNOWN
    component is pinned (else its first pixel in reading order becomes KNOWN) -- volume_np.unpinned_components then finds nothing
    (tests/test_volume_host.py checks that)."""
    rng = np.random.default_rng(6000 + seed + 11 * H + W + 101 * T)
    st = pattern_state(pattern, T, H, W, C, rng)
    rows, cols = volume_np.unknowns(sides, periodic, H, W)
    inside = ~direct_np.dirichlet_mask(sides, periodic, H, W)
    for c in range(C):
        if not ((st[:, :, :, c] == 0) & inside).any():
            t = 0 if pattern != "split" or T // 2 else 1
            st[t, (rows.start + rows.stop - 1) // 2, (cols.start + cols.stop - 1) // 2, c] = 0
    while True:
        loose = volume_np.unpinned_components(sides, periodic, st, weight)
        if not loose.any():
            return st
        st[tuple(np.argwhere(loose)[0])] = 1


def make_input(border, H, W, C, T, tau, pattern, wkind, seed=0):
    """One input as a dict: sides, periodic, tau, state, data, weight (None without wkind), lap, gx, gy, gt, boundary; float32
    T x H x W x C (gt: T - 1 frames), every element set (nan_unread() spoils the ones a call must not read)"""
    sides, periodic = {b[0]: b[1:] for b in BORDERS}[border]
    rng = np.random.default_rng(7000 + seed + 7 * H + W + 13 * T)
    shape = (T, H, W, C)
    data, boundary = rng.standard_normal((2,) + shape).astype(np.float32)
    lap = (0.1 * rng.standard_normal(shape)).astype(np.float32)
    gx, gy = (0.1 * rng.standard_normal((2,) + shape)).astype(np.float32)
    gt = (0.1 * rng.standard_normal((T - 1, H, W, C))).astype(np.float32)
    weight = None if wkind is None else wb.weights(wkind, shape, 300 + seed + H + T)
    state = states(pattern, sides, periodic, T, H, W, C, weight, seed)
    return dict(sides=sides, periodic=periodic, tau=float(tau), state=state, data=data, weight=weight, lap=lap, gx=gx, gy=gy, gt=gt, boundary=boundary)


def nan_unread(p):
    """a copy of the input with NaN in every element the header says is not read: weight and lap off the UNKNOWN pixels, gx and gy where
    the link is not live in the region, gt at dead temporal links, data at UNKNOWN pixels when there is no weight, boundary off its
    Dirichlet lines, state on them"""
    q = dict(p)
    nan = np.float32(np.nan)
    k = volume_np.kinds(p["sides"], p["periodic"], p["state"])
    unk = k == volume_np.UNKNOWN
    lx, ly, lt = volume_np.live_links(p["sides"], p["periodic"], p["state"])
    q["lap"] = np.where(unk, p["lap"], nan)
    if p["weight"] is not None:
        q["weight"] = np.where(unk, p["weight"], nan)
    else:
        q["data"] = np.where(unk, nan, p["data"])
    for name, live in (("gx", lx), ("gy", ly), ("gt", lt)):
        q[name] = np.where(live, p[name], nan)
    q["boundary"] = np.where(k == volume_np.DIRICHLET, p["boundary"], nan)
    q["state"] = np.where(k == volume_np.DIRICHLET, nan, p["state"])
    return {n: (a.astype(np.float32) if isinstance(a, np.ndarray) else a) for n, a in q.items()}


def call_args(p, form):
    """the keyword arguments of capi.Instance.volume / volume_np for an input in one of FORMS: (gx, gy, gt, lap)"""
    if form == "lap":
        return dict(gx=None, gy=None, gt=None, lap=p["lap"])
    return dict(gx=p["gx"], gy=p["gy"], gt=p["gt"] if form == "gt" else None, lap=None)


def np_args(p, form="lap"):
    """volume_np's positional arguments (sides .. lap) of an input; a guidance form: lap is volume_np.divergence of gx, gy (and gt)"""
    a = call_args(p, form)
    lap = a["lap"] if form == "lap" else volume_np.divergence(p["sides"], p["periodic"], p["state"], p["tau"], a["gx"], a["gy"], a["gt"])
    return p["sides"], p["periodic"], p["state"], p["weight"], p["tau"], p["data"], lap


def err_and_res(args, boundary, u, want):
    sides, periodic, state, weight, tau, data, lap = args
    k = volume_np.kinds(sides, periodic, state)
    unk = k == volume_np.UNKNOWN
    blk = (slice(None),) + volume_np.unknowns(sides, periodic, *k.shape[1:3])
    b = volume_np.folded_rhs(sides, periodic, state, weight, tau, data, lap, boundary)
    r = volume_np.residual(sides, periodic, state, weight, tau, u, data, lap, boundary)
    w = volume_np._thwc(np.asarray(want, np.float64))
    scale_u, scale_b = float(np.abs(w[unk]).max()), float(np.abs(b[unk[blk]]).max())
    err = float(np.abs(volume_np._thwc(np.asarray(u, np.float64)) - w)[unk].max()) / scale_u
    return err, (float(np.abs(r[unk[blk]]).max()) / scale_b if scale_b > 0 else 0.0)


class Yardstick:
    """One input's references: want = solve_exact, and pcg_f32's (ERR, RES, iterations) on it.  precond_lambda: the preconditioner's
    constant where it is not the input's own (a member of a batch: the chunk's)."""

    def __init__(self, p, form="lap", tol=1e-5, precond_lambda=None):
        self.args = np_args(p, form)
        self.boundary = p["boundary"] if volume_np.has_dirichlet(p["sides"], p["periodic"]) else None
        self.want = volume_np.solve_exact(*self.args, self.boundary)
        u32, self.iters32, self.rel32 = volume_np.pcg_f32(*self.args, self.boundary, tol=tol, max_iters=MAX_ITERS, precond_lambda=precond_lambda)
        self.err32, self.res32 = self.measure(u32)

    def measure(self, out):
        return err_and_res(self.args, self.boundary, out, self.want)

    def max_sweeps(self):
        return 2 * self.iters32 + POLL

    def bounds(self):
        return max(ERR_FACTOR * self.err32, ERR_FLOOR), max(RES_FACTOR * self.res32, RES_FLOOR)

    def check(self, out):
        """[(quantity, measured, bound)] that fail, and the measured (ERR, RES)"""
        err, res = self.measure(out)
        eb, rb = self.bounds()
        bad = ([("ERR", err, eb)] if not err <= eb else []) + ([("RES", res, rb)] if not res <= rb else [])
        return bad, err, res


@functools.lru_cache(maxsize=None)
def matrix_case(i):
    """(input, its form, its Yardstick) of matrix()[i], computed once per process and shared; nobody writes into them"""
    border, H, W, C, T, tau, pattern, wkind, form = matrix()[i]
    p = make_input(border, H, W, C, T, tau, pattern, wkind)
    return p, form, Yardstick(p, form)
