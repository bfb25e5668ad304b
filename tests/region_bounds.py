"""The quantities the region GPU tests hold the library to, their bounds and their inputs (tests/test_gpu_region.py), after the pattern
of tests/wls_bounds.py with the masked operator of tests/region_np.py:

    ERR  max |u - solve_exact| / max |solve_exact|      both maxima over the UNKNOWN pixels
    RES  max |L u - b| / max |b|                         likewise; b the library's float32 right-hand side, the rest in float64

Bounds:  measured <= max(FACTOR x the same quantity for region_np.pcg_f32 on the same input, FLOOR).  pcg_f32 is the same iteration with
the same preconditioner, start and stop rule, so both stop somewhere below tol; the library runs up to SC_WEIGHTED_POLL iterations longer
and adds its sums in another order.  The four constants come from one MI355X run of tools/region_probe.py --lengths over a length walk
and the tests' own inputs (DESIGN.md section 4 holds the table, profiles/region_lengths.txt the record), by wls_bounds' rule: each
factor is the worst ratio to the restatement, times 2, rounded up to one digit; each floor twice the worst absolute value among the
inputs where the restatement needed no iteration at all.
Iterations:  sweeps <= 2 x pcg_f32's count + SC_WEIGHTED_POLL, both from the reference iteration."""
import numpy as np

import direct_np
import region_np
import weighted_bounds as wb
import wls_bounds as lb

POLL = wb.POLL
RES_FACTOR, RES_FLOOR = 5.0, 6.0e-7            # measured: worst ratio 2.12 (neumann 9 x 7, scatter, log-uniform links, no weight), worst value without an iteration 2.96e-7 (periodic xy, 2 x 7, every state 0)
ERR_FACTOR, ERR_FLOOR = 9.0, 7.1e-7            # measured: worst ratio 4.40 (neumann 2 x 7, scatter, log-uniform links, no weight), worst value without an iteration 3.55e-7 (neumann 300 x 9, every state 0)

BORDERS = wb.BORDERS
SIZES = [(47, 33), (5, 16), (9, 300), (7, 2)]  # rows x columns; 300 columns: the 256-column group boundary runs through a region
PATTERNS = ["ellipse", "scatter", "split", "seam"]
LINKS = [None, "constant", "loguniform"]       # None: no link arrays (every link 1)
WEIGHTS = [None, "constant", "sparse"]         # None: no data term
MAX_ITERS = 400                                # sc_region_params' default


def matrix():
    """the inputs of the GPU tests' walk (and of tools/region_probe.py): (border, H, W, C, pattern, wkind, skind, form).  Three channels:
    every border x size x pattern, links and weights rotating through LINKS and WEIGHTS and the right-hand side through its two forms
    (a frame around 2 x 7 pixels leaves no unknown and is left out).  One channel: every border x LINKS x WEIGHTS at 33 x 47, ellipse."""
    out = []
    for bi, (border, _, _) in enumerate(BORDERS):
        for si, (H, W) in enumerate(SIZES):
            if border == "frame" and min(H, W) < 3:
                continue
            for pi, pattern in enumerate(PATTERNS):
                i = bi + si + pi
                out.append((border, H, W, 3, pattern, WEIGHTS[i % 3], LINKS[(i // 3 + pi) % 3], "guidance" if (bi + pi) % 2 else "lap"))
        for li, skind in enumerate(LINKS):
            for wi, wkind in enumerate(WEIGHTS):
                out.append((border, 47, 33, 1, "ellipse", wkind, skind, "guidance" if (bi + li + wi) % 2 else "lap"))
    return out


def pattern_state(pattern, H, W, C, rng):
    y, x = np.mgrid[0:H, 0:W]
    st = np.zeros((H, W, C), np.float32)
    for c in range(C):
        if pattern == "ellipse":          # UNKNOWN inside, KNOWN outside; the centre moves a little with the channel
            cy, cx = (H - 1) / 2 + 0.3 * c, (W - 1) / 2 - 0.4 * c
            st[:, :, c] = np.where(((y - cy) / max(0.42 * H, 0.8)) ** 2 + ((x - cx) / max(0.42 * W, 0.8)) ** 2 <= 1.0, 0, 1)
        elif pattern == "scatter":        # about 1 in 30 KNOWN, plus an OUTSIDE blob
            st[:, :, c] = rng.random((H, W)) < 1 / 30
            by, bx, r = 0.3 * H + c, 0.65 * W - c, 0.18 * min(H, W)
            st[:, :, c][(y - by) ** 2 + (x - bx) ** 2 <= r * r] = 2
        elif pattern == "split":          # an OUTSIDE line cuts the domain in two (down the middle column, or across where there are
            if W >= 4:                    # too few columns), a few KNOWN pixels in each half
                st[:, W // 2 + (c % 2), c] = 2
            else:
                st[H // 2, :, c] = 2
            pins = rng.random((H, W)) < 1 / 12
            st[:, :, c][pins & (st[:, :, c] == 0)] = 1
        elif pattern == "seam":           # UNKNOWN in a band of rows towards both ends of x -- one region across the wrap of a periodic
            band = (y >= H // 5) & (y < H - H // 5 + (1 if H < 5 else 0))          # x axis --, KNOWN elsewhere
            st[:, :, c] = np.where(band & ((x < (W + 3) // 4) | (x >= W - (W + 3) // 4 - c % 2)), 0, 1)
        else:
            raise ValueError(pattern)
    return st


def states(pattern, sides, periodic, H, W, C, weight=None, seed=0):
    """state, float32 H x W x C, of one pattern under these borders, mended so that the input is a fair one: every channel has an UNKNOWN
    pixel inside the borders (else its centre pixel becomes one), and every UNKNOWN component is pinned (else its first pixel in reading
    order becomes KNOWN) -- region_np.unpinned_components then finds nothing (tests/test_region_host.py checks that)."""
    rng = np.random.default_rng(4000 + seed + 11 * H + W)
    st = pattern_state(pattern, H, W, C, rng)
    rows, cols = region_np.unknowns(sides, periodic, H, W)
    inside = ~direct_np.dirichlet_mask(sides, periodic, H, W)
    for c in range(C):
        if not ((st[:, :, c] == 0) & inside).any():
            st[(rows.start + rows.stop - 1) // 2, (cols.start + cols.stop - 1) // 2, c] = 0
    while True:
        loose = region_np.unpinned_components(sides, periodic, st, weight)
        if not loose.any():
            return st
        st[tuple(np.argwhere(loose)[0])] = 1


def make_input(border, H, W, C, pattern, wkind, skind, seed=0):
    """One input as a dict: sides, periodic, state, data, weight (None without wkind), sx, sy (None without skind), lap, gx, gy, boundary;
    float32 H x W x C, every element set (nan_unread() spoils the ones a call must not read)"""
    sides, periodic = {b[0]: b[1:] for b in BORDERS}[border]
    data, _, lap, boundary = wb.make_input(H, W, C, "constant", seed)
    weight = None if wkind is None else wb.weights(wkind, (H, W, C), 300 + seed + H)
    sx, sy = (None, None) if skind is None else lb.links(skind, (H, W, C), 2000 + seed + 3 * H + W)
    rng = np.random.default_rng(5000 + seed + 5 * H + W)
    gx, gy = (0.1 * rng.standard_normal((2, H, W, C))).astype(np.float32)
    state = states(pattern, sides, periodic, H, W, C, weight, seed)
    return dict(sides=sides, periodic=periodic, state=state, data=data, weight=weight, sx=sx, sy=sy, lap=lap, gx=gx, gy=gy, boundary=boundary)


def nan_unread(p):
    """a copy of the input with NaN in every element the header says is not read: weight and lap off the UNKNOWN pixels, links and
    guidance where the link is not live in the region, data at UNKNOWN pixels when there is no weight, boundary off its Dirichlet lines,
    state on them"""
    q = dict(p)
    nan = np.float32(np.nan)
    k = region_np.kinds(p["sides"], p["periodic"], p["state"])
    unk = k == region_np.UNKNOWN
    lx, ly = region_np.live_links(p["sides"], p["periodic"], p["state"])
    q["lap"] = np.where(unk, p["lap"], nan)
    if p["weight"] is not None:
        q["weight"] = np.where(unk, p["weight"], nan)
    else:
        q["data"] = np.where(unk, nan, p["data"])
    for name, live in (("sx", lx), ("gx", lx), ("sy", ly), ("gy", ly)):
        if p[name] is not None:
            q[name] = np.where(live, p[name], nan)
    q["boundary"] = np.where(k == region_np.DIRICHLET, p["boundary"], nan)
    q["state"] = np.where(k == region_np.DIRICHLET, nan, p["state"])
    return {n: (a.astype(np.float32) if isinstance(a, np.ndarray) else a) for n, a in q.items()}


def np_args(p, form="lap"):
    """region_np's positional arguments (sides .. lap) of an input; form "guidance": lap is region_np.divergence of gx, gy"""
    lap = p["lap"] if form == "lap" else region_np.divergence(p["sides"], p["periodic"], p["state"], p["sx"], p["sy"], p["gx"], p["gy"])
    return p["sides"], p["periodic"], p["state"], p["weight"], p["sx"], p["sy"], p["data"], lap


def err_and_res(args, boundary, u, want):
    sides, periodic, state, weight, sx, sy, data, lap = args
    k = region_np.kinds(sides, periodic, state)
    unk = k == region_np.UNKNOWN
    blk = region_np.unknowns(sides, periodic, *k.shape[:2])
    b = region_np.folded_rhs(sides, periodic, state, weight, sx, sy, data, lap, boundary)
    r = region_np.residual(sides, periodic, state, weight, sx, sy, u, data, lap, boundary)
    w = region_np._hwc(np.asarray(want, np.float64))
    scale_u, scale_b = float(np.abs(w[unk]).max()), float(np.abs(b[unk[blk]]).max())
    err = float(np.abs(region_np._hwc(np.asarray(u, np.float64)) - w)[unk].max()) / scale_u
    return err, (float(np.abs(r[unk[blk]]).max()) / scale_b if scale_b > 0 else 0.0)


class Yardstick:
    """One input's references: want = solve_exact, and pcg_f32's (ERR, RES, iterations) on it.  precond_lambda, precond_smooth: the
    preconditioner's constants where they are not the input's own (a member of a batch: the chunk's)."""

    def __init__(self, p, form="lap", tol=1e-5, precond_lambda=None, precond_smooth=None):
        self.args = np_args(p, form)
        self.boundary = p["boundary"] if region_np.has_dirichlet(p["sides"], p["periodic"]) else None
        self.want = region_np.solve_exact(*self.args, self.boundary)
        u32, self.iters32, self.rel32 = region_np.pcg_f32(*self.args, self.boundary, tol=tol, max_iters=MAX_ITERS,
                                                          precond_lambda=precond_lambda, precond_smooth=precond_smooth)
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
