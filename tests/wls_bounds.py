"""The quantities the WLS GPU tests hold the library to, their bounds and their inputs (tests/test_gpu_wls.py), after the pattern of
tests/weighted_bounds.py with the variable-coefficient operator L of tests/wls_np.py in place of A - W:

    RES  max |L u - rhs| / max |rhs|        rhs = div(s g) - w d in the library's float32 order, the rest in float64
    ERR  max |u - solve_exact| / R,  R = max |solve_exact|

Bounds:  measured <= max(FACTOR x the same quantity for wls_np.pcg_f32 on the same input, FLOOR).  pcg_f32 is the same iteration with the
same preconditioner, start and stop rule, so both stop somewhere below tol; the library runs up to SC_WEIGHTED_POLL iterations longer
and adds its sums in another order.  The four constants come from one MI355X run of tools/wls_probe.py --lengths over a length walk and
the tests' own inputs (DESIGN.md section 4 holds the table, profiles/wls_lengths.txt the record): each factor is the worst ratio to the
restatement, times 2, rounded up to one digit; each floor twice the worst absolute value among the inputs where the restatement needed
no iteration at all (constant links and a constant weight: the error is one direct solve's, not the stop rule's).
Iterations:  sweeps <= 2 x pcg_f32's count + SC_WEIGHTED_POLL, both from the reference iteration."""
import numpy as np

import weighted_bounds as wb
import wls_np

POLL = wb.POLL
RES_FACTOR, RES_FLOOR = 20.0, 9.2e-7           # measured: worst ratio 6.13 (neumann 6 x 2, log-uniform links, sparse weights), worst value without an iteration 4.57e-7 (periodic x, 16 x 5)
ERR_FACTOR, ERR_FLOOR = 7.0, 7.1e-7            # measured: worst ratio 3.18 (the same input), worst value without an iteration 3.55e-7 (neumann 300 x 9)

BORDERS = wb.BORDERS
SIZES = [(47, 33), (5, 16), (7, 2), (9, 300)]  # rows x columns; 300 columns: the 256-column group boundary the west link is read across
LINKS = ["constant", "loguniform", "edges"]
WEIGHTS = ["constant", "sparse"]
MAX_ITERS = 400                                # sc_wls_params' default


def links(kind, shape, seed):
    """(smooth_x, smooth_y), float32, every element set.  constant: 0.7; loguniform: log-uniform in [1e-2, 1], independent per channel and
    axis; edges: 1 / (|forward difference|^1.2 + 0.01) of a checkerboard of 8-pixel squares (heights 0 and 1, its phase and the noise
    of sigma 0.05 on top seeded per channel) -- links of about 1 across the squares' edges and 10 to 100 inside them"""
    rng = np.random.default_rng(seed)
    H, W, C = shape
    if kind == "constant":
        return np.full(shape, 0.7, np.float32), np.full(shape, 0.7, np.float32)
    if kind == "loguniform":
        return tuple(np.exp(rng.uniform(np.log(1e-2), 0.0, shape)).astype(np.float32) for _ in range(2))
    if kind == "edges":
        y, x = np.mgrid[0:H, 0:W]
        img = np.stack([(((y + rng.integers(8)) // 8 + (x + rng.integers(8)) // 8) % 2).astype(np.float64) for _ in range(C)], 2)
        img += 0.05 * rng.standard_normal(shape)
        dx, dy = np.roll(img, -1, 1) - img, np.roll(img, -1, 0) - img
        return tuple((1.0 / (np.abs(d) ** 1.2 + 0.01)).astype(np.float32) for d in (dx, dy))
    raise ValueError(kind)


def dead_to_nan(sides, periodic, sx, sy):
    """copies of the link arrays with NaN in every element that is not live under these borders"""
    lx, ly = wls_np.live_links(sides, periodic, *sx.shape[:2])
    return (np.where(lx[:, :, None], sx, np.float32(np.nan)).astype(np.float32),
            np.where(ly[:, :, None], sy, np.float32(np.nan)).astype(np.float32))


def make_input(H, W, C, wkind, skind, seed=0):
    """(data, weight, smooth_x, smooth_y, lap, boundary), float32 H x W x C: weighted_bounds.make_input's arrays and links(skind)"""
    data, weight, lap, boundary = wb.make_input(H, W, C, wkind, seed)
    sx, sy = links(skind, (H, W, C), 2000 + seed + 3 * H + W)
    return data, weight, sx, sy, lap, boundary


def err_and_res(sides, periodic, weight, sx, sy, u, data, lap, want):
    f = np.abs(wls_np.rhs(sides, periodic, weight, data, lap).astype(np.float64)).max()
    return (float(np.abs(np.asarray(u, np.float64).reshape(want.shape) - want).max()) / float(np.abs(want).max()),
            float(np.abs(wls_np.residual(sides, periodic, weight, sx, sy, u, data, lap)).max()) / float(f))


class Yardstick:
    """One input's references: want = solve_exact, and pcg_f32's (ERR, RES, iterations) on it.  precond_lambda, precond_smooth: the
    preconditioner's constants where they are not the input's own means (a member of a batch: the chunk's)."""

    def __init__(self, sides, periodic, weight, sx, sy, data, lap, boundary, tol=1e-5, precond_lambda=None, precond_smooth=None):
        self.args = (sides, periodic, weight, sx, sy)
        self.data, self.lap = data, lap
        b = boundary if wls_np.has_dirichlet(sides, periodic) else None
        self.want = wls_np.solve_exact(sides, periodic, weight, sx, sy, data, lap, b)
        u32, self.iters32, self.rel32 = wls_np.pcg_f32(sides, periodic, weight, sx, sy, data, lap, b, tol=tol, max_iters=MAX_ITERS,
                                                       precond_lambda=precond_lambda, precond_smooth=precond_smooth)
        self.err32, self.res32 = self.measure(u32)

    def measure(self, out):
        return err_and_res(*self.args, out, self.data, self.lap, self.want)

    def max_sweeps(self):
        return 2 * self.iters32 + POLL

    def check(self, out):
        """[(quantity, measured, bound)] that fail, and the measured (ERR, RES)"""
        err, res = self.measure(out)
        eb, rb = max(ERR_FACTOR * self.err32, ERR_FLOOR), max(RES_FACTOR * self.res32, RES_FLOOR)
        bad = ([("ERR", err, eb)] if not err <= eb else []) + ([("RES", res, rb)] if not res <= rb else [])
        return bad, err, res
