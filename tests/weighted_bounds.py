"""The quantities the weighted GPU tests hold the library to, their bounds and their inputs (tests/test_gpu_weighted.py), after the
pattern of tests/direct_bounds.py with W = diag(w) in place of lambda:

    RES  max |(A - W) u - rhs| / max |rhs|        rhs = lap - w d in the library's float32 order, the rest in float64
    ERR  max |u - solve_exact| / R,  R = max |solve_exact|

Bounds:  measured <= max(FACTOR x the same quantity for weighted_np.pcg_f32 on the same input, FLOOR).  pcg_f32 is the same iteration
with the same stop rule, so both stop somewhere below tol; the library runs up to SC_WEIGHTED_POLL iterations longer and adds its sums
in another order.  The four constants come from one MI355X run of tools/weighted_probe.py --lengths over the length walk and the
tests' own inputs (DESIGN.md section 4 holds the table, profiles/weighted_lengths.txt the record): each factor is the worst ratio to
the restatement, times 2, rounded up to one digit; each floor twice the worst absolute value among the inputs where the restatement
needed no iteration at all (a constant weight: its error is one direct solve's, not the stop rule's).
Iterations:  sweeps <= 2 x pcg_f32's count + SC_WEIGHTED_POLL, both from the reference iteration."""
import numpy as np

import weighted_np

POLL = 4                                       # SC_WEIGHTED_POLL
RES_FACTOR, RES_FLOOR = 4.0, 8.7e-7            # measured: worst ratio 1.59 (neumann 6 x 2, sparse), worst value without an iteration 4.33e-7 (periodic x, 16 x 5)
ERR_FACTOR, ERR_FLOOR = 8.0, 2.9e-7            # measured: worst ratio 3.58 (neumann 6 x 2, log-uniform), worst value without an iteration 1.44e-7 (periodic xy, 2 x 7)

# (name, sides, periodic): Neumann, a frame, free left + top, periodic x with Dirichlet lines across y, periodic both ways
BORDERS = [("neumann", "lrtb", ""), ("frame", "", ""), ("free_lt", "lt", ""), ("periodic_x", "", "x"), ("periodic_xy", "", "xy")]
SIZES = [(47, 33), (5, 16), (7, 2)]            # rows x columns: 33 x 47, 16 x 5 and 2 x 7 pixels
WEIGHTS = ["constant", "loguniform", "sparse"]


def weights(kind, shape, seed):
    """constant 0.3; log-uniform in [1e-2, 1]; 1 on a seeded 10 % of the pixels (per channel), 0 elsewhere"""
    rng = np.random.default_rng(seed)
    if kind == "constant":
        return np.full(shape, 0.3, np.float32)
    if kind == "loguniform":
        return np.exp(rng.uniform(np.log(1e-2), 0.0, shape)).astype(np.float32)
    if kind == "sparse":
        return (rng.random(shape) < 0.1).astype(np.float32)
    if kind == "halfplane":
        w = np.zeros(shape, np.float32)
        w[:, :shape[1] // 2] = 1.0
        return w
    raise ValueError(kind)


# seeds of the sparse weights, fixed so that every channel of every size has a pixel set among its unknowns under every border
SPARSE_SEED = {(47, 33): 10, (5, 16): 10, (7, 2): 13}


def make_input(H, W, C, wkind, seed=0):
    """(data, weight, lap, boundary), float32 H x W x C: random data and boundary, lap the divergence of a small random guidance field"""
    rng = np.random.default_rng(1000 + seed + 7 * H + W)
    data = rng.standard_normal((H, W, C)).astype(np.float32)
    boundary = rng.standard_normal((H, W, C)).astype(np.float32)
    lap = (0.1 * rng.standard_normal((H, W, C))).astype(np.float32)
    wseed = SPARSE_SEED.get((H, W), 5) + seed if wkind == "sparse" else 100 + seed + H
    return data, weights(wkind, (H, W, C), wseed), lap, boundary


def err_and_res(sides, periodic, weight, u, data, lap, want):
    f = np.abs(weighted_np.rhs(sides, periodic, weight, data, lap).astype(np.float64)).max()
    return (float(np.abs(np.asarray(u, np.float64).reshape(want.shape) - want).max()) / float(np.abs(want).max()),
            float(np.abs(weighted_np.residual(sides, periodic, weight, u, data, lap)).max()) / float(f))


class Yardstick:
    """One input's references: want = solve_exact, and pcg_f32's (ERR, RES, iterations) on it.  precond_lambda: the preconditioner's
    constant where it is not the input's own mean weight (a member of a batch: the chunk's)."""

    def __init__(self, sides, periodic, weight, data, lap, boundary, tol=1e-5, precond_lambda=None):
        self.sides, self.periodic, self.weight, self.data, self.lap = sides, periodic, weight, data, lap
        b = boundary if weighted_np.has_dirichlet(sides, periodic) else None
        self.want = weighted_np.solve_exact(sides, periodic, weight, data, lap, b)
        u32, self.iters32, self.rel32 = weighted_np.pcg_f32(sides, periodic, weight, data, lap, b, tol=tol, precond_lambda=precond_lambda)
        self.err32, self.res32 = self.measure(u32)

    def measure(self, out):
        return err_and_res(self.sides, self.periodic, self.weight, out, self.data, self.lap, self.want)

    def max_sweeps(self):
        return 2 * self.iters32 + POLL

    def check(self, out):
        """[(quantity, measured, bound)] that fail, and the measured (ERR, RES)"""
        err, res = self.measure(out)
        eb, rb = max(ERR_FACTOR * self.err32, ERR_FLOOR), max(RES_FACTOR * self.res32, RES_FLOOR)
        bad = ([("ERR", err, eb)] if not err <= eb else []) + ([("RES", res, rb)] if not res <= rb else [])
        return bad, err, res
