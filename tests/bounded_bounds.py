"""The quantities the bounded GPU tests hold the library to, their bounds and their inputs (tests/test_gpu_bounded.py), after the pattern
of tests/region_bounds.py with the rounds of tests/bounded_np.py:

    ERR       max |u - solve_exact| / max |solve_exact|     both maxima over the UNKNOWN pixels; solve_exact: bounded_np's, float64
    RES_FREE  max |L u - b| / max |b| over the UNKNOWN pixels strictly inside both bounds          (bounded_np.kkt)
    SIGN      the largest wrong-signed L u - b at a pixel on a bound / max |b|                      (bounded_np.kkt)

Conditions, not measurements: RANGE (the largest excursion outside the bounds) == 0 exactly; converged == 1; the library's rounds <= 2 x
the float64 reference's + 2 (under inner solves perturbed by 1e-5 of their norm the float64 method needed at most two rounds more than
with exact ones); every input of the matrix needs at most MAX_REFERENCE_ROUNDS reference rounds (tests/test_bounded_host.py checks it).

Measured bounds:  measured <= max(FACTOR x the same quantity for bounded_np.pdas_f32 on the same input, FLOOR).  pdas_f32 is the same
method with the library's inner iteration, preconditioner and stop rule (cold-started every round, where the library starts warm), so
both end with inner residuals somewhere below tol.  The constants come from one MI355X run of tools/bounded_probe.py --lengths over the
matrix and a length walk (DESIGN.md section 4 holds the table, profiles/bounded_lengths.txt the record), by wls_bounds' rule: each
factor is the worst ratio to the yardstick, times 2, rounded up to one digit; each floor twice the worst absolute value among the
inputs where the yardstick's quantity is 0 or it needed no iteration at all."""
import functools

import numpy as np

import bounded_np
import region_bounds as rb
import region_np

ERR_FACTOR, ERR_FLOOR = 5.0, 0.0              # measured: worst ratio 2.01 (neumann 32 x 9, scatter, no links, no weight, guidance, arrays); the yardstick iterated and erred on every input: no floor
RES_FACTOR, RES_FLOOR = 2.0, 0.0              # measured: worst ratio 0.753 (neumann 300 x 9, scatter, log-uniform links, no weight, guidance, upper); likewise no floor
SIGN_FACTOR, SIGN_FLOOR = 2.0, 0.0            # measured: 0 on all 140 inputs, library and yardstick alike: no ratio to take (the factor is RES_FREE's), twice the worst value is 0

SIZES = [(47, 33), (5, 16), (9, 300)]          # rows x columns; 300 columns: the 256-column group boundary runs through the region and the contact set
BOUNDS = ["both", "upper", "lower", "arrays"]
MAX_REFERENCE_ROUNDS = 10
MAX_ROUNDS = 30                                # sc_bounded_params' default


def matrix():
    """the inputs of the GPU tests' walk (and of tools/bounded_probe.py): (border, H, W, C, pattern, wkind, skind, form, bkind).  Three
    channels: every border x size x pattern, with links, weights, the right-hand side's form and the bound kind rotating.  One channel:
    every border x bound kind at 33 x 47, scatter."""
    out = []
    for bi, (border, _, _) in enumerate(rb.BORDERS):
        for si, (H, W) in enumerate(SIZES):
            for pi, pattern in enumerate(rb.PATTERNS):
                i = bi + si + pi
                out.append((border, H, W, 3, pattern, rb.WEIGHTS[i % 3], rb.LINKS[(i // 3 + pi) % 3], "guidance" if (bi + pi) % 2 else "lap",
                            BOUNDS[(bi + 2 * si + pi) % 4]))
        for ki, bkind in enumerate(BOUNDS):
            out.append((border, 47, 33, 1, "scatter", rb.WEIGHTS[(bi + ki) % 3], rb.LINKS[ki % 3], "guidance" if (bi + ki) % 2 else "lap", bkind))
    return out


def case_id(case):
    b, H, W, C, p, wk, sk, f, bk = case
    return f"{b}-{W}x{H}x{C}-{p}-{wk}-{sk}-{f}-{bk}"


def make_bounds(bkind, args, boundary):
    """(lower, upper) of one kind for an input: the 0.25 / 0.75 quantiles over the UNKNOWN pixels of its float64 unconstrained answer,
    as float32 -- both, one side only (the other infinite), or per-pixel arrays: the quantile plus a ramp across x of a fifth of the
    quartiles' distance"""
    sides, periodic, state = args[:3]
    unk = region_np.kinds(sides, periodic, state) == region_np.UNKNOWN
    free = region_np._hwc(region_np.solve_exact(*args, boundary, dense=False))
    q25, q75 = (np.float32(q) for q in np.quantile(free[unk], (0.25, 0.75)))
    if bkind == "both":
        return q25, q75
    if bkind == "upper":
        return np.float32(-np.inf), q75
    if bkind == "lower":
        return q25, np.float32(np.inf)
    W = unk.shape[1]
    ramp = (np.float32(0.2) * (q75 - q25) * (np.arange(W, dtype=np.float32) / np.float32(max(W - 1, 1)) - np.float32(0.5)))[None, :, None]
    return (np.broadcast_to(q25 + ramp, unk.shape).astype(np.float32), np.broadcast_to(q75 + ramp, unk.shape).astype(np.float32))


def nan_unread_bounds(p, lower, upper):
    """bound arrays with NaN wherever the header says they are not read: everywhere but the UNKNOWN pixels"""
    unk = region_np.kinds(p["sides"], p["periodic"], p["state"]) == region_np.UNKNOWN
    return tuple(np.where(unk, b, np.float32(np.nan)).astype(np.float32) if np.ndim(b) else b for b in (lower, upper))


class Yardstick:
    """One input's references: want, set, rounds = bounded_np.solve_exact, and pdas_f32's (ERR, RES_FREE, SIGN, rounds, inner
    iterations) on it."""

    def __init__(self, p, form, bkind=None, bounds=None, f32=True):
        self.args = rb.np_args(p, form)
        self.boundary = p["boundary"] if region_np.has_dirichlet(p["sides"], p["periodic"]) else None
        self.lower, self.upper = bounds if bounds is not None else make_bounds(bkind, self.args, self.boundary)
        self.want, self.set, self.rounds = bounded_np.solve_exact(self.args, self.boundary, self.lower, self.upper)
        self.unk = region_np.kinds(*self.args[:3]) == region_np.UNKNOWN
        if f32:
            u32, _, self.rounds32, self.iters32 = bounded_np.pdas_f32(self.args, self.boundary, self.lower, self.upper, max_iters=rb.MAX_ITERS)
            self.err32, self.res32, self.sign32 = self.measure(u32)[1:]

    def measure(self, out):
        """(RANGE, ERR, RES_FREE, SIGN) of an answer"""
        u = region_np._hwc(np.asarray(out, np.float64))
        rng, res, sign = bounded_np.kkt(self.args, self.boundary, u, self.lower, self.upper)
        scale = float(np.abs(self.want[self.unk]).max())
        return rng, float(np.abs(u - self.want)[self.unk].max()) / (scale if scale > 0 else 1.0), res, sign

    def max_rounds(self):
        return 2 * self.rounds + 2

    def bounds(self):
        return (max(ERR_FACTOR * self.err32, ERR_FLOOR), max(RES_FACTOR * self.res32, RES_FLOOR), max(SIGN_FACTOR * self.sign32, SIGN_FLOOR))

    def check(self, out):
        """[(quantity, measured, bound)] that fail, and the measured (RANGE, ERR, RES_FREE, SIGN)"""
        m = self.measure(out)
        bad = [("RANGE", m[0], 0.0)] if m[0] != 0.0 else []
        bad += [(n, v, b) for n, v, b in zip(("ERR", "RES_FREE", "SIGN"), m[1:], self.bounds()) if not v <= b]
        return bad, m


@functools.lru_cache(maxsize=None)
def case_input(case, nan=True, f32=True):
    """(input dict with lower / upper, its Yardstick) of one case of the matrix; nan: NaN in every element that is not read"""
    border, H, W, C, pattern, wk, sk, form, bkind = case
    p = rb.make_input(border, H, W, C, pattern, wk, sk)
    if nan:
        p = rb.nan_unread(p)
    y = Yardstick(p, form, bkind, f32=f32)
    p["lower"], p["upper"] = nan_unread_bounds(p, y.lower, y.upper) if nan else (y.lower, y.upper)
    return p, y
