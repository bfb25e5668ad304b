"""The test side's restatement of the bounded solve (sc_hip_bounded*), numpy only, built on region_np.

The problem is the region solve's (region_np's head comment: borders, state, links, the data term) under lower <= u <= upper at every
UNKNOWN pixel.  args is region_np's positional tuple (sides, periodic, state, weight, sx, sy, data, lap) -- region_bounds.np_args --,
lower and upper are numbers or arrays of data's shape (read at UNKNOWN pixels only; -inf / +inf: no bound).

The method is the library's, the primal-dual active set method: a round solves the region system in which the ACTIVE pixels are KNOWN
with data = their bound, then r = L u - b of the ORIGINAL system (region_np.residual on the original state: u of an active pixel is its
bound) decides the next set -- a free pixel with u > upper becomes upper-active, one with u < lower lower-active, an upper-active pixel
stays while r > 0, a lower-active one while r < 0, every other pixel is free -- until the set no longer changes.  r = - dE/du: at the
constrained minimiser r = 0 at pixels strictly inside their bounds, r >= 0 on the upper bound, r <= 0 on the lower (the KKT conditions).

solve_exact() runs the rounds with region_np.solve_exact (float64, direct) as the inner solve; pdas_f32() with region_np.pcg_f32, the
library's arithmetic and stop rule (each round cold-started: the yardstick of tests/bounded_bounds.py); kkt() measures an answer
against the three conditions; projected_gauss_seidel() is an independent solver for tiny inputs."""
from __future__ import annotations

import numpy as np

import region_np

_hwc = region_np._hwc
MAX_ROUNDS = 60


def _bounds(shape, lower, upper):
    """(lower, upper) as float64 H x W x C arrays holding the float32 values the library reads"""
    return tuple(np.broadcast_to(_hwc(np.asarray(b, np.float32)) if np.ndim(b) else np.float32(b), shape).astype(np.float64) for b in (lower, upper))


def _unknown(args):
    sides, periodic, state = args[:3]
    return region_np.kinds(sides, periodic, state) == region_np.UNKNOWN


def held_args(args, act, lo, hi):
    """args of the round's system: the pixels of `act` (+1 upper, -1 lower) KNOWN with data = their bound"""
    sides, periodic, state, weight, sx, sy, data, lap = args
    st = np.where(act != 0, np.float32(1), _hwc(np.asarray(state, np.float32)))
    d = np.where(act > 0, hi, np.where(act < 0, lo, _hwc(np.asarray(data, np.float32)))).astype(np.float32)
    return sides, periodic, st, weight, sx, sy, d, lap


def residual(args, boundary, u):
    """r = L u - b of the original system, float64 H x W x C, 0 where the pixel is not UNKNOWN"""
    sides, periodic, state = args[:3]
    k = region_np.kinds(sides, periodic, state)
    r = np.zeros(k.shape)
    r[region_np.unknowns(sides, periodic, *k.shape[:2])] = region_np.residual(*args[:6], u, *args[6:], boundary)
    return r


def next_set(act, unk, u, r, lo, hi):
    free = np.where(u > hi, 1, np.where(u < lo, -1, 0))
    kept = np.where(act > 0, np.where(r > 0, 1, 0), np.where(r < 0, -1, 0))
    return np.where(unk, np.where(act == 0, free, kept), 0)


def _rounds(args, boundary, lower, upper, inner, max_rounds):
    shape = _hwc(np.asarray(args[6])).shape
    lo, hi = _bounds(shape, lower, upper)
    unk = _unknown(args)
    assert (lo[unk] <= hi[unk]).all()
    act = np.zeros(shape, int)
    iters = []
    for rounds in range(1, max_rounds + 1):
        u, it = inner(held_args(args, act, lo, hi))
        u = _hwc(np.asarray(u, np.float64))
        iters.append(it)
        new = next_set(act, unk, u, residual(args, boundary, u), lo, hi)
        if (new == act).all():
            break
        act = new
    return np.where(unk, np.clip(u, lo, hi), u), act, rounds, iters


def solve_exact(args, boundary, lower, upper, max_rounds=MAX_ROUNDS):
    """(u, active set, rounds): float64, every round a direct solve.  u: H x W x C, composed like out; the set: +1 / -1 / 0; rounds: the
    solves it took, the one that confirmed the set included"""
    u, act, rounds, _ = _rounds(args, boundary, lower, upper, lambda a: (region_np.solve_exact(*a, boundary, dense=False), 0), max_rounds)
    return u, act, rounds


def pdas_f32(args, boundary, lower, upper, tol=1e-5, max_iters=400, max_rounds=MAX_ROUNDS):
    """(u, active set, rounds, inner iterations per round) with region_np.pcg_f32 as the inner solve"""
    def inner(a):
        u, it, _ = region_np.pcg_f32(*a, boundary, tol=tol, max_iters=max_iters)
        return u, it
    return _rounds(args, boundary, lower, upper, inner, max_rounds)


def kkt(args, boundary, u, lower, upper):
    """(RANGE, RES_FREE, SIGN) of an answer u (H x W x C or data's shape).  RANGE: the largest excursion outside [lower, upper] at
    UNKNOWN pixels, absolute.  RES_FREE: max |r| over the UNKNOWN pixels strictly inside both bounds.  SIGN: the largest wrong-signed r
    at pixels on a bound (a pixel on both at once may have any r).  The last two over max |b| of the original system."""
    sides, periodic, state, weight, sx, sy, data, lap = args
    u = _hwc(np.asarray(u, np.float64))
    lo, hi = _bounds(u.shape, lower, upper)
    unk = _unknown(args)
    if not unk.any():
        return 0.0, 0.0, 0.0
    r = residual(args, boundary, u)
    b = region_np.folded_rhs(sides, periodic, state, weight, sx, sy, data, lap, boundary)
    scale = float(np.abs(b).max())
    scale = scale if scale > 0 else 1.0
    rng = float(np.maximum(np.maximum(u - hi, lo - u), 0.0)[unk].max())
    inside = unk & (u > lo) & (u < hi)
    on_hi, on_lo = unk & (u == hi) & (lo < hi), unk & (u == lo) & (lo < hi)
    res_free = float(np.abs(r[inside]).max()) / scale if inside.any() else 0.0
    wrong = max(float(np.maximum(-r[on_hi], 0.0).max()) if on_hi.any() else 0.0, float(np.maximum(r[on_lo], 0.0).max()) if on_lo.any() else 0.0)
    return rng, res_free, wrong / scale


def projected_gauss_seidel(args, boundary, lower, upper, sweeps=100000, tol=1e-16):
    """The constrained minimiser by projected Gauss-Seidel in float64 (tiny inputs only: a Python loop over the UNKNOWN pixels): every
    pixel in turn takes the value that zeroes its own residual, clipped into its bounds.  H x W x C, composed like out."""
    sides, periodic, state, weight, sx, sy, data, lap = args
    k = region_np.kinds(sides, periodic, state)
    H, W, C = k.shape
    lo, hi = _bounds(k.shape, lower, upper)
    west, east, north, south = region_np._links(sides, periodic, state, sx, sy, np.float64)
    w = np.zeros(k.shape) if weight is None else _hwc(np.asarray(weight, np.float64))
    d = _hwc(np.asarray(data, np.float64))
    # lap - w d as the library takes it: in float32 (region_np.folded_rhs)
    f = _hwc(np.asarray(lap, np.float32))
    if weight is not None:
        f = f - _hwc(np.asarray(weight, np.float32)) * _hwc(np.asarray(data, np.float32))
    f = f.astype(np.float64)
    u = d.copy()
    if region_np.has_dirichlet(sides, periodic):
        line = k == region_np.DIRICHLET
        u[line] = _hwc(np.asarray(boundary, np.float64))[line]
    unk = k == region_np.UNKNOWN
    u[unk] = np.clip(0.0, lo[unk], hi[unk])
    pix = [tuple(p) for p in np.argwhere(unk)]
    for _ in range(sweeps):
        change = 0.0
        for y, x, c in pix:
            num, den = -f[y, x, c], w[y, x, c]
            for s, yy, xx in ((west[y, x, c], y, (x - 1) % W), (east[y, x, c], y, (x + 1) % W), (north[y, x, c], (y - 1) % H, x),
                              (south[y, x, c], (y + 1) % H, x)):
                if s != 0:
                    num += s * u[yy, xx, c]
                    den += s
            v = min(max(num / den, lo[y, x, c]), hi[y, x, c])
            change = max(change, abs(v - u[y, x, c]))
            u[y, x, c] = v
        if change <= tol:
            break
    return u
