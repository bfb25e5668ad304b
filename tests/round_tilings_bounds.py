"""The robust volume, coupled volume, robust region and bounded families at the tilings of their work planes (csrc/sc_pcg.hip: pcg_geo)
that none of their own tests launches: the shapes, the cases and the regime facts of tests/test_gpu_round_tilings.py,
tests/test_round_tilings_host.py and tools/round_tilings_probe.py.

    three groups      9 x 601 unknowns        a column group with a neighbour group on both sides (pcg_steps_bounds.SHAPES)
    many parts        2101 x 5                234 parts per plane: every round's sums, esum and the bounded counts are folded over 234
    stacked frames    64 frames of 33 x 5     235 bands of 9 rows that start at every offset inside a frame; C = 3: 192 planes, one chunk
    long time         17 frames of 7 x 6      T * T > 256: k_volume_tables' stride loop, run again by every round's new means
    wide frames       3 frames of 3 x 601     three column groups beside bands of 5 rows that straddle frames of 3 (this file's own)

The bounds are the families' own, unchanged: volume_robust_bounds' 3 / 6 / 4e-7, volume_coupled_bounds' 4 / 9 / 4e-7,
region_robust_bounds' 3 / 6 / 4e-7 and bounded_bounds' ERR 5, RES_FREE 2 -- ratios to the float32 restatement on the same input, so they
scale with the shape.  Every run is ROUNDS = 3 fixed rounds (round_tol = -1) behind the quadratic one, held round by round.

One yardstick is this file's own.  s-bar, t-bar and w-bar only steer the preconditioner, and a round whose inner solve converges lands
on the same iterate whatever they were: no ERR or RES sees a part left out of a round's sums.  CAPPED runs do: max_iters = CAP <
SC_WEIGHTED_POLL inner iterations per round (no norm is read before a solve stops, the rounds go on from its last iterate), one round,
and pcg_steps_bounds' distance D = max |u - u64| / max |u64| over the UNKNOWN pixels to the float64 twin of that round
(capped_round(dtype=float64): from the same float32 iterate u_0 of the capped quadratic round, the same float32 links, weights and
means, the same CAP warm steps without the vectors' rounding), under pcg_steps_bounds' own rule and constant: D <= STEP_FACTOR x D of
capped_round(dtype=float32).  On the device u_0 is the region call's output with max_iters = CAP, the quadratic round's bytes.
tests/test_round_tilings_host.py holds the sharpness of both kinds of bound."""
import functools

import numpy as np

import pcg_steps_bounds as sb
import region_np
import region_robust_bounds as gr
import region_robust_np as rr
import volume_coupled_bounds as cb
import volume_coupled_np as vc
import volume_robust_bounds as rb
import weighted_np
import wls_np

ROUNDS = 3
CAP = 3                                        # inner iterations per round of a capped run: below SC_WEIGHTED_POLL
STEP_FACTOR = sb.STEP_FACTOR

SHAPES = {name: sb.SHAPES[name] for name in ("three_groups", "many_parts", "stacked_frames", "long_time")}
SHAPES["wide_frames"] = (3, 601, 3)            # rows, columns of a frame's unknown block, frames
VOLUME_SHAPES = ("stacked_frames", "long_time", "wide_frames")
PLANE_SHAPES = ("three_groups", "many_parts")
image_size = sb.image_size
BORDERS = sb.BORDERS
S, T, J = vc.SPACE, vc.TIME, vc.CHANNELS
COUPLINGS = (0,) + tuple(vc.LEGAL)             # 0: through sc_hip_volume_robust


def regime(shape, plan):
    """the facts of sc_hip_pcg_plan's answer (capi.pcg_plan) a shape is there for, as [(fact, holds)]"""
    if shape != "wide_frames":
        return sb.regime(shape, plan)
    ny, nx, frames = SHAPES[shape]
    return [("the unknown block", (plan["nx"], plan["ny"]) == (nx, ny * frames)), ("cg == 3", plan["cg"] == 3),
            ("rows does not divide a frame", ny % plan["rows"] != 0 and plan["rows"] % ny != 0), ("bands >= 2", plan["bands"] >= 2),
            ("n % 4 == 1", (plan["nx"] * plan["ny"]) % 4 == 1)]


# ---- a. robust and coupled volumes ------------------------------------------------------------------------------------------------------
VOLUME_BORDERS = {"stacked_frames": ("neumann", "free_lt"), "long_time": ("neumann", "free_lt"), "wide_frames": ("neumann", "free_lt", "periodic_x")}
TIMES = ("free", "periodic")
TAUS = (1.0, 0.1, 10.0)
EPS = (1e-2, 1e-3)


def volume_matrix():
    """[(shape, border, time, coupling, C, exponents, eps factor, tau)]: every coupling (0: the uncoupled call) at every shape, the
    shape's borders and the two kinds of time rotating against it -- case n of a shape takes border n mod its borders, time (n + n // 2)
    mod 2 --, then two more per shape with the border and the time the rotation has not paired with a form of CHANNELS.  Scatter states
    (they differ between the channels), sparse weights, log-uniform links in x, y and t, gt carried; exponents, eps (1e-2 or 1e-3 of the
    range; 1e-2 at stacked frames) and tau rotating, every exponent of a gradient term below 2 so that every form is effective.  C = 3
    throughout: a stacked-frames volume is 192 planes, exactly one chunk."""
    out = []
    for si, shape in enumerate(VOLUME_SHAPES):
        borders = VOLUME_BORDERS[shape]
        rows = []
        for n, cpl in enumerate(COUPLINGS + (S | J, S | T | J)):
            b, t = (n + si) % len(borders), (n + n // 2 + si) % 2
            if n >= len(COUPLINGS):            # the two extra cases: the other time of the same form's first appearance, the next border
                first = next(r for r in rows if r[3] == cpl)
                b, t = (borders.index(first[1]) + 1) % len(borders), 1 - TIMES.index(first[2])
            exps = cb.TIME_EXPONENTS[(n + si) % 3] if cpl & T else cb.EXPONENTS[(n + si) % 3]          # (p < 2: every form is effective)
            # (stacked frames: eps 1e-2 throughout -- at 31 680 unknowns the restatement's inner iterations are the test's time, and eps
            # 1e-3 triples them)
            epsf = EPS[0] if shape == "stacked_frames" else CHANGED_EPS.get((shape, borders[b], TIMES[t], cpl), EPS[(n + si) % 2])
            rows.append((shape, borders[b], TIMES[t], cpl, 3, exps, epsf, TAUS[(n + si) % 3]))
        out += rows
    return out


# The one input the rotation gave that broke a condition of the GPU tests (tests/test_round_tilings_host.py: every inner solve of the
# restatement ends before max_iters = 400): wide frames, periodic x, free time, CHANNELS, (1.5, 0.8, 2), tau 10 with eps 1e-3 of the
# range -- rounds 2 and 3 of irls_f32 ran 395 and 400 iterations (r = 0.8 at eps 1e-3 spreads the temporal links over four decades,
# times tau 10).  Its eps is 1e-2; nothing else of it changed.
CHANGED_EPS = {("wide_frames", "periodic_x", "free", J): 1e-2}


def volume_id(case):
    shape, border, time, cpl, C, exps, epsf, tau = case
    return f"{shape}-{border}-{time}-{vc.NAMES[cpl]}-p{exps[0]:g}r{exps[1]:g}q{exps[2]:g}-eps{epsf:g}-tau{tau:g}"


def volume_input(shape, border, time, C, tau, seed=0):
    ny, nx, frames = SHAPES[shape]
    H, W = image_size(border, ny, nx)
    return rb.make_input(border, H, W, C, frames, tau, "scatter", "sparse", "xyt", time, True, seed)


def volume_yardstick(p, pen, coupling, **kw):
    return cb.Yardstick(p, pen, coupling, rounds=ROUNDS, **kw) if coupling else rb.Yardstick(p, pen, rounds=ROUNDS, **kw)


@functools.lru_cache(maxsize=None)
def volume_case(i):
    """(input, its penalties, its coupling, its Yardstick over ROUNDS rounds) of volume_matrix()[i], made once per process; nobody writes
    into them"""
    shape, border, time, cpl, C, exps, epsf, tau = volume_matrix()[i]
    p = volume_input(shape, border, time, C, tau)
    pen = rb.penalties(p, exps, epsf)
    return p, pen, cpl, volume_yardstick(p, pen, cpl)


# ---- b. robust regions -----------------------------------------------------------------------------------------------------------------
REGION_BORDERS = ("neumann", "frame", "periodic_xy")
REGION_PATTERNS = ("scatter", "split")


def region_matrix():
    """[(shape, border, pattern, coupling, exponents, eps factor)]: the two plane shapes under three borders twice; coupling (bi + 2 j +
    si) mod 4 -- all four at either shape --, the pattern (bi + j + si) mod 2; three channels, sparse weights, log-uniform links"""
    out = []
    for si, shape in enumerate(PLANE_SHAPES):
        for bi, border in enumerate(REGION_BORDERS):
            for j in range(2):
                out.append((shape, border, REGION_PATTERNS[(bi + j + si) % 2], gr.COUPLINGS[(bi + 2 * j + si) % 4], gr.EXPONENTS[(bi + j + 2 * si) % 4],
                            EPS[(bi + j) % 2]))
    return out


def region_id(case):
    shape, border, pattern, cpl, exps, epsf = case
    return f"{shape}-{border}-{pattern}-coupling{cpl}-p{exps[0]:g}q{exps[1]:g}-eps{epsf:g}"


def region_input(shape, border, pattern, seed=0):
    ny, nx, _ = SHAPES[shape]
    H, W = image_size(border, ny, nx)
    return gr.make_input(border, H, W, 3, pattern, "sparse", "loguniform", seed)


@functools.lru_cache(maxsize=None)
def region_case(i):
    """(input, its penalties, its coupling, its Yardstick over ROUNDS rounds) of region_matrix()[i], made once per process"""
    shape, border, pattern, cpl, exps, epsf = region_matrix()[i]
    p = region_input(shape, border, pattern)
    pen = gr.penalties(p, exps, epsf)
    return p, pen, cpl, gr.Yardstick(p, pen, cpl, rounds=ROUNDS)


# ---- c. bounded regions ----------------------------------------------------------------------------------------------------------------
BOUNDED_BORDERS = ("neumann", "frame", "free_lt", "periodic_x")


def bounded_matrix():
    """bounded_bounds' case tuples (border, H, W, C, pattern, wkind, skind, form, bkind): the two plane shapes under four borders, the
    bound forms `both` and `arrays`, the patterns and the right-hand side's form alternating; three channels, sparse weights, log-uniform
    links"""
    out = []
    for si, shape in enumerate(PLANE_SHAPES):
        ny, nx, _ = SHAPES[shape]
        for bi, border in enumerate(BOUNDED_BORDERS):
            H, W = image_size(border, ny, nx)
            out.append((border, H, W, 3, REGION_PATTERNS[(bi + si) % 2], "sparse", "loguniform", ("guidance", "lap")[(bi // 2 + si) % 2],
                        ("both", "arrays")[bi % 2]))
    return out


def bounded_shape(case):
    """the name of the shape a bounded case's unknown block has"""
    return next(name for name in PLANE_SHAPES if image_size(case[0], *SHAPES[name][:2]) == (case[1], case[2]))


def violated(p, y):
    """(how many UNKNOWN pixels of the unconstrained float64 answer lie outside the bounds, how many of all UNKNOWN pixels lie within
    `slack` of a bound they are inside of or outside of -- the pixels an answer within the ERR bound of the reference may put on the
    other side), slack = y's ERR bound in the answer's units"""
    free = region_np._hwc(region_np.solve_exact(*y.args, y.boundary, dense=False))
    lo, hi = (np.broadcast_to(np.asarray(b, np.float64), free.shape) for b in (y.lower, y.upper))
    slack = y.bounds()[0] * float(np.abs(y.want[y.unk]).max())
    out = ((free > hi) | (free < lo)) & y.unk
    near = (np.minimum(np.abs(free - lo), np.abs(free - hi)) <= slack) & y.unk
    return int(out.sum()), int(near.sum())


# ---- capped rounds (the regions: the sums of 234 parts steer only the preconditioner) -----------------------------------------------------
def _warm(args, boundary, means, u, iters, dtype):
    """region_robust_np._warm_round in dtype, exactly `iters` iterations (no norm read): the next composed iterate"""
    sides, periodic, state, weight, sx, sy, data, lap = args
    k = region_np.kinds(sides, periodic, state)
    H, W, C = k.shape
    blk = region_np.unknowns(sides, periodic, H, W)
    links, dg = region_np._planes(sides, periodic, state, weight, sx, sy, dtype)
    sbar, wbar = means
    lam = dtype(np.float32(wbar / sbar))
    b = region_np.folded_rhs(sides, periodic, state, weight, sx, sy, data, lap, boundary, dtype)
    x = np.where(k[blk] == region_np.UNKNOWN, region_np._hwc(np.asarray(u, dtype))[blk], dtype(0))
    dot = lambda a, c: np.einsum("yxc,yxc->c", a.astype(np.float64), c.astype(np.float64))
    apply = lambda v: wls_np.block_operator(links, dg, v)
    precond = lambda r: weighted_np._precond(sides, periodic, lam, r, (H, W, C), dtype)
    div = lambda a, c: np.where(c != 0, a / np.where(c != 0, c, 1.0), 0.0).astype(dtype)
    r = b - apply(x)
    z = precond(r)
    pp, rz = z.copy(), dot(r, z)
    for _ in range(iters):
        qq = apply(pp)
        alpha = div(rz, dot(pp, qq))
        x, r = x + alpha * pp, r - alpha * qq
        z = precond(r)
        rz_new = dot(r, z)
        pp, rz = z + div(rz_new, rz) * pp, rz_new
        assert x.dtype == dtype and pp.dtype == dtype
    return region_np._hwc(region_np._compose(sides, periodic, state, data, boundary, x, dtype))


def capped_start(p, cap=CAP):
    """iterate `cap` of the quadratic round in the restatement's float32 (region_np.pcg from its cold start), composed like out"""
    keep = []
    region_np.pcg(*rr.round_args(p), rr._boundary(p), 0.0, cap, None, None, np.float32, keep)
    return region_np._hwc(keep[-1])


def capped_round(p, pen, coupling, u0, dtype, sbar_factor=1.0, cap=CAP):
    """round 1 of a robust region call with max_iters = cap, from the float32 iterate u0 the capped quadratic round left: the system
    u0 gives, float32 links and weights as the call forms them, under that system's own means, and `cap` warm iterations of it on
    vectors of dtype.  sbar_factor: on s-bar (the sharpness condition: a part left out of the sum)."""
    args = rr.round_args(p, pen, np.asarray(u0, np.float32), coupling)
    sbar, wbar = rr.chunk_means([args])
    return _warm(args, rr._boundary(p), (sbar_factor * sbar, wbar), u0, cap, dtype)


def capped_bound(p, pen, coupling, u0):
    """(the float64 twin's round-1 iterate from u0, the bound on D: STEP_FACTOR x D of the float32 restatement's)"""
    u64 = capped_round(p, pen, coupling, u0, np.float64)
    return u64, STEP_FACTOR * distance(p, capped_round(p, pen, coupling, u0, np.float32), u64)


def distance(p, u, u64):
    """pcg_steps_bounds' D of an iterate against the float64 one, over the UNKNOWN pixels"""
    m = region_np.kinds(p["sides"], p["periodic"], p["state"]) == region_np.UNKNOWN
    u, u64 = (region_np._hwc(np.asarray(a, np.float64)) for a in (u, u64))
    return float(np.abs(u - u64)[m].max()) / float(np.abs(u64[m]).max())


# the capped runs: many parts, no coupling and both couplings
CAPPED = [next(i for i, c in enumerate(region_matrix()) if c[0] == "many_parts" and c[3] == cpl) for cpl in (0, 3)]


# ---- d, e. chunks of volumes -------------------------------------------------------------------------------------------------------------
SMALL = ("neumann", 5, 16, 3)                  # border, H, W, C of the batch members


def batch_inputs(n, frames, time="free", scale_last=True):
    """n volumes of `frames` frames of 5 x 16 x 3 under Neumann borders, seeds 30 .. 30 + n - 1, scatter, sparse weights, links in x, y
    and t; the last member's data, guidance and boundary are member 0's times 3 with its own state, weight and links (scale_last), so a
    rho or an energy read from another member's table shows: the same residual pattern at three times the size has other rho"""
    probs = [rb.make_input(*SMALL, frames, 1.0, "scatter", "sparse", "xyt", time, True, 30 + k) for k in range(n)]
    if scale_last:
        last = dict(probs[-1])
        for name in ("data", "gx", "gy", "gt", "boundary"):
            last[name] = (np.float32(3) * probs[0][name]).astype(np.float32)
        last["range"] = float(last["data"].max() - last["data"].min())
        probs[-1] = last
    return probs
