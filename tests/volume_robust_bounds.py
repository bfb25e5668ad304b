"""The quantities the robust volume GPU tests hold the library to, their bounds and their inputs (tests/test_gpu_volume_robust.py), after
the pattern of tests/robust_bounds.py with the rounds of tests/volume_robust_np.py around the WLS volume solve.  Every run is ROUNDS = 4
fixed rounds (round_tol = -1) behind the quadratic one:

    ERR     max |u - irls_exact| / R        over the UNKNOWN pixels; u the last iterate, irls_exact the float64 rounds with exact inner
                                            solves, R the data's range
    RES     max |L u - b| / max |b|         of the last round's system: L and b from the iterate before the last (the library's own, read
                                            from a run of ROUNDS - 1 rounds, whose bytes are that iterate's)
    ENERGY  |sc_hip_robust_trace's last energy - volume_robust_np.energy of the written iterate| / that energy

Bounds:  ERR and RES <= max(FACTOR x the same quantity for volume_robust_np.irls_f32 on the same input, FLOOR); ENERGY <= ENERGY_REL.
irls_f32 is the same rounds with the same inner iteration, start and stop rule; the inner solves stop at tol = 1e-5 and the rounds carry
what they leave on, so ERR is of the order of 1e-5 of the range in both.  The constants come from one MI355X run of
tools/volume_robust_probe.py --lengths over matrix() and a length walk (DESIGN.md section 4 holds the table,
profiles/volume_robust_lengths.txt the record): each factor is twice the worst ratio to the restatement, rounded up to one digit; each
floor twice the worst value among the inputs where the restatement's figure is 0; ENERGY_REL twice the worst relative difference, rounded
up to one digit."""
import functools

import numpy as np

import volume_robust_np as vr
import volume_wls_bounds as vwb
import volume_wls_np as vw

ROUNDS = 4
ERR_FACTOR, ERR_FLOOR = 3.0, 0.0               # measured: worst ratio 1.04 (periodic xy 7 x 2, 8 frames x 3, tau 1, every state 0, periodic time, (1, 2, 1), eps 1e-3); no input where irls_f32's ERR is 0
RES_FACTOR, RES_FLOOR = 6.0, 0.0               # measured: worst ratio 2.72 (free left + top 7 x 3, 3 frames x 3, tau 1, split, sparse, links xy, periodic time, (1, 2, 1), eps 1e-3); no input where irls_f32's RES is 0
ENERGY_REL = 4e-7                              # measured: worst 1.50e-7 (neumann 3 x 6, 4 frames, tau 10, split, sparse, links t, (1.5, 0.8, 2), eps 1e-2)

BORDERS = vwb.BORDERS
SIZES = [(5, 260), (12, 19), (7, 2), (5, 16)]  # rows x columns: 260 columns cross the 256-column group; 12 x 19 under a frame: bands of 8 rows start anywhere in a frame; 7 x 2: under periodic x east and west are one pixel
FRAMES = vwb.FRAMES                            # 2 (free time only), 3, 5, 8
CHANNELS = vwb.CHANNELS
TAUS = vwb.TAUS
PATTERNS = vwb.PATTERNS
WEIGHTS = vwb.WEIGHTS
LINKS = vwb.LINKS
TIMES = vwb.TIMES
GT = [True, False]                             # the call carries gt, or NULL: zeros
EXPONENTS = [(1.0, 1.0, 2.0), (1.0, 2.0, 1.0), (1.5, 0.8, 2.0), (2.0, 1.0, 2.0)]          # (p, r, q): space, time, data
EPS = [1e-2, 1e-3]                             # times the data's range


def matrix():
    """the inputs of the GPU tests' walk (and of tools/volume_robust_probe.py): (border, H, W, C, T, tau, pattern, wkind, links, time, gt,
    exponents, eps factor).  Every border x size twice (a frame around 2 x 7 pixels leaves no unknown and is left out).  Every other axis
    takes the value (a bi + b si + c j) mod n of its n values -- bi, si the border's and the size's number, j the repetition -- with
    (a, b, c) chosen so that every value meets every border and every size; 2 frames go with free time.
    tests/test_volume_robust_host.py checks the coverage."""
    pick = lambda values, bi, si, j, a, b, c: values[(a * bi + b * si + c * j) % len(values)]
    out = []
    for bi, (border, _, _) in enumerate(BORDERS):
        for si, (H, W) in enumerate(SIZES):
            if border == "frame" and min(H, W) < 3:
                continue
            for j in range(2):
                T = pick(FRAMES, bi, si, j, 1, 1, 1)
                out.append((border, H, W, pick(CHANNELS, bi, si, j, 0, 1, 1), T, pick(TAUS, bi, si, j, 1, 1, 1), pick(PATTERNS, bi, si, j, 1, 1, 4),
                            pick(WEIGHTS, bi, si, j, 1, 2, 1), pick(LINKS, bi, si, j, 3, 1, 2),
                            "free" if T == 2 else pick(TIMES, bi, si, j, 1, 0, 1), pick(GT, bi, si, j, 1, 1, 1), pick(EXPONENTS, bi, si, j, 1, 1, 3),
                            pick(EPS, bi, si, j, 0, 1, 1)))
    return out


def make_input(border, H, W, C, T, tau, pattern, wkind, links="none", time="free", gt=True, seed=0):
    """One input as a dict: volume_wls_bounds.make_input's fields (gt None when the call carries none) and range, the data's range"""
    p = vwb.make_input(border, H, W, C, T, tau, pattern, wkind, links, time, seed)
    del p["lap"]
    if not gt:
        p["gt"] = None
    p["range"] = float(p["data"].max() - p["data"].min())
    return p


def nan_unread(p):
    """a copy of the input with NaN in every element the header says is not read (volume_wls_bounds.nan_unread's; there is no lap)"""
    T = p["state"].shape[0]
    gt = p["gt"] if p["gt"] is not None else np.zeros(((T if p["tper"] else T - 1),) + p["state"].shape[1:], np.float32)
    q = vwb.nan_unread(dict(p, gt=gt, lap=np.zeros_like(p["data"])))
    del q["lap"]
    if p["gt"] is None:
        q["gt"] = None
    return q


def penalties(p, exps, epsf):
    """pen of volume_robust_np: (p, r, q, eps_g, eps_t, eps_d), every eps epsf times the data's range, rounded to float32 as the call takes it"""
    eps = float(np.float32(epsf * p["range"]))
    return tuple(exps) + (eps, eps, eps)


def call_args(p, pen, **kw):
    """the arguments of capi.Instance.volume_robust for an input and its penalties"""
    b = p["boundary"] if vw.has_dirichlet(p["sides"], p["periodic"]) else None
    return dict(gx=p["gx"], gy=p["gy"], data=p["data"], state=p["state"], weight=p["weight"], smooth_x=p["sx"], smooth_y=p["sy"], smooth_t=p["smt"],
                gt=p["gt"], boundary=b, tau=p["tau"], loop=p["tper"], free_sides=p["sides"], periodic=p["periodic"], p_grad=pen[0], eps_grad=pen[3],
                p_time=pen[1], eps_time=pen[4], p_data=pen[2], eps_data=pen[5], **kw)


def _unknown(p):
    return vw.kinds(p["sides"], p["periodic"], p["state"]) == vw.UNKNOWN


class Yardstick:
    """One input's references: the exact rounds' iterates, and irls_f32's iterates with their (ERR, RES) round by round.  u32, iters32:
    where the restatement's rounds ran in a chunk with others (the batch test), that chunk's"""

    def __init__(self, p, pen, rounds=ROUNDS, u32=None, iters32=None):
        self.p, self.pen, self.rounds = p, pen, rounds
        self.unk = _unknown(p)
        self.exact = vr.irls_exact(p, pen, rounds)
        if u32 is None:
            u32, iters32 = vr.irls_f32(p, pen, rounds)
        self.u32, self.iters32 = u32, iters32
        self.fig32 = [self.measure(u32[k - 1] if k else None, u32[k], k) for k in range(len(u32))]
        self.err32, self.res32 = self.fig32[-1]

    def energy(self, u):
        return vr.energy(self.p, self.pen, u)

    def measure(self, prev, out, k=None):
        """(ERR, RES) of round k's iterate `out` (k None: the last round), `prev` the iterate before it (round 0: the caller's system)"""
        k = len(self.exact) - 1 if k is None else k
        want = self.exact[k]
        out = vw._thwc(np.asarray(out))
        err = float(np.abs(out.astype(np.float64) - want)[self.unk].max()) / self.p["range"]
        res = vr.round_residual(self.p, self.pen, prev, out) if k else self._res0(out)
        return err, res

    def _res0(self, out):
        args = vr.round_args(self.p)
        k = vw.kinds(self.p["sides"], self.p["periodic"], self.p["state"])
        blk = (slice(None),) + vw.unknowns(self.p["sides"], self.p["periodic"], *k.shape[1:3])
        unk = self.unk[blk]
        b = vw.folded_rhs(*args, vr._boundary(self.p))
        r = vw.residual(args, out, vr._boundary(self.p))
        scale = float(np.abs(b[unk]).max())
        return float(np.abs(r[unk]).max()) / scale if scale > 0 else 0.0

    def bounds(self, k=None):
        err32, res32 = self.fig32[-1 if k is None else k]
        return max(ERR_FACTOR * err32, ERR_FLOOR), max(RES_FACTOR * res32, RES_FLOOR)

    def check(self, prev, out, k=None):
        """[(quantity, measured, bound)] that fail, and the measured (ERR, RES)"""
        err, res = self.measure(prev, out, k)
        eb, rb = self.bounds(k)
        bad = ([("ERR", err, eb)] if not err <= eb else []) + ([("RES", res, rb)] if not res <= rb else [])
        return bad, err, res


@functools.lru_cache(maxsize=None)
def matrix_case(i):
    """(input, its penalties, its Yardstick) of matrix()[i], computed once per process and shared; nobody writes into them"""
    border, H, W, C, T, tau, pattern, wkind, links, time, gt, exps, epsf = matrix()[i]
    p = make_input(border, H, W, C, T, tau, pattern, wkind, links, time, gt)
    pen = penalties(p, exps, epsf)
    return p, pen, Yardstick(p, pen)


# ---- the outlier problem (tests/test_volume_robust_host.py, tests/test_gpu_volume_robust.py)
def outlier_problem(T, H, W, loop=False):
    """(problem, the true video): one channel, Neumann borders; the truth robust_bounds.clean_image per frame with a brightness that
    drifts with t; gx, gy, gt its exact wrapped differences with robust_bounds.corrupt's lattice in every frame and temporal outliers of
    +-0.5 at x mod 7 = 5, y mod 5 = 0 on every other temporal link (no two neighbouring pixels both touch a corrupted link); KNOWN pixels
    on a lattice of frame 0 only (x mod 6 = 2, y mod 4 = 1), no weight, no base links"""
    import robust_bounds as rb
    t = np.arange(T, dtype=np.float64)
    truth = np.stack([rb.clean_image(H, W, 1) + 0.05 * k for k in t])
    gx, gy = zip(*(rb.corrupt(*rb.forward_differences(f)) for f in truth))
    gt = np.roll(truth, -1, 0) - truth
    if loop:
        gt[T - 1] = truth[0] - truth[T - 1]
    y, x = np.mgrid[0:H, 0:W]
    spot = ((x % 7 == 5) & (y % 5 == 0))[None, :, :, None] & (np.arange(T) % 2 == 0)[:, None, None, None]
    sign = np.where((x + y) % 2 == 0, 1.0, -1.0)[None, :, :, None]
    gt = gt + 0.5 * sign * spot
    if not loop:
        gt = gt[:T - 1]
    state = np.zeros(truth.shape, np.float32)
    state[0, (y % 4 == 1) & (x % 6 == 2)] = 1
    p = dict(sides="lrtb", periodic="", tper=loop, state=state, weight=None, sx=None, sy=None, smt=None, tau=1.0, gx=np.stack(gx).astype(np.float32),
             gy=np.stack(gy).astype(np.float32), gt=gt.astype(np.float32), data=truth.astype(np.float32), boundary=truth.astype(np.float32),
             range=float(truth.max() - truth.min()))
    return p, truth
