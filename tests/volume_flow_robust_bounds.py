"""The quantities the robust flow volume GPU tests hold the library to, their bounds and their inputs
(tests/test_gpu_volume_flow_robust.py), after the pattern of tests/volume_robust_bounds.py with the rounds of
tests/volume_flow_robust_np.py around the flow volume solve.  Every run is ROUNDS = 4 fixed rounds (round_tol = -1) behind the
quadratic one:

    ERR     max |u - irls_exact| / R        over the UNKNOWN pixels; u the last iterate, irls_exact the float64 rounds with exact inner
                                            solves, R the data's range
    RES     max |L u - b| / max |b|         of the last round's system: L and b from the iterate before the last (the library's own, read
                                            from a run of ROUNDS - 1 rounds, whose bytes are that iterate's)
    ENERGY  |sc_hip_robust_trace's last energy - volume_flow_robust_np.energy of the written iterate| / that energy

Bounds:  ERR and RES <= max(FACTOR x the same quantity for volume_flow_robust_np.irls_f32 on the same input, FLOOR); ENERGY <=
ENERGY_REL.  irls_f32 is the same rounds with the same inner iteration, (straight-link) preconditioner, start and stop rule.  The
constants come from one MI355X run of tools/volume_flow_robust_probe.py --lengths over matrix() and a length walk (DESIGN.md section 4
holds the table, profiles/volume_flow_robust_lengths.txt the record), by the project's rule: each factor is twice the worst ratio to the
restatement, rounded up to one digit; each floor twice the worst value among the inputs where the restatement's figure is 0; ENERGY_REL
twice the worst relative difference, rounded up to one digit.

Condition on the inputs: on every one of them every round of irls_f32 stops by its rule (rel <= 1e-5) within max_iters = 400
(tests/test_volume_flow_robust_host.py asserts it).  The preconditioner has straight time links, and an Lp temporal penalty with r < 2
raises a temporal link's weight by up to eps^(r - 2) where the iterate is flat along the flow: strong temporal coupling with several
pixels of motion, the regime the flow call's section names as slow.  Of the matrix before the rule, scanned on the CPU, 54 of 57 inputs
stop as they stand (worst 365 of 400); the three that do not (5 x 260 x 3 x 3 periodic under pan, the same under random with tau 10,
12 x 19 x 3 x 8 under pan) share one regime, which the substitution rule, substitute(), names:

    exponents (2, 1, 2) -- nothing but time is reweighted, so the temporal weights outgrow the spatial ones, which stay 1 -- at eps 1e-3
    of the range, under a flow that moves pixels (pan, pan1, split, random; under the others, STILL_FLOWS, a link is straight or
    there is one per frame), run at eps 1e-2 in place of 1e-3 and with tau 1 in place of 10.  The flow stays.

With it the three stop within 233 iterations.  pan1 is among the moving flows because of the probe's length walk: its 6 x 33 x 4 inputs
under pan1 and periodic time ran 400 iterations in every round at eps 1e-3.  It alters the inputs ALTERED (six of 57, at most one in eight); every flow kind, every
exponent triple and both time modes still occur with a flow that is not zero at least twice (the host test checks all three)."""
import functools

import numpy as np

import volume_flow_bounds as vfb
import volume_flow_np as vf
import volume_flow_robust_np as vfr
import volume_robust_bounds as vrb
import volume_wls_np as vw

ROUNDS = vrb.ROUNDS
MAX_ITERS = 400                                # sc_volume_robust_params' default
ERR_FACTOR, ERR_FLOOR = 3.0, 0.0               # measured: worst ratio 1.04 (neumann 6 x 3, 4 frames, tau 10, split, sparse, links t, free time, (1.5, 0.8, 2), eps 1e-2, random); no input where irls_f32's ERR is 0
RES_FACTOR, RES_FLOOR = 20.0, 0.0              # measured: worst ratio 7.23 (the same input); no input where irls_f32's RES is 0
ENERGY_REL = 3e-7                              # measured: worst 1.35e-7 (neumann 5 x 7 x 3, 3 frames, tau 10, scatter, no weight, links t, (1.5, 0.8, 2), eps 1e-2, pan1)

BORDERS = vrb.BORDERS
SIZES = vrb.SIZES                              # rows x columns: 5 x 260, 12 x 19, 7 x 2, 5 x 16
FRAMES, CHANNELS, TAUS, PATTERNS, WEIGHTS, LINKS, TIMES = vrb.FRAMES, vrb.CHANNELS, vrb.TAUS, vrb.PATTERNS, vrb.WEIGHTS, vrb.LINKS, vrb.TIMES
GT, EXPONENTS, EPS = vrb.GT, vrb.EXPONENTS, vrb.EPS
FLOWS = vfb.FLOWS
REPS = 3                                       # a frame has three sizes: 9 inputs for 7 flows


STILL_FLOWS = ("zero", "collapse", "far")


def substitute(case):
    """the substitution rule of the module's docstring on one matrix tuple"""
    border, H, W, C, T, tau, pattern, wkind, links, time, gt, exps, epsf, flow = case
    if exps == (2.0, 1.0, 2.0) and epsf == 1e-3 and flow not in STILL_FLOWS:
        epsf, tau = 1e-2, min(tau, 1.0)
    return (border, H, W, C, T, tau, pattern, wkind, links, time, gt, exps, epsf, flow)


def raw_matrix():
    """matrix() before the substitution rule"""
    pick = lambda values, bi, si, j, a, b, c: values[(a * bi + b * si + c * j) % len(values)]
    out = []
    for bi, (border, _, _) in enumerate(BORDERS):
        for si, (H, W) in enumerate(SIZES):
            if border == "frame" and min(H, W) < 3:
                continue
            for j in range(REPS):
                T = pick(FRAMES, bi, si, j, 1, 1, 1)
                out.append((border, H, W, pick(CHANNELS, bi, si, j, 0, 1, 1), T, pick(TAUS, bi, si, j, 1, 1, 1), pick(PATTERNS, bi, si, j, 1, 1, 4),
                            pick(WEIGHTS, bi, si, j, 1, 2, 1), pick(LINKS, bi, si, j, 3, 1, 2),
                            "free" if T == 2 else pick(TIMES, bi, si, j, 1, 0, 1), pick(GT, bi, si, j, 1, 1, 1), pick(EXPONENTS, bi, si, j, 1, 1, 3),
                            pick(EPS, bi, si, j, 0, 1, 1), FLOWS[len(out) % len(FLOWS)]))
    return out


def matrix():
    """the inputs of the GPU tests' walk (and of tools/volume_flow_robust_probe.py): volume_robust_bounds.matrix()'s tuple and the flow,
    (border, H, W, C, T, tau, pattern, wkind, links, time, gt, exponents, eps factor, flow).  Every border x size REPS times (a frame
    around 2 x 7 pixels leaves no unknown and is left out); every other axis by volume_robust_bounds.matrix()'s picks, the flows dealt
    in turn along the list (a border's 9 or 12 inputs lie together, a size's three apart), so that every flow meets every border and
    every size; then substitute().  tests/test_volume_flow_robust_host.py checks the
    coverage."""
    return [substitute(c) for c in raw_matrix()]


ALTERED = [i for i, (a, b) in enumerate(zip(raw_matrix(), matrix())) if a != b]


def make_input(border, H, W, C, T, tau, pattern, wkind, links="none", time="free", gt=True, flow="zero", seed=0, **flow_args):
    """One input as a dict: volume_robust_bounds.make_input's fields, and flow and links = (fwd, bwd) with the states mended through the
    matched links (volume_flow_bounds.make_input)"""
    p = vfb.make_input(border, H, W, C, T, tau, pattern, wkind, links, time, flow, seed, **flow_args)
    del p["lap"]
    if not gt:
        p["gt"] = None
    p["range"] = float(p["data"].max() - p["data"].min())
    return p


def nan_unread(p):
    """a copy of the input with NaN in every element the header says is not read: volume_robust_bounds.nan_unread's, gt and smooth_t
    where no live matched link has its source, and the flow off the work rectangle"""
    q = vrb.nan_unread(p)
    _, _, lt = vf.live_links(p["sides"], p["periodic"], p["tper"], p["state"], p["links"])
    nan = np.float32(np.nan)
    q["gt"] = None if p["gt"] is None else np.where(lt, p["gt"], nan).astype(np.float32)
    q["smt"] = None if p["smt"] is None else np.where(lt, p["smt"], nan).astype(np.float32)
    f = np.full(p["flow"].shape, nan, np.float32)
    blk = (slice(None),) + vw.unknowns(p["sides"], p["periodic"], *p["flow"].shape[1:3])
    f[blk] = p["flow"][blk]
    q["flow"] = f
    return q


penalties = vrb.penalties


def call_args(p, pen, **kw):
    """the arguments of capi.Instance.volume_flow_robust for an input and its penalties"""
    return dict(vrb.call_args(p, pen, **kw), flow=p["flow"])


class Yardstick:
    """One input's references: the exact rounds' iterates, and irls_f32's iterates with their (ERR, RES) round by round and every inner
    solve's final rel.  u32, iters32: where the restatement's rounds ran in a chunk with others (the batch test), that chunk's"""

    def __init__(self, p, pen, rounds=ROUNDS, u32=None, iters32=None):
        self.p, self.pen, self.rounds = p, pen, rounds
        self.unk = vw.kinds(p["sides"], p["periodic"], p["state"]) == vw.UNKNOWN
        self.exact = vfr.irls_exact(p, pen, rounds)
        self.rels32 = None
        if u32 is None:
            self.rels32 = []
            u32, iters32 = vfr.irls_f32(p, pen, rounds, max_iters=MAX_ITERS, rels=self.rels32)
        self.u32, self.iters32 = u32, iters32
        self.fig32 = [self.measure(u32[k - 1] if k else None, u32[k], k) for k in range(len(u32))]
        self.err32, self.res32 = self.fig32[-1]

    def energy(self, u):
        return vfr.energy(self.p, self.pen, u)

    def measure(self, prev, out, k=None):
        """(ERR, RES) of round k's iterate `out` (k None: the last round), `prev` the iterate before it (round 0: the caller's system)"""
        k = len(self.exact) - 1 if k is None else k
        out = vw._thwc(np.asarray(out))
        err = float(np.abs(out.astype(np.float64) - self.exact[k])[self.unk].max()) / self.p["range"]
        return err, vfr.round_residual(self.p, self.pen, prev if k else None, out)

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
    border, H, W, C, T, tau, pattern, wkind, links, time, gt, exps, epsf, flow = matrix()[i]
    p = make_input(border, H, W, C, T, tau, pattern, wkind, links, time, gt, flow)
    pen = penalties(p, exps, epsf)
    return p, pen, Yardstick(p, pen)


@functools.lru_cache(maxsize=None)
def batch_trio():
    """(three volumes of one shape under split, random and pan, their penalties): the batch tests' members; nobody writes into them"""
    probs = [make_input("free_lt", 23, 17, 3, 4, 1.0, pat, "constant", "xyt", "periodic", True, flow, seed=20 + k)
             for k, (pat, flow) in enumerate((("hole", "split"), ("scatter", "random"), ("keyframes", "pan")))]
    return probs, penalties(probs[0], (1.0, 1.0, 2.0), 1e-2)


# ---- what the call is for (tests/test_gpu_volume_flow_robust.py)
PAN = (2, 1)


def pan_flow(T, H, W, pan=PAN, loop=False):
    return np.broadcast_to(np.float32(pan), ((T if loop else T - 1), H, W, 2)).copy()


def panning_outlier_problem(T, H, W, pan=PAN, gross=8.0):
    """(problem, the true video): volume_robust_bounds.outlier_problem's truth with frame t moved by t pans (it wraps); gx, gy its exact
    forward differences, gt the exact differences ALONG the flow `pan` -- gt(x, y, t) = u_(t+1)(x + dx, y + dy) - u_t(x, y), stored at
    the source -- with temporal outliers on outlier_problem's lattice, `gross` times its +-0.5; KNOWN pixels on its lattice of frame 0,
    one channel, Neumann borders, free time.  (+-4: against an outlier of a the four L1 spatial links of a pixel, 8 |h| for a move of h,
    hold it under a quadratic temporal penalty only while a <= 4 -- (a - h)^2 + h^2 + 8 h has its minimum at h = (a - 4) / 2 --, so at
    +-0.5 p_time = 2 recovers the truth as well as p_time = 1 does; under the L1 temporal penalty 2 |a - h| + 2 |h| is flat and the pixel
    stays whatever a is.)"""
    import robust_bounds
    p0, still = vrb.outlier_problem(T, H, W)
    truth = np.stack([np.roll(still[t], (t * pan[1], t * pan[0]), (0, 1)) for t in range(T)])
    gx, gy = zip(*(robust_bounds.forward_differences(f) for f in truth))
    partner = np.stack([np.roll(truth[t + 1], (-pan[1], -pan[0]), (0, 1)) for t in range(T - 1)])
    outliers = p0["gt"].astype(np.float64) - (still[1:] - still[:-1])
    gt = (partner - truth[:-1]) + gross * outliers
    p = dict(p0, gx=np.stack(gx).astype(np.float32), gy=np.stack(gy).astype(np.float32), gt=gt.astype(np.float32), data=truth.astype(np.float32),
             boundary=truth.astype(np.float32), range=float(truth.max() - truth.min()), flow=pan_flow(T, H, W, pan))
    p["links"] = vfb.links_of(p)
    return p, truth


def panning_texture(T, H, W, pan=PAN, sigma=0.1, seed=3):
    """(the clean video, the noisy one) float32 T x H x W: a texture of waves and a grid of steps that moves by `pan` per frame (it
    wraps), noise of `sigma`"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    base = 0.5 + 0.25 * np.sin(x / 3.7) * np.cos(y / 4.3) + 0.4 * ((x % 12 >= 6) ^ (y % 10 >= 5))
    clean = np.stack([np.roll(base, (t * pan[1], t * pan[0]), (0, 1)) for t in range(T)])
    return clean.astype(np.float32), (clean + sigma * rng.standard_normal(clean.shape)).astype(np.float32)
