"""The quantities the robust sub-pixel flow volume GPU tests hold the library to, their bounds and their inputs
(tests/test_gpu_volume_subflow_robust.py), after the pattern of tests/volume_flow_robust_bounds.py with the rounds of
tests/volume_subflow_robust_np.py around the sub-pixel volume solve.  Every run is ROUNDS = 4 fixed rounds (round_tol = -1) behind the
quadratic one:

    ERR     max |u - irls_exact| / R        over the UNKNOWN pixels; u the last iterate, irls_exact the float64 rounds with exact inner
                                            solves, R the data's range
    RES     max |L u - b| / max |b|         of the last round's system: L and b from the iterate before the last (the library's own, read
                                            from a run of ROUNDS - 1 rounds, whose bytes are that iterate's)
    ENERGY  |sc_hip_robust_trace's last energy - volume_subflow_robust_np.energy of the written iterate| / that energy

Bounds:  ERR and RES <= max(FACTOR x the same quantity for volume_subflow_robust_np.irls_f32 on the same input, FLOOR); ENERGY <=
ENERGY_REL.  irls_f32 is the same rounds with the same inner iteration, (straight-link) preconditioner, start and stop rule.  The
constants come from one MI355X run of tools/volume_subflow_robust_probe.py --lengths over matrix() and a length walk (DESIGN.md
section 4 holds the table, profiles/volume_subflow_robust_lengths.txt the record), by the project's rule: each factor is twice the
worst ratio to the restatement, rounded up to one digit; each floor twice the worst value among the inputs where the restatement's
figure is 0; ENERGY_REL twice the worst relative difference, rounded up to one digit.  Never against the library itself.

Condition on the inputs: on every one of them every round of irls_f32 stops by its rule (rel <= 1e-5) within max_iters = 400
(tests/test_volume_subflow_robust_host.py asserts it).  The preconditioner has straight time links, and an Lp temporal penalty with
r < 2 raises a temporal link's weight by up to eps^(r - 2) where the iterate is flat along the flow: strong temporal coupling under
motion, the regime the sub-pixel call's section names as slow.  Of the matrix before the rule, scanned on the CPU, 53 of 57 inputs stop
as they stand (worst 356 of 400); SLOW names the four that do not, with what the scan saw.  Two are volume_flow_robust_bounds'
regime -- exponents (2, 1, 2): nothing but time is reweighted, so the temporal weights outgrow the spatial ones, which stay 1 -- at eps
1e-3 under a flow that moves pixels (pan, collapse); the others are tau 10 with r < 2 under pan and under collapse.  The substitution rule, substitute(), is that module's:

    an input of SLOW runs at eps 1e-2 of the range in place of 1e-3 and with tau 1 in place of 10 -- under `collapse`, where a whole
    frame's links meet in one point, with tau 0.1.  The flow stays.

With it the four stop within 272 iterations.  It alters four inputs of 57 (at most one in eight); every flow kind, every exponent
triple and both time modes still occur with a flow that is not zero at least twice (the host test checks all three).  The probe's
length walk applies the same rule to an input whose reference rounds do not stop, and says so on the input's line."""
import functools

import numpy as np

import volume_robust_bounds as vrb
import volume_subflow_bounds as vsb
import volume_subflow_np as vs
import volume_subflow_robust_np as vsr
import volume_wls_np as vw

ROUNDS = vrb.ROUNDS
MAX_ITERS = 400                                # sc_volume_robust_params' default
ERR_FACTOR, ERR_FLOOR = 3.0, 0.0               # measured: worst ratio 1.41 (neumann 5 x 260, 2 frames, tau 0.1, every state 0, no weight, (1, 1, 2), eps 1e-2, zero); no input where irls_f32's ERR is 0
RES_FACTOR, RES_FLOOR = 20.0, 0.0              # measured: worst ratio 5.86 (neumann 7 x 5 x 3, 3 frames, tau 10, scatter, no weight, links t, (1.5, 0.8, 2), eps 1e-2, pan); no input where irls_f32's RES is 0
ENERGY_REL = 3e-7                              # measured: worst 1.26e-7 (neumann 3 x 6, 4 frames, tau 10, split, sparse, links t, (1.5, 0.8, 2), eps 1e-2, random); the trace's worst rise from one round to the next: 1.3e-8

BORDERS = vrb.BORDERS
SIZES = vrb.SIZES                              # rows x columns: 5 x 260, 12 x 19, 7 x 2, 5 x 16
FRAMES, CHANNELS, TAUS, PATTERNS, WEIGHTS, LINKS, TIMES = vrb.FRAMES, vrb.CHANNELS, vrb.TAUS, vrb.PATTERNS, vrb.WEIGHTS, vrb.LINKS, vrb.TIMES
GT, EXPONENTS, EPS = vrb.GT, vrb.EXPONENTS, vrb.EPS
FLOWS = vsb.FLOWS                              # zero, half, pan, axis, random, whole, collapse, edge
REPS = 3

# raw_matrix()'s inputs on which a round of irls_f32 does not stop: index -> (the rounds' iterations, the worst final rel) of the scan
SLOW = {2: ([132, 400, 400, 376, 332], 5.75e-05),           # neumann 5 x 260, 5 frames, tau 10, (1.5, 0.8, 2), eps 1e-2, pan
        13: ([170, 400, 400, 400, 400], 5.26e-04),          # frame 5 x 260 x 3, 5 frames, tau 10, every state 0, (1, 1, 2), eps 1e-3, collapse
        46: ([224, 400, 400, 400, 400], 6.49e-03),          # periodic xy 5 x 260 x 3, 3 frames, periodic time, tau 10, (2, 1, 2), eps 1e-3, pan
        50: ([77, 327, 400, 400, 314], 1.28e-05)}           # periodic xy 12 x 19 x 3, 8 frames, tau 1, (2, 1, 2), eps 1e-3, collapse


def substitute(case):
    """the substitution rule of the module's docstring on one matrix tuple (of SLOW, or of the probe's walk)"""
    border, H, W, C, T, tau, pattern, wkind, links, time, gt, exps, epsf, flow = case
    return (border, H, W, C, T, 0.1 if flow == "collapse" else min(tau, 1.0), pattern, wkind, links, time, gt, exps, 1e-2, flow)


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
                            pick(EPS, bi, si, j, 0, 1, 1), FLOWS[(len(out) + bi) % len(FLOWS)]))
    return out


def matrix():
    """the inputs of the GPU tests' walk (and of tools/volume_subflow_robust_probe.py): volume_robust_bounds.matrix()'s tuple and the
    flow, (border, H, W, C, T, tau, pattern, wkind, links, time, gt, exponents, eps factor, flow).  Every border x size REPS times (a
    frame around 2 x 7 pixels leaves no unknown and is left out); every other axis by volume_robust_bounds.matrix()'s picks, the eight
    sub-pixel flows dealt in turn along the list with one step more at every new border (dealt plainly, 7 x 2 would never meet `pan`),
    so that every flow meets every border and every size; then substitute().
    tests/test_volume_subflow_robust_host.py checks the coverage."""
    return [substitute(c) if i in SLOW else c for i, c in enumerate(raw_matrix())]


ALTERED = [i for i, (a, b) in enumerate(zip(raw_matrix(), matrix())) if a != b]


def make_input(border, H, W, C, T, tau, pattern, wkind, links="none", time="free", gt=True, flow="zero", seed=0, **flow_args):
    """One input as a dict: volume_robust_bounds.make_input's fields, and flow and links = (idx, b) with the states mended through the
    bilinear links (volume_subflow_bounds.make_input)"""
    p = vsb.make_input(border, H, W, C, T, tau, pattern, wkind, links, time, flow, seed, **flow_args)
    del p["lap"]
    if not gt:
        p["gt"] = None
    p["range"] = float(p["data"].max() - p["data"].min())
    return p


def nan_unread(p):
    """a copy of the input with NaN in every element the header says is not read: volume_robust_bounds.nan_unread's, gt and smooth_t
    where no live link has its source, and the flow off the work rectangle"""
    q = vrb.nan_unread(p)
    _, _, lt = vs.live_links(p["sides"], p["periodic"], p["tper"], p["state"], p["links"])
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
    """the arguments of capi.Instance.volume_subflow_robust for an input and its penalties"""
    return dict(vrb.call_args(p, pen, **kw), flow=p["flow"])


class Yardstick:
    """One input's references: the exact rounds' iterates, and irls_f32's iterates with their (ERR, RES) round by round and every inner
    solve's final rel.  u32, iters32: where the restatement's rounds ran in a chunk with others (the batch test), that chunk's"""

    def __init__(self, p, pen, rounds=ROUNDS, u32=None, iters32=None):
        self.p, self.pen, self.rounds = p, pen, rounds
        self.unk = vw.kinds(p["sides"], p["periodic"], p["state"]) == vw.UNKNOWN
        self.exact = vsr.irls_exact(p, pen, rounds)
        self.rels32 = None
        if u32 is None:
            self.rels32 = []
            u32, iters32 = vsr.irls_f32(p, pen, rounds, max_iters=MAX_ITERS, rels=self.rels32)
        self.u32, self.iters32 = u32, iters32
        self.fig32 = [self.measure(u32[k - 1] if k else None, u32[k], k) for k in range(len(u32))]
        self.err32, self.res32 = self.fig32[-1]

    def energy(self, u):
        return vsr.energy(self.p, self.pen, u)

    def measure(self, prev, out, k=None):
        """(ERR, RES) of round k's iterate `out` (k None: the last round), `prev` the iterate before it (round 0: the caller's system)"""
        k = len(self.exact) - 1 if k is None else k
        out = vw._thwc(np.asarray(out))
        err = float(np.abs(out.astype(np.float64) - self.exact[k])[self.unk].max()) / self.p["range"]
        return err, vsr.round_residual(self.p, self.pen, prev if k else None, out)

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
    """(three volumes of one shape under half, random and pan, their penalties): the batch tests' members; nobody writes into them"""
    probs = [make_input("free_lt", 23, 17, 3, 4, 1.0, pat, "constant", "xyt", "periodic", True, flow, seed=20 + k)
             for k, (pat, flow) in enumerate((("hole", "half"), ("scatter", "random"), ("keyframes", "pan")))]
    return probs, penalties(probs[0], (1.0, 1.0, 2.0), 1e-2)


# ---- what the call is for (tests/test_gpu_volume_subflow_robust.py; tests/test_volume_subflow_robust_host.py checks both premises on
# the float64 rounds)
HALF_PAN = (0.5, 0.5)          # np.rint rounds it to (0, 0): the rounded call's links are straight
DENOISE = dict(lam=40.0, tau=3.0, p=1.0, p_time=1.0, eps=1e-2, max_rounds=4, round_tol=-1.0)


def pan_flow(T, H, W, pan=HALF_PAN, loop=False):
    return np.broadcast_to(np.float32(pan), ((T if loop else T - 1), H, W, 2)).copy()


def panning_texture(T, H, W, pan=HALF_PAN, sigma=0.1, seed=3):
    """(the clean video, the noisy one) float32 T x H x W: volume_subflow_bounds.moving_video's smooth texture moving by the real-valued
    `pan` per frame, noise of `sigma`"""
    clean = vsb.moving_video(T, H, W, 1, pan, seed)[..., 0].astype(np.float64)
    rng = np.random.default_rng(seed)
    return clean.astype(np.float32), (clean + sigma * rng.standard_normal(clean.shape)).astype(np.float32)


def denoise_problem(noisy, flow, lam=DENOISE["lam"], tau=DENOISE["tau"]):
    """tv_denoise_video's problem as an input dict: zero guidance, every state 0, weight lam, reflecting borders; flow None: straight links"""
    v = noisy[..., None]
    zero = np.zeros_like(v)
    p = dict(sides="lrtb", periodic="", tper=False, tau=tau, state=zero, data=v, weight=np.full(v.shape, lam, np.float32), sx=None, sy=None, smt=None,
             boundary=None, gx=zero, gy=zero, gt=None, range=float(v.max() - v.min()))
    if flow is not None:
        p["flow"] = np.asarray(flow, np.float32)
        p["links"] = vsb.links_of(p)
    return p


def subpixel_outlier_problem(T, H, W, pan=HALF_PAN, gross=4.0):
    """(problem, the true video): a smooth texture moving by `pan` (moving_video); gx, gy its exact wrapped forward differences with
    robust_bounds.corrupt's lattice in every frame, gt the exact differences ALONG the bilinear link -- gt(p, t) = sum_k b_k
    u_(t+1)(q_k) - u_t(p), stored at the source -- plus outliers of +-gross at x mod 7 = 5, y mod 5 = 0 on every other temporal link;
    KNOWN pixels on a lattice of frame 0 only (x mod 6 = 2, y mod 4 = 1), one channel, Neumann borders, free time, no weight"""
    import robust_bounds
    from seamlesscloneoptimization_amd import seamless_clone
    truth = vsb.moving_video(T, H, W, 1, pan, 2).astype(np.float64)
    gx, gy = zip(*(robust_bounds.corrupt(*robust_bounds.forward_differences(f)) for f in truth))
    flow = pan_flow(T, H, W, pan)
    partner, _ = seamless_clone._along_subpixel_flow(truth, flow)
    y, x = np.mgrid[0:H, 0:W]
    spot = ((x % 7 == 5) & (y % 5 == 0))[None, :, :, None] & (np.arange(T - 1) % 2 == 0)[:, None, None, None]
    sign = np.where((x + y) % 2 == 0, 1.0, -1.0)[None, :, :, None]
    gt = (partner - truth[:-1]) + gross * sign * spot
    state = np.zeros(truth.shape, np.float32)
    state[0, (y % 4 == 1) & (x % 6 == 2)] = 1
    p = dict(sides="lrtb", periodic="", tper=False, state=state, weight=None, sx=None, sy=None, smt=None, tau=1.0, gx=np.stack(gx).astype(np.float32),
             gy=np.stack(gy).astype(np.float32), gt=gt.astype(np.float32), data=truth.astype(np.float32), boundary=truth.astype(np.float32),
             range=float(truth.max() - truth.min()), flow=flow)
    p["links"] = vsb.links_of(p)
    return p, truth
