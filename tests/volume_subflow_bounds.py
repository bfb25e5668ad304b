"""The quantities the sub-pixel flow volume GPU tests hold the library to, their bounds and their inputs
(tests/test_gpu_volume_subflow.py), after the pattern of tests/volume_flow_bounds.py with the operator of tests/volume_subflow_np.py:

    ERR  max |u - solve_exact| / max |solve_exact|      both maxima over the UNKNOWN pixels of all frames
    RES  max |L u - b| / max |b|                         likewise; b the library's float32 right-hand side, the rest in float64

Bounds:  measured <= max(FACTOR x the same quantity for volume_subflow_np.pcg_f32 on the same input, FLOOR).  pcg_f32 is the same
iteration with the same (straight-link) preconditioner, start and stop rule.  The four constants come from one MI355X run of
tools/volume_subflow_probe.py --lengths over a length walk and the tests' own inputs (DESIGN.md section 4 holds the table,
profiles/volume_subflow_lengths.txt the record), by volume_bounds' rule: each factor is the worst ratio to the restatement, times 2,
rounded up to one digit; each floor twice the worst absolute value among the inputs where the restatement needed no iteration at all.
Iterations:  sweeps <= 2 x pcg_f32's count + SC_WEIGHTED_POLL, both from the reference iteration.

Condition on the inputs: the reference iteration stays within the call's budget on every one of them, 2 x pcg_f32's count +
SC_WEIGHTED_POLL <= 400 with rel <= 1e-5 (tests/test_volume_subflow_host.py asserts it).  The preconditioner has straight time links, so
strong temporal coupling with motion is expensive: tau = 10 goes only with the flows `zero` and `half`."""
import functools

import numpy as np

import volume_bounds as vb
import volume_flow_bounds as fb
import volume_subflow_np as vs
import volume_wls_bounds as vwb

POLL = vb.POLL
RES_FACTOR, RES_FLOOR = 4.0, 9.3e-7             # measured: worst ratio 1.71 (neumann 300 x 9, 2 frames, tau 1, scatter, sparse, links xyt, free time, edge), worst value without an iteration 4.62e-7 (periodic xy 2 x 7, 3 frames, tau 0.1, constant links, periodic time, zero flow)
ERR_FACTOR, ERR_FLOOR = 3.0, 1.9e-6             # measured: worst ratio 1.10 (periodic x 300 x 9, 3 frames, tau 1, scatter, no weight, free time, collapse), worst value without an iteration 9.21e-7 (periodic xy 2 x 7, 3 frames, tau 0.1, constant links, periodic time, zero flow)

BORDERS = vb.BORDERS
SIZES = vb.SIZES                                # rows x columns: 47 x 33, 9 x 300 (crosses the 256-column group), 7 x 2, 5 x 16
FRAMES = vb.FRAMES                              # 2 (free time only), 3, 5, 8
CHANNELS = vb.CHANNELS
TAUS = vb.TAUS
PATTERNS = vb.PATTERNS
WEIGHTS = vb.WEIGHTS
FORMS = vb.FORMS
LINKS = vwb.LINKS
TIMES = vwb.TIMES
FLOWS = ["zero", "half", "pan", "axis", "random", "whole", "collapse", "edge"]
STRONG_TAU_FLOWS = ("zero", "half")             # the flows that tau = 10 goes with
MAX_ITERS = 400                                 # sc_volume_wls_params' default
REPS = 4


def matrix():
    """the inputs of the GPU tests' walk (and of tools/volume_subflow_probe.py): (border, H, W, C, T, tau, pattern, wkind, form, links,
    time, flow), chosen as volume_flow_bounds.matrix chooses them: every border x size REPS times (a frame around 2 x 7 pixels leaves no
    unknown and is left out), every other axis the value (a bi + b si + c j) mod n of its n values; 2 frames go with free time, tau = 10
    only with STRONG_TAU_FLOWS (elsewhere 1 takes its place), and `collapse` on states that are all UNKNOWN comes with a sparse weight.
    tests/test_volume_subflow_host.py checks the coverage."""
    pick = lambda values, bi, si, j, a, b, c: values[(a * bi + b * si + c * j) % len(values)]
    out = []
    for bi, (border, _, _) in enumerate(BORDERS):
        for si, (H, W) in enumerate(SIZES):
            if border == "frame" and min(H, W) < 3:
                continue
            for j in range(REPS):
                T = pick(FRAMES, bi, si, j, 1, 1, 1)
                flow = pick(FLOWS, bi, si, j, 1, 1, 2)
                tau = pick(TAUS, bi, si, j, 1, 1, 1)
                if tau == 10.0 and flow not in STRONG_TAU_FLOWS:
                    tau = 1.0
                pattern, wkind = pick(PATTERNS, bi, si, j, 1, 1, 4), pick(WEIGHTS, bi, si, j, 1, 2, 1)
                if flow == "collapse" and pattern == "all" and wkind is None:
                    wkind = "sparse"          # (every link of a frame onto one point: without a weight a single mended pixel would hold each frame)
                out.append((border, H, W, pick(CHANNELS, bi, si, j, 0, 1, 1), T, tau, pattern, wkind, pick(FORMS, bi, si, j, 2, 1, 1), pick(LINKS, bi, si, j, 3, 1, 2),
                            "free" if T == 2 else pick(TIMES, bi, si, j, 1, 0, 1), flow))
    return out


def make_flow(kind, T, H, W, tper, seed=0, amount=3, column=None, row=None, rect=None):
    """float32 (T - 1) x H x W x 2 (periodic time: T) of (dx, dy), one of FLOWS.  amount: random's and whole's pixels of motion; column:
    the column and the row collapse points at (None: the middle); rect = (rows, cols): the work rectangle's slices, whose last row and column `edge`
    aims at (None: the whole frame)"""
    Tf = T if tper else T - 1
    f = np.zeros((Tf, H, W, 2), np.float32)
    y, x = np.mgrid[0:H, 0:W]
    rng = np.random.default_rng(9700 + seed + 3 * H + W + 29 * T)
    if kind == "zero":
        pass
    elif kind == "half":
        f[...] = 0.5
    elif kind == "pan":
        f[..., 0], f[..., 1] = 2.25, -0.75
    elif kind == "axis":              # fractional along x alone: two taps
        f[..., 0] = 1.5
    elif kind == "random":            # uniform +-amount, 10 % occluded
        f[...] = rng.uniform(-amount, amount, f.shape)
        f[rng.random(f.shape[:3]) < 0.1] = np.nan
    elif kind == "whole":             # whole numbers +-amount: one tap each, and collisions
        f[...] = rng.integers(-amount, amount + 1, f.shape)
    elif kind == "collapse":          # every pixel of a frame onto one fractional point: rows as long as a frame
        f[..., 0], f[..., 1] = ((W // 2 if column is None else column) - 0.5 - x)[None], ((H // 2 if row is None else row) - 0.25 - y)[None]
    elif kind == "edge":              # zero flow (-0.0 among it); targets on the rectangle's last row or column, a quarter pixel beyond, and far away
        rows, cols = (slice(0, H), slice(0, W)) if rect is None else rect
        f[:, (y + x) % 2 == 1] = -0.0
        what = rng.integers(0, 10, f.shape[:3])
        lastx, lasty = (cols.stop - 1 - x).astype(np.float32), (rows.stop - 1 - y).astype(np.float32)
        f[..., 0] = np.where(what == 0, lastx, f[..., 0])                              # on the last column: one tap
        f[..., 1] = np.where(what == 0, np.float32(-0.0), f[..., 1])
        f[..., 0] = np.where(what == 1, lastx, f[..., 0])                              # on the last column, half a row down: two taps
        f[..., 1] = np.where(what == 1, np.where(y < rows.stop - 1, 0.5, -0.5), f[..., 1])
        f[..., 1] = np.where(what == 2, lasty, f[..., 1])                              # on the last row
        f[..., 0] = np.where(what == 3, lastx + np.float32(0.25), f[..., 0])           # a quarter pixel beyond: no link
        f[..., 1] = np.where(what == 4, lasty + np.float32(0.25), f[..., 1])
        values = np.array([1e9, -1e9, np.inf, -np.inf], np.float32)
        far = values[rng.integers(0, len(values), f.shape[:3])]
        axis = rng.integers(0, 2, f.shape[:3])
        f[..., 0] = np.where((what == 5) & (axis == 0), far, f[..., 0])
        f[..., 1] = np.where((what == 5) & (axis == 1), far, f[..., 1])
    else:
        raise ValueError(kind)
    return f


def links_of(p):
    return vs.taps(p["sides"], p["periodic"], p["tper"], p["state"].shape[:3], p["flow"])


def make_input(border, H, W, C, T, tau, pattern, wkind, links="none", time="free", flow="zero", seed=0, **flow_args):
    """volume_wls_bounds.make_input's dict with `flow` and the links (idx, b) that volume_subflow_np.taps makes of it; the states mended
    once more so that every UNKNOWN component is pinned through the bilinear links too (its first loose pixel becomes KNOWN)"""
    p = vwb.make_input(border, H, W, C, T, tau, pattern, wkind, links, time, seed)
    rect = vs.unknowns(p["sides"], p["periodic"], H, W)
    p["flow"] = make_flow(flow, T, H, W, p["tper"], seed, rect=rect, **flow_args)
    p["links"] = links_of(p)
    state = p["state"] = p["state"].copy()
    while True:
        loose = vs.unpinned_components((p["sides"], p["periodic"], p["tper"], state, p["weight"]), p["links"])
        if not loose.any():
            return p
        state[tuple(np.argwhere(loose)[0])] = 1


def nan_unread(p):
    """a copy of the input with NaN in every element the header says is not read: volume_wls_bounds.nan_unread's, gt and smooth_t where
    no live link has its source"""
    q = vwb.nan_unread(p)
    _, _, lt = vs.live_links(p["sides"], p["periodic"], p["tper"], p["state"], p["links"])
    nan = np.float32(np.nan)
    q["gt"] = np.where(lt, p["gt"], nan).astype(np.float32)
    q["smt"] = None if p["smt"] is None else np.where(lt, p["smt"], nan).astype(np.float32)
    return q


def call_args(p, form):
    """the keyword arguments of capi.Instance.volume_subflow for an input in one of FORMS"""
    return dict(vwb.call_args(p, form), flow=p["flow"])


def np_args(p, form="lap"):
    """volume_subflow_np's args tuple of an input; a guidance form: lap is volume_subflow_np.divergence of gx, gy (and gt)"""
    a = vb.call_args(p, form)
    head = (p["sides"], p["periodic"], p["tper"], p["state"])
    lap = a["lap"] if form == "lap" else vs.divergence(*head, p["sx"], p["sy"], p["smt"], p["tau"], a["gx"], a["gy"], a["gt"], p["links"])
    return head + (p["weight"], p["sx"], p["sy"], p["smt"], p["tau"], p["data"], lap)


def err_and_res(args, links, boundary, u, want):
    sides, periodic, tper, state = args[:4]
    k = vs.kinds(sides, periodic, state)
    unk = k == vs.UNKNOWN
    blk = (slice(None),) + vs.unknowns(sides, periodic, *k.shape[1:3])
    b = vs.folded_rhs(args, links, boundary)
    r = vs.residual(args, links, u, boundary)
    w = vs._thwc(np.asarray(want, np.float64))
    scale_u, scale_b = float(np.abs(w[unk]).max()), float(np.abs(b[unk[blk]]).max())
    err = float(np.abs(vs._thwc(np.asarray(u, np.float64)) - w)[unk].max()) / scale_u
    return err, (float(np.abs(r[unk[blk]]).max()) / scale_b if scale_b > 0 else 0.0)


class Yardstick:
    """One input's references: want = solve_exact, and pcg_f32's (ERR, RES, iterations, rel) on it.  means: the preconditioner's
    (s-bar, tau-bar, w-bar) where they are not the input's own (a member of a batch: the chunk's)."""

    def __init__(self, p, form="lap", tol=1e-5, means=None):
        self.args = np_args(p, form)
        self.links = p["links"]
        self.boundary = p["boundary"] if vs.has_dirichlet(p["sides"], p["periodic"]) else None
        self.want = vs.solve_exact(self.args, self.links, self.boundary)
        u32, self.iters32, self.rel32 = vs.pcg_f32(self.args, self.links, self.boundary, tol=tol, max_iters=MAX_ITERS, means=means)
        self.err32, self.res32 = self.measure(u32)

    def measure(self, out):
        return err_and_res(self.args, self.links, self.boundary, out, self.want)

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


def chunk_means(probs):
    """(s-bar, tau-bar, w-bar) as the library takes them for a chunk: every mean over all its members' links or UNKNOWN pixels"""
    m = [vs.precond_means(np_args(p)[:9], p["links"]) for p in probs]
    ns, nt, nu = (sum(c[3][i] for c in m) for i in range(3))
    sbar = sum(c[0] * c[3][0] for c in m) / ns if ns and probs[0]["sx"] is not None else 1.0
    tbar = sum(c[1] * c[3][1] for c in m) / nt if nt and probs[0]["smt"] is not None else float(np.float32(probs[0]["tau"]))
    return sbar, tbar, (sum(c[2] * c[3][2] for c in m) / nu if nu else 1.0)


def as_flow_input(p):
    """the input as volume_flow_bounds sees it: the same arrays with the links volume_flow_np.match makes of the (whole-numbered) flow"""
    q = dict(p)
    q["links"] = fb.links_of(q)
    return q


@functools.lru_cache(maxsize=None)
def matrix_case(i):
    """(input, its form, its Yardstick) of matrix()[i], computed once per process and shared; nobody writes into them"""
    border, H, W, C, T, tau, pattern, wkind, form, links, time, flow = matrix()[i]
    p = make_input(border, H, W, C, T, tau, pattern, wkind, links, time, flow)
    return p, form, Yardstick(p, form)


# ---- the motion test's input (tests/test_gpu_volume_subflow.py; tests/test_volume_subflow_host.py checks its premise on the float64 solves)
MOTION_TAU = 4.0


def moving_video(T, H, W, C, pan, seed):
    """a smooth texture that moves by `pan` = (dx, dy) pixels per frame, real-valued (it wraps), float32 T x H x W x C"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    ph = rng.uniform(0, 2 * np.pi, 4)
    base = lambda xx, yy: (2.0 + np.sin(2 * np.pi * 2 * xx / W + ph[0]) * np.cos(2 * np.pi * yy / H + ph[1])
                           + 0.7 * np.sin(2 * np.pi * 3 * xx / W + 2 * np.pi * 2 * yy / H + ph[2]) + 0.5 * np.cos(2 * np.pi * 4 * yy / H + ph[3]))
    frames = np.stack([base(x - t * pan[0], y - t * pan[1]) for t in range(T)])
    return np.ascontiguousarray(np.broadcast_to(frames[..., None], (T, H, W, C)) * (1 + 0.1 * np.arange(C)), np.float32)


def motion_case():
    """(truth, holes, frames, flow): a smooth texture moving by (0.5, 0.5) per frame under a hole that stands still"""
    T, H, W, C, pan = 6, 20, 24, 1, (0.5, 0.5)
    truth = moving_video(T, H, W, C, pan, 1)
    holes = np.zeros((T, H, W), bool)
    holes[:, 8:12, 10:14] = True
    frames = np.where(holes[..., None], np.float32(0), truth)
    flow = np.ascontiguousarray(np.broadcast_to(np.float32(pan), (T - 1, H, W, 2)))
    return truth, holes, frames, flow


def motion_problem(frames, holes, flow):
    """inpaint_video's problem on the motion case as an input dict: reflecting borders, no weight, no link arrays, lap = 0"""
    state = np.ascontiguousarray(np.broadcast_to(np.where(holes, 0, 1).astype(np.float32)[..., None], frames.shape))
    p = dict(sides="lrtb", periodic="", tper=False, tau=MOTION_TAU, state=state, data=frames, weight=None, sx=None, sy=None, smt=None, boundary=None,
             lap=np.zeros_like(frames), gx=None, gy=None, gt=None, flow=np.asarray(flow, np.float32))
    p["links"] = links_of(p)
    return p
