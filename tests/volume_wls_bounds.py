"""The quantities the WLS volume GPU tests hold the library to, their bounds and their inputs (tests/test_gpu_volume_wls.py), after the
pattern of tests/volume_bounds.py with the operator of tests/volume_wls_np.py:

    ERR  max |u - solve_exact| / max |solve_exact|      both maxima over the UNKNOWN pixels of all frames
    RES  max |L u - b| / max |b|                         likewise; b the library's float32 right-hand side, the rest in float64

Bounds:  measured <= max(FACTOR x the same quantity for volume_wls_np.pcg_f32 on the same input, FLOOR).  pcg_f32 is the same iteration
with the same preconditioner, start and stop rule, so both stop somewhere below tol; the library runs up to SC_WEIGHTED_POLL iterations
longer, adds its sums in another order and transforms by chirp convolutions where the restatement uses pocketfft.  The four constants come
from one MI355X run of tools/volume_wls_probe.py --lengths over a length walk and the tests' own inputs (DESIGN.md section 4 holds the
table, profiles/volume_wls_lengths.txt the record), by volume_bounds' rule: each factor is the worst ratio to the restatement, times 2,
rounded up to one digit; each floor twice the worst absolute value among the inputs where the restatement needed no iteration at all.
Iterations:  sweeps <= 2 x pcg_f32's count + SC_WEIGHTED_POLL, both from the reference iteration."""
import functools

import numpy as np

import volume_bounds as vb
import volume_wls_np as vw

POLL = vb.POLL
RES_FACTOR, RES_FLOOR = 5.0, 1.1e-6             # measured: worst ratio 2.25 (neumann 6 x 32, 4 frames, tau 10, split, sparse, links xyt, free time), worst value without an iteration 5.19e-7 (periodic xy 2 x 7, 3 frames, tau 0.1, constant links, periodic time)
ERR_FACTOR, ERR_FLOOR = 3.0, 1.8e-6             # measured: worst ratio 1.26 (free left + top 2 x 7, 3 frames, tau 10, scatter, constant, links t, periodic time), worst value without an iteration 8.96e-7 (periodic xy 300 x 9, 8 frames, tau 10, constant links, free time)

BORDERS = vb.BORDERS
SIZES = vb.SIZES                                # rows x columns: 47 x 33, 9 x 300 (crosses the 256-column group), 7 x 2, 5 x 16
FRAMES = vb.FRAMES                              # 2 (free time only), 3, 5, 8
CHANNELS = vb.CHANNELS
TAUS = vb.TAUS
PATTERNS = vb.PATTERNS
WEIGHTS = vb.WEIGHTS
FORMS = vb.FORMS
LINKS = ["none", "xy", "t", "xyt"]              # which link arrays the call carries: log-uniform over two decades, seeded
TIMES = ["free", "periodic"]
MAX_ITERS = 400                                 # sc_volume_wls_params' default
DECADES = 2.0


def matrix():
    """the inputs of the GPU tests' walk (and of tools/volume_wls_probe.py): (border, H, W, C, T, tau, pattern, wkind, form, links, time).
    Every border x size twice (a frame around 2 x 7 pixels leaves no unknown and is left out).  Every other axis takes the value
    (a bi + b si + c j) mod n of its n values -- bi, si the border's and the size's number, j the repetition -- with (a, b, c) chosen so
    that every value meets every border and every size; 2 frames go with free time.  tests/test_volume_wls_host.py checks the coverage."""
    pick = lambda values, bi, si, j, a, b, c: values[(a * bi + b * si + c * j) % len(values)]
    out = []
    for bi, (border, _, _) in enumerate(BORDERS):
        for si, (H, W) in enumerate(SIZES):
            if border == "frame" and min(H, W) < 3:
                continue
            for j in range(2):
                T = pick(FRAMES, bi, si, j, 1, 1, 1)
                out.append((border, H, W, pick(CHANNELS, bi, si, j, 0, 1, 1), T, pick(TAUS, bi, si, j, 1, 1, 1), pick(PATTERNS, bi, si, j, 1, 1, 4),
                            pick(WEIGHTS, bi, si, j, 1, 2, 1), pick(FORMS, bi, si, j, 2, 1, 1), pick(LINKS, bi, si, j, 3, 1, 2),
                            "free" if T == 2 else pick(TIMES, bi, si, j, 1, 0, 1)))
    return out


def loguniform(shape, seed, decades=DECADES):
    """float32, log-uniform over `decades` decades around 1"""
    rng = np.random.default_rng(seed)
    half = 0.5 * decades * np.log(10.0)
    return np.exp(rng.uniform(-half, half, shape)).astype(np.float32)


def make_input(border, H, W, C, T, tau, pattern, wkind, links="none", time="free", seed=0):
    """One input as a dict: volume_bounds.make_input's fields (gt at the temporal arrays' length), tper, and sx, sy, smt (None where
    `links` does not name them); float32, every element set (nan_unread() spoils the ones a call must not read).  The states are
    volume_bounds' -- pinned under free time, and so under periodic time, which only adds links."""
    p = vb.make_input(border, H, W, C, T, tau, pattern, wkind, seed)
    tper = time == "periodic"
    assert not (tper and T < 3)
    tshape = ((T if tper else T - 1), H, W, C)
    rng = np.random.default_rng(9000 + seed + 5 * H + W + 17 * T)
    p["gt"] = (0.1 * rng.standard_normal(tshape)).astype(np.float32)
    p["tper"] = tper
    p["sx"] = loguniform((T, H, W, C), 9100 + seed + H + 3 * T) if "xy" in links else None
    p["sy"] = loguniform((T, H, W, C), 9200 + seed + H + 3 * T) if "xy" in links else None
    p["smt"] = loguniform(tshape, 9300 + seed + H + 3 * T) if links.endswith("t") else None
    return p


def nan_unread(p):
    """a copy of the input with NaN in every element the header says is not read: volume_bounds.nan_unread's, gt at the temporal arrays'
    length, and the link arrays where their link is not live"""
    gt = p["gt"]
    q = vb.nan_unread(dict(p, gt=gt[:p["state"].shape[0] - 1]))
    lx, ly, lt = vw.live_links(p["sides"], p["periodic"], p["tper"], p["state"])
    nan = np.float32(np.nan)
    q["gt"] = np.where(lt, gt, nan).astype(np.float32)
    for name, live in (("sx", lx), ("sy", ly), ("smt", lt)):
        q[name] = None if p[name] is None else np.where(live, p[name], nan).astype(np.float32)
    return q


def call_args(p, form):
    """the keyword arguments of capi.Instance.volume_wls for an input in one of FORMS"""
    a = vb.call_args(p, form)
    return dict(a, smooth_x=p["sx"], smooth_y=p["sy"], smooth_t=p["smt"], loop=p["tper"])


def np_args(p, form="lap"):
    """volume_wls_np's args tuple of an input; a guidance form: lap is volume_wls_np.divergence of gx, gy (and gt)"""
    a = vb.call_args(p, form)
    head = (p["sides"], p["periodic"], p["tper"], p["state"])
    lap = a["lap"] if form == "lap" else vw.divergence(*head, p["sx"], p["sy"], p["smt"], p["tau"], a["gx"], a["gy"], a["gt"])
    return head + (p["weight"], p["sx"], p["sy"], p["smt"], p["tau"], p["data"], lap)


def err_and_res(args, boundary, u, want):
    sides, periodic, tper, state = args[:4]
    k = vw.kinds(sides, periodic, state)
    unk = k == vw.UNKNOWN
    blk = (slice(None),) + vw.unknowns(sides, periodic, *k.shape[1:3])
    b = vw.folded_rhs(*args, boundary)
    r = vw.residual(args, u, boundary)
    w = vw._thwc(np.asarray(want, np.float64))
    scale_u, scale_b = float(np.abs(w[unk]).max()), float(np.abs(b[unk[blk]]).max())
    err = float(np.abs(vw._thwc(np.asarray(u, np.float64)) - w)[unk].max()) / scale_u
    return err, (float(np.abs(r[unk[blk]]).max()) / scale_b if scale_b > 0 else 0.0)


class Yardstick:
    """One input's references: want = solve_exact, and pcg_f32's (ERR, RES, iterations) on it.  means: the preconditioner's (s-bar,
    tau-bar, w-bar) where they are not the input's own (a member of a batch: the chunk's)."""

    def __init__(self, p, form="lap", tol=1e-5, means=None):
        self.args = np_args(p, form)
        self.boundary = p["boundary"] if vw.has_dirichlet(p["sides"], p["periodic"]) else None
        self.want = vw.solve_exact(self.args, self.boundary)
        u32, self.iters32, self.rel32 = vw.pcg_f32(self.args, self.boundary, tol=tol, max_iters=MAX_ITERS, means=means)
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


def chunk_means(probs):
    """(s-bar, tau-bar, w-bar) as the library takes them for a chunk: every mean over all its members' links or UNKNOWN pixels"""
    m = [vw.precond_means(p["sides"], p["periodic"], p["tper"], p["state"], p["weight"], p["sx"], p["sy"], p["smt"], p["tau"]) for p in probs]
    ns, nt, nu = (sum(c[3][i] for c in m) for i in range(3))
    sbar = sum(c[0] * c[3][0] for c in m) / ns if ns and probs[0]["sx"] is not None else 1.0
    tbar = sum(c[1] * c[3][1] for c in m) / nt if nt and probs[0]["smt"] is not None else float(np.float32(probs[0]["tau"]))
    return sbar, tbar, (sum(c[2] * c[3][2] for c in m) / nu if nu else 1.0)


@functools.lru_cache(maxsize=None)
def matrix_case(i):
    """(input, its form, its Yardstick) of matrix()[i], computed once per process and shared; nobody writes into them"""
    border, H, W, C, T, tau, pattern, wkind, form, links, time = matrix()[i]
    p = make_input(border, H, W, C, T, tau, pattern, wkind, links, time)
    return p, form, Yardstick(p, form)
