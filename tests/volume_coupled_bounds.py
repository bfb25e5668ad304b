"""The quantities the coupled volume GPU tests hold the library to, their bounds and their inputs (tests/test_gpu_volume_coupled.py):
tests/volume_robust_bounds.py's ERR, RES and ENERGY with the rounds of tests/volume_coupled_np.py, on that file's inputs -- chosen for
the failure modes of this walk: 260 columns cross the 256-column group, 12 x 19 under a frame makes bands start inside a frame, 7 x 2
under periodic x makes east and west one pixel, T = 2 with free time, T = 3 with periodic time where the wrap's owner is frame T - 1.
Every run is ROUNDS = 4 fixed rounds (round_tol = -1) behind the quadratic one.

Bounds:  ERR and RES <= max(FACTOR x the same quantity for volume_coupled_np.irls_f32 on the same input, FLOOR); ENERGY <= ENERGY_REL.
The constants start from the uncoupled family's 3 / 6 / 4e-7 (tests/volume_robust_bounds.py: the coupled rounds differ from the uncoupled
ones only in how rho is formed) and follow one MI355X run over matrix() (DESIGN.md section 4 holds the table and the two sentences on
what it widened, profiles/volume_coupled_lengths.txt the record; tools/volume_coupled_probe.py --lengths repeats it with a length walk)
by the family's rule: a factor is twice the worst measured ratio to the restatement, rounded up to one digit."""
import functools

import numpy as np

import volume_coupled_np as vc
import volume_robust_bounds as rb
import volume_wls_np as vw

ROUNDS = rb.ROUNDS
ERR_FACTOR, ERR_FLOOR = 4.0, 0.0               # measured: worst ratio 1.59 (periodic x 7 x 2, 3 frames x 3, tau 10, every state 0, constant weight, links xyt, periodic time, (0.8, 0.8, 2), eps 1e-2, SPACE|TIME|CHANNELS: 1.05e-6 against 6.6e-7 of the range, both at float32 resolution); no input where irls_f32's ERR is 0
RES_FACTOR, RES_FLOOR = 9.0, 0.0               # measured: worst ratio 4.45 (neumann 5 x 16, 8 frames x 3, tau 0.1, scatter, no weight, links xyt, free time, (1, 1, 2), eps 1e-3, SPACE|TIME|CHANNELS: 1.7e-5 against 3.9e-6, links over three decades; the stop rule is the 2-norm's, RES the max norm's); no input where irls_f32's RES is 0
ENERGY_REL = 4e-7                              # the uncoupled call's; measured: worst 6.82e-8 (periodic xy 5 x 16, 2 frames, tau 10, keyframes, sparse, links xy, (1.5, 0.8, 2), eps 1e-2, SPACE)

BORDERS, SIZES, FRAMES, CHANNELS, TAUS, PATTERNS, WEIGHTS, LINKS, TIMES, GT, EPS = (rb.BORDERS, rb.SIZES, rb.FRAMES, rb.CHANNELS, rb.TAUS,
                                                                                    rb.PATTERNS, rb.WEIGHTS, rb.LINKS, rb.TIMES, rb.GT, rb.EPS)
COUPLINGS = list(vc.LEGAL)
EXPONENTS = rb.EXPONENTS                                                      # (p, r, q) of the forms without TIME
TIME_EXPONENTS = [(1.0, 1.0, 2.0), (1.5, 1.5, 1.0), (0.8, 0.8, 2.0)]          # ... with TIME: one penalty over space and time, p = r
make_input, nan_unread, penalties = rb.make_input, rb.nan_unread, rb.penalties


def matrix():
    """the inputs of the GPU tests' walk (and of tools/volume_coupled_probe.py): volume_robust_bounds.matrix()'s tuple with the coupling
    behind it -- (border, H, W, C, T, tau, pattern, wkind, links, time, gt, exponents, eps factor, coupling).  Every border x size twice
    (a frame around 2 x 7 pixels leaves no unknown and is left out); every other axis by that matrix's rule, the five legal couplings
    among them.  A form with CHANNELS takes 3 channels; a form with TIME its exponents from TIME_EXPONENTS.
    tests/test_volume_coupled_host.py checks the coverage."""
    pick = lambda values, bi, si, j, a, b, c: values[(a * bi + b * si + c * j) % len(values)]
    out = []
    for bi, (border, _, _) in enumerate(BORDERS):
        for si, (H, W) in enumerate(SIZES):
            if border == "frame" and min(H, W) < 3:
                continue
            for j in range(2):
                T = pick(FRAMES, bi, si, j, 1, 1, 1)
                coupling = pick(COUPLINGS, bi, si, j, 1, 3, 2)
                C = 3 if coupling & vc.CHANNELS else pick(CHANNELS, bi, si, j, 0, 1, 1)
                exps = pick(TIME_EXPONENTS, bi, si, j, 1, 1, 2) if coupling & vc.TIME else pick(EXPONENTS, bi, si, j, 1, 1, 3)
                out.append((border, H, W, C, T, pick(TAUS, bi, si, j, 1, 1, 1), pick(PATTERNS, bi, si, j, 1, 1, 4),
                            pick(WEIGHTS, bi, si, j, 1, 2, 1), pick(LINKS, bi, si, j, 3, 1, 2),
                            "free" if T == 2 else pick(TIMES, bi, si, j, 1, 0, 1), pick(GT, bi, si, j, 1, 1, 1), exps, pick(EPS, bi, si, j, 0, 1, 1),
                            coupling))
    return out


def call_args(p, pen, coupling, **kw):
    """the arguments of capi.Instance.volume_coupled for an input, its penalties and its coupling"""
    return dict(rb.call_args(p, pen, **kw), coupling=coupling)


class Yardstick(rb.Yardstick):
    """volume_robust_bounds.Yardstick with the rounds, the energy and the residual of volume_coupled_np under `coupling`"""

    def __init__(self, p, pen, coupling, rounds=ROUNDS, u32=None, iters32=None):
        self.p, self.pen, self.coupling, self.rounds = p, pen, coupling, rounds
        self.unk = vw.kinds(p["sides"], p["periodic"], p["state"]) == vw.UNKNOWN
        self.exact = vc.irls_exact(p, pen, rounds, coupling)
        if u32 is None:
            u32, iters32 = vc.irls_f32(p, pen, rounds, coupling)
        self.u32, self.iters32 = u32, iters32
        self.fig32 = [self.measure(u32[k - 1] if k else None, u32[k], k) for k in range(len(u32))]
        self.err32, self.res32 = self.fig32[-1]

    def energy(self, u):
        return vc.energy(self.p, self.pen, u, self.coupling)

    def measure(self, prev, out, k=None):
        k = len(self.exact) - 1 if k is None else k
        out = vw._thwc(np.asarray(out))
        err = float(np.abs(out.astype(np.float64) - self.exact[k])[self.unk].max()) / self.p["range"]
        return err, vc.round_residual(self.p, self.pen, prev if k else None, out, self.coupling)

    def bounds(self, k=None):
        err32, res32 = self.fig32[-1 if k is None else k]
        return max(ERR_FACTOR * err32, ERR_FLOOR), max(RES_FACTOR * res32, RES_FLOOR)


@functools.lru_cache(maxsize=None)
def matrix_case(i):
    """(input, its penalties, its coupling, its Yardstick) of matrix()[i], computed once per process and shared; nobody writes into them"""
    border, H, W, C, T, tau, pattern, wkind, links, time, gt, exps, epsf, coupling = matrix()[i]
    p = make_input(border, H, W, C, T, tau, pattern, wkind, links, time, gt)
    pen = penalties(p, exps, epsf)
    return p, pen, coupling, Yardstick(p, pen, coupling)


# ---- the disc (tests/test_gpu_volume_coupled.py: isotropic against anisotropic total variation)
def disc_problem(T=4, H=16, W=16, lam=4.0, noise=0.05, seed=5):
    """(problem, pen): tv_denoise_video's problem on a noisy disc that drifts by a pixel per frame -- one channel, Neumann borders, every
    state UNKNOWN, zero guidance, weight lam, p = r = 1, q = 2"""
    y, x = np.mgrid[0:H, 0:W]
    clean = np.stack([((x - (W / 2 - 1 + t)) ** 2 + (y - H / 2) ** 2 <= (min(H, W) / 3.2) ** 2).astype(np.float64) for t in range(T)])
    frames = (clean + noise * np.random.default_rng(seed).standard_normal(clean.shape)).astype(np.float32).reshape(T, H, W, 1)
    zero = np.zeros_like(frames)
    p = dict(sides="lrtb", periodic="", tper=False, state=zero.copy(), weight=np.full(frames.shape, lam, np.float32), sx=None, sy=None, smt=None,
             tau=1.0, gx=zero, gy=zero, gt=None, data=frames, boundary=None, range=float(frames.max() - frames.min()))
    eps = float(np.float32(1e-2))
    return p, (1.0, 1.0, 2.0, eps, eps, eps)
