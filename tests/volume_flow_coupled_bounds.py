"""The quantities the coupled flow volume GPU tests hold the library to, their bounds and their inputs
(tests/test_gpu_volume_flow_coupled.py): tests/volume_flow_robust_bounds.py's ERR, RES and ENERGY with the rounds of
tests/volume_flow_coupled_np.py, on that file's inputs with a coupling behind each.  Every run is ROUNDS = 4 fixed rounds (round_tol =
-1) behind the quadratic one.  The shapes are the family's, already the smallest at which the walk can go wrong: 5 x 260 crosses the
256-column group, 12 x 19 under a frame starts bands inside a frame, 7 x 2 under periodic x makes east and west one pixel, T = 2 with
free time, T = 3 with periodic time.

Bounds:  ERR and RES <= max(FACTOR x the same quantity for volume_flow_coupled_np.irls_f32 on the same input, FLOOR); ENERGY <=
ENERGY_REL.  irls_f32 is the same rounds with the same inner iteration, (straight-link) preconditioner, start and stop rule: the
yardstick is the restatement, never the library.  The constants start from the wider of the two parent families' -- ERR 4
(volume_coupled_bounds), RES 20 (volume_flow_robust_bounds), ENERGY 4e-7: the rounds differ from the parents' only in how rho is formed
and where the neighbours are read -- and follow one MI355X run of tools/volume_flow_coupled_probe.py --lengths over matrix() and a length
walk (DESIGN.md section 4 holds the table, profiles/volume_flow_coupled_lengths.txt the record) by the project's rule: each factor is
twice the worst ratio to the restatement, rounded up to one digit; each floor twice the worst value among the inputs where the
restatement's figure is 0; ENERGY_REL twice the worst relative difference, rounded up to one digit.  Measured over the 57 inputs of matrix() and 44 of the walk: ERR ratio at most
1.51, RES 4.05, ENERGY 1.01e-7, so ERR stays 4, RES comes down to 9 (the uncoupled flow call's 7.23 was one input's, which has another
coupling here) and ENERGY_REL to 3e-7.

Condition on the inputs: on every one of them every round of irls_f32 stops by its rule (rel <= 1e-5) within max_iters = 400
(tests/test_volume_flow_coupled_host.py asserts it).  The matrix before the rule, raw_matrix(), was scanned on the CPU; what does not
stop lies in the regime volume_flow_robust_bounds names -- temporal weights that outgrow the spatial ones under a flow that moves
pixels, against a preconditioner with straight time links -- and substitute() is that module's rule, stated on this matrix's tuple:

    exponents (2, 1, 2) -- nothing but time is reweighted; no form with TIME has them, and SPACE changes nothing at p = 2 -- at eps 1e-3
    of the range, under a flow that moves pixels (not one of STILL_FLOWS), run at eps 1e-2 in place of 1e-3 and with tau 1 in place of
    10.  The flow and the coupling stay.

Of raw_matrix() 56 of 57 inputs stop as they stand (worst 315 of 400); the one that does not, 12 x 19 x 3 x 8 under periodic x and y
with pan and SPACE (ineffective at p = 2: the uncoupled launch), ran 400 iterations in three rounds (rel 2.4e-5) and stops under the
rule.  The rule alters the inputs ALTERED, at most one in eight; every coupling, every flow kind and both time modes still occur with
a flow that is not zero at least twice (the host test checks all of it)."""
import functools

import numpy as np

import volume_coupled_bounds as vcb
import volume_flow_bounds as vfb
import volume_flow_coupled_np as vfc
import volume_flow_robust_bounds as frb
import volume_wls_np as vw

ROUNDS = frb.ROUNDS
MAX_ITERS = frb.MAX_ITERS                      # sc_volume_robust_params' default
ERR_FACTOR, ERR_FLOOR = 4.0, 0.0               # measured: worst ratio 1.51 (neumann 6 x 3 x 3, 4 frames, tau 10, split, sparse, links t, free time, (1.5, 0.8, 2), eps 1e-2, random, SPACE|CHANNELS: the length walk's); no input where irls_f32's ERR is 0
RES_FACTOR, RES_FLOOR = 9.0, 0.0               # measured: worst ratio 4.05 (free left + top 31 x 7 x 3, 3 frames, tau 10, split, sparse, links xy, periodic time, (1, 2, 1), eps 1e-3, collapse, CHANNELS: the stop rule is the 2-norm's, RES the max norm's); no input where irls_f32's RES is 0
ENERGY_REL = 3e-7                              # measured: worst 1.01e-7 (periodic xy 16 x 5 x 3, 3 frames, tau 0.1, every state 0, no weight, links xyt, free time, (0.8, 0.8, 2), eps 1e-3, zero, SPACE|TIME)

BORDERS, SIZES, FLOWS, TIMES = frb.BORDERS, frb.SIZES, frb.FLOWS, frb.TIMES
COUPLINGS = list(vfc.LEGAL)
TIME_EXPONENTS = vcb.TIME_EXPONENTS
STILL_FLOWS = frb.STILL_FLOWS


def raw_matrix():
    """matrix() before the substitution rule: volume_flow_robust_bounds.raw_matrix()'s tuple with a coupling behind it -- (border, H,
    W, C, T, tau, pattern, wkind, links, time, gt, exponents, eps factor, flow, coupling).  Input i has flow FLOWS[i mod 7] there and
    takes coupling COUPLINGS[i mod 5] here: 5 and 7 share no factor, so the first 35 inputs hold every coupling with every flow.  A
    form with CHANNELS takes 3 channels; a form with TIME its exponents from TIME_EXPONENTS, in turn."""
    out = []
    for i, (border, H, W, C, T, tau, pattern, wkind, links, time, gt, exps, epsf, flow) in enumerate(frb.raw_matrix()):
        coupling = COUPLINGS[i % len(COUPLINGS)]
        if coupling & vfc.CHANNELS:
            C = 3
        if coupling & vfc.TIME:
            exps = TIME_EXPONENTS[i % len(TIME_EXPONENTS)]
        out.append((border, H, W, C, T, tau, pattern, wkind, links, time, gt, exps, epsf, flow, coupling))
    return out


def substitute(case):
    """the substitution rule of the module's docstring on one matrix tuple: larger eps, tau capped at 1; the flow and the coupling stay"""
    border, H, W, C, T, tau, pattern, wkind, links, time, gt, exps, epsf, flow, coupling = case
    if exps == (2.0, 1.0, 2.0) and epsf == 1e-3 and flow not in STILL_FLOWS:
        epsf, tau = 1e-2, min(tau, 1.0)
    return (border, H, W, C, T, tau, pattern, wkind, links, time, gt, exps, epsf, flow, coupling)


def matrix():
    """the inputs of the GPU tests' walk (and of tools/volume_flow_coupled_probe.py): raw_matrix() under substitute().
    tests/test_volume_flow_coupled_host.py checks the coverage."""
    return [substitute(c) for c in raw_matrix()]


ALTERED = [i for i, (a, b) in enumerate(zip(raw_matrix(), matrix())) if a != b]

make_input, nan_unread, penalties = frb.make_input, frb.nan_unread, frb.penalties


def call_args(p, pen, coupling, **kw):
    """the arguments of capi.Instance.volume_flow_coupled for an input, its penalties and its coupling"""
    return dict(frb.call_args(p, pen, **kw), coupling=coupling)


class Yardstick(frb.Yardstick):
    """volume_flow_robust_bounds.Yardstick with the rounds, the energy and the residual of volume_flow_coupled_np under `coupling`"""

    def __init__(self, p, pen, coupling, rounds=ROUNDS, u32=None, iters32=None):
        self.p, self.pen, self.coupling, self.rounds = p, pen, coupling, rounds
        self.unk = vw.kinds(p["sides"], p["periodic"], p["state"]) == vw.UNKNOWN
        self.exact = vfc.irls_exact(p, pen, rounds, coupling)
        self.rels32 = None
        if u32 is None:
            self.rels32 = []
            u32, iters32 = vfc.irls_f32(p, pen, rounds, coupling, max_iters=MAX_ITERS, rels=self.rels32)
        self.u32, self.iters32 = u32, iters32
        self.fig32 = [self.measure(u32[k - 1] if k else None, u32[k], k) for k in range(len(u32))]
        self.err32, self.res32 = self.fig32[-1]

    def energy(self, u):
        return vfc.energy(self.p, self.pen, u, self.coupling)

    def measure(self, prev, out, k=None):
        k = len(self.exact) - 1 if k is None else k
        out = vw._thwc(np.asarray(out))
        err = float(np.abs(out.astype(np.float64) - self.exact[k])[self.unk].max()) / self.p["range"]
        return err, vfc.round_residual(self.p, self.pen, prev if k else None, out, self.coupling)

    def bounds(self, k=None):
        err32, res32 = self.fig32[-1 if k is None else k]
        return max(ERR_FACTOR * err32, ERR_FLOOR), max(RES_FACTOR * res32, RES_FLOOR)


@functools.lru_cache(maxsize=None)
def matrix_case(i):
    """(input, its penalties, its coupling, its Yardstick) of matrix()[i], computed once per process and shared; nobody writes into them"""
    border, H, W, C, T, tau, pattern, wkind, links, time, gt, exps, epsf, flow, coupling = matrix()[i]
    p = make_input(border, H, W, C, T, tau, pattern, wkind, links, time, gt, flow)
    pen = penalties(p, exps, epsf)
    return p, pen, coupling, Yardstick(p, pen, coupling)


BATCH_COUPLING = vfc.SPACE | vfc.CHANNELS


@functools.lru_cache(maxsize=None)
def batch_trio():
    """(three volumes of one shape under split, random and pan, their penalties, the coupling): the batch tests' members -- those of
    volume_flow_robust_bounds.batch_trio(); nobody writes into them"""
    probs, pen = frb.batch_trio()
    return probs, pen, BATCH_COUPLING


# ---- what the call is for (tests/test_gpu_volume_flow_coupled.py): a disc that pans by PAN per frame
PAN = frb.PAN


def panning_disc(T=4, H=24, W=24, lam=4.0, noise=0.05, seed=5, pan=PAN):
    """(problem with flow and links, pen, the clean video T x H x W): volume_coupled_bounds.disc_problem's problem with the disc moved
    by `pan` per frame (it wraps) and the flow that follows it -- tv_denoise_video_along_flow's problem: one channel, Neumann borders,
    every state UNKNOWN, zero guidance, weight lam, p = r = 1, q = 2, eps 1e-2"""
    y, x = np.mgrid[0:H, 0:W]
    base = ((x - W / 2 + 4) ** 2 + (y - H / 2 + 2) ** 2 <= (min(H, W) / 3.2) ** 2).astype(np.float64)
    clean = np.stack([np.roll(base, (t * pan[1], t * pan[0]), (0, 1)) for t in range(T)])
    frames = (clean + noise * np.random.default_rng(seed).standard_normal(clean.shape)).astype(np.float32).reshape(T, H, W, 1)
    zero = np.zeros_like(frames)
    p = dict(sides="lrtb", periodic="", tper=False, state=zero.copy(), weight=np.full(frames.shape, lam, np.float32), sx=None, sy=None, smt=None,
             tau=1.0, gx=zero, gy=zero, gt=None, data=frames, boundary=None, range=float(frames.max() - frames.min()),
             flow=frb.pan_flow(T, H, W, pan))
    p["links"] = vfb.links_of(p)
    eps = float(np.float32(1e-2))
    return p, (1.0, 1.0, 2.0, eps, eps, eps), clean
