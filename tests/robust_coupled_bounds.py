"""The quantities the GPU tests of the robust solve's coupled forms hold the library to (tests/test_gpu_robust_coupled.py), their bounds
and their cases, after the pattern of tests/robust_bounds.py with tests/robust_coupled_np.py as the restatement.  Every run is ROUNDS = 8
fixed rounds (round_tol = -1) behind the quadratic one:

    ERR     max |u - irls_exact| / R        u the last iterate, irls_exact the float64 rounds with exact inner solves, R the data's range
    RES     max |L u - rhs| / max |rhs|     of the last round's system: L and rhs from the iterate before the last (the library's own,
                                            read from a run of ROUNDS - 1 rounds): every link weight of the coupled rule enters it
    ENERGY  |sc_hip_robust_trace's last energy - robust_coupled_np.energy of the written iterate| / that energy

Bounds:  ERR and RES <= max(FACTOR x the same quantity for robust_coupled_np.irls_f32 on the same input, FLOOR); ENERGY <= ENERGY_REL.
The constants are this family's own, not robust_bounds': they come from one MI355X run of tools/robust_probe.py --lengths --coupling all
over these cases and a length walk (DESIGN.md section 4 holds the table, profiles/robust_coupled_lengths.txt the record): each factor is
twice the worst ratio to the restatement, rounded up to one digit; each floor twice the worst value among the inputs where the
restatement's figure is 0 (none occurred: the floors are 0); ENERGY_REL twice the worst relative difference, rounded up to one digit.
The library and the restatement share the algorithm but not the summation order of the device's dot products."""
import numpy as np

import robust_bounds as rb
import robust_coupled_np as rc

ROUNDS = rb.ROUNDS
ERR_FACTOR, ERR_FLOOR = 8.0, 0.0               # measured: worst ratio 3.98 (isotropic, neumann 6 x 4 x 3, p = 1, q = 2, eps 1e-3, sparse weights); no input where irls_f32's ERR is 0
RES_FACTOR, RES_FLOOR = 4.0, 0.0               # measured: worst ratio 1.58 (both bits, neumann 6 x 3 x 3, p = 1, q = 2, eps 1e-3, sparse weights); no input where irls_f32's RES is 0
ENERGY_REL = 2e-7                              # measured: worst 8.57e-8 (both bits, free left + top 16 x 5 x 3, p = 1.5, q = 2, eps 1e-2, dense weights)

ISO, JOINT = rc.ISO, rc.JOINT
COUPLINGS = (ISO, JOINT, ISO | JOINT)
BORDERS = rb.BORDERS
SMALL = [(47, 33), (5, 16), (7, 2)]              # rows x columns: several row bands, a block smaller than a band, a two-row image
# rows x columns, channels: the west neighbour's rho lies across the 256-column group; two column groups and three row bands, a
# north-west corner read across both boundaries at once
LARGE = [((9, 300), 2), ((17, 300), 3)]
LARGE_BORDERS = ["neumann", "frame", "periodic_xy"]


def accuracy_cases():
    """[(border, (H, W), (p, q), eps factor, base links?, weight kind, C, coupling)]: every border at every small size, three channels,
    the couplings and the exponents taking turns so that each occurs at every size and under every border and every pair of them
    occurs, the other options in turn as in robust_bounds.accuracy_cases; then the full product of the couplings and the options at
    16 x 5 under free left + top"""
    cases, i = [], 0
    for bi, (b, _, _) in enumerate(BORDERS):
        for si, (H, W) in enumerate(SMALL):
            cases.append((b, (H, W), rb.PQ[(2 * bi + si) % 3], rb.EPS[(i // 3) % 2], bool((i // 2) % 2), rb.WEIGHTS[i % 2], 3, COUPLINGS[(bi + si) % 3]))
            i += 1
    for cpl in COUPLINGS:
        for pq in rb.PQ:
            for eps in rb.EPS:
                for links in (False, True):
                    for wk in rb.WEIGHTS:
                        cases.append(("free_lt", (5, 16), pq, eps, links, wk, 3, cpl))
    return [c for c in dict.fromkeys(cases) if not (c[0] == "frame" and min(c[1]) < 3)]


def large_cases():
    """the same tuples at the two 300-column shapes: RES and ENERGY only (no dense solve of 5100 unknowns); every coupling under a
    border without Dirichlet lines, under a frame (both low-side Dirichlet lines own live links) and under two periodic axes"""
    cases, i = [], 0
    for (size, C) in LARGE:
        for b in LARGE_BORDERS:
            for cpl in COUPLINGS:
                cases.append((b, size, rb.PQ[i % 3], rb.EPS[(i // 3) % 2], bool((i // 2) % 2), rb.WEIGHTS[i % 2], C, cpl))
                i += 1
    return cases


def case_id(c):
    border, (H, W), (p, q), epsf, links, wk, C, cpl = c
    return f"{rc.NAMES[cpl]}-{border}-{W}x{H}x{C}-p{p}-q{q}-eps{epsf:g}-{'links' if links else 'unit'}-{wk}"


class Yardstick:
    """One input's references under one coupling: the exact rounds' iterates (exact=False: none, ERR is not measured) and irls_f32's
    (ERR, RES, inner iterations) on it"""

    def __init__(self, sides, periodic, p, q, eps_g, eps_d, a, coupling, rounds=ROUNDS, exact=True):
        self.border = (sides, periodic)
        self.pen = (p, q, eps_g, eps_d)
        self.a = a
        self.coupling = coupling
        self.fixed = (a["weight"], a["cx"], a["cy"], a["gx"], a["gy"], a["data"])
        self.exact = rc.irls_exact(sides, periodic, p, q, eps_g, eps_d, *self.fixed, a["boundary"], rounds, coupling) if exact else None
        self.want = self.exact[-1] if exact else None
        self.u32, self.iters32 = rc.irls_f32(sides, periodic, p, q, eps_g, eps_d, *self.fixed, a["boundary"], rounds, coupling)
        self.err32, self.res32 = self.measure(self.u32[-2], self.u32[-1])

    def energy(self, u, coupling=None):
        return rc.energy(*self.border, *self.pen, *self.fixed, u, self.coupling if coupling is None else coupling)

    def measure(self, prev, out):
        """(ERR, RES) of the last iterate `out`, `prev` the iterate before it; ERR is 0 without the exact rounds"""
        shape = self.u32[0].shape
        err = float(np.abs(np.asarray(out, np.float64).reshape(shape) - self.want).max()) / self.a["range"] if self.want is not None else 0.0
        res = rc.round_residual(*self.border, *self.pen, *self.fixed, np.asarray(prev).reshape(shape), np.asarray(out).reshape(shape), self.coupling)
        return err, res

    def check(self, prev, out):
        """[(quantity, measured, bound)] that fail, and the measured (ERR, RES)"""
        err, res = self.measure(prev, out)
        eb, rb_ = max(ERR_FACTOR * self.err32, ERR_FLOOR), max(RES_FACTOR * self.res32, RES_FLOOR)
        bad = ([("ERR", err, eb)] if not err <= eb else []) + ([("RES", res, rb_)] if not res <= rb_ else [])
        return bad, err, res


_yard = {}


def yardstick(case, exact=True):
    """(Yardstick, the problem with NaN in its dead links, sides, periodic, eps) of one case, computed once"""
    if case not in _yard:
        border, (H, W), (p, q), epsf, links, wk, C, cpl = case
        sides, periodic = {b[0]: b[1:] for b in BORDERS}[border]
        a = rb.with_dead_nan(sides, periodic, rb.make_input(H, W, C, wk, links))
        eps = epsf * a["range"]
        _yard[case] = (Yardstick(sides, periodic, p, q, eps, eps, a, cpl, exact=exact), a, sides, periodic, eps)
    return _yard[case]


def disc_image():
    """Test 8's image, float32 20 x 24 x 3: a disc of radius 7 about (x, y) = (11.3, 9.6), channel amplitudes (1, 0.7, -0.5), noise of
    sigma 0.1 from default_rng(5)"""
    y, x = np.mgrid[0:20, 0:24].astype(np.float64)
    disc = ((x - 11.3) ** 2 + (y - 9.6) ** 2 <= 49.0).astype(np.float64)
    img = disc[:, :, None] * np.array([1.0, 0.7, -0.5])[None, None, :]
    return (img + 0.1 * np.random.default_rng(5).standard_normal(img.shape)).astype(np.float32)
