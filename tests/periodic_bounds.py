"""The two quantities the GPU tests of the periodic axes (SC_POISSON_PERIODIC_X / _Y) hold the solver to, their bounds, and the inputs
of the length walk (shared by tests/test_gpu_periodic.py, tests/test_gpu_periodic_lengths.py and tools/periodic_probe.py).

    RES  max |(A - lam) u - rhs| / max |rhs|       A: the operator of the border combination, with wrap, in float64
                                                   (periodic_np.residual; a singular system: rhs less its mean, which the solve ignores)
    ERR  max |u - solve_exact| / R,  R = max |solve_exact|      (a singular system: solve_exact plus the mean of boundary)

Float32 transforms:  measured <= max(FACTOR x the same quantity for periodic_np.solve_f32 on the same input, FLOOR).  The four
constants come from one MI355X run of tools/periodic_probe.py --lengths over length_cases() (DESIGN.md section 4 holds the table,
profiles/periodic_lengths.txt the record), by the project's rule: each factor is the worst ratio to the restatement over the inputs
with a periodic length above 3, times 2, rounded up to one digit; each floor twice the worst absolute value at lengths 2 and 3, where
the restatement is unusually exact, rounded up likewise.  Nothing is taken from the Neumann, the screened or the mixed constants: the
restatement here is a plain complex FFT, and a periodic axis's lowest non-zero eigenvalue is ~(2 pi / n)^2, four times the free-free
axis's.  The smooth low-mode reconstructions (from 256 pixels up) have a factor of their own, by the same rule over them alone: there
the restatement sits at a float32 ulp of the image while a chirp convolution rounds relative to the largest product in the row.
Double transforms (SC_FLAG_FFT_FP64), the project's existing bounds:  ERR within F64_ULPS float32 ulps of max |exact| (the result is
stored in float32); RES <= 1e-6 on the white-noise reconstruction only."""
import numpy as np

import periodic_np

RES_FACTOR, RES_FLOOR = 10.0, 6e-6            # measured: worst ratio 4.51 (8192 along x, top and bottom Dirichlet lines, random guidance), worst value at lengths 2 and 3 2.91e-6
ERR_FACTOR, ERR_FLOOR = 40.0, 4e-6            # measured: worst ratio 19.6 (8192 along x, free top and bottom, reconstruction), worst value at lengths 2 and 3 1.93e-6
ERR_SMOOTH_FACTOR = 700.0                     # measured: worst ratio 345 (4096 along x, y periodic too), on the smooth inputs alone
F64_ULPS, F64_RES = 4, 1e-6

LENGTHS = [2, 3, 4, 5, 24, 32, 33, 40, 129, 300]      # pixels along the periodic axis: even, odd and Nyquist classes; n = M / 2 at M = 48 (r = 3), 64, 80 (r = 5) and one beyond it; more than one element per thread
STRIP32, STRIP64 = 8192, 4096                         # one strip each way: the float32 limit in float32, the double limit in both precisions
OTHER = 9                                             # pixels the other way
# the other axis: between two Dirichlet lines, free at both ends, a Dirichlet line at its low end and a free high end, periodic too
OTHER_KINDS = ["dd", "ff", "df", "p"]


def _center(f, blk):
    f = f.copy()
    f[blk] -= f[blk].mean(axis=(0, 1), dtype=np.float64).astype(f.dtype)
    return f


def err_and_res(sides, periodic, lam, u, data, lap, want):
    """(ERR, RES) of u against want"""
    f = periodic_np.rhs(sides, periodic, lam, data, lap)
    scale = float(np.abs(f).max())
    shape = f.shape
    r = periodic_np.operator(sides, periodic, lam, np.asarray(u).reshape(shape))
    f64 = f.astype(np.float64)
    if periodic_np.singular(sides, periodic, lam):
        f64 = _center(f64, periodic_np.unknowns(sides, periodic, *shape[:2]))
    res = float(np.abs(r - f64).max()) / (scale if scale > 0 else 1.0)
    return float(np.abs(np.asarray(u, np.float64) - want).max()) / float(np.abs(want).max()), res


class Yardstick:
    """One input's references: want = solve_exact (a singular system: plus the per-channel mean of boundary, 0 without one), and the
    float32 restatement's (ERR, RES) on it."""

    def __init__(self, sides, periodic, lam, data, lap, boundary):
        self.args = (sides, periodic, lam, data, lap)
        mean = 0.0
        if periodic_np.singular(sides, periodic, lam) and boundary is not None:
            b = np.asarray(boundary, np.float64)
            mean = b.mean(axis=(0, 1))
        self.want = periodic_np.solve_exact(sides, periodic, lam, data, lap, boundary) + mean
        self.R = float(np.abs(self.want).max())
        f32 = periodic_np.solve_f32(sides, periodic, lam, data, lap, boundary) + np.asarray(mean, np.float32)
        self.err32, self.res32 = err_and_res(sides, periodic, lam, f32, data, lap, self.want)

    def bounds(self, smooth=False):
        return max((ERR_SMOOTH_FACTOR if smooth else ERR_FACTOR) * self.err32, ERR_FLOOR), max(RES_FACTOR * self.res32, RES_FLOOR)

    def measure(self, out):
        sides, periodic, lam, data, lap = self.args
        return err_and_res(sides, periodic, lam, out, data, lap, self.want)

    def check(self, out, fp64, rough=True, reconstruction=False):
        """[(quantity, measured, bound)] that fail, and the measured (ERR, RES).  rough: RES is asserted as well -- float32: every input
        but the smooth ones (their max |rhs| is as small as one likes); double: the white-noise reconstruction only."""
        err, res = self.measure(out)
        if fp64:
            ulps = err * self.R / float(np.spacing(np.float32(self.R)))
            bad = [("ERR ulps", ulps, F64_ULPS)] if not ulps <= F64_ULPS else []
            if rough and reconstruction and not res <= F64_RES:
                bad.append(("RES", res, F64_RES))
        else:
            eb, rb = self.bounds(smooth=not rough)
            bad = ([("ERR", err, eb)] if not err <= eb else []) + ([("RES", res, rb)] if rough and not res <= rb else [])
        return bad, err, res


def rough_inputs(W, H, C, seed, periodic):
    """[(name, gx, gy, boundary)]: the reconstruction of a white-noise image (its wrapped forward differences), and a random guidance
    field (sigma 20) with a random boundary -- mixed_bounds.rough_inputs' distributions"""
    rng = np.random.default_rng(seed)
    img = rng.uniform(-50, 300, (H, W, C)).astype(np.float32)
    fx, fy = periodic_np.forward_differences(img, periodic)
    b = rng.uniform(-100, 400, (H, W, C)).astype(np.float32)
    gx = rng.normal(0, 20, (H, W, C)).astype(np.float32)
    gy = rng.normal(0, 20, (H, W, C)).astype(np.float32)
    return [("reconstruction", fx, fy, img), ("random", gx, gy, b)]


def smooth_input(W, H, C, seed, periodic):
    sm = periodic_np.smooth_image(H, W, C, seed)
    fx, fy = periodic_np.forward_differences(sm, periodic)
    return ("smooth", fx, fy, sm)


def walked_borders(axis, other):
    """(sides, periodic): `axis` periodic, the other axis of kind `other` (OTHER_KINDS)"""
    lo, hi = ("t", "b") if axis == "x" else ("l", "r")
    if other == "p":
        return "", "xy"
    return {"dd": "", "ff": lo + hi, "df": hi}[other], axis


def length_cases():
    """[(n, axis, sides, periodic, W, H, precisions)]: every length class the kernel can get wrong, once along x and once along y, for
    each kind of the other axis; n pixels along the periodic axis are n unknowns."""
    cases = []
    for n in LENGTHS + [STRIP64, STRIP32]:
        for axis in "xy":
            for other in OTHER_KINDS:
                sides, periodic = walked_borders(axis, other)
                W, H = (n, OTHER) if axis == "x" else (OTHER, n)
                cases.append((n, axis, sides, periodic, W, H, ("f32",) if n > STRIP64 else ("f32", "f64")))
    return cases
