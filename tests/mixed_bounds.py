"""The two quantities the GPU tests of the per-side free borders (SC_POISSON_FREE_*) hold the solver to, their bounds, and the inputs
of the length walk (shared by tests/test_gpu_mixed.py, tests/test_gpu_mixed_lengths.py and tools/mixed_border_probe.py).

    RES  max |(A - lam) u - rhs| / max |rhs|       A: the operator of the side combination, in float64 (mixed_np.residual)
    ERR  max |u - solve_exact| / R,  R = max |solve_exact|

Float32 transforms:  measured <= max(FACTOR x the same quantity for mixed_np.solve_f32 on the same input, FLOOR).  The four constants
come from one MI355X run of tools/mixed_border_probe.py --lengths over length_cases() (DESIGN.md section 4 holds the table,
profiles/mixed_lengths.txt the record), by the project's rule: each factor is the worst ratio to the restatement over the inputs with
more than 3 unknowns along the walked axis, times 2, rounded up to one digit; each floor twice the worst absolute value at 1 to 3
unknowns, where the restatement is unusually exact, rounded up likewise.  Nothing is taken from the Neumann or the screened constants:
an axis with one Dirichlet end has its lowest eigenvalue at ~(pi / (2n + 1))^2, a quarter of the Dirichlet axis's.
The smooth low-mode reconstructions have a factor of their own, by the same rule over them alone.  There the restatement sits at its
floor -- 3e-7 .. 9e-7, a float32 ulp of the image, whatever the length: pocketfft's rounding is relative to each coefficient -- while a
chirp convolution rounds relative to the largest product in the row, and the lowest eigenvalue amplifies that: beside two free ends 9
pixels apart the strips of 2048 and 4096 unknowns reach 5e-5 .. 4e-4 (125 to 688 times the restatement), beside two Dirichlet lines
1e-6 (2 times).  The finding of DESIGN.md section 4; a wrong low coefficient is an error of the size of the image, 1000 times the bound.
Double transforms (SC_FLAG_FFT_FP64), the project's existing bounds:  ERR within F64_ULPS float32 ulps of max |exact| (the result is
stored in float32); RES <= 1e-6 on the white-noise reconstruction only."""
import numpy as np

import mixed_np

RES_FACTOR, RES_FLOOR = 8.0, 8e-6             # measured: worst ratio 3.73 (5 unknowns along y, reconstruction), worst value at 1 to 3 unknowns 3.68e-6
ERR_FACTOR, ERR_FLOOR = 70.0, 2e-6            # measured: worst ratio 34.2 (300 along x, N-D, free top and bottom, reconstruction), worst value at 1 to 3 unknowns 6.02e-7
ERR_SMOOTH_FACTOR = 2000.0                    # measured: worst ratio 688 (4096 along x, D-N, free top and bottom), on the smooth inputs alone
F64_ULPS, F64_RES = 4, 1e-6

LENGTHS = [1, 2, 3, 5, 24, 32, 40, 129, 300]      # unknowns along the walked axis: 1 .. 5; M = 48 (r = 3), 64, 80 (r = 5); more than one element per thread; 300
STRIP32, STRIP64 = 4096, 2048                     # one strip each way per precision
OTHER = 9                                         # pixels the other way


def err_and_res(sides, lam, u, data, lap, want):
    """(ERR, RES) of u against want = solve_exact(...)"""
    f = mixed_np.rhs(sides, lam, data, lap)
    scale = float(np.abs(f).max())
    shape = f.shape
    res = float(np.abs(mixed_np.residual(sides, lam, np.asarray(u).reshape(shape), data, lap)).max()) / (scale if scale > 0 else 1.0)
    return float(np.abs(np.asarray(u, np.float64) - want).max()) / float(np.abs(want).max()), res


class Yardstick:
    """One input's references: want = solve_exact, and the float32 restatement's (ERR, RES) on it."""

    def __init__(self, sides, lam, data, lap, boundary):
        self.args = (sides, lam, data, lap)
        self.want = mixed_np.solve_exact(sides, lam, data, lap, boundary)
        self.R = float(np.abs(self.want).max())
        self.err32, self.res32 = err_and_res(sides, lam, mixed_np.solve_f32(sides, lam, data, lap, boundary), data, lap, self.want)

    def bounds(self, smooth=False):
        return max((ERR_SMOOTH_FACTOR if smooth else ERR_FACTOR) * self.err32, ERR_FLOOR), max(RES_FACTOR * self.res32, RES_FLOOR)

    def measure(self, out):
        sides, lam, data, lap = self.args
        return err_and_res(sides, lam, out, data, lap, self.want)

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


def rough_inputs(W, H, C, seed):
    """[(name, gx, gy, boundary)]: the reconstruction of a white-noise image, and a random guidance field (sigma 20) with a random
    boundary"""
    rng = np.random.default_rng(seed)
    img = rng.uniform(-50, 300, (H, W, C)).astype(np.float32)
    fx, fy = mixed_np.forward_differences(img)
    b = rng.uniform(-100, 400, (H, W, C)).astype(np.float32)
    gx = rng.normal(0, 20, (H, W, C)).astype(np.float32)
    gy = rng.normal(0, 20, (H, W, C)).astype(np.float32)
    return [("reconstruction", fx, fy, img), ("random", gx, gy, b)]


def smooth_input(W, H, C, seed):
    sm = mixed_np.smooth_image(H, W, C, seed)
    fx, fy = mixed_np.forward_differences(sm)
    return ("smooth", fx, fy, sm)


def walked_sides(axis, reverse, other_free):
    """the side combination whose `axis` has a Dirichlet line at its low end and a free high end (reverse: the other way round), the
    other axis between two Dirichlet lines or, other_free, between two free ends"""
    if axis == "x":
        return ("l" if reverse else "r") + ("tb" if other_free else "")
    return ("t" if reverse else "b") + ("lr" if other_free else "")


def length_cases():
    """[(n, axis, sides, W, H, precisions)]: every length class the kernel can get wrong, once along x and once along y, for both
    orders of the two ends and both kinds of the other axis; n unknowns are n + 1 pixels beside one Dirichlet line."""
    cases = []
    for n in LENGTHS + [STRIP64, STRIP32]:
        for axis in "xy":
            for reverse in (False, True):
                for other_free in (False, True):
                    W, H = (n + 1, OTHER) if axis == "x" else (OTHER, n + 1)
                    cases.append((n, axis, walked_sides(axis, reverse, other_free), W, H, ("f32",) if n > STRIP64 else ("f32", "f64")))
    return cases
