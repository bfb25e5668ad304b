"""The two quantities the GPU tests hold the direct float32 Poisson and screened solves to, their bounds per family of borders, and the
inputs of the length walks (shared by the tests/test_gpu_{neumann,screened,mixed,periodic}*.py files, their host companions and the
probes under tools/).

    RES  max |(A - lam) u - rhs| / max |rhs|       A: the operator of the border combination, in float64 (direct_np.operator); a
                                                   singular system: rhs less its mean, which the solve ignores
    ERR  max |u - solve_exact| / R,  R = max |solve_exact|      (a singular system: solve_exact plus the mean of boundary)

RES is not amplified by 1 / lambda_min: the float32 restatement (direct_np.solve_f32) stays within 2.5e-8 .. 5.5e-7 from 2 x 2 to
8192 x 64 of the Neumann problem where its ERR varies a thousandfold, so a wrong coefficient at any but the lowest few k shows in it
at full size.

Float32 transforms:  measured <= max(FACTOR x the same quantity for direct_np.solve_f32 on the same input, FLOOR).  Each family's
constants come from one MI355X run over its length walk (DESIGN.md section 4 holds the tables, profiles/*_lengths.txt the records),
by the project's rule: each factor is the worst ratio to the restatement over the inputs with more than 3 unknowns along the walked
axis, times 2, rounded up to one digit; each floor twice the worst absolute value at 1 to 3 unknowns, where the restatement is
unusually exact, rounded up likewise.  No family takes a constant from another: an axis with one Dirichlet end has its lowest
eigenvalue at ~(pi / (2n + 1))^2, a quarter of the Dirichlet axis's; a periodic axis's lowest non-zero one is ~(2 pi / n)^2, four
times the free-free axis's, and its restatement is a plain complex FFT.
The smooth low-mode reconstructions have a factor of their own where a family measured one, by the same rule over them alone.
There the restatement sits at its floor -- 3e-7 .. 9e-7, a float32 ulp of the image, whatever the length: pocketfft's rounding is
relative to each coefficient -- while a chirp convolution rounds relative to the largest product in the row, and the lowest
eigenvalue amplifies that: beside two free ends 9 pixels apart the strips of 2048 and 4096 unknowns reach 5e-5 .. 4e-4 (125 to 688
times the restatement), beside two Dirichlet lines 1e-6 (2 times).  The finding of DESIGN.md section 4; a wrong low coefficient is
an error of the size of the image, 1000 times the bound.
Double transforms (SC_FLAG_FFT_FP64):  ERR within f64_ulps float32 ulps of max |want| (the result is stored in float32: half an ulp,
and the mean's addition another); RES <= f64_res on rough inputs only (five terms of size <= R rounded to 6e-8 each, against max
|lap| >~ R on a rough input; a smooth input's max |lap| ~ R lambda is as small as one likes) -- of these the white-noise
reconstruction only, except for the Neumann family (the solution of a random guidance field is a random walk, R ~ 10 max |lap|
along a strip of 4096: the float32 rounding of the stored result alone leaves RES 1.9e-6 there, and its callers pass rough=False)."""
from dataclasses import dataclass

import numpy as np

import direct_np as dn


@dataclass(frozen=True)
class Bounds:
    """One family's constants, and the three conventions of the restatement they were measured against: a bound is a factor over the
    restatement's own figure, so the figure has to be the one of the measuring run, to the bit."""
    res_factor: float
    res_floor: float
    err_factor: float
    err_floor: float
    err_smooth_factor: float = None          # None: the smooth inputs are held to err_factor
    f64_ulps: int = 4
    f64_res: float = None                    # None: RES is not asserted under double transforms
    f64_res_needs_reconstruction: bool = True
    order: str = dn.ROWS_FIRST               # of solve_f32's real transforms
    exact_order: str = dn.ROWS_FIRST         # of solve_exact's (rounding only; ERR of the restatement is measured against it)
    by_differences: bool = False             # direct_np.operator's form, and max |rhs| taken after the singular system's centring

    def yardstick(self, sides, periodic, lam, data, lap, boundary):
        return Yardstick(sides, periodic, lam, data, lap, boundary, bounds=self)


# measured against neumann_np (tests/test_gpu_neumann_lengths.py, profiles/neumann_lengths.txt), the problem ("lrtb", ""), lam = 0
NEUMANN = Bounds(res_factor=8.0, res_floor=1.5e-6,           # measured: worst ratio 3.6 (8192 x 64), worst value at 2 or 3 pixels 7.1e-7
                 err_factor=60.0, err_floor=1.3e-6,          # measured: worst ratio 29.8 (2048 x 9, random guidance), worst value at 2 or 3 pixels 6.2e-7
                 f64_res=1e-6, f64_res_needs_reconstruction=False, exact_order=dn.COLUMNS_FIRST, by_differences=True)
# measured against screened_np's Neumann form (tools/screened_probe.py --lengths, profiles/screened_lengths.txt), ("lrtb", ""), lam > 0
SCREENED = Bounds(res_factor=7.0, res_floor=3.3e-6,          # measured: worst ratio 3.19 (6 x 9, lam 1e-3), worst value at 2 or 3 pixels 1.62e-6 (3 x 7, lam 0.1)
                  err_factor=40.0, err_floor=1.8e-5,         # measured: worst ratio 16.5 (33 x 7, lam 1e-3), worst value at 2 or 3 pixels 8.8e-6 (2 x 7, lam 1e-3)
                  exact_order=dn.COLUMNS_FIRST, by_differences=True)
# measured against mixed_np (tools/mixed_border_probe.py --lengths over mixed_length_cases(), profiles/mixed_lengths.txt)
MIXED = Bounds(res_factor=8.0, res_floor=8e-6,               # measured: worst ratio 3.73 (5 unknowns along y, reconstruction), worst value at 1 to 3 unknowns 3.68e-6
               err_factor=70.0, err_floor=2e-6,              # measured: worst ratio 34.2 (300 along x, N-D, free top and bottom, reconstruction), worst value at 1 to 3 unknowns 6.02e-7
               err_smooth_factor=2000.0,                     # measured: worst ratio 688 (4096 along x, D-N, free top and bottom), on the smooth inputs alone
               f64_res=1e-6)
# measured against periodic_np (tools/periodic_probe.py --lengths over periodic_length_cases(), profiles/periodic_lengths.txt): factors
# over the inputs with a periodic length above 3, floors at lengths 2 and 3; the smooth reconstructions from 256 pixels up
PERIODIC = Bounds(res_factor=10.0, res_floor=6e-6,           # measured: worst ratio 4.51 (8192 along x, top and bottom Dirichlet lines, random guidance), worst value at lengths 2 and 3 2.91e-6
                  err_factor=40.0, err_floor=4e-6,           # measured: worst ratio 19.6 (8192 along x, free top and bottom, reconstruction), worst value at lengths 2 and 3 1.93e-6
                  err_smooth_factor=700.0,                   # measured: worst ratio 345 (4096 along x, y periodic too), on the smooth inputs alone
                  f64_res=1e-6, order=dn.ROWS_FIRST_BOTH_WAYS, exact_order=dn.ROWS_FIRST_BOTH_WAYS)


def err_and_res(sides, periodic, lam, u, data, lap, want, by_differences=False):
    """(ERR, RES) of u against want"""
    f = dn.rhs(sides, periodic, lam, data, lap)
    r = dn.operator(sides, periodic, lam, np.asarray(u).reshape(f.shape), by_differences)
    f64 = f.astype(np.float64)
    if dn.singular(sides, periodic, lam):
        blk = dn.unknowns(sides, periodic, *f.shape[:2])
        f64[blk] -= f64[blk].mean(axis=(0, 1))
    scale = float(np.abs(f64 if by_differences else f).max())
    res = float(np.abs(r - f64).max()) / (scale if scale > 0 else 1.0)
    return float(np.abs(np.asarray(u, np.float64) - want).max()) / float(np.abs(want).max()), res


class Yardstick:
    """One input's references: want = solve_exact (a singular system: plus the per-channel mean of boundary, 0 without one), and the
    float32 restatement's (ERR, RES) on it."""

    def __init__(self, sides, periodic, lam, data, lap, boundary, *, bounds):
        self.args = (sides, periodic, lam, data, lap)
        self.b = bounds
        mean = 0.0
        if dn.singular(sides, periodic, lam) and boundary is not None:
            mean = dn.mean_of(boundary)
        self.want = dn.solve_exact(sides, periodic, lam, data, lap, boundary, order=bounds.exact_order) + mean
        self.R = float(np.abs(self.want).max())
        self.u32 = dn.solve_f32(sides, periodic, lam, data, lap, boundary, order=bounds.order) + np.asarray(mean, np.float32)
        self.err32, self.res32 = self.measure(self.u32)

    def bounds(self, smooth=False):
        b = self.b
        return max((b.err_smooth_factor if smooth and b.err_smooth_factor else b.err_factor) * self.err32, b.err_floor), max(b.res_factor * self.res32, b.res_floor)

    def measure(self, out):
        return err_and_res(*self.args[:3], out, *self.args[3:], self.want, self.b.by_differences)

    def check(self, out, fp64, rough=True, reconstruction=False):
        """[(quantity, measured, bound)] that fail, and the measured (ERR, RES).  rough: RES is asserted as well -- float32: every input
        but the smooth ones (their max |rhs| is as small as one likes); double: where the family has an f64_res, and but for the
        Neumann family on the white-noise reconstruction only."""
        err, res = self.measure(out)
        if fp64:
            ulps = err * self.R / float(np.spacing(np.float32(self.R)))
            bad = [("ERR ulps", ulps, self.b.f64_ulps)] if not ulps <= self.b.f64_ulps else []
            asserted = self.b.f64_res is not None and rough and (reconstruction or not self.b.f64_res_needs_reconstruction)
            if asserted and not res <= self.b.f64_res:
                bad.append(("RES", res, self.b.f64_res))
        else:
            eb, rb = self.bounds(smooth=not rough)
            bad = ([("ERR", err, eb)] if not err <= eb else []) + ([("RES", res, rb)] if rough and not res <= rb else [])
        return bad, err, res


def rough_inputs(W, H, C, seed, periodic=""):
    """[(name, gx, gy, boundary)]: the reconstruction of a white-noise image (its forward differences, wrapped along a periodic axis),
    and a random guidance field (sigma 20) with a random boundary"""
    rng = np.random.default_rng(seed)
    img = rng.uniform(-50, 300, (H, W, C)).astype(np.float32)
    fx, fy = dn.forward_differences(img, periodic)
    b = rng.uniform(-100, 400, (H, W, C)).astype(np.float32)
    gx = rng.normal(0, 20, (H, W, C)).astype(np.float32)
    gy = rng.normal(0, 20, (H, W, C)).astype(np.float32)
    return [("reconstruction", fx, fy, img), ("random", gx, gy, b)]


def smooth_input(W, H, C, seed, periodic=""):
    sm = dn.smooth_image(H, W, C, seed)
    fx, fy = dn.forward_differences(sm, periodic)
    return ("smooth", fx, fy, sm)


# ---- the length walk of the free sides: an axis between a Dirichlet line and a free end
MIXED_LENGTHS = [1, 2, 3, 5, 24, 32, 40, 129, 300]      # unknowns along the walked axis: 1 .. 5; M = 48 (r = 3), 64, 80 (r = 5); more than one element per thread; 300
MIXED_STRIP32, MIXED_STRIP64 = 4096, 2048               # one strip each way per precision
OTHER = 9                                               # pixels the other way, in both walks


def walked_sides(axis, reverse, other_free):
    """the side combination whose `axis` has a Dirichlet line at its low end and a free high end (reverse: the other way round), the
    other axis between two Dirichlet lines or, other_free, between two free ends"""
    if axis == "x":
        return ("l" if reverse else "r") + ("tb" if other_free else "")
    return ("t" if reverse else "b") + ("lr" if other_free else "")


def mixed_length_cases():
    """[(n, axis, sides, W, H, precisions)]: every length class the kernel can get wrong, once along x and once along y, for both
    orders of the two ends and both kinds of the other axis; n unknowns are n + 1 pixels beside one Dirichlet line."""
    cases = []
    for n in MIXED_LENGTHS + [MIXED_STRIP64, MIXED_STRIP32]:
        for axis in "xy":
            for reverse in (False, True):
                for other_free in (False, True):
                    W, H = (n + 1, OTHER) if axis == "x" else (OTHER, n + 1)
                    cases.append((n, axis, walked_sides(axis, reverse, other_free), W, H, ("f32",) if n > MIXED_STRIP64 else ("f32", "f64")))
    return cases


# ---- the length walk of the periodic axes
PERIODIC_LENGTHS = [2, 3, 4, 5, 24, 32, 33, 40, 129, 300]      # pixels along the periodic axis: even, odd and Nyquist classes; n = M / 2 at M = 48 (r = 3), 64, 80 (r = 5) and one beyond it; more than one element per thread
PERIODIC_STRIP32, PERIODIC_STRIP64 = 8192, 4096                # one strip each way: the float32 limit in float32, the double limit in both precisions
# the other axis: between two Dirichlet lines, free at both ends, a Dirichlet line at its low end and a free high end, periodic too
OTHER_KINDS = ["dd", "ff", "df", "p"]


def walked_borders(axis, other):
    """(sides, periodic): `axis` periodic, the other axis of kind `other` (OTHER_KINDS)"""
    lo, hi = ("t", "b") if axis == "x" else ("l", "r")
    if other == "p":
        return "", "xy"
    return {"dd": "", "ff": lo + hi, "df": hi}[other], axis


def periodic_length_cases():
    """[(n, axis, sides, periodic, W, H, precisions)]: every length class the kernel can get wrong, once along x and once along y, for
    each kind of the other axis; n pixels along the periodic axis are n unknowns."""
    cases = []
    for n in PERIODIC_LENGTHS + [PERIODIC_STRIP64, PERIODIC_STRIP32]:
        for axis in "xy":
            for other in OTHER_KINDS:
                sides, periodic = walked_borders(axis, other)
                W, H = (n, OTHER) if axis == "x" else (OTHER, n)
                cases.append((n, axis, sides, periodic, W, H, ("f32",) if n > PERIODIC_STRIP64 else ("f32", "f64")))
    return cases
