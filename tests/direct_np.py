"""The test side's restatement of the direct float32 Poisson and screened solves (sc_hip_poisson*, sc_hip_screened*), numpy only.

A problem's borders are (sides, periodic).  `sides` is a string over "lrtb": the sides WITHOUT a Dirichlet line.  A side that is not
named keeps known values on its outermost row or column (corners included); a named side's outermost pixels are unknowns and the
stencil lacks the neighbour beyond them.  `periodic` is "", "x", "y" or "xy", the axes that wrap: all pixels of a periodic axis are
unknowns, the neighbour beyond either end is the pixel at the other end (at length 2 the same pixel twice), and `sides` names no side
of it.  ("", ""): the Dirichlet frame; ("lrtb", ""): the Neumann problem (SC_POISSON_NEUMANN).  Per channel the library solves
    (A - lam) u = lap - lam d        at the unknowns (lam = 0: the unscreened system, no data term),
lap given (SC_POISSON_LAPLACIAN) or the float32 divergence of a guidance field (divergence()).  rhs() is the library's float32
right-hand side to the letter: the product lam * d rounded to float32, then subtracted from lap.  Without a Dirichlet line and with
lam = 0 the system is singular: the solves return the mean-zero solution of the right-hand side less its mean.

operator() applies the stencil directly: what the host tests check the solves against, next to a dense assembly.  solve_exact()
solves in float64 by explicit transforms, each axis under the transform of its two ends, every one a pocketfft FFT of the axis's
odd / even extension: DST-I (length 2n + 2) between two Dirichlet lines, DCT-II (length 2n) between two free ends, between a
Dirichlet line and a free end the sine transform of odd half-frequencies (length 4n + 2), a plain complex FFT along a periodic
axis -- the real transforms first, the FFTs between them and their inverses.  No code is shared with the library, which runs chirp
convolutions.  solve_f32() is the same in single precision (complex64 FFTs, float32 denominators): the yardstick of the GPU tests'
float32 bounds (tests/direct_bounds.py).  tests/poisson_np.py solves the frame problem through the oracle's DST instead: an
independent check, not a copy.  Arrays are H x W x C (H x W accepted)."""
from __future__ import annotations

import numpy as np

ALL_SIDES = ["".join(s for s, on in zip("lrtb", (m & 1, m & 2, m & 4, m & 8)) if on) for m in range(16)]
MIXED_SIDES = ALL_SIDES[1:15]                      # the 14 combinations between the Dirichlet frame and the Neumann problem
PERIODIC = ["x", "y", "xy"]
# the nine combinations with a periodic axis: (sides, periodic), the other axis under D-D, free-D, D-free, free-free, or periodic too
COMBOS = [(s, "x") for s in ("", "t", "b", "tb")] + [(s, "y") for s in ("", "l", "r", "lr")] + [("", "xy")]
DD, NN, DN, ND, PP = 0, 1, 2, 3, 4                 # an axis's ends (low, high): D a Dirichlet line, N free; PP a periodic axis

# The order of the two real transforms, (forward, inverse) as array axes: 1 runs along the rows (x), 0 along the columns (y).  The
# float64 results differ by rounding only; every float32 bound is a factor over solve_f32's own error, so each family of tests keeps
# the order its constants were measured against (tests/direct_bounds.py names it per family).  With a periodic axis there is at most
# one real transform and the orders coincide.
ROWS_FIRST = "rows first"                          # x then y, back y then x: the library's documented order.
#                                                    The float32 yardstick of the Neumann, screened and free-side (mixed) constants.
ROWS_FIRST_BOTH_WAYS = "rows first both ways"      # x then y, back x then y.  The float32 yardstick of the periodic constants, and
#                                                    the preconditioner of the PCG yardsticks (weighted_np._precond) of the weighted,
#                                                    WLS and robust constants.
COLUMNS_FIRST = "columns first"                    # y then x, back x then y.  The table of tests/test_neumann_lengths_host.py, and
#                                                    the float64 reference the Neumann and screened constants were measured against.
ORDERS = {ROWS_FIRST: ((1, 0), (0, 1)), ROWS_FIRST_BOTH_WAYS: ((1, 0), (1, 0)), COLUMNS_FIRST: ((0, 1), (1, 0))}


def _hwc(a):
    return a[:, :, None] if a.ndim == 2 else a


def check_borders(sides, periodic=""):
    if not isinstance(sides, str) or any(ch not in "lrtb" for ch in sides):
        raise ValueError(f"sides {sides!r}: a string over 'lrtb'")
    if not isinstance(periodic, str) or any(ch not in "xy" for ch in periodic):
        raise ValueError(f"periodic {periodic!r}: a string over 'xy'")
    if ("x" in periodic and ("l" in sides or "r" in sides)) or ("y" in periodic and ("t" in sides or "b" in sides)):
        raise ValueError(f"sides {sides!r} name a side of a periodic axis ({periodic!r})")
    return sides, periodic


def axis_kinds(sides, periodic=""):
    """(x axis, y axis) of DD, NN, DN, ND, PP"""
    kind = lambda lo, hi: (NN if hi else ND) if lo else (DN if hi else DD)
    check_borders(sides, periodic)
    return (PP if "x" in periodic else kind("l" in sides, "r" in sides)), (PP if "y" in periodic else kind("t" in sides, "b" in sides))


def singular(sides, periodic="", lam=0.0):
    """no Dirichlet line on either axis and no screening"""
    ax, ay = axis_kinds(sides, periodic)
    return ax in (NN, PP) and ay in (NN, PP) and not lam


def unknowns(sides, periodic, H, W):
    """(rows, columns) of the unknown block as slices"""
    check_borders(sides, periodic)
    rows = slice(0, H) if "y" in periodic else slice(0 if "t" in sides else 1, H if "b" in sides else H - 1)
    cols = slice(0, W) if "x" in periodic else slice(0 if "l" in sides else 1, W if "r" in sides else W - 1)
    return rows, cols


def dirichlet_mask(sides, periodic, H, W):
    """True on the Dirichlet lines"""
    m = np.ones((H, W), bool)
    m[unknowns(sides, periodic, H, W)] = False
    return m


def forward_differences(img, periodic=""):
    """(gx, gy) in img's dtype: gx[y][x] = img[y][x+1] - img[y][x]; the last column (row of gy) holds the difference from the last pixel to
    the first along a periodic axis, 0 otherwise (never read)"""
    img = np.asarray(img)
    gx, gy = np.zeros_like(img), np.zeros_like(img)
    gx[:, :-1] = img[:, 1:] - img[:, :-1]
    gy[:-1] = img[1:] - img[:-1]
    if "x" in periodic:
        gx[:, -1] = img[:, 0] - img[:, -1]
    if "y" in periodic:
        gy[-1] = img[0] - img[-1]
    return gx, gy


def divergence(gx, gy, periodic=""):
    """(a - b) + (c - d) in float32, in this order: a = gx(q), b = gx(q - x), c = gy(q), d = gy(q - y); along a periodic axis every
    element is read and the backward neighbour of column / row 0 is the last one; otherwise a term that would reach beyond the image is
    0.  At every unknown of every border combination the library's right-hand side (an unknown in an outermost column or row exists
    only where that side is free or the axis wraps); rhs() clears the Dirichlet lines."""
    gx, gy = np.asarray(gx, np.float32), np.asarray(gy, np.float32)
    a, c = gx.copy(), gy.copy()
    b, d = np.zeros_like(gx), np.zeros_like(gy)
    b[:, 1:] = gx[:, :-1]
    d[1:] = gy[:-1]
    if "x" in periodic:
        b[:, 0] = gx[:, -1]
    else:
        a[:, -1] = 0
    if "y" in periodic:
        d[0] = gy[-1]
    else:
        c[-1] = 0
    out = (a - b) + (c - d)
    assert out.dtype == np.float32
    return out


def rhs(sides, periodic, lam, data, lap):
    """lap - lam * d in float32 at the unknowns (one multiply, then one subtract; lam = 0: lap itself), 0 on the Dirichlet lines"""
    lap = _hwc(np.asarray(lap, np.float32))
    f = lap - np.float32(lam) * _hwc(np.asarray(data, np.float32)) if lam else lap
    assert f.dtype == np.float32
    out = np.zeros_like(f)
    blk = unknowns(sides, periodic, *f.shape[:2])
    out[blk] = f[blk]
    return out


def operator(sides, periodic, lam, u, by_differences=False):
    """(A - lam) u in float64 at the unknowns (the Dirichlet lines of u hold the known values), 0 on the Dirichlet lines.  The four
    neighbours are summed and 4 u taken off; by_differences: the four differences u(p) - u(q) are summed instead, the same number up
    to float64 rounding (the form the Neumann and screened constants of tests/direct_bounds.py were measured with)."""
    u = _hwc(np.asarray(u, np.float64))
    lam = float(np.float32(lam))
    P = np.pad(u, ((1, 1), (1, 1), (0, 0)), mode="edge")          # beyond a free side: the pixel's own value, the term vanishes
    if "x" in periodic:
        P[1:-1, 0], P[1:-1, -1] = u[:, -1], u[:, 0]
    if "y" in periodic:
        P[0, 1:-1], P[-1, 1:-1] = u[-1], u[0]
    left, right, up, down = P[1:-1, :-2], P[1:-1, 2:], P[:-2, 1:-1], P[2:, 1:-1]
    if by_differences:
        full = ((((right - u) + (left - u)) + (down - u)) + (up - u)) - lam * u
    else:
        full = (left + right + up + down - 4.0 * u) - lam * u
    r = np.zeros_like(u)
    blk = unknowns(sides, periodic, *u.shape[:2])
    r[blk] = full[blk]
    return r


def residual(sides, periodic, lam, u, data, lap):
    """operator(u) - rhs in float64 (0 on the Dirichlet lines); a singular system: the right-hand side is not centred here"""
    return operator(sides, periodic, lam, u) - rhs(sides, periodic, lam, data, lap).astype(np.float64)


def fold(sides, periodic, boundary):
    """the Dirichlet neighbours' values at each unknown, float64 [ny][nx][C] (what moves to the right-hand side); a Dirichlet line lies
    across a non-periodic axis only, so no wrapped neighbour is ever on one"""
    b = _hwc(np.asarray(boundary, np.float64))
    H, W = b.shape[:2]
    fr = np.where(dirichlet_mask(sides, periodic, H, W)[:, :, None], b, 0.0)
    P = np.pad(fr, ((1, 1), (1, 1), (0, 0)))
    s = P[1:-1, :-2] + P[1:-1, 2:] + P[:-2, 1:-1] + P[2:, 1:-1]
    return s[unknowns(sides, periodic, H, W)]


# ---- the transforms along one axis: float64, or f32: float32 in, pocketfft in complex64 (numpy >= 2 keeps single precision), float32 out
def _one(x, axis):
    z = list(x.shape)
    z[axis] = 1
    return z


def _along(n, ndim, axis):
    shape = [1] * ndim
    shape[axis] = n
    return shape


def dst1(x, axis, f32=False):
    """X_k = sum_{j=1..n} x_j sin(pi j k / (n + 1)) through the FFT of the odd extension (length 2n + 2); its own inverse up to 2 / (n + 1)"""
    n = x.shape[axis]
    zero = np.zeros(_one(x, axis), x.dtype)
    ext = np.concatenate([zero, x, zero, -np.flip(x, axis)], axis)
    F = np.take(np.fft.rfft(ext, axis=axis), np.arange(1, n + 1), axis)
    out = F.imag * (np.float32(-0.5) if f32 else -0.5)
    assert not f32 or (F.dtype == np.complex64 and out.dtype == np.float32)
    return out


def dct2(x, axis, f32=False):
    """X_k = sum_j x_j cos(pi (2j + 1) k / 2n) through the FFT of the even extension (length 2n)"""
    n = x.shape[axis]
    ext = np.concatenate([x, np.flip(x, axis)], axis)
    F = np.take(np.fft.rfft(ext, axis=axis), np.arange(n), axis)
    w = np.exp(-1j * np.pi * np.arange(n) / (2.0 * n)).reshape(_along(n, x.ndim, axis))
    out = (F * (w.astype(np.complex64) if f32 else w)).real * (np.float32(0.5) if f32 else 0.5)
    assert not f32 or (ext.dtype == np.float32 and F.dtype == np.complex64 and out.dtype == np.float32)
    return out


def idct2(X, axis, f32=False):
    """the inverse of dct2 (normalisation included)"""
    n = X.shape[axis]
    w = np.exp(1j * np.pi * np.arange(n) / (2.0 * n)).reshape(_along(n, X.ndim, axis))
    F = (X * (np.float32(2.0) if f32 else 2.0)) * (w.astype(np.complex64) if f32 else w)
    F = np.concatenate([F, np.zeros(_one(X, axis), F.dtype)], axis)          # the even extension's coefficient n is zero
    out = np.take(np.fft.irfft(F, 2 * n, axis=axis), np.arange(n), axis)
    assert not f32 or (F.dtype == np.complex64 and out.dtype == np.float32)
    return out


def sdn(x, axis, f32=False):
    """X_k = sum_j x_j sin(pi (2k+1) (j+1) / (2n+1)): the odd coefficients of the FFT of the length 4n + 2 extension that is odd about
    the Dirichlet line (position 0) and even about the free end (position n + 1/2)"""
    n = x.shape[axis]
    half = np.concatenate([np.zeros(_one(x, axis), x.dtype), x, np.flip(x, axis)], axis)      # positions 0 .. 2n
    ext = np.concatenate([half, -half], axis)                                     # y(t + N) = -y(t): 0 .. 4n + 1
    F = np.take(np.fft.rfft(ext, axis=axis), 2 * np.arange(n) + 1, axis)
    out = F.imag * (np.float32(-0.25) if f32 else -0.25)
    assert not f32 or (F.dtype == np.complex64 and out.dtype == np.float32)
    return out


def isdn(X, axis, f32=False):
    """the inverse of sdn, normalisation 4 / (2n + 1) included: the inverse FFT of the odd spectrum"""
    n = X.shape[axis]
    shape = list(X.shape)
    shape[axis] = 2 * n + 2                                                       # rfft layout of length 4n + 2
    F = np.zeros(shape, np.complex64 if f32 else complex)
    idx = [slice(None)] * X.ndim
    idx[axis] = slice(1, 2 * n, 2)
    F[tuple(idx)] = X * (np.complex64(-4j) if f32 else -4j)
    out = np.take(np.fft.irfft(F, 4 * n + 2, axis=axis), np.arange(1, n + 1), axis)
    assert not f32 or out.dtype == np.float32
    return out


def forward(kind, x, axis, f32=False):
    """the real transform of an axis of kind DD, NN, DN or ND (ND: DN's of the mirror image)"""
    if kind == DD:
        return dst1(x, axis, f32)
    if kind == NN:
        return dct2(x, axis, f32)
    return sdn(np.flip(x, axis) if kind == ND else x, axis, f32)


def inverse(kind, X, axis, f32=False):
    if kind == DD:
        s = 2.0 / (X.shape[axis] + 1.0)
        return dst1(X, axis, f32) * (np.float32(s) if f32 else s)
    if kind == NN:
        return idct2(X, axis, f32)
    x = isdn(X, axis, f32)
    return np.flip(x, axis) if kind == ND else x


def axis_eigenvalues(kind, n):
    """the 1-D operator's eigenvalues in float64, in the transform's order (a periodic axis: np.fft.fft's)"""
    k = np.arange(n)
    if kind == PP:
        return 2.0 * np.cos(2.0 * np.pi * k / n) - 2.0
    if kind == DD:
        return 2.0 * np.cos(np.pi * (k + 1) / (n + 1.0)) - 2.0
    if kind == NN:
        return 2.0 * np.cos(np.pi * k / n) - 2.0
    return 2.0 * np.cos(np.pi * (2 * k + 1) / (2.0 * n + 1.0)) - 2.0


def solve_rhs(sides, periodic, lam, f, boundary=None, f32=False, order=ROWS_FIRST):
    """the solve for a right-hand side given as an array (its values at the unknowns, taken in the working precision): what solve_exact
    and solve_f32 run on rhs(), and what a host test runs on a right-hand side formed in float64"""
    f = np.asarray(f)
    shape = f.shape
    f = _hwc(f)
    H, W, C = f.shape
    blk = unknowns(sides, periodic, H, W)
    kind = dict(zip((1, 0), axis_kinds(sides, periodic)))
    real, cplx = (np.float32, np.complex64) if f32 else (np.float64, np.complex128)
    g = f[blk].astype(real)
    if all(k in (NN, PP) for k in kind.values()):
        out = np.zeros((H, W, C), real)
    else:
        b = _hwc(np.asarray(boundary, real))
        out = b.copy()
        g = g - fold(sides, periodic, b).astype(real)
    ny, nx = g.shape[:2]
    den = (axis_eigenvalues(kind[1], nx)[None, :] + axis_eigenvalues(kind[0], ny)[:, None]) - float(np.float32(lam))
    sing = singular(sides, periodic, lam)
    if sing:
        den[0, 0] = 1.0
    den = den.astype(real)[:, :, None]
    there, back = ORDERS[order]
    X = g
    for axis in there:                                # the real transforms first: they take real input
        if kind[axis] != PP:
            X = forward(kind[axis], X, axis, f32)
    for axis in (1, 0):
        if kind[axis] == PP:
            X = np.fft.fft(X, axis=axis)
            assert X.dtype == cplx
    X = X / den
    if sing:
        X[0, 0] = 0.0
    for axis in (1, 0):
        if kind[axis] == PP:
            X = np.fft.ifft(X, axis=axis)
            assert X.dtype == cplx
    u = X.real if np.iscomplexobj(X) else X           # (real up to rounding: the data were real and den is symmetric in k and n - k)
    for axis in back:
        if kind[axis] != PP:
            u = inverse(kind[axis], u, axis, f32)
    assert u.dtype == real
    out[blk] = u
    return out.reshape(shape)


def solve_exact(sides, periodic, lam, data, lap, boundary=None, order=ROWS_FIRST):
    """float64 solution of (A - lam) u = rhs(sides, periodic, lam, data, lap): boundary's values on the Dirichlet lines (boundary's other
    elements are not used), the solution at the unknowns.  lam = 0: data unused (None).  Singular (no Dirichlet line, lam = 0): the
    mean-zero solution of the right-hand side less its mean; boundary unused."""
    return solve_rhs(sides, periodic, lam, rhs(sides, periodic, lam, data, lap), boundary, False, order).reshape(np.shape(lap))


def solve_f32(sides, periodic, lam, data, lap, boundary=None, order=ROWS_FIRST):
    """solve_exact restated in float32: pocketfft in complex64, float32 denominators (rounded from double), a float32 result: what a
    plain float32 solve of another algorithm than the library's chirp convolution loses on the same input.  On rough inputs the order
    changes nothing beyond the scatter from image to image; on a smooth input with a rough short side it decides whether the long
    transform's rounding (relative to the largest coefficient of its row) reaches the lowest modes along the long side."""
    return solve_rhs(sides, periodic, lam, rhs(sides, periodic, lam, data, lap), boundary, True, order).reshape(np.shape(lap))


def mean_of(boundary):
    """per channel mean over the H x W elements, in float64"""
    return np.asarray(boundary, np.float64).mean(axis=(0, 1))


def solve_free(lap, boundary=None):
    """the library's Neumann problem for a float32 right-hand side: the float64 solve of ("lrtb", ""), mean(u) = mean(boundary) (None: 0)"""
    u = solve_exact("lrtb", "", 0.0, None, lap)
    return u if boundary is None else u + mean_of(boundary)


def smooth_image(H, W, C, seed):
    """A sum of six cosine modes cos(pi (2x+1) k / 2W) cos(pi (2y+1) l / 2H), k <= min(4, W // 256), l <= min(4, H // 256), (k, l) !=
    (0, 0), amplitudes uniform in [-40, 40], around a level of 125: computed in float64, returned as float32.  A side shorter than
    256 pixels carries no mode: four half-waves across 9 or 64 pixels are not smooth, their eigenvalue (pi l / H)^2 makes the
    right-hand side as large as a rough image's, and whichever solver transforms the long side first then loses the long side's
    lowest modes to that transform's rounding -- the amplified loss the rough inputs measure, not a low coefficient's value."""
    rng = np.random.default_rng(seed)
    x = (2.0 * np.arange(W) + 1.0) / (2.0 * W)
    y = (2.0 * np.arange(H) + 1.0) / (2.0 * H)
    img = np.full((H, W, C), 125.0)
    for c in range(C):
        for _ in range(6):
            k, l = int(rng.integers(0, min(4, W // 256) + 1)), int(rng.integers(0, min(4, H // 256) + 1))
            if k == l == 0:
                k, l = (1, 0) if W >= H else (0, 1)
            img[:, :, c] += rng.uniform(-40, 40) * np.cos(np.pi * l * y)[:, None] * np.cos(np.pi * k * x)[None, :]
    return img.astype(np.float32)
