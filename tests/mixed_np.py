"""The test side's restatement of the Poisson and screened solves with per-side free borders (SC_POISSON_FREE_*), numpy only.

`sides` is a string over "lrtb": the sides WITHOUT a Dirichlet line.  A side that is not named keeps known values on its outermost row
or column (corners included); a named side's outermost pixels are unknowns and the stencil lacks the neighbour beyond them.  Per
channel the library solves
    (A - lam) u = lap - lam d        at the unknowns (lam = 0: the unscreened system, no data term),
lap given or the float32 divergence of a guidance field (divergence(): (a - b) + (c - d), a term 0 where its neighbour lies beyond a
free side -- at the unknowns this is the Neumann formula, whatever the sides).

operator() applies the stencil directly (what tests/test_mixed_host.py checks the solve against, next to a dense assembly).
solve_exact() solves in float64 by explicit transforms, each axis under the transform of its two ends, every one computed as a
periodic FFT of the axis's odd / even extension: DST-I (length 2n + 2) between two Dirichlet lines, DCT-II (length 2n) between two
free ends, and between a Dirichlet line and a free end the sine transform of odd half-frequencies, X_k = sum_j x_j
sin(pi (2k+1) (j+1) / (2n+1)), as the odd coefficients of the length 4n + 2 extension that is odd about the line and even about the
free end.  No code is shared with the library, which runs chirp convolutions of length >= 2n - 1.  solve_f32() is solve_exact() in
single precision (complex64 FFTs, float32 denominators), the yardstick of the GPU tests' float32 bounds (tests/mixed_bounds.py).
Arrays are H x W x C (H x W accepted)."""
from __future__ import annotations

import numpy as np

import neumann_np
import screened_np

ALL_SIDES = ["".join(s for s, on in zip("lrtb", (m & 1, m & 2, m & 4, m & 8)) if on) for m in range(16)]
MIXED_SIDES = ALL_SIDES[1:15]                      # the 14 combinations between the Dirichlet frame and the Neumann problem
DD, NN, DN, ND = 0, 1, 2, 3                        # an axis's ends (low, high): D a Dirichlet line, N free


def _hwc(a):
    return a[:, :, None] if a.ndim == 2 else a


def check_sides(sides):
    if not isinstance(sides, str) or any(ch not in "lrtb" for ch in sides):
        raise ValueError(f"sides {sides!r}: a string over 'lrtb'")
    return sides


def axis_kinds(sides):
    """(x axis, y axis) of DD, NN, DN, ND"""
    kind = lambda lo, hi: (NN if hi else ND) if lo else (DN if hi else DD)
    check_sides(sides)
    return kind("l" in sides, "r" in sides), kind("t" in sides, "b" in sides)


def unknowns(sides, H, W):
    """(rows, columns) of the unknown block as slices"""
    check_sides(sides)
    return (slice(0 if "t" in sides else 1, H if "b" in sides else H - 1), slice(0 if "l" in sides else 1, W if "r" in sides else W - 1))


def dirichlet_mask(sides, H, W):
    """True on the Dirichlet lines"""
    m = np.ones((H, W), bool)
    m[unknowns(sides, H, W)] = False
    return m


def forward_differences(img):
    return neumann_np.forward_differences(img)


def divergence(gx, gy):
    """(a - b) + (c - d) in float32, a term 0 where it would reach beyond the image: at every unknown of every side combination the
    library's right-hand side (an unknown in an outermost column or row exists only where that side is free)."""
    return neumann_np.divergence(gx, gy)


def rhs(sides, lam, data, lap):
    """lap - lam * d in float32 at the unknowns (one multiply, then one subtract; lam = 0: lap itself), 0 on the Dirichlet lines"""
    lap = _hwc(np.asarray(lap, np.float32))
    f = lap - np.float32(lam) * _hwc(np.asarray(data, np.float32)) if lam else lap
    assert f.dtype == np.float32
    out = np.zeros_like(f)
    blk = unknowns(sides, *f.shape[:2])
    out[blk] = f[blk]
    return out


def operator(sides, lam, u):
    """(A - lam) u in float64 at the unknowns (the Dirichlet lines of u hold the known values), 0 on the Dirichlet lines"""
    u = _hwc(np.asarray(u, np.float64))
    lam = float(np.float32(lam))
    P = np.pad(u, ((1, 1), (1, 1), (0, 0)), mode="edge")          # beyond a free side: the pixel's own value, the term vanishes
    full = (P[1:-1, :-2] + P[1:-1, 2:] + P[:-2, 1:-1] + P[2:, 1:-1] - 4.0 * u) - lam * u
    r = np.zeros_like(u)
    blk = unknowns(sides, *u.shape[:2])
    r[blk] = full[blk]
    return r


def residual(sides, lam, u, data, lap):
    """operator(u) - rhs in float64 (0 on the Dirichlet lines)"""
    return operator(sides, lam, u) - rhs(sides, lam, data, lap).astype(np.float64)


def _fold(sides, boundary):
    """the Dirichlet neighbours' values at each unknown, float64 [ny][nx][C] (what moves to the right-hand side)"""
    b = _hwc(np.asarray(boundary, np.float64))
    H, W = b.shape[:2]
    fr = np.where(dirichlet_mask(sides, H, W)[:, :, None], b, 0.0)
    P = np.pad(fr, ((1, 1), (1, 1), (0, 0)))
    s = P[1:-1, :-2] + P[1:-1, 2:] + P[:-2, 1:-1] + P[2:, 1:-1]
    return s[unknowns(sides, H, W)]


def _sdn(x, axis, f32):
    """X_k = sum_j x_j sin(pi (2k+1) (j+1) / (2n+1)) along `axis`: the odd coefficients of the FFT of the length 4n + 2 extension that
    is odd about the Dirichlet line (position 0) and even about the free end (position n + 1/2)"""
    n = x.shape[axis]
    z = list(x.shape)
    z[axis] = 1
    zero = np.zeros(z, x.dtype)
    half = np.concatenate([zero, x, np.flip(x, axis)], axis)                      # positions 0 .. 2n
    ext = np.concatenate([half, -half], axis)                                     # y(t + N) = -y(t): 0 .. 4n + 1
    F = np.take(np.fft.rfft(ext, axis=axis), 2 * np.arange(n) + 1, axis)
    out = F.imag * (np.float32(-0.25) if f32 else -0.25)
    assert not f32 or (F.dtype == np.complex64 and out.dtype == np.float32)
    return out


def _isdn(X, axis, f32):
    """the inverse of _sdn, normalisation 4 / (2n + 1) included: the inverse FFT of the odd spectrum"""
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


def _forward(kind, x, axis, f32=False):
    if kind == DD:
        return screened_np._dst1(x, axis, f32)
    if kind == NN:
        return neumann_np._dct2_f32(x, axis) if f32 else neumann_np._dct2(x, axis)
    return _sdn(np.flip(x, axis) if kind == ND else x, axis, f32)


def _inverse(kind, X, axis, f32=False):
    n = X.shape[axis]
    if kind == DD:
        s = 2.0 / (n + 1.0)
        return screened_np._dst1(X, axis, f32) * (np.float32(s) if f32 else s)
    if kind == NN:
        return neumann_np._idct2_f32(X, axis) if f32 else neumann_np._idct2(X, axis)
    x = _isdn(X, axis, f32)
    return np.flip(x, axis) if kind == ND else x


def axis_eigenvalues(kind, n):
    """the 1-D operator's eigenvalues in float64, in the transform's order"""
    k = np.arange(n)
    if kind == DD:
        return 2.0 * np.cos(np.pi * (k + 1) / (n + 1.0)) - 2.0
    if kind == NN:
        return 2.0 * np.cos(np.pi * k / n) - 2.0
    return 2.0 * np.cos(np.pi * (2 * k + 1) / (2.0 * n + 1.0)) - 2.0


def _solve(sides, lam, data, lap, boundary, f32):
    shape = np.asarray(lap).shape
    f = rhs(sides, lam, data, lap)
    H, W, C = f.shape
    blk = unknowns(sides, H, W)
    ax, ay = axis_kinds(sides)
    real = np.float32 if f32 else np.float64
    g = f[blk].astype(real)
    if len(sides) < 4:
        b = _hwc(np.asarray(boundary, real))
        out = b.copy()
        g = g - _fold(sides, b).astype(real)
    else:
        out = np.zeros((H, W, C), real)
    ny, nx = g.shape[:2]
    den = (axis_eigenvalues(ax, nx)[None, :] + axis_eigenvalues(ay, ny)[:, None]) - float(np.float32(lam))
    singular = len(sides) == 4 and not lam                # the Neumann problem: the mean-zero solution of the right-hand side less its mean
    if singular:
        den[0, 0] = 1.0
    den = den.astype(real)[:, :, None]
    X = _forward(ay, _forward(ax, g, 1, f32), 0, f32) / den        # rows first, as the library
    if singular:
        X[0, 0] = 0.0
    u = _inverse(ax, _inverse(ay, X, 0, f32), 1, f32)
    assert u.dtype == real
    out[blk] = u
    return out.reshape(shape)


def solve_exact(sides, lam, data, lap, boundary=None):
    """float64 solution of (A - lam) u = rhs(sides, lam, data, lap): boundary's values on the Dirichlet lines (boundary's other elements
    are not used), the solution at the unknowns.  lam = 0: data unused (None).  All four sides free and lam = 0: the singular Neumann
    system's mean-zero solution."""
    return _solve(sides, lam, data, lap, boundary, False)


def solve_f32(sides, lam, data, lap, boundary=None):
    """solve_exact restated in float32: the same extension FFTs run by pocketfft in complex64, rows first, float32 denominators
    (rounded from double), a float32 result: what a plain float32 solve of another algorithm than the library's chirp convolution
    loses on the same input."""
    return _solve(sides, lam, data, lap, boundary, True)


def smooth_image(H, W, C, seed):
    """the low-mode input of the long sides' error figures (neumann_np.smooth_image: a side shorter than 256 pixels carries no mode)"""
    return neumann_np.smooth_image(H, W, C, seed)
