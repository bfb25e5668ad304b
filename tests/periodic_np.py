"""The test side's restatement of the Poisson and screened solves with periodic axes (SC_POISSON_PERIODIC_X / _Y), numpy only.

A problem's borders are (sides, periodic): `periodic` is "", "x", "y" or "xy", the axes that wrap; `sides` a string over "lrtb", the
sides WITHOUT a Dirichlet line, as in mixed_np, and names no side of a periodic axis.  A periodic axis has no Dirichlet line: all its
pixels are unknowns and the stencil's neighbour beyond either end is the pixel at the other end (at length 2 the same pixel twice).
Per channel the library solves
    (A - lam) u = lap - lam d        at the unknowns (lam = 0: the unscreened system, no data term),
lap given or the float32 divergence of a guidance field (divergence(): (a - b) + (c - d); along a periodic axis the last column of gx /
row of gy holds the difference from the last pixel to the first, and column / row 0 takes it as its backward difference).

operator() applies the stencil directly, with wrap (what tests/test_periodic_host.py checks the solve against, next to a dense
assembly).  solve_exact() solves in float64: a periodic axis under a plain complex FFT (np.fft.fft), any other axis under mixed_np's
extension transforms -- the real transform first, the FFT second, the way back in the opposite order.  No code is shared with the
library, which runs a real Hartley transform as a chirp convolution.  solve_f32() is the same in single precision (complex64 FFTs,
float32 denominators), the yardstick of the GPU tests' float32 bounds (tests/periodic_bounds.py).  Without a Dirichlet line on either
axis the unscreened system is singular: both return the mean-zero solution of the right-hand side less its mean.
With periodic == "" everything here is mixed_np's problem.  Arrays are H x W x C (H x W accepted)."""
from __future__ import annotations

import numpy as np

import mixed_np

DD, NN, DN, ND = mixed_np.DD, mixed_np.NN, mixed_np.DN, mixed_np.ND
PP = 4                                              # a periodic axis
PERIODIC = ["x", "y", "xy"]
# the nine combinations with a periodic axis: (sides, periodic), the other axis under D-D, free-D, D-free, free-free, or periodic too
COMBOS = [(s, "x") for s in ("", "t", "b", "tb")] + [(s, "y") for s in ("", "l", "r", "lr")] + [("", "xy")]


def _hwc(a):
    return a[:, :, None] if a.ndim == 2 else a


def check_borders(sides, periodic):
    mixed_np.check_sides(sides)
    if not isinstance(periodic, str) or any(ch not in "xy" for ch in periodic):
        raise ValueError(f"periodic {periodic!r}: a string over 'xy'")
    if ("x" in periodic and ("l" in sides or "r" in sides)) or ("y" in periodic and ("t" in sides or "b" in sides)):
        raise ValueError(f"sides {sides!r} name a side of a periodic axis ({periodic!r})")
    return sides, periodic


def axis_kinds(sides, periodic):
    """(x axis, y axis) of DD, NN, DN, ND, PP"""
    check_borders(sides, periodic)
    ax, ay = mixed_np.axis_kinds(sides)
    return (PP if "x" in periodic else ax), (PP if "y" in periodic else ay)


def singular(sides, periodic, lam=0.0):
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
    the first along a periodic axis, 0 otherwise"""
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
    """(a - b) + (c - d) in float32: a = gx(q), b = gx(q - x), c = gy(q), d = gy(q - y); along a periodic axis every element is read and
    the backward neighbour of column / row 0 is the last one; otherwise a term that would reach beyond the image is 0"""
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


def operator(sides, periodic, lam, u):
    """(A - lam) u in float64 at the unknowns (the Dirichlet lines of u hold the known values), 0 on the Dirichlet lines"""
    u = _hwc(np.asarray(u, np.float64))
    lam = float(np.float32(lam))
    P = np.pad(u, ((1, 1), (1, 1), (0, 0)), mode="edge")          # beyond a free side: the pixel's own value, the term vanishes
    if "x" in periodic:
        P[1:-1, 0], P[1:-1, -1] = u[:, -1], u[:, 0]
    if "y" in periodic:
        P[0, 1:-1], P[-1, 1:-1] = u[-1], u[0]
    full = (P[1:-1, :-2] + P[1:-1, 2:] + P[:-2, 1:-1] + P[2:, 1:-1] - 4.0 * u) - lam * u
    r = np.zeros_like(u)
    blk = unknowns(sides, periodic, *u.shape[:2])
    r[blk] = full[blk]
    return r


def residual(sides, periodic, lam, u, data, lap):
    """operator(u) - rhs in float64 (0 on the Dirichlet lines)"""
    return operator(sides, periodic, lam, u) - rhs(sides, periodic, lam, data, lap).astype(np.float64)


def _fold(sides, periodic, boundary):
    """the Dirichlet neighbours' values at each unknown, float64 [ny][nx][C] (what moves to the right-hand side); a Dirichlet line lies
    across a non-periodic axis only, so no wrapped neighbour is ever on one"""
    b = _hwc(np.asarray(boundary, np.float64))
    H, W = b.shape[:2]
    fr = np.where(dirichlet_mask(sides, periodic, H, W)[:, :, None], b, 0.0)
    P = np.pad(fr, ((1, 1), (1, 1), (0, 0)))
    s = P[1:-1, :-2] + P[1:-1, 2:] + P[:-2, 1:-1] + P[2:, 1:-1]
    return s[unknowns(sides, periodic, H, W)]


def axis_eigenvalues(kind, n):
    """the 1-D operator's eigenvalues in float64, in the transform's order (a periodic axis: np.fft.fft's)"""
    if kind == PP:
        return 2.0 * np.cos(2.0 * np.pi * np.arange(n) / n) - 2.0
    return mixed_np.axis_eigenvalues(kind, n)


def _solve(sides, periodic, lam, data, lap, boundary, f32):
    shape = np.asarray(lap).shape
    f = rhs(sides, periodic, lam, data, lap)
    H, W, C = f.shape
    blk = unknowns(sides, periodic, H, W)
    ax, ay = axis_kinds(sides, periodic)
    real, cplx = (np.float32, np.complex64) if f32 else (np.float64, np.complex128)
    g = f[blk].astype(real)
    if ax in (NN, PP) and ay in (NN, PP):
        out = np.zeros((H, W, C), real)
    else:
        b = _hwc(np.asarray(boundary, real))
        out = b.copy()
        g = g - _fold(sides, periodic, b).astype(real)
    ny, nx = g.shape[:2]
    den = (axis_eigenvalues(ax, nx)[None, :] + axis_eigenvalues(ay, ny)[:, None]) - float(np.float32(lam))
    sing = singular(sides, periodic, lam)
    if sing:
        den[0, 0] = 1.0
    den = den.astype(real)[:, :, None]
    kinds = ((ax, 1), (ay, 0))
    X = g
    for kind, axis in kinds:                          # the real transforms first: they take real input
        if kind != PP:
            X = mixed_np._forward(kind, X, axis, f32)
    for kind, axis in kinds:
        if kind == PP:
            X = np.fft.fft(X, axis=axis)
            assert X.dtype == cplx
    X = X / den
    if sing:
        X[0, 0] = 0.0
    for kind, axis in kinds:
        if kind == PP:
            X = np.fft.ifft(X, axis=axis)
            assert X.dtype == cplx
    u = X.real if np.iscomplexobj(X) else X           # (real up to rounding: the data were real and den is symmetric in k and n - k)
    for kind, axis in kinds:
        if kind != PP:
            u = mixed_np._inverse(kind, u, axis, f32)
    assert u.dtype == real
    out[blk] = u
    return out.reshape(shape)


def solve_exact(sides, periodic, lam, data, lap, boundary=None):
    """float64 solution of (A - lam) u = rhs(sides, periodic, lam, data, lap): boundary's values on the Dirichlet lines (boundary's other
    elements are not used), the solution at the unknowns.  lam = 0: data unused (None).  Singular (no Dirichlet line, lam = 0): the
    mean-zero solution of the right-hand side less its mean; boundary unused."""
    return _solve(sides, periodic, lam, data, lap, boundary, False)


def solve_f32(sides, periodic, lam, data, lap, boundary=None):
    """solve_exact restated in float32: pocketfft in complex64, float32 denominators (rounded from double), a float32 result: what a
    plain float32 solve of another algorithm than the library's chirp convolution loses on the same input."""
    return _solve(sides, periodic, lam, data, lap, boundary, True)


def smooth_image(H, W, C, seed):
    """the low-mode input of the long sides' error figures (mixed_np.smooth_image: a side shorter than 256 pixels carries no mode)"""
    return mixed_np.smooth_image(H, W, C, seed)
