"""The test side's restatement of the Neumann problem of sc_hip_poisson (SC_POISSON_NEUMANN), numpy only.

All H x W pixels of every channel are unknowns; the 5-point stencil reflects at the border:
    sum over the 2, 3 or 4 neighbours p of q inside the image of (u(p) - u(q)) = lap(q).
divergence() is the library's float32 right-hand side of a guidance field, to the letter; solve_exact() solves the system in float64
by DCT-II transforms computed as FFTs of the even extension (no code shared with the library: numpy's pocketfft on 2n points, where
the library runs a chirp convolution), fixes the free constant by the mean asked for, and ignores the right-hand side's mean (the
system is solvable only for a right-hand side of sum zero).  operator() applies the reflecting stencil directly: what
tests/test_neumann_host.py checks the solve against.  Arrays are H x W x C."""
from __future__ import annotations

import numpy as np


def forward_differences(img):
    """gx(x, y) = I(x+1, y) - I(x, y), gy(x, y) = I(x, y+1) - I(x, y) in the image's dtype; 0 in the last column / row (never read)."""
    gx = np.zeros_like(img)
    gy = np.zeros_like(img)
    gx[:, :-1] = img[:, 1:] - img[:, :-1]
    gy[:-1] = img[1:] - img[:-1]
    return gx, gy


def divergence(gx, gy):
    """lap(q) = (a - b) + (c - d) in float32, in this order: a = gx(q) (0 in the last column), b = gx(q - x) (0 in column 0),
    c = gy(q) (0 in the last row), d = gy(q - y) (0 in row 0)."""
    gx = np.asarray(gx, np.float32)
    gy = np.asarray(gy, np.float32)
    a = gx.copy(); a[:, -1] = 0
    b = np.zeros_like(gx); b[:, 1:] = gx[:, :-1]
    c = gy.copy(); c[-1] = 0
    d = np.zeros_like(gy); d[1:] = gy[:-1]
    return ((a - b) + (c - d)).astype(np.float32)


def operator(u):
    """The reflecting 5-point operator in float64: sum over the neighbours inside the image of (u(p) - u(q))."""
    u = np.asarray(u, np.float64)
    r = np.zeros_like(u)
    r[:, :-1] += u[:, 1:] - u[:, :-1]
    r[:, 1:] += u[:, :-1] - u[:, 1:]
    r[:-1] += u[1:] - u[:-1]
    r[1:] += u[:-1] - u[1:]
    return r


def _dct2(x, axis):
    """X_k = sum_j x_j cos(pi (2j + 1) k / 2n) along `axis`, through the FFT of the even extension (length 2n)."""
    n = x.shape[axis]
    ext = np.concatenate([x, np.flip(x, axis)], axis)
    F = np.take(np.fft.rfft(ext, axis=axis), np.arange(n), axis)
    shape = [1] * x.ndim
    shape[axis] = n
    w = np.exp(-1j * np.pi * np.arange(n) / (2.0 * n)).reshape(shape)
    return (F * w).real / 2.0


def _idct2(X, axis):
    """the inverse of _dct2 (normalisation included)"""
    n = X.shape[axis]
    shape = [1] * X.ndim
    shape[axis] = n
    w = np.exp(1j * np.pi * np.arange(n) / (2.0 * n)).reshape(shape)
    F = 2.0 * X * w
    pad = list(X.shape)
    pad[axis] = 1
    F = np.concatenate([F, np.zeros(pad, complex)], axis)          # the even extension's coefficient n is zero
    return np.take(np.fft.irfft(F, 2 * n, axis=axis), np.arange(n), axis)


def solve_exact(lap, mean=None):
    """float64 solution u (H x W x C) of the reflecting system for lap - mean(lap), with mean(u) = mean per channel (None: 0)."""
    lap = np.asarray(lap, np.float64)
    H, W, C = lap.shape
    out = np.empty_like(lap)
    den = (2.0 * np.cos(np.pi * np.arange(W) / W) - 2.0)[None, :] + (2.0 * np.cos(np.pi * np.arange(H) / H) - 2.0)[:, None]
    den[0, 0] = 1.0
    for c in range(C):                         # per channel: the even extensions of a large image are big
        X = _dct2(_dct2(lap[:, :, c], 0), 1)
        X /= den
        X[0, 0] = 0.0
        out[:, :, c] = _idct2(_idct2(X, 1), 0)
    if mean is not None:
        out += np.asarray(mean, np.float64).reshape(1, 1, C)
    return out


def mean_of(boundary):
    """per channel mean over the H x W elements, in float64 (None: zeros are the caller's business)"""
    return np.asarray(boundary, np.float64).mean(axis=(0, 1))


def solve_guidance(gx, gy, boundary=None):
    """the library's problem for a float32 guidance field: float32 divergence, float64 solve, mean(u) = mean(boundary)"""
    return solve_exact(divergence(gx, gy), None if boundary is None else mean_of(boundary))


def solve_laplacian(lap, boundary=None):
    return solve_exact(np.asarray(lap, np.float32), None if boundary is None else mean_of(boundary))
