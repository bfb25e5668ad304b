"""The test side's restatement of the Neumann problem of sc_hip_poisson (SC_POISSON_NEUMANN), numpy only.

All H x W pixels of every channel are unknowns; the 5-point stencil reflects at the border:
    sum over the 2, 3 or 4 neighbours p of q inside the image of (u(p) - u(q)) = lap(q).
divergence() is the library's float32 right-hand side of a guidance field, to the letter; solve_exact() solves the system in float64
by DCT-II transforms computed as FFTs of the even extension (no code shared with the library: numpy's pocketfft on 2n points, where
the library runs a chirp convolution), fixes the free constant by the mean asked for, and ignores the right-hand side's mean (the
system is solvable only for a right-hand side of sum zero).  operator() applies the reflecting stencil directly: what
tests/test_neumann_host.py checks the solve against.  solve_f32() is solve_exact() in single precision, the yardstick of the GPU
tests' float32 bounds (tests/neumann_bounds.py); residual() what a solution leaves of the system; smooth_image() the low-mode input.
Arrays are H x W x C."""
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


def _dct2_f32(x, axis):
    """_dct2 in single precision: float32 in, pocketfft in complex64, float32 out"""
    n = x.shape[axis]
    ext = np.concatenate([x, np.flip(x, axis)], axis)
    F = np.take(np.fft.rfft(ext, axis=axis), np.arange(n), axis)
    shape = [1] * x.ndim
    shape[axis] = n
    w = np.exp(-1j * np.pi * np.arange(n) / (2.0 * n)).astype(np.complex64).reshape(shape)
    out = (F * w).real * np.float32(0.5)
    assert ext.dtype == np.float32 and F.dtype == np.complex64 and out.dtype == np.float32
    return out


def _idct2_f32(X, axis):
    """_idct2 in single precision"""
    n = X.shape[axis]
    shape = [1] * X.ndim
    shape[axis] = n
    w = np.exp(1j * np.pi * np.arange(n) / (2.0 * n)).astype(np.complex64).reshape(shape)
    F = (X * np.float32(2.0)) * w
    pad = list(X.shape)
    pad[axis] = 1
    F = np.concatenate([F, np.zeros(pad, np.complex64)], axis)
    out = np.take(np.fft.irfft(F, 2 * n, axis=axis), np.arange(n), axis)
    assert F.dtype == np.complex64 and out.dtype == np.float32
    return out


def solve_f32(lap, mean=None, x_first=True):
    """solve_exact restated in float32: the same even-extension FFTs run by pocketfft in complex64 (numpy >= 2 keeps single
    precision), float32 denominators (rounded from double), a float32 result.  What a plain float32 solve of another algorithm
    than the library's chirp convolution loses on the same input: the yardstick of the GPU tests' float32 bounds.  x_first: the
    order of the axes, rows first as the library documents -- on rough inputs the order changes nothing
    beyond the scatter from image to image, on a smooth input with a rough short side it decides whether the long transform's
    rounding (relative to the largest coefficient of its row) reaches the lowest modes along the long side."""
    lap = np.asarray(lap, np.float32)
    H, W, C = lap.shape
    out = np.empty((H, W, C), np.float32)
    den = ((2.0 * np.cos(np.pi * np.arange(W) / W) - 2.0)[None, :] + (2.0 * np.cos(np.pi * np.arange(H) / H) - 2.0)[:, None])
    den[0, 0] = 1.0
    den = den.astype(np.float32)
    for c in range(C):
        a, b = (1, 0) if x_first else (0, 1)
        X = _dct2_f32(_dct2_f32(lap[:, :, c], a), b)
        X = X / den
        X[0, 0] = 0.0
        assert X.dtype == np.float32
        out[:, :, c] = _idct2_f32(_idct2_f32(X, b), a)
    if mean is not None:
        out += np.asarray(mean, np.float32).reshape(1, 1, C)
    return out


def residual(u, lap):
    """operator(u) - (lap - mean(lap)) in float64, per channel: what is left of the reflecting system (not amplified by 1 / lambda)"""
    lap = np.asarray(lap, np.float64)
    return operator(u) - (lap - lap.mean(axis=(0, 1), keepdims=True))


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


def mean_of(boundary):
    """per channel mean over the H x W elements, in float64 (None: zeros are the caller's business)"""
    return np.asarray(boundary, np.float64).mean(axis=(0, 1))


def solve_guidance(gx, gy, boundary=None):
    """the library's problem for a float32 guidance field: float32 divergence, float64 solve, mean(u) = mean(boundary)"""
    return solve_exact(divergence(gx, gy), None if boundary is None else mean_of(boundary))


def solve_laplacian(lap, boundary=None):
    return solve_exact(np.asarray(lap, np.float32), None if boundary is None else mean_of(boundary))
