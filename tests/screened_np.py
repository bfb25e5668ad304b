"""The test side's restatement of the screened Poisson solve (sc_hip_screened*), numpy only.

Per channel the library solves
    (A - lam) u = lap - lam d,         lam > 0,
A the 5-point operator with a Dirichlet frame (the unknowns are the interior, u = boundary on the frame) or reflecting at the border
(every pixel an unknown).  lap is given (SC_POISSON_LAPLACIAN) or the float32 divergence of a guidance field by the documented formula
of the boundary kind (divergence()).  rhs() is the library's float32 right-hand side to the letter: the product lam * d rounded to
float32, then subtracted from lap -- numpy's float32 arithmetic does exactly that, one rounding per operation.

solve_exact() solves the system in float64 by explicit transforms -- DST-I as the FFT of the odd extension, DCT-II as the FFT of the
even extension (no code shared with the library, which runs chirp convolutions) -- and divides by eigenvalue - lam.  operator() and
residual() apply the stencil directly: what tests/test_screened_host.py checks the solve against.  solve_f32() is solve_exact() in
single precision, the yardstick of the GPU tests' float32 bounds (tests/screened_bounds.py).  Arrays are H x W x C (H x W accepted)."""
from __future__ import annotations

import numpy as np

import neumann_np
import poisson_np

DIRICHLET, NEUMANN = "dirichlet", "neumann"


def _hwc(a):
    return a[:, :, None] if a.ndim == 2 else a


def forward_differences(img):
    """gx(x, y) = I(x+1, y) - I(x, y), gy(x, y) = I(x, y+1) - I(x, y) in the image's dtype; 0 in the last column / row"""
    return neumann_np.forward_differences(img)


def divergence(kind, gx, gy):
    """the library's float32 right-hand side of a guidance field under this boundary kind (Dirichlet: 0 on the frame)"""
    gx, gy = np.asarray(gx, np.float32), np.asarray(gy, np.float32)
    return neumann_np.divergence(gx, gy) if kind == NEUMANN else poisson_np.divergence(gx, gy)


def rhs(kind, lam, data, lap):
    """lap - lam * d in float32: one multiply, then one subtract.  Dirichlet: on the interior, 0 on the frame (never read)."""
    lap, d = np.asarray(lap, np.float32), np.asarray(data, np.float32)
    f = lap - np.float32(lam) * d
    assert f.dtype == np.float32
    if kind == DIRICHLET:
        g = np.zeros_like(f)
        g[1:-1, 1:-1] = f[1:-1, 1:-1]
        f = g
    return f


def _frame_fold(boundary):
    """the frame neighbours' values at each interior pixel, float64 (what moves to the right-hand side of the interior system)"""
    b = np.asarray(boundary, np.float64)
    fr = np.zeros_like(b)
    fr[0], fr[-1], fr[:, 0], fr[:, -1] = b[0], b[-1], b[:, 0], b[:, -1]
    return fr[1:-1, :-2] + fr[1:-1, 2:] + fr[:-2, 1:-1] + fr[2:, 1:-1]


def _dst1(x, axis, f32=False):
    """X_k = sum_{j=1..n} x_j sin(pi j k / (n + 1)) along `axis`, through the FFT of the odd extension (length 2n + 2)"""
    n = x.shape[axis]
    z = list(x.shape)
    z[axis] = 1
    zero = np.zeros(z, x.dtype)
    ext = np.concatenate([zero, x, zero, -np.flip(x, axis)], axis)
    F = np.take(np.fft.rfft(ext, axis=axis), np.arange(1, n + 1), axis)
    out = F.imag * (np.float32(-0.5) if f32 else -0.5)
    assert not f32 or (F.dtype == np.complex64 and out.dtype == np.float32)
    return out


def _eig(kind, H, W):
    """the operator's eigenvalues [H][W] in float64 (Dirichlet: of the (H - 2) x (W - 2) interior system)"""
    if kind == NEUMANN:
        return (2.0 * np.cos(np.pi * np.arange(W) / W) - 2.0)[None, :] + (2.0 * np.cos(np.pi * np.arange(H) / H) - 2.0)[:, None]
    w, h = W - 2, H - 2
    return ((2.0 * np.cos(np.pi * np.arange(1, w + 1) / (w + 1.0)))[None, :] + (2.0 * np.cos(np.pi * np.arange(1, h + 1) / (h + 1.0)))[:, None]) - 4.0


def solve_exact(kind, lam, data, lap, boundary=None):
    """float64 solution of (A - lam) u = rhs(kind, lam, data, lap); Dirichlet: the frame is boundary's.  The shape of data."""
    shape = np.asarray(data).shape
    f = _hwc(rhs(kind, lam, data, lap)).astype(np.float64)
    H, W, C = f.shape
    den = _eig(kind, H, W) - float(np.float32(lam))
    if kind == NEUMANN:
        out = np.empty_like(f)
        for c in range(C):
            X = neumann_np._dct2(neumann_np._dct2(f[:, :, c], 0), 1) / den
            out[:, :, c] = neumann_np._idct2(neumann_np._idct2(X, 1), 0)
        return out.reshape(shape)
    b = _hwc(np.asarray(boundary))
    out = b.astype(np.float64).copy()
    g = f[1:-1, 1:-1] - _frame_fold(b)
    X = _dst1(_dst1(g, 0), 1) / den[:, :, None]
    out[1:-1, 1:-1] = _dst1(_dst1(X, 1), 0) * (4.0 / ((W - 1.0) * (H - 1.0)))
    return out.reshape(shape)


def solve_f32(kind, lam, data, lap, boundary=None):
    """solve_exact restated in float32: the same extension FFTs run by pocketfft in complex64, rows first as the library documents,
    float32 denominators (rounded from double), a float32 result: what a plain float32 solve of another algorithm than the
    library's chirp convolution loses on the same input."""
    shape = np.asarray(data).shape
    f = _hwc(rhs(kind, lam, data, lap))
    H, W, C = f.shape
    den = (_eig(kind, H, W) - float(np.float32(lam))).astype(np.float32)
    if kind == NEUMANN:
        out = np.empty((H, W, C), np.float32)
        for c in range(C):
            X = neumann_np._dct2_f32(neumann_np._dct2_f32(f[:, :, c], 1), 0) / den
            assert X.dtype == np.float32
            out[:, :, c] = neumann_np._idct2_f32(neumann_np._idct2_f32(X, 0), 1)
        return out.reshape(shape)
    b = _hwc(np.asarray(boundary, np.float32))
    out = b.copy()
    g = f[1:-1, 1:-1] - _frame_fold(b).astype(np.float32)
    X = _dst1(_dst1(g, 1, True), 0, True) / den[:, :, None]
    u = _dst1(_dst1(X, 0, True), 1, True) * np.float32(4.0 / ((W - 1.0) * (H - 1.0)))
    assert u.dtype == np.float32
    out[1:-1, 1:-1] = u
    return out.reshape(shape)


def operator(kind, lam, u):
    """(A - lam) u in float64.  Neumann: at every pixel; Dirichlet: on the interior (the frame of u holds the boundary values), 0 on
    the frame."""
    u = np.asarray(u, np.float64)
    lam = float(np.float32(lam))
    if kind == NEUMANN:
        return neumann_np.operator(u) - lam * u
    r = np.zeros_like(u)
    c = u[1:-1, 1:-1]
    r[1:-1, 1:-1] = (u[1:-1, :-2] + u[1:-1, 2:] + u[:-2, 1:-1] + u[2:, 1:-1] - 4.0 * c) - lam * c
    return r


def residual(kind, lam, u, data, lap):
    """operator(u) - rhs in float64: what u leaves of the system (Dirichlet: on the interior, 0 on the frame)"""
    return operator(kind, lam, u) - rhs(kind, lam, data, lap).astype(np.float64)
