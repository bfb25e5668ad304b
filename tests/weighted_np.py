"""The test side's restatement of the weighted solve (sc_hip_weighted*), numpy only.

A problem's borders are (sides, periodic) as in direct_np: `sides` names the sides WITHOUT a Dirichlet line, `periodic` the axes
that wrap.  Per channel the library solves
    (A - W) u = lap - w d        at the unknowns,        W = diag(w), w >= 0,
lap given or the float32 divergence of a guidance field (direct_np.divergence), u = boundary on the Dirichlet lines.  rhs() is the
library's float32 right-hand side to the letter: the product w * d rounded to float32, then subtracted from lap.

solve_exact() assembles A - W in float64 from the two axes' 1-D operators (axis_matrix: a Kronecker sum) and solves it with LAPACK --
above DENSE_LIMIT unknowns the same entries sparse, factored by scipy: no transform, nothing shared with the library or with the other
restatements.  operator() and residual() apply the stencil
directly (direct_np.operator).  pcg_f32() is the library's iteration restated in numpy: float32 vectors, float64 dot products,
preconditioned by direct_np.solve_f32 with the constant lambda-bar -- the yardstick of the GPU tests' bounds and iteration counts
(tests/weighted_bounds.py); pcg(dtype=float64) is its float64 twin, the yardstick of single iterates (tests/pcg_steps_bounds.py).  Arrays are H x W x C (H x W accepted)."""
from __future__ import annotations

import numpy as np

import pcg_np
import direct_np

DD, NN, DN, ND, PP = direct_np.DD, direct_np.NN, direct_np.DN, direct_np.ND, direct_np.PP


def _hwc(a):
    return a[:, :, None] if a.ndim == 2 else a


def unknowns(sides, periodic, H, W):
    return direct_np.unknowns(sides, periodic, H, W)


def has_dirichlet(sides, periodic):
    ax, ay = direct_np.axis_kinds(sides, periodic)
    return not (ax in (NN, PP) and ay in (NN, PP))


def rhs(sides, periodic, weight, data, lap):
    """lap - w * d in float32 at the unknowns (one multiply, then one subtract), 0 on the Dirichlet lines"""
    lap, d, w = (_hwc(np.asarray(a, np.float32)) for a in (lap, data, weight))
    f = lap - w * d
    assert f.dtype == np.float32
    out = np.zeros_like(f)
    blk = unknowns(sides, periodic, *f.shape[:2])
    out[blk] = f[blk]
    return out


def operator(sides, periodic, weight, u):
    """(A - W) u in float64 at the unknowns (the Dirichlet lines of u hold the known values), 0 on the Dirichlet lines"""
    u = _hwc(np.asarray(u, np.float64))
    w = _hwc(np.asarray(weight, np.float32)).astype(np.float64)
    r = direct_np.operator(sides, periodic, 0.0, u)
    blk = unknowns(sides, periodic, *u.shape[:2])
    r[blk] -= (w * u)[blk]
    return r


def residual(sides, periodic, weight, u, data, lap):
    """operator(u) - rhs in float64 (0 on the Dirichlet lines)"""
    return operator(sides, periodic, weight, u) - rhs(sides, periodic, weight, data, lap).astype(np.float64)


def _low_d(kind):
    return kind in (DD, DN)


def _high_d(kind):
    return kind in (DD, ND)


def _axis_apply(u, axis, kind):
    """the 1-D operator along `axis` of the unknown block u, in u's dtype: sum over the neighbours that exist of (u_n - u); beyond a
    Dirichlet line u_n = 0, beyond a free end no term, beyond the end of a periodic axis the pixel at the other end"""
    n = u.shape[axis]
    lo, hi = np.roll(u, 1, axis) - u, np.roll(u, -1, axis) - u
    first = [slice(None)] * u.ndim
    last = [slice(None)] * u.ndim
    first[axis], last[axis] = slice(0, 1), slice(n - 1, n)
    first, last = tuple(first), tuple(last)
    if kind != PP:
        lo[first] = -u[first] if _low_d(kind) else 0
        hi[last] = -u[last] if _high_d(kind) else 0
    return lo + hi


def axis_matrix(kind, n):
    """the 1-D operator of an axis of n unknowns as a dense float64 matrix"""
    return _axis_apply(np.eye(n), 0, kind)


def block_operator(ax, ay, w, u):
    """(A - W) u on the unknown block [ny][nx][C], homogeneous Dirichlet lines, in u's dtype"""
    return (_axis_apply(u, 1, ax) + _axis_apply(u, 0, ay)) - w * u


def folded_rhs(sides, periodic, weight, data, lap, boundary, dtype=np.float64):
    """the interior system's right-hand side on the unknown block: rhs less the neighbouring Dirichlet lines' values"""
    f = rhs(sides, periodic, weight, data, lap)
    blk = unknowns(sides, periodic, *f.shape[:2])
    g = f[blk].astype(dtype)
    if has_dirichlet(sides, periodic):
        g = g - direct_np.fold(sides, periodic, _hwc(np.asarray(boundary, dtype))).astype(dtype)
    return g


DENSE_LIMIT = 4000                                 # unknowns per channel up to which the exact solves assemble a dense matrix


def sparse_solve(M, g):
    """the float64 solution of M x = g for a scipy.sparse matrix M, factored by scipy.sparse.linalg.splu: the dense solves' twin above
    DENSE_LIMIT -- the same entries, another factorisation"""
    import scipy.sparse.linalg
    return scipy.sparse.linalg.splu(M.tocsc()).solve(np.asarray(g, np.float64))


def solve_exact(sides, periodic, weight, data, lap, boundary=None, dense=None):
    """float64 solution of (A - W) u = rhs: boundary's values on the Dirichlet lines, the solution at the unknowns; data's shape.
    dense: None: a dense matrix and LAPACK up to DENSE_LIMIT unknowns, above it the same entries sparse (sparse_solve); True / False
    force one of the two."""
    shape = np.asarray(data).shape
    w = _hwc(np.asarray(weight, np.float32)).astype(np.float64)
    H, W, C = w.shape
    blk = unknowns(sides, periodic, H, W)
    ax, ay = direct_np.axis_kinds(sides, periodic)
    g = folded_rhs(sides, periodic, weight, data, lap, boundary)
    ny, nx = g.shape[:2]
    out = _hwc(np.asarray(boundary, np.float64)).copy() if has_dirichlet(sides, periodic) else np.zeros((H, W, C))
    if dense if dense is not None else ny * nx <= DENSE_LIMIT:
        A = np.kron(np.eye(ny), axis_matrix(ax, nx)) + np.kron(axis_matrix(ay, ny), np.eye(nx))
        for c in range(C):
            M = A - np.diag(w[blk][:, :, c].reshape(-1))
            out[blk[0], blk[1], c] = np.linalg.solve(M, g[:, :, c].reshape(-1)).reshape(ny, nx)
        return out.reshape(shape)
    import scipy.sparse as sp
    A = sp.kron(sp.identity(ny), sp.csr_matrix(axis_matrix(ax, nx))) + sp.kron(sp.csr_matrix(axis_matrix(ay, ny)), sp.identity(nx))
    for c in range(C):
        M = A - sp.diags(w[blk][:, :, c].reshape(-1))
        out[blk[0], blk[1], c] = sparse_solve(M, g[:, :, c].reshape(-1)).reshape(ny, nx)
    return out.reshape(shape)


def mean_weight(sides, periodic, weight):
    """the library's automatic lambda-bar of one problem: the mean of w over its unknowns (summed in double), as a float32"""
    w = _hwc(np.asarray(weight, np.float32))
    return np.float32(w[unknowns(sides, periodic, *w.shape[:2])].astype(np.float64).mean())


def _precond(sides, periodic, lam, r_blk, shape, dtype=np.float32):
    """(A - lam)^-1 r on the unknown block in float32 (direct_np.solve_f32 with zero data and a zero boundary, rows first
    both ways: the order the weighted, WLS and robust constants were measured with); dtype float64: the float64 direct solve of the
    same right-hand side with the same lam"""
    H, W, C = shape
    full = np.zeros((H, W, C), dtype)
    blk = unknowns(sides, periodic, H, W)
    full[blk] = r_blk
    zero = np.zeros((H, W, C), dtype)
    if dtype == np.float64:
        return direct_np.solve_rhs(sides, periodic, float(lam), full, zero, False, direct_np.ROWS_FIRST_BOTH_WAYS)[blk]
    z = direct_np.solve_f32(sides, periodic, float(lam), zero if lam else None, full, zero, order=direct_np.ROWS_FIRST_BOTH_WAYS)
    return np.asarray(z, np.float32)[blk]


def _placed(out, blk, u):
    """a copy of out with u at blk"""
    o = out.copy()
    o[blk] = u
    return o


def pcg(sides, periodic, weight, data, lap, boundary=None, tol=1e-5, max_iters=200, precond_lambda=None, dtype=np.float32, keep=None):
    """The library's iteration in numpy: conjugate gradients on (A - W) u = b in float32 with float64 dot products, per channel its own
    alpha and beta, preconditioned by the float32 direct solve of A - lambda-bar (default: the mean weight), started from M^-1 b;
    stops when ||r|| <= tol ||b|| on every channel, r the iteration's own residual.  dtype float64: the same iteration on float64
    vectors with the float64 direct solve (lambda-bar the same float32).  keep: a list that receives every iterate, composed like the
    return value's first element.  Returns (u of data's shape with boundary's values on the
    Dirichlet lines, iterations, the worst channel's final ||r|| / ||b||)."""
    shape = np.asarray(data).shape
    w_full = _hwc(np.asarray(weight, np.float32))
    H, W, C = w_full.shape
    blk = unknowns(sides, periodic, H, W)
    ax, ay = direct_np.axis_kinds(sides, periodic)
    w = w_full[blk].astype(dtype)
    lam = mean_weight(sides, periodic, weight) if precond_lambda is None else np.float32(precond_lambda)
    b = folded_rhs(sides, periodic, weight, data, lap, boundary, dtype)
    out = _hwc(np.asarray(boundary, dtype)).copy() if has_dirichlet(sides, periodic) else np.zeros((H, W, C), dtype)
    us = []
    out, it, rel = pcg_np.pcg(b, lambda p: block_operator(ax, ay, w, p), lambda r: _precond(sides, periodic, lam, r, (H, W, C), dtype), None,
                              tol, max_iters, out, blk, dtype, us)
    if keep is not None:
        keep += [_placed(out, blk, u).reshape(shape) for u in us]
    return out.reshape(shape), it, rel


def pcg_f32(sides, periodic, weight, data, lap, boundary=None, tol=1e-5, max_iters=200, precond_lambda=None):
    """pcg() in the library's arithmetic: float32 vectors, the float32 direct solve"""
    return pcg(sides, periodic, weight, data, lap, boundary, tol, max_iters, precond_lambda, np.float32)
