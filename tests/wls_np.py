"""The test side's restatement of the WLS solve (sc_hip_wls*), numpy only.

Borders are (sides, periodic) as in weighted_np.  Per channel the library solves, at every unknown p,
    (L u)(p) = sum_q s(p, q) (u(q) - u(p)) - w(p) u(p)  =  div(s g)(p) - w(p) d(p),
q over the neighbours that exist, u = boundary on the Dirichlet lines.  smooth_x[y, x] is the link (x, y) - (x + 1, y), smooth_y[y, x] the
link (x, y) - (x, y + 1); the last column / row holds the wrapping link of a periodic axis.  live_links() names the elements a call may
read: links with at least one unknown end.  Nothing here reads any other element (the GPU tests put NaN there).

divergence() and folded_rhs(dtype=float32) are the library's float32 right-hand side to the letter of seamlessclone_hip.h: every
product s * g rounded on its own, (a - b) + (c - d), then - w * d (one multiply, one subtract), then the Dirichlet terms s * boundary
subtracted west, north, east, south.  operator() / residual() apply the stencil in float64.  solve_exact() assembles L in float64 from
the links, entry by entry, and solves with LAPACK (above DENSE_LIMIT unknowns: the same entries sparse, factored by scipy).  pcg_f32()
is the library's iteration: float32 vectors, float64 dot products, preconditioned by direct_np.solve_f32 with lam = w-bar / s-bar,
started from u0 = (1 / s-bar) (A - lam)^-1 b -- the yardstick of tests/wls_bounds.py; pcg(dtype=float64) is its float64 twin, the
yardstick of single iterates (tests/pcg_steps_bounds.py).  Arrays are H x W x C (H x W accepted)."""
from __future__ import annotations

import numpy as np

import pcg_np
import direct_np
import weighted_np

_hwc = weighted_np._hwc
unknowns = weighted_np.unknowns
has_dirichlet = weighted_np.has_dirichlet


def live_links(sides, periodic, H, W):
    """(live_x, live_y), boolean H x W"""
    unk = ~direct_np.dirichlet_mask(sides, periodic, H, W)
    lx, ly = unk | np.roll(unk, -1, 1), unk | np.roll(unk, -1, 0)
    if "x" not in periodic:
        lx[:, -1] = False
    if "y" not in periodic:
        ly[-1] = False
    return lx, ly


def _links(sides, periodic, sx, sy, dtype):
    """(west, east, north, south) of every pixel, H x W x C in dtype: the weight of the link to that neighbour, 0 where the neighbour
    does not exist.  Only live elements of sx, sy are taken (at an unknown every existing link is live; elsewhere 0 stands for the rest)."""
    sx, sy = _hwc(np.asarray(sx, np.float32)), _hwc(np.asarray(sy, np.float32))
    H, W = sx.shape[:2]
    lx, ly = live_links(sides, periodic, H, W)
    ex = np.where(lx[:, :, None], sx, np.float32(0)).astype(dtype)
    ey = np.where(ly[:, :, None], sy, np.float32(0)).astype(dtype)
    return np.roll(ex, 1, 1), ex, np.roll(ey, 1, 0), ey


def divergence(sides, periodic, sx, sy, gx, gy):
    """div(s g) in float32, H x W x C: (a - b) + (c - d), a = sx gx at the pixel, b = sx gx of its left neighbour (column 0: of the last
    column along a periodic axis, else 0), c, d likewise along y; each product rounded to float32 before any difference"""
    gx, gy = _hwc(np.asarray(gx, np.float32)), _hwc(np.asarray(gy, np.float32))
    _, east, _, south = _links(sides, periodic, sx, sy, np.float32)
    a = np.where(east != 0, east * np.where(east != 0, gx, np.float32(0)), np.float32(0))
    c = np.where(south != 0, south * np.where(south != 0, gy, np.float32(0)), np.float32(0))
    out = (a - np.roll(a, 1, 1)) + (c - np.roll(c, 1, 0))
    assert out.dtype == np.float32
    return out


rhs = weighted_np.rhs          # lap - w * d in float32 at the unknowns, 0 on the Dirichlet lines (lap: given, or divergence())


def folded_rhs(sides, periodic, weight, sx, sy, data, lap, boundary, dtype=np.float64):
    """b on the unknown block: rhs less the Dirichlet neighbours' s * boundary, west, north, east, south (float32: the library's b)"""
    f = rhs(sides, periodic, weight, data, lap)
    H, W = f.shape[:2]
    blk = unknowns(sides, periodic, H, W)
    g = f[blk].astype(dtype)
    if has_dirichlet(sides, periodic):
        fr = np.where(direct_np.dirichlet_mask(sides, periodic, H, W)[:, :, None], _hwc(np.asarray(boundary, np.float32)), np.float32(0)).astype(dtype)
        west, east, north, south = _links(sides, periodic, sx, sy, dtype)
        for link, shift, axis in ((west, 1, 1), (north, 1, 0), (east, -1, 1), (south, -1, 0)):
            g = g - (link * np.roll(fr, shift, axis))[blk]          # (a wrapped neighbour is never on a Dirichlet line)
    assert g.dtype == dtype
    return g


def operator(sides, periodic, weight, sx, sy, u):
    """L u in float64 at the unknowns (the Dirichlet lines of u hold the known values), 0 on the Dirichlet lines"""
    u = _hwc(np.asarray(u, np.float64))
    w = _hwc(np.asarray(weight, np.float32)).astype(np.float64)
    west, east, north, south = _links(sides, periodic, sx, sy, np.float64)
    full = (west * (np.roll(u, 1, 1) - u) + east * (np.roll(u, -1, 1) - u) + north * (np.roll(u, 1, 0) - u) + south * (np.roll(u, -1, 0) - u)) - w * u
    r = np.zeros_like(u)
    blk = unknowns(sides, periodic, *u.shape[:2])
    r[blk] = full[blk]
    return r


def residual(sides, periodic, weight, sx, sy, u, data, lap):
    """operator(u) - rhs in float64 (0 on the Dirichlet lines)"""
    return operator(sides, periodic, weight, sx, sy, u) - rhs(sides, periodic, weight, data, lap).astype(np.float64)


DENSE_LIMIT = weighted_np.DENSE_LIMIT


def solve_entries(entries, n, g, dense):
    """the float64 solution of M x = g, M the n x n matrix of the entries [(rows, columns, values)] (an entry named twice counts
    twice): dense through LAPACK, or sparse through weighted_np.sparse_solve"""
    rows, cols, vals = (np.concatenate([e[i] for e in entries]) for i in range(3))
    if dense:
        M = np.zeros((n, n))
        np.add.at(M, (rows, cols), vals)
        return np.linalg.solve(M, g)
    import scipy.sparse
    return weighted_np.sparse_solve(scipy.sparse.coo_matrix((vals, (rows, cols)), shape=(n, n)), g)


def solve_exact(sides, periodic, weight, sx, sy, data, lap, boundary=None, dense=None):
    """float64 solution of L u = rhs: boundary's values on the Dirichlet lines, the solution at the unknowns; data's shape.  The matrix
    is assembled link by link: a link between two unknowns enters both rows, a link to a Dirichlet pixel the diagonal only.  dense:
    None: a dense matrix and LAPACK up to DENSE_LIMIT unknowns, above it the same entries sparse (weighted_np.sparse_solve); True / False
    force one of the two."""
    shape = np.asarray(data).shape
    w = _hwc(np.asarray(weight, np.float32)).astype(np.float64)
    sxf, syf = _hwc(np.asarray(sx, np.float32)), _hwc(np.asarray(sy, np.float32))
    H, W, C = w.shape
    blk = unknowns(sides, periodic, H, W)
    unk = ~direct_np.dirichlet_mask(sides, periodic, H, W)
    lx, ly = live_links(sides, periodic, H, W)
    index = np.full((H, W), -1)
    index[blk] = np.arange(unk.sum()).reshape(index[blk].shape)
    n = int(unk.sum())
    g = folded_rhs(sides, periodic, weight, sx, sy, data, lap, boundary)
    out = _hwc(np.asarray(boundary, np.float64)).copy() if has_dirichlet(sides, periodic) else np.zeros((H, W, C))
    dense = dense if dense is not None else n <= DENSE_LIMIT
    for c in range(C):
        # the entries (row, column, value); an entry named twice counts twice
        entries = [(np.arange(n), np.arange(n), -w[blk][:, :, c].reshape(-1))]
        for live, s, axis in ((lx, sxf, 1), (ly, syf, 0)):
            ys, xs = np.nonzero(live)
            i, j = index[ys, xs], np.roll(index, -1, axis)[ys, xs]
            v = s[ys, xs, c].astype(np.float64)
            for a, b in ((i, j), (j, i)):
                ok = a >= 0
                entries.append((a[ok], a[ok], -v[ok]))
                both = ok & (b >= 0)
                entries.append((a[both], b[both], v[both]))
        out[blk[0], blk[1], c] = solve_entries(entries, n, g[:, :, c].reshape(-1), dense).reshape(g.shape[:2])
    return out.reshape(shape)


def mean_link(sides, periodic, sx, sy):
    """the library's automatic s-bar of one problem: the arithmetic mean of its live links, in float64"""
    sx, sy = _hwc(np.asarray(sx, np.float32)), _hwc(np.asarray(sy, np.float32))
    lx, ly = live_links(sides, periodic, *sx.shape[:2])
    v = np.concatenate([sx[lx].reshape(-1), sy[ly].reshape(-1)]).astype(np.float64)
    return float(v.mean()) if v.size else 1.0


def mean_weight(sides, periodic, weight):
    """the automatic w-bar: the mean of w over the unknowns, in float64"""
    w = _hwc(np.asarray(weight, np.float32))
    return float(w[unknowns(sides, periodic, *w.shape[:2])].astype(np.float64).mean())


def block_operator(links, dg, u):
    """L u on the unknown block [ny][nx][C] in float32, in the kernel's order; links: (west, east, north, south) on the block with the
    links to Dirichlet pixels taken out (they live in dg alone)"""
    west, east, north, south = links
    return ((west * np.roll(u, 1, 1) + east * np.roll(u, -1, 1)) + (north * np.roll(u, 1, 0) + south * np.roll(u, -1, 0))) - dg * u


def pcg(sides, periodic, weight, sx, sy, data, lap, boundary=None, tol=1e-5, max_iters=400, precond_lambda=None, precond_smooth=None,
        dtype=np.float32, keep=None):
    """The library's iteration in numpy; dtype float64: the same iteration on float64 vectors, links and diagonal with the float64
    direct solve (lam and the start's factor the same float32).  keep: a list that receives every iterate, composed like the return
    value's first element.  Returns (u of data's shape with boundary's values on the Dirichlet
    lines, iterations, the worst channel's final ||r|| / ||b||)."""
    shape = np.asarray(data).shape
    w_full = _hwc(np.asarray(weight, np.float32))
    H, W, C = w_full.shape
    blk = unknowns(sides, periodic, H, W)
    unk = ~direct_np.dirichlet_mask(sides, periodic, H, W)
    full = _links(sides, periodic, sx, sy, dtype)
    dg = (((full[0] + full[1]) + (full[2] + full[3])) + w_full.astype(dtype))[blk]
    # the links between two unknowns: the neighbour in that direction (with wrap) is an unknown too
    links = tuple(np.where(np.roll(unk, shift, axis)[:, :, None], f, dtype(0))[blk]
                  for f, shift, axis in zip(full, (1, -1, 1, -1), (1, 1, 0, 0)))
    sbar = mean_link(sides, periodic, sx, sy) if precond_smooth is None else float(np.float32(precond_smooth))
    wbar = mean_weight(sides, periodic, weight) if precond_lambda is None else float(np.float32(precond_lambda))
    lam, scale = np.float32(wbar / sbar), np.float32(1.0 / sbar)
    b = folded_rhs(sides, periodic, weight, sx, sy, data, lap, boundary, dtype)
    out = _hwc(np.asarray(boundary, dtype)).copy() if has_dirichlet(sides, periodic) else np.zeros((H, W, C), dtype)
    us = []
    out, it, rel = pcg_np.pcg(b, lambda p: block_operator(links, dg, p), lambda r: weighted_np._precond(sides, periodic, lam, r, (H, W, C), dtype),
                              dtype(scale), tol, max_iters, out, blk, dtype, us)
    if keep is not None:
        keep += [weighted_np._placed(out, blk, u).reshape(shape) for u in us]
    return out.reshape(shape), it, rel


def pcg_f32(sides, periodic, weight, sx, sy, data, lap, boundary=None, tol=1e-5, max_iters=400, precond_lambda=None, precond_smooth=None):
    """pcg() in the library's arithmetic: float32 vectors, the float32 direct solve"""
    return pcg(sides, periodic, weight, sx, sy, data, lap, boundary, tol, max_iters, precond_lambda, precond_smooth, np.float32)
