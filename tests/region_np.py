"""The test side's restatement of the region solve (sc_hip_region*), numpy only, after wls_np.

Borders are (sides, periodic) as in weighted_np.  state (H x W x C, float32) holds 0 (UNKNOWN: solved for), 1 (KNOWN: u = data) or 2
(OUTSIDE: not part of the domain) at every pixel the borders call an unknown; on the Dirichlet lines it is not consulted.  Per channel
the library solves, at every UNKNOWN pixel p,
    sum_q s(p, q) (u(q) - u(p)) - w(p) u(p)  =  div(s g)(p) - w(p) d(p),
q over the neighbours that exist and are not OUTSIDE; u(q) = data(q) at a KNOWN q and boundary(q) on a Dirichlet line.  weight None: no
data term.  sx, sy None: every link 1.

kinds() classifies every pixel; live_links() names the link elements a call may read: live in the WLS sense, neither end OUTSIDE, at
least one end UNKNOWN.  Nothing here reads any other element of the links or the guidance, weight or lap off the UNKNOWN pixels, data
at UNKNOWN pixels without a weight, or boundary off its Dirichlet lines (the GPU tests put NaN there).

folded_rhs(dtype=float32) is the library's b to the letter of seamlessclone_hip.h: (a - b) + (c - d) of separately rounded products
s * g (or lap), then - w * d, then the Dirichlet lines' s * boundary west, north, east, south, then the KNOWN neighbours' s * data west,
north, east, south, each a rounded product subtracted in turn; 0 at every pixel of the block that is not UNKNOWN.  solve_exact()
assembles the matrix over the UNKNOWN pixels only, link by link, in float64 and solves it with LAPACK (above wls_np.DENSE_LIMIT UNKNOWN
pixels: the same entries sparse, factored by scipy).  pcg_f32() is the library's iteration: on the whole unknown block, with coefficient
planes that are 0 at every pixel that is not UNKNOWN, preconditioned by the rectangle's direct solve (weighted_np._precond) -- the
yardstick of tests/region_bounds.py; pcg(dtype=float64) is its float64 twin, the yardstick of single iterates
(tests/pcg_steps_bounds.py).  unpinned_components() finds the UNKNOWN components that nothing holds (the library does not)."""
from __future__ import annotations

import numpy as np

import direct_np
import pcg_np
import weighted_np
import wls_np

_hwc = weighted_np._hwc
unknowns = weighted_np.unknowns
has_dirichlet = weighted_np.has_dirichlet

UNKNOWN, KNOWN, OUTSIDE, DIRICHLET = 0, 1, 2, 3          # a pixel's kind (DIRICHLET: on a Dirichlet line of the borders)
_SHIFTS = ((1, 1), (-1, 1), (1, 0), (-1, 0))             # (shift, axis) that brings the west, east, north, south neighbour to a pixel (_links' order)
_FOLD_ORDER = (0, 2, 1, 3)                               # west, north, east, south: the order the header subtracts the neighbours' terms in


def kinds(sides, periodic, state):
    """int H x W x C: UNKNOWN, KNOWN, OUTSIDE by state inside the borders (anything but 0 and 1 counts as OUTSIDE), DIRICHLET on the lines"""
    st = _hwc(np.asarray(state, np.float32))
    H, W = st.shape[:2]
    k = np.where(st == 0, UNKNOWN, np.where(st == 1, KNOWN, OUTSIDE))
    return np.where(direct_np.dirichlet_mask(sides, periodic, H, W)[:, :, None], DIRICHLET, k)


def _neighbour(a, shift, axis, periodic, fill):
    """a's value at the neighbour across one link: np.roll, with `fill` where the neighbour does not exist (beyond a non-periodic end)"""
    r = np.roll(a, shift, axis).copy()
    if "xy"[1 - axis] not in periodic:
        edge = [slice(None)] * a.ndim
        edge[axis] = 0 if shift == 1 else -1
        r[tuple(edge)] = fill
    return r


def live_links(sides, periodic, state):
    """(live_x, live_y), boolean H x W x C: the elements of smooth_x / smooth_y (and of gx / gy) a region call reads"""
    k = kinds(sides, periodic, state)
    out = []
    for axis in (1, 0):
        q = _neighbour(k, -1, axis, periodic, OUTSIDE)
        out.append((k != OUTSIDE) & (q != OUTSIDE) & ((k == UNKNOWN) | (q == UNKNOWN)))
    return out[0], out[1]


def _links(sides, periodic, state, sx, sy, dtype):
    """(west, east, north, south) of every pixel, H x W x C in dtype: the weight of the link to that neighbour where the link is live in
    the region, 0 elsewhere (sx None: 1 on every link that is live in the region)"""
    lx, ly = live_links(sides, periodic, state)
    one = np.ones(lx.shape, np.float32)
    sx, sy = (one if a is None else _hwc(np.asarray(a, np.float32)) for a in (sx, sy))
    ex = np.where(lx, sx, np.float32(0)).astype(dtype)
    ey = np.where(ly, sy, np.float32(0)).astype(dtype)
    return np.roll(ex, 1, 1), ex, np.roll(ey, 1, 0), ey


def divergence(sides, periodic, state, sx, sy, gx, gy):
    """the guidance sum in float32, H x W x C: (a - b) + (c - d) of products rounded on their own, a link that is not live in the region
    counting 0 (valid at the UNKNOWN pixels)"""
    gx, gy = _hwc(np.asarray(gx, np.float32)), _hwc(np.asarray(gy, np.float32))
    _, east, _, south = _links(sides, periodic, state, sx, sy, np.float32)
    a = np.where(east != 0, east * np.where(east != 0, gx, np.float32(0)), np.float32(0))
    c = np.where(south != 0, south * np.where(south != 0, gy, np.float32(0)), np.float32(0))
    out = (a - np.roll(a, 1, 1)) + (c - np.roll(c, 1, 0))
    assert out.dtype == np.float32
    return out


def folded_rhs(sides, periodic, state, weight, sx, sy, data, lap, boundary, dtype=np.float64):
    """b on the unknown block [ny][nx][C]: at UNKNOWN pixels lap (given, or divergence()) - w * d in float32, then in dtype less the
    Dirichlet neighbours' s * boundary (west, north, east, south) and the KNOWN neighbours' s * data (likewise); 0 elsewhere"""
    k = kinds(sides, periodic, state)
    unk = k == UNKNOWN
    zero = np.float32(0)
    f = np.where(unk, _hwc(np.asarray(lap, np.float32)), zero)
    d = _hwc(np.asarray(data, np.float32))
    if weight is not None:
        w = np.where(unk, _hwc(np.asarray(weight, np.float32)), zero)
        f = f - w * np.where(unk, d, zero)
    assert f.dtype == np.float32
    g = f.astype(dtype)
    links = _links(sides, periodic, state, sx, sy, dtype)
    b = zero if boundary is None else _hwc(np.asarray(boundary, np.float32))
    for kind, values in ((DIRICHLET, b), (KNOWN, d)):
        held = np.where(k == kind, values, zero).astype(dtype)
        for i in _FOLD_ORDER:
            shift, axis = _SHIFTS[i]
            q = _neighbour(k, shift, axis, periodic, OUTSIDE)
            g = g - np.where(unk & (q == kind), links[i] * np.roll(held, shift, axis), dtype(0))
    assert g.dtype == dtype
    return g[unknowns(sides, periodic, *k.shape[:2])]


def _compose(sides, periodic, state, data, boundary, u_blk, dtype):
    """the call's out: u at UNKNOWN pixels, data at KNOWN and OUTSIDE ones, boundary on the Dirichlet lines"""
    k = kinds(sides, periodic, state)
    blk = unknowns(sides, periodic, *k.shape[:2])
    out = _hwc(np.asarray(data, dtype)).copy()
    if has_dirichlet(sides, periodic):
        m = direct_np.dirichlet_mask(sides, periodic, *k.shape[:2])
        out[m] = _hwc(np.asarray(boundary, dtype))[m]
    out[blk] = np.where(k[blk] == UNKNOWN, u_blk, out[blk])
    return out


def solve_exact(sides, periodic, state, weight, sx, sy, data, lap, boundary=None, dense=None):
    """float64 solution: the system over the UNKNOWN pixels only, assembled link by link (a link between two UNKNOWN pixels enters
    both rows, a link to a KNOWN or Dirichlet pixel the diagonal of its UNKNOWN end only); data's shape, composed like out.  dense: None:
    a dense matrix and LAPACK up to wls_np.DENSE_LIMIT UNKNOWN pixels per channel, above it the same entries sparse; True / False force
    one of the two."""
    shape = np.asarray(data).shape
    k = kinds(sides, periodic, state)
    H, W, C = k.shape
    blk = unknowns(sides, periodic, H, W)
    lx, ly = live_links(sides, periodic, state)
    one = np.ones(k.shape, np.float32)
    sxf, syf = (one if a is None else _hwc(np.asarray(a, np.float32)) for a in (sx, sy))
    g = folded_rhs(sides, periodic, state, weight, sx, sy, data, lap, boundary)
    u = np.zeros(g.shape)
    for c in range(C):
        unk = k[:, :, c] == UNKNOWN
        n = int(unk.sum())
        if not n:
            continue
        index = np.full((H, W), -1)
        index[unk] = np.arange(n)
        entries = []          # (row, column, value); an entry named twice counts twice
        if weight is not None:
            entries.append((np.arange(n), np.arange(n), -_hwc(np.asarray(weight, np.float32))[:, :, c][unk].astype(np.float64)))
        for live, s, axis in ((lx[:, :, c], sxf[:, :, c], 1), (ly[:, :, c], syf[:, :, c], 0)):
            ys, xs = np.nonzero(live)
            i, j = index[ys, xs], np.roll(index, -1, axis)[ys, xs]
            v = s[ys, xs].astype(np.float64)
            for a, b in ((i, j), (j, i)):
                ok = a >= 0
                entries.append((a[ok], a[ok], -v[ok]))
                both = ok & (b >= 0)
                entries.append((a[both], b[both], v[both]))
        sol = np.zeros((H, W))
        sol[unk] = wls_np.solve_entries(entries, n, g[:, :, c][unk[blk]], dense if dense is not None else n <= wls_np.DENSE_LIMIT)
        u[:, :, c] = sol[blk]
    return _compose(sides, periodic, state, data, boundary, u, np.float64).reshape(shape)


def _planes(sides, periodic, state, weight, sx, sy, dtype):
    """the operator's coefficients on the unknown block: (west, east, north, south) kept only where both ends are UNKNOWN, and the
    diagonal: the incident links live in the region plus w; all 0 at a pixel that is not UNKNOWN"""
    k = kinds(sides, periodic, state)
    blk = unknowns(sides, periodic, *k.shape[:2])
    unk = k == UNKNOWN
    full = _links(sides, periodic, state, sx, sy, dtype)
    w = dtype(0) if weight is None else _hwc(np.asarray(weight, np.float32)).astype(dtype)
    dg = np.where(unk, ((full[0] + full[1]) + (full[2] + full[3])) + np.where(unk, w, dtype(0)), dtype(0))
    links = tuple(np.where(unk & (_neighbour(k, shift, axis, periodic, OUTSIDE) == UNKNOWN), f, dtype(0))[blk]
                  for f, (shift, axis) in zip(full, _SHIFTS))
    return links, dg[blk]


def residual(sides, periodic, state, weight, sx, sy, u, data, lap, boundary=None):
    """L u - b in float64 on the unknown block (0 where the pixel is not UNKNOWN); u: a call's out"""
    links, dg = _planes(sides, periodic, state, weight, sx, sy, np.float64)
    k = kinds(sides, periodic, state)
    blk = unknowns(sides, periodic, *k.shape[:2])
    ub = np.where(k[blk] == UNKNOWN, _hwc(np.asarray(u, np.float64))[blk], 0.0)
    return wls_np.block_operator(links, dg, ub) - folded_rhs(sides, periodic, state, weight, sx, sy, data, lap, boundary)


def precond_means(sides, periodic, state, weight, sx, sy):
    """(s-bar, w-bar) as the library takes them for one problem: the mean of the links live in the region, and (sum of w over the UNKNOWN
    pixels + sum of the UNKNOWN - KNOWN links) / (UNKNOWN pixels); also the counts (live links, UNKNOWN pixels) a chunk's means weigh by"""
    k = kinds(sides, periodic, state)
    lx, ly = live_links(sides, periodic, state)
    one = np.ones(k.shape, np.float32)
    sxf, syf = (one if a is None else _hwc(np.asarray(a, np.float32)) for a in (sx, sy))
    v = np.concatenate([sxf[lx], syf[ly]]).astype(np.float64)
    uk = 0.0
    for live, s, axis in ((lx, sxf, 1), (ly, syf, 0)):
        q = _neighbour(k, -1, axis, periodic, OUTSIDE)
        uk += float(s[live & (k + q == KNOWN)].astype(np.float64).sum())          # one end UNKNOWN (0), the other KNOWN (1)
    unk = k == UNKNOWN
    wsum = 0.0 if weight is None else float(_hwc(np.asarray(weight, np.float32))[unk].astype(np.float64).sum())
    n = int(unk.sum())
    sbar = float(v.mean()) if v.size and sx is not None else 1.0
    return sbar, ((wsum + uk) / n if n else sbar), v.size, n


def pcg(sides, periodic, state, weight, sx, sy, data, lap, boundary=None, tol=1e-5, max_iters=400, precond_lambda=None, precond_smooth=None,
        dtype=np.float32, keep=None):
    """The library's iteration in numpy, on the whole unknown block; dtype float64: the same iteration on float64 vectors and
    coefficient planes with the float64 direct solve (lam and the start's factor the same float32).  keep: a list that receives every iterate,
    composed like out.  Returns (out, iterations, the worst channel's final ||r|| / ||b||)."""
    shape = np.asarray(data).shape
    k = kinds(sides, periodic, state)
    H, W, C = k.shape
    blk = unknowns(sides, periodic, H, W)
    links, dg = _planes(sides, periodic, state, weight, sx, sy, dtype)
    sbar, wbar, _, _ = precond_means(sides, periodic, state, weight, sx, sy)
    sbar = sbar if precond_smooth is None else float(np.float32(precond_smooth))
    wbar = wbar if precond_lambda is None else float(np.float32(precond_lambda))
    lam, scale = np.float32(wbar / sbar), np.float32(1.0 / sbar)
    b = folded_rhs(sides, periodic, state, weight, sx, sy, data, lap, boundary, dtype)
    scratch = np.zeros((H, W, C), dtype)
    us = []
    scratch, it, rel = pcg_np.pcg(b, lambda p: wls_np.block_operator(links, dg, p),
                                  lambda r: weighted_np._precond(sides, periodic, lam, r, (H, W, C), dtype), dtype(scale), tol, max_iters, scratch, blk,
                                  dtype, us)
    if keep is not None:
        keep += [_compose(sides, periodic, state, data, boundary, u, dtype).reshape(shape) for u in us]
    return _compose(sides, periodic, state, data, boundary, scratch[blk], dtype).reshape(shape), it, rel


def pcg_f32(sides, periodic, state, weight, sx, sy, data, lap, boundary=None, tol=1e-5, max_iters=400, precond_lambda=None, precond_smooth=None):
    """pcg() in the library's arithmetic: float32 vectors, the float32 direct solve"""
    return pcg(sides, periodic, state, weight, sx, sy, data, lap, boundary, tol, max_iters, precond_lambda, precond_smooth, np.float32)


def unpinned_components(sides, periodic, state, weight=None):
    """boolean H x W x C: the UNKNOWN pixels of connected components (through links between UNKNOWN pixels) that have no KNOWN or
    Dirichlet neighbour and no positive weight.  Components: scipy.ndimage.label per channel (4-connected), and the labels that meet
    across the wrap of a periodic axis joined."""
    import scipy.ndimage
    k = kinds(sides, periodic, state)
    unk = k == UNKNOWN
    held = np.zeros(k.shape, bool)
    for shift, axis in _SHIFTS:
        q = _neighbour(k, shift, axis, periodic, OUTSIDE)
        held |= (q == KNOWN) | (q == DIRICHLET)
    if weight is not None:
        held |= np.where(unk, _hwc(np.asarray(weight, np.float32)), np.float32(0)) > 0
    out = np.zeros(k.shape, bool)
    for c in range(k.shape[2]):
        label, n = scipy.ndimage.label(unk[:, :, c])
        root = np.arange(n + 1)

        def find(i):
            while root[i] != i:
                root[i] = root[root[i]]
                i = root[i]
            return i
        for name, first, last in (("x", label[:, 0], label[:, -1]), ("y", label[0], label[-1])):
            if name in periodic:
                for a, b in zip(first, last):
                    if a and b:
                        root[find(a)] = find(b)
        root = np.array([find(i) for i in range(n + 1)])
        pinned = np.zeros(n + 1, bool)
        pinned[root[label[unk[:, :, c] & held[:, :, c]]]] = True
        out[:, :, c] = unk[:, :, c] & ~pinned[root[label]]
    return out
