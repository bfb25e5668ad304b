"""The test side's restatement of the volume solve (sc_hip_volume*), numpy only, built on region_np.

A volume is T frames: every array is T x H x W x C (gt: (T - 1) x H x W x C), borders are (sides, periodic) as in weighted_np.  Within a
frame the problem is region_np's with every spatial link 1; pixel q of frame t and pixel q of frame t + 1 are joined by a temporal link of
the constant weight tau, live when neither end is OUTSIDE or on a Dirichlet line and at least one end is UNKNOWN.  A KNOWN temporal
neighbour adds tau to the diagonal of its unknown end and tau * data to the right-hand side; the ends of time are free.

kinds() classifies every pixel; live_links() names the elements of gx, gy and gt a call may read (three arrays).  divergence() is steps 1
and 2 of the header's right-hand side, folded_rhs(dtype=float32) the whole of it to the letter: the region call's guidance sum of the
frame, + (e - f) of the rounded products tau * gt at the live forward and backward temporal links, - w * d, the Dirichlet terms, the
KNOWN spatial neighbours west, north, east, south, the KNOWN temporal neighbours previous, then next -- each a rounded product
subtracted in turn; 0 at every pixel that is not UNKNOWN.  solve_exact() is the float64 answer: dense LAPACK up to DENSE_LIMIT unknowns
per channel, above that conjugate gradients in float64 with the exact constant-coefficient preconditioner, run to a relative residual of
1e-13.  pcg_f32() is the library's iteration -- one system per channel over all frames, preconditioned by the orthonormal DCT-II along
the frames (table computed in double, rounded to float32), the float32 direct solve of every mode (weighted_np._precond) with the shift
w-bar + tau (2 - 2 cos(pi k / T)), and the transposed transform -- the yardstick of tests/volume_bounds.py.  unpinned_components() finds
the UNKNOWN components, through all three link kinds, that nothing holds (the library does not)."""
from __future__ import annotations

import numpy as np

import direct_np
import pcg_np
import region_np
import weighted_np

UNKNOWN, KNOWN, OUTSIDE, DIRICHLET = region_np.UNKNOWN, region_np.KNOWN, region_np.OUTSIDE, region_np.DIRICHLET
unknowns = weighted_np.unknowns
has_dirichlet = weighted_np.has_dirichlet
DENSE_LIMIT = 3000


def _thwc(a):
    return a[:, :, :, None] if a.ndim == 3 else a


def kinds(sides, periodic, state):
    """int T x H x W x C: region_np.kinds of every frame"""
    st = _thwc(np.asarray(state, np.float32))
    return np.stack([region_np.kinds(sides, periodic, f) for f in st])


def _time_live(k):
    """boolean (T - 1) x H x W x C: the temporal link from frame t to t + 1 is live"""
    a, b = k[:-1], k[1:]
    inside = (a <= KNOWN) & (b <= KNOWN)          # neither OUTSIDE nor on a Dirichlet line
    return inside & ((a == UNKNOWN) | (b == UNKNOWN))


def live_links(sides, periodic, state):
    """(live_x, live_y, live_t): the elements of gx, gy (T x H x W x C) and gt ((T - 1) x H x W x C) a volume call reads"""
    st = _thwc(np.asarray(state, np.float32))
    per = [region_np.live_links(sides, periodic, f) for f in st]
    return np.stack([p[0] for p in per]), np.stack([p[1] for p in per]), _time_live(kinds(sides, periodic, st))


def _time_links(k, tau, dtype):
    """(back, forward), T x H x W x C in dtype: tau where the temporal link to the previous / next frame is live, else 0"""
    lt = np.where(_time_live(k), np.float32(tau), np.float32(0)).astype(dtype)
    zero = np.zeros((1,) + k.shape[1:], dtype)
    return np.concatenate([zero, lt]), np.concatenate([lt, zero])


def divergence(sides, periodic, state, tau, gx, gy, gt=None):
    """steps 1 and 2 of the right-hand side in float32, T x H x W x C: the frame's guidance sum + (e - f) (valid at the UNKNOWN pixels)"""
    st = _thwc(np.asarray(state, np.float32))
    gx, gy = _thwc(np.asarray(gx, np.float32)), _thwc(np.asarray(gy, np.float32))
    div = np.stack([region_np.divergence(sides, periodic, st[t], None, None, gx[t], gy[t]) for t in range(st.shape[0])])
    live = _time_live(kinds(sides, periodic, st))
    zero = np.float32(0)
    if gt is None:
        prod = np.zeros(live.shape, np.float32)
    else:
        prod = np.where(live, np.float32(tau) * np.where(live, _thwc(np.asarray(gt, np.float32)), zero), zero)
    pad = np.zeros((1,) + prod.shape[1:], np.float32)
    out = div + (np.concatenate([prod, pad]) - np.concatenate([pad, prod]))
    assert out.dtype == np.float32
    return out


def folded_rhs(sides, periodic, state, weight, tau, data, lap, boundary, dtype=np.float64):
    """b on the unknown blocks [T][ny][nx][C]; lap: steps 1 and 2 (divergence(), or the caller's lap)"""
    st, d, lap = (_thwc(np.asarray(a, np.float32)) for a in (state, data, lap))
    w = None if weight is None else _thwc(np.asarray(weight, np.float32))
    bd = None if boundary is None else _thwc(np.asarray(boundary, np.float32))
    k = kinds(sides, periodic, st)
    T, H, W, _ = k.shape
    blk = unknowns(sides, periodic, H, W)
    g = np.stack([region_np.folded_rhs(sides, periodic, st[t], None if w is None else w[t], None, None, d[t], lap[t],
                                       None if bd is None else bd[t], dtype) for t in range(T)])
    tau_d = np.float32(tau) * np.where(k == KNOWN, d, np.float32(0)) if dtype == np.float32 else \
        np.float64(np.float32(tau)) * np.where(k == KNOWN, d, np.float32(0)).astype(np.float64)
    unk = k == UNKNOWN
    zero = np.zeros((1,) + k.shape[1:], dtype)
    prev = np.concatenate([zero, np.where(unk[1:] & (k[:-1] == KNOWN), tau_d[:-1], dtype(0))])
    nxt = np.concatenate([np.where(unk[:-1] & (k[1:] == KNOWN), tau_d[1:], dtype(0)), zero])
    g = (g - prev[(slice(None),) + blk]) - nxt[(slice(None),) + blk]
    assert g.dtype == dtype
    return g


def _planes(sides, periodic, state, weight, tau, dtype):
    """the operator's coefficients on the unknown blocks [T][ny][nx][C]: (west, east, north, south, back, forward) kept only where both
    ends are UNKNOWN, and the diagonal in the kernel's order; all 0 at a pixel that is not UNKNOWN"""
    st = _thwc(np.asarray(state, np.float32))
    k = kinds(sides, periodic, st)
    T, H, W, _ = k.shape
    blk = (slice(None),) + unknowns(sides, periodic, H, W)
    unk = k == UNKNOWN
    full = [np.stack(f) for f in zip(*(region_np._links(sides, periodic, st[t], None, None, dtype) for t in range(T)))]
    back, fwd = _time_links(k, tau, dtype)
    w = dtype(0) if weight is None else _thwc(np.asarray(weight, np.float32)).astype(dtype)
    dg = np.where(unk, (((full[0] + full[1]) + (full[2] + full[3])) + (back + fwd)) + np.where(unk, w, dtype(0)), dtype(0))
    links = [np.stack([np.where(unk[t] & (region_np._neighbour(k[t], shift, axis, periodic, OUTSIDE) == UNKNOWN), f[t], dtype(0)) for t in range(T)])
             for f, (shift, axis) in zip(full, region_np._SHIFTS)]
    pad = np.zeros((1,) + k.shape[1:], bool)
    links.append(np.where(unk & np.concatenate([pad, unk[:-1]]), back, dtype(0)))
    links.append(np.where(unk & np.concatenate([unk[1:], pad]), fwd, dtype(0)))
    return tuple(l[blk] for l in links), dg[blk]


def block_operator(links, dg, u):
    """L u on the unknown blocks [T][ny][nx][C] in u's dtype, in the kernel's order"""
    west, east, north, south, back, fwd = links
    zero = np.zeros_like(u[:1])
    up, dn = np.concatenate([zero, u[:-1]]), np.concatenate([u[1:], zero])
    return (((west * np.roll(u, 1, 2) + east * np.roll(u, -1, 2)) + (north * np.roll(u, 1, 1) + south * np.roll(u, -1, 1)))
            + (back * up + fwd * dn)) - dg * u


def residual(sides, periodic, state, weight, tau, u, data, lap, boundary=None):
    """L u - b in float64 on the unknown blocks (0 where the pixel is not UNKNOWN); u: a call's out"""
    links, dg = _planes(sides, periodic, state, weight, tau, np.float64)
    k = kinds(sides, periodic, state)
    blk = (slice(None),) + unknowns(sides, periodic, *k.shape[1:3])
    ub = np.where(k[blk] == UNKNOWN, _thwc(np.asarray(u, np.float64))[blk], 0.0)
    return block_operator(links, dg, ub) - folded_rhs(sides, periodic, state, weight, tau, data, lap, boundary)


def precond_mean(sides, periodic, state, weight, tau):
    """(w-bar, UNKNOWN pixels) as the library takes them for one volume: (sum of w over the UNKNOWN pixels + sum of the UNKNOWN - KNOWN
    links, spatial 1 and temporal tau) / (UNKNOWN pixels)"""
    st = _thwc(np.asarray(state, np.float32))
    k = kinds(sides, periodic, st)
    uk = 0.0
    for f, kf in zip(st, k):
        for live, axis in zip(region_np.live_links(sides, periodic, f), (1, 0)):
            uk += int((live & (kf + region_np._neighbour(kf, -1, axis, periodic, OUTSIDE) == KNOWN)).sum())
    uk += float(np.float32(tau)) * int((_time_live(k) & (k[:-1] + k[1:] == KNOWN)).sum())
    unk = k == UNKNOWN
    wsum = 0.0 if weight is None else float(_thwc(np.asarray(weight, np.float32))[unk].astype(np.float64).sum())
    n = int(unk.sum())
    return ((wsum + uk) / n if n else 1.0), n


def dct_table(T):
    """the orthonormal DCT-II along T frames, D[k][t], in float64"""
    k, t = np.mgrid[0:T, 0:T]
    return np.sqrt(np.where(k > 0, 2.0, 1.0) / T) * np.cos(np.pi * (2 * t + 1) * k / (2.0 * T))


def mode_shifts(T, wbar, tau):
    """w-bar + tau (2 - 2 cos(pi k / T)), computed in float64 and rounded to float32"""
    return np.float32(wbar + float(np.float32(tau)) * (2.0 - 2.0 * np.cos(np.pi * np.arange(T) / T)))


def _precond_exact(sides, periodic, shape, wbar, tau):
    """r -> M^-1 r in float64 on the unknown blocks, M = A - w-bar + tau A_t, through the three axes' eigenvectors"""
    T, ny, nx = shape
    ax, ay = direct_np.axis_kinds(sides, periodic)
    ex, qx = np.linalg.eigh(weighted_np.axis_matrix(ax, nx))
    ey, qy = np.linalg.eigh(weighted_np.axis_matrix(ay, ny))
    et, qt = np.linalg.eigh(weighted_np.axis_matrix(direct_np.NN, T))
    den = (float(np.float32(tau)) * et[:, None, None] + ey[None, :, None] + ex[None, None, :]) - wbar
    den = np.where(np.abs(den) < 1e-12, np.inf, den)[:, :, :, None]          # (w-bar = 0 without a Dirichlet line: the constant mode)

    def apply(r):
        z = np.einsum("st,yv,xu,syxc->tvuc", qt, qy, qx, r, optimize=True) / den
        return np.einsum("st,yv,xu,tvuc->syxc", qt, qy, qx, z, optimize=True)
    return apply


def solve_exact(sides, periodic, state, weight, tau, data, lap, boundary=None, dense=None):
    """float64 solution, data's shape, composed like out.  dense: None: LAPACK up to DENSE_LIMIT unknowns per channel, else conjugate
    gradients in float64 to a relative residual of 1e-13; True / False force one of the two"""
    shape = np.asarray(data).shape
    k = kinds(sides, periodic, state)
    T, H, W, C = k.shape
    blk = (slice(None),) + unknowns(sides, periodic, H, W)
    g = folded_rhs(sides, periodic, state, weight, tau, data, lap, boundary)
    links, dg = _planes(sides, periodic, state, weight, tau, np.float64)
    unk = k[blk] == UNKNOWN
    u = np.zeros(g.shape)
    wbar, _ = precond_mean(sides, periodic, state, weight, tau)
    M_inv = None
    for c in range(C):
        m = unk[:, :, :, c]
        n = int(m.sum())
        if not n:
            continue
        lc, dc = tuple(l[:, :, :, c:c + 1] for l in links), dg[:, :, :, c:c + 1]
        if dense if dense is not None else n <= DENSE_LIMIT:
            index = np.full(m.shape, -1)
            index[m] = np.arange(n)
            A = np.zeros((n, n))
            A[np.arange(n), np.arange(n)] = -dc[:, :, :, 0][m]
            for l, (shift, axis) in zip(lc, ((1, 2), (-1, 2), (1, 1), (-1, 1), (1, 0), (-1, 0))):
                j = np.roll(index, shift, axis)[m]
                v = l[:, :, :, 0][m]
                ok = v != 0
                np.add.at(A, (np.arange(n)[ok], j[ok]), v[ok])
            sol = np.zeros(m.shape)
            sol[m] = np.linalg.solve(A, g[:, :, :, c][m])
            u[:, :, :, c] = sol
            continue
        if M_inv is None:
            M_inv = _precond_exact(sides, periodic, m.shape, wbar, tau)
        b = g[:, :, :, c:c + 1]
        bn = float(np.sqrt((b * b).sum()))
        x = M_inv(b)
        r = b - block_operator(lc, dc, x)
        z = M_inv(r)
        p, rho = z.copy(), float((r * z).sum())
        for _ in range(5000):
            if float(np.sqrt((r * r).sum())) <= 1e-13 * bn:
                break
            q = block_operator(lc, dc, p)
            alpha = rho / float((p * q).sum())
            x, r = x + alpha * p, r - alpha * q
            z = M_inv(r)
            rho_new = float((r * z).sum())
            p, rho = z + (rho_new / rho) * p, rho_new
        else:
            raise RuntimeError("volume_np.solve_exact: the float64 conjugate gradients did not reach 1e-13")
        u[:, :, :, c] = np.where(m, x[:, :, :, 0], 0.0)
    return _compose(sides, periodic, state, data, boundary, u, np.float64).reshape(shape)


def _compose(sides, periodic, state, data, boundary, u_blk, dtype):
    st, d = _thwc(np.asarray(state, np.float32)), _thwc(np.asarray(data, dtype))
    bd = None if boundary is None else _thwc(np.asarray(boundary, dtype))
    return np.stack([region_np._compose(sides, periodic, st[t], d[t], None if bd is None else bd[t], u_blk[t], dtype) for t in range(st.shape[0])])


def pcg(sides, periodic, state, weight, tau, data, lap, boundary=None, tol=1e-5, max_iters=400, precond_lambda=None, dtype=np.float32, keep=None):
    """The library's iteration in numpy: one system per channel over all frames; dtype float64: the same iteration on float64 vectors and
    coefficient planes, the table along the frames unrounded and every mode's direct solve in float64 (the modes' shifts the same
    float32).  keep: a list that receives every iterate, composed like out.  Returns (out, iterations, the worst channel's final
    ||r|| / ||b||)."""
    shape = np.asarray(data).shape
    k = kinds(sides, periodic, state)
    T, H, W, C = k.shape
    links, dg = _planes(sides, periodic, state, weight, tau, dtype)
    wbar = precond_mean(sides, periodic, state, weight, tau)[0] if precond_lambda is None else float(np.float32(precond_lambda))
    D = dct_table(T).astype(dtype)
    shifts = mode_shifts(T, wbar, tau)
    b = folded_rhs(sides, periodic, state, weight, tau, data, lap, boundary, dtype)
    _, ny, nx, _ = b.shape
    tall = lambda a: a.reshape(T * ny, nx, C)
    frames = lambda a: a.reshape(T, ny, nx, C)

    def precond(r):
        X = np.einsum("kt,tyxc->kyxc", D, frames(r))
        Z = np.stack([weighted_np._precond(sides, periodic, shifts[m], X[m], (H, W, C), dtype) for m in range(T)])
        return tall(np.einsum("kt,kyxc->tyxc", D, Z).astype(dtype))

    scratch = np.zeros((T * ny, nx, C), dtype)
    us = []
    scratch, it, rel = pcg_np.pcg(tall(b), lambda p: tall(block_operator(links, dg, frames(p))), precond, None, tol, max_iters, scratch,
                                  (slice(None), slice(None)), dtype, us)
    if keep is not None:
        keep += [_compose(sides, periodic, state, data, boundary, frames(u), dtype).reshape(shape) for u in us]
    return _compose(sides, periodic, state, data, boundary, frames(scratch), dtype).reshape(shape), it, rel


def pcg_f32(sides, periodic, state, weight, tau, data, lap, boundary=None, tol=1e-5, max_iters=400, precond_lambda=None):
    """pcg() in the library's arithmetic: float32 vectors, table and direct solves"""
    return pcg(sides, periodic, state, weight, tau, data, lap, boundary, tol, max_iters, precond_lambda, np.float32)


def unpinned_components(sides, periodic, state, weight=None):
    """boolean T x H x W x C: the UNKNOWN pixels of connected components (through spatial and temporal links between UNKNOWN pixels)
    that have no KNOWN or Dirichlet neighbour in space, no KNOWN neighbour in time and no positive weight"""
    k = kinds(sides, periodic, state)
    unk = k == UNKNOWN
    big = k.size
    label = np.where(unk, np.arange(k.size).reshape(k.shape), big)

    def around(a, fill):          # a at the six neighbours
        f = np.full((1,) + a.shape[1:], fill, a.dtype)
        return [np.stack([region_np._neighbour(a[t], shift, axis, periodic, fill) for t in range(a.shape[0])]) for shift, axis in region_np._SHIFTS] + \
               [np.concatenate([f, a[:-1]]), np.concatenate([a[1:], f])]
    while True:
        new = label
        for q in around(label, big):
            new = np.minimum(new, q)
        new = np.where(unk, new, big)
        if np.array_equal(new, label):
            break
        label = new
    held = np.zeros(k.shape, bool)
    for i, q in enumerate(around(k, OUTSIDE)):
        held |= (q == KNOWN) | ((q == DIRICHLET) & (i < 4))
    if weight is not None:
        held |= np.where(unk, _thwc(np.asarray(weight, np.float32)), np.float32(0)) > 0
    pinned = np.unique(label[unk & held])
    return unk & ~np.isin(label, pinned)
