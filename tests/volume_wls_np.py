"""The test side's restatement of the WLS volume solve (sc_hip_volume_wls*), numpy only, built on volume_np and region_np.

A volume is T frames: every array is T x H x W x C, borders are (sides, periodic) as in weighted_np; tper says whether time is periodic.
sx, sy (T x H x W x C, or None: every spatial link 1) weigh the links within a frame as region_np's, stored at the link's low end.  smt
(None: 1) and gt hold the temporal links' weights and guidance: element [t] belongs to the link from frame t to frame t + 1, T - 1
frames; with periodic time T frames, frame T - 1 of them the link from the last frame to frame 0.  The weight of a temporal link is lt =
tau * smt, one rounded float32 product.  A temporal link is live when neither end is OUTSIDE or on a Dirichlet line and at least one end
is UNKNOWN, whether it wraps or not.

A problem travels as the tuple args = (sides, periodic, tper, state, weight, sx, sy, smt, tau, data, lap).

kinds() classifies every pixel; live_links() names the elements of sx / gx, sy / gy and smt / gt a call may read (three arrays, the
third at the temporal arrays' length).  divergence() is steps 1 and 2 of the header's right-hand side, folded_rhs(dtype=float32) the
whole of it to the letter: the frame's guidance sum of rounded products s * g, + (e - f) of the rounded products lt * gt at the live
forward and backward temporal links, - w * d, the Dirichlet terms and the KNOWN spatial neighbours with their link's s, the KNOWN
temporal neighbours previous, then next with their lt -- each a rounded product subtracted in turn; 0 at every pixel that is not
UNKNOWN.  solve_exact() is the float64 answer: dense LAPACK up to DENSE_LIMIT unknowns per channel, above that conjugate gradients in
float64 with the exact constant-coefficient preconditioner, run to a relative residual of 1e-13.  precond_means() gives s-bar, tau-bar
and w-bar as the library takes them; time_table() the orthonormal table along the frames (DCT-II, periodic: Hartley), mode_shifts() the
modes' shifts.  pcg_f32() is the library's iteration -- the yardstick of tests/volume_wls_bounds.py.  unpinned_components() finds the
UNKNOWN components, through all three link kinds and the wrap of time, that nothing holds (the library does not)."""
from __future__ import annotations

import numpy as np

import direct_np
import pcg_np
import region_np
import volume_np
import weighted_np

UNKNOWN, KNOWN, OUTSIDE, DIRICHLET = region_np.UNKNOWN, region_np.KNOWN, region_np.OUTSIDE, region_np.DIRICHLET
unknowns = weighted_np.unknowns
has_dirichlet = weighted_np.has_dirichlet
DENSE_LIMIT = 3000
_thwc = volume_np._thwc
kinds = volume_np.kinds


def _f32(a):
    return None if a is None else _thwc(np.asarray(a, np.float32))


def _next(a, tper):
    """a at the next frame, aligned with the temporal arrays: T frames with periodic time (frame 0 behind the last), else T - 1"""
    return np.roll(a, -1, 0) if tper else a[1:]


def _here(a, tper):
    return a if tper else a[:-1]


def _time_live(k, tper):
    """boolean, the temporal arrays' shape: the link from frame t to the next is live"""
    a, b = _here(k, tper), _next(k, tper)
    return (a <= KNOWN) & (b <= KNOWN) & ((a == UNKNOWN) | (b == UNKNOWN))


def live_links(sides, periodic, tper, state):
    """(live_x, live_y, live_t): the elements of sx / gx, sy / gy (T x H x W x C) and smt / gt (T - 1 frames, periodic time: T) that a call
    reads"""
    st = _f32(state)
    per = [region_np.live_links(sides, periodic, f) for f in st]
    return np.stack([p[0] for p in per]), np.stack([p[1] for p in per]), _time_live(kinds(sides, periodic, st), tper)


def _lt(k, tper, smt, tau):
    """float32, the temporal arrays' shape: lt = tau * smt (one rounded product; smt None: tau) where the link is live, else 0"""
    live = _time_live(k, tper)
    tau = np.float32(tau)
    v = np.full(live.shape, tau, np.float32) if smt is None else tau * np.where(live, _f32(smt), np.float32(1))
    assert v.dtype == np.float32
    return np.where(live, v, np.float32(0))


def _to_frames(v, tper, T):
    """(back, forward), T frames each: a temporal array's value at every frame's link to the previous / next frame (0: no such link)"""
    if tper:
        return np.roll(v, 1, 0), v
    zero = np.zeros((1,) + v.shape[1:], v.dtype)
    return np.concatenate([zero, v]), np.concatenate([v, zero])


def _time_links(k, tper, smt, tau, dtype):
    return tuple(a.astype(dtype) for a in _to_frames(_lt(k, tper, smt, tau), tper, k.shape[0]))


def _frame(a, t):
    return None if a is None else a[t]


def divergence(sides, periodic, tper, state, sx, sy, smt, tau, gx, gy, gt=None):
    """steps 1 and 2 of the right-hand side in float32, T x H x W x C (valid at the UNKNOWN pixels)"""
    st, sx, sy = _f32(state), _f32(sx), _f32(sy)
    gx, gy = _f32(gx), _f32(gy)
    T = st.shape[0]
    div = np.stack([region_np.divergence(sides, periodic, st[t], _frame(sx, t), _frame(sy, t), gx[t], gy[t]) for t in range(T)])
    k = kinds(sides, periodic, st)
    lt = _lt(k, tper, smt, tau)
    if gt is None:
        prod = np.zeros(lt.shape, np.float32)
    else:
        prod = np.where(lt != 0, lt * np.where(lt != 0, _f32(gt), np.float32(0)), np.float32(0))
    f, e = _to_frames(prod, tper, T)
    out = div + (e - f)
    assert out.dtype == np.float32
    return out


def folded_rhs(sides, periodic, tper, state, weight, sx, sy, smt, tau, data, lap, boundary=None, dtype=np.float64):
    """b on the unknown blocks [T][ny][nx][C]; lap: steps 1 and 2 (divergence(), or the caller's lap)"""
    st, d, lap, w, sx, sy, bd = (_f32(a) for a in (state, data, lap, weight, sx, sy, boundary))
    k = kinds(sides, periodic, st)
    T, H, W, _ = k.shape
    blk = (slice(None),) + unknowns(sides, periodic, H, W)
    g = np.stack([region_np.folded_rhs(sides, periodic, st[t], _frame(w, t), _frame(sx, t), _frame(sy, t), d[t], lap[t], _frame(bd, t), dtype)
                  for t in range(T)])
    back, fwd = _time_links(k, tper, smt, tau, dtype)
    held = np.where(k == KNOWN, d, np.float32(0)).astype(dtype)
    unk = k == UNKNOWN
    kb, kf = (np.roll(k, 1, 0), np.roll(k, -1, 0))          # (beyond a free end the link is 0: whatever the roll brings counts nothing)
    prev = np.where(unk & (kb == KNOWN) & (back != 0), back * np.roll(held, 1, 0), dtype(0))
    nxt = np.where(unk & (kf == KNOWN) & (fwd != 0), fwd * np.roll(held, -1, 0), dtype(0))
    g = (g - prev[blk]) - nxt[blk]
    assert g.dtype == dtype
    return g


def _planes(sides, periodic, tper, state, weight, sx, sy, smt, tau, dtype):
    """the operator's coefficients on the unknown blocks [T][ny][nx][C]: (west, east, north, south, back, forward) kept only where both
    ends are UNKNOWN, and the diagonal in the kernel's order; all 0 at a pixel that is not UNKNOWN"""
    st, sx, sy = _f32(state), _f32(sx), _f32(sy)
    k = kinds(sides, periodic, st)
    T, H, W, _ = k.shape
    blk = (slice(None),) + unknowns(sides, periodic, H, W)
    unk = k == UNKNOWN
    full = [np.stack(f) for f in zip(*(region_np._links(sides, periodic, st[t], _frame(sx, t), _frame(sy, t), dtype) for t in range(T)))]
    back, fwd = _time_links(k, tper, smt, tau, dtype)
    w = dtype(0) if weight is None else _f32(weight).astype(dtype)
    dg = np.where(unk, (((full[0] + full[1]) + (full[2] + full[3])) + (back + fwd)) + np.where(unk, w, dtype(0)), dtype(0))
    links = [np.stack([np.where(unk[t] & (region_np._neighbour(k[t], shift, axis, periodic, OUTSIDE) == UNKNOWN), f[t], dtype(0)) for t in range(T)])
             for f, (shift, axis) in zip(full, region_np._SHIFTS)]
    links.append(np.where(unk & np.roll(unk, 1, 0), back, dtype(0)))
    links.append(np.where(unk & np.roll(unk, -1, 0), fwd, dtype(0)))
    return tuple(l[blk] for l in links), dg[blk]


def block_operator(links, dg, u):
    """L u on the unknown blocks [T][ny][nx][C] in u's dtype, in the kernel's order (a temporal coefficient is 0 where time has no link,
    so the frames may roll round)"""
    west, east, north, south, back, fwd = links
    return (((west * np.roll(u, 1, 2) + east * np.roll(u, -1, 2)) + (north * np.roll(u, 1, 1) + south * np.roll(u, -1, 1)))
            + (back * np.roll(u, 1, 0) + fwd * np.roll(u, -1, 0))) - dg * u


def residual(args, u, boundary=None):
    """L u - b in float64 on the unknown blocks (0 where the pixel is not UNKNOWN); u: a call's out"""
    sides, periodic, tper, state, weight, sx, sy, smt, tau, data, lap = args
    links, dg = _planes(sides, periodic, tper, state, weight, sx, sy, smt, tau, np.float64)
    k = kinds(sides, periodic, state)
    blk = (slice(None),) + unknowns(sides, periodic, *k.shape[1:3])
    ub = np.where(k[blk] == UNKNOWN, _thwc(np.asarray(u, np.float64))[blk], 0.0)
    return block_operator(links, dg, ub) - folded_rhs(*args, boundary)


def precond_means(sides, periodic, tper, state, weight, sx, sy, smt, tau):
    """(s-bar, tau-bar, w-bar) as the library takes them for one volume, and the counts a chunk's means weigh by: (spatial links live in
    the region, live temporal links, UNKNOWN pixels).  s-bar: the mean of the spatial links live in the region (1 without sx or without
    one); tau-bar: the mean of the live lt (tau without smt or without one); w-bar: (sum of w over the UNKNOWN pixels + sum of the
    UNKNOWN - KNOWN links' weights) / (UNKNOWN pixels)"""
    st, sxf, syf = _f32(state), _f32(sx), _f32(sy)
    k = kinds(sides, periodic, st)
    lx, ly, _ = live_links(sides, periodic, tper, st)
    one = np.ones(k.shape, np.float32)
    sxf, syf = (one if a is None else a for a in (sxf, syf))
    v = np.concatenate([sxf[lx], syf[ly]]).astype(np.float64)
    uk = 0.0
    for live, s, axis in ((lx, sxf, 2), (ly, syf, 1)):
        q = np.stack([region_np._neighbour(k[t], -1, axis - 1, periodic, OUTSIDE) for t in range(k.shape[0])])
        uk += float(s[live & (k + q == KNOWN)].astype(np.float64).sum())
    lt = _lt(k, tper, smt, tau)
    tl = _time_live(k, tper)
    uk += float(lt[tl & (_here(k, tper) + _next(k, tper) == KNOWN)].astype(np.float64).sum())
    unk = k == UNKNOWN
    wsum = 0.0 if weight is None else float(_f32(weight)[unk].astype(np.float64).sum())
    n = int(unk.sum())
    sbar = float(v.mean()) if v.size and sx is not None else 1.0
    tbar = float(lt[tl].astype(np.float64).mean()) if tl.any() and smt is not None else float(np.float32(tau))
    return sbar, tbar, ((wsum + uk) / n if n else 1.0), (v.size, int(tl.sum()), n)


def time_table(T, periodic):
    """the orthonormal table along T frames, D[k][t], in float64: the DCT-II, or -- periodic time -- the Hartley table
    (cos + sin)(2 pi k t / T) / sqrt(T), which is symmetric and its own inverse"""
    k, t = np.mgrid[0:T, 0:T]
    if not periodic:
        return volume_np.dct_table(T)
    a = 2.0 * np.pi * ((k * t) % T) / T
    return (np.cos(a) + np.sin(a)) / np.sqrt(T)


def time_modes(T, periodic):
    """mu_k: 2 - 2 cos(pi k / T), periodic time 2 - 2 cos(2 pi k / T)"""
    return 2.0 - 2.0 * np.cos((2.0 if periodic else 1.0) * np.pi * np.arange(T) / T)


def mode_shifts(T, wbar, tbar, sbar, periodic):
    """(w-bar + tau-bar mu_k) / s-bar, computed in float64 and rounded to float32"""
    return np.float32((wbar + tbar * time_modes(T, periodic)) / sbar)


def _precond_exact(sides, periodic, tper, shape, sbar, tbar, wbar):
    """r -> M^-1 r in float64 on the unknown blocks, M = s-bar A - w-bar + tau-bar A_t, through the three axes' eigenvectors"""
    T, ny, nx = shape
    ax, ay = direct_np.axis_kinds(sides, periodic)
    ex, qx = np.linalg.eigh(weighted_np.axis_matrix(ax, nx))
    ey, qy = np.linalg.eigh(weighted_np.axis_matrix(ay, ny))
    et, qt = np.linalg.eigh(weighted_np.axis_matrix(direct_np.PP if tper else direct_np.NN, T))
    den = (tbar * et[:, None, None] + sbar * (ey[None, :, None] + ex[None, None, :])) - wbar
    den = np.where(np.abs(den) < 1e-12, np.inf, den)[:, :, :, None]

    def apply(r):
        z = np.einsum("st,yv,xu,syxc->tvuc", qt, qy, qx, r, optimize=True) / den
        return np.einsum("st,yv,xu,tvuc->syxc", qt, qy, qx, z, optimize=True)
    return apply


def solve_exact(args, boundary=None, dense=None):
    """float64 solution, data's shape, composed like out.  dense: None: LAPACK up to DENSE_LIMIT unknowns per channel, else conjugate
    gradients in float64 to a relative residual of 1e-13; True / False force one of the two"""
    sides, periodic, tper, state, weight, sx, sy, smt, tau, data, lap = args
    shape = np.asarray(data).shape
    k = kinds(sides, periodic, state)
    T, H, W, C = k.shape
    blk = (slice(None),) + unknowns(sides, periodic, H, W)
    g = folded_rhs(*args, boundary)
    links, dg = _planes(sides, periodic, tper, state, weight, sx, sy, smt, tau, np.float64)
    unk = k[blk] == UNKNOWN
    u = np.zeros(g.shape)
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
            sbar, tbar, wbar, _ = precond_means(sides, periodic, tper, state, weight, sx, sy, smt, tau)
            M_inv = _precond_exact(sides, periodic, tper, m.shape, sbar, tbar, wbar)
        b = g[:, :, :, c:c + 1]
        bn = float(np.sqrt((b * b).sum()))
        x = M_inv(b)
        r = b - block_operator(lc, dc, x)
        z = M_inv(r)
        p, rho = z.copy(), float((r * z).sum())
        for _ in range(20000):
            if float(np.sqrt((r * r).sum())) <= 1e-13 * bn:
                break
            q = block_operator(lc, dc, p)
            alpha = rho / float((p * q).sum())
            x, r = x + alpha * p, r - alpha * q
            z = M_inv(r)
            rho_new = float((r * z).sum())
            p, rho = z + (rho_new / rho) * p, rho_new
        else:
            raise RuntimeError("volume_wls_np.solve_exact: the float64 conjugate gradients did not reach 1e-13")
        u[:, :, :, c] = np.where(m, x[:, :, :, 0], 0.0)
    return volume_np._compose(sides, periodic, state, data, boundary, u, np.float64).reshape(shape)


def pcg(args, boundary=None, tol=1e-5, max_iters=400, means=None, dtype=np.float32, keep=None):
    """The library's iteration in numpy: one system per channel over all frames, preconditioned by the table product along the frames
    (time_table in float32), the float32 direct solve of every mode with mode_shifts' shift, and the transposed product; the start is
    M^-1 b times 1 / s-bar.  means: (s-bar, tau-bar, w-bar) where they are not the input's own (a member of a batch: the chunk's).
    dtype float64: the same iteration on float64 vectors and coefficient planes, the table unrounded and every mode's direct solve in
    float64 (the modes' shifts and the start's factor the same float32).  keep: a list that receives every iterate, composed like out.
    Returns (out, iterations, the worst channel's final ||r|| / ||b||)."""
    sides, periodic, tper, state, weight, sx, sy, smt, tau, data, lap = args
    shape = np.asarray(data).shape
    k = kinds(sides, periodic, state)
    T, H, W, C = k.shape
    links, dg = _planes(sides, periodic, tper, state, weight, sx, sy, smt, tau, dtype)
    sbar, tbar, wbar = precond_means(sides, periodic, tper, state, weight, sx, sy, smt, tau)[:3] if means is None else means
    D = time_table(T, tper).astype(dtype)
    shifts = mode_shifts(T, wbar, tbar, sbar, tper)
    scale = np.float32(1.0 / sbar)
    b = folded_rhs(*args, boundary, dtype)
    _, ny, nx, _ = b.shape
    tall = lambda a: a.reshape(T * ny, nx, C)
    frames = lambda a: a.reshape(T, ny, nx, C)

    def precond(r):
        X = np.einsum("kt,tyxc->kyxc", D, frames(r))
        Z = np.stack([weighted_np._precond(sides, periodic, shifts[m], X[m], (H, W, C), dtype) for m in range(T)])
        return tall(np.einsum("kt,kyxc->tyxc", D, Z).astype(dtype))

    scratch = np.zeros((T * ny, nx, C), dtype)
    us = []
    scratch, it, rel = pcg_np.pcg(tall(b), lambda p: tall(block_operator(links, dg, frames(p))), precond, None if scale == 1 else dtype(scale), tol,
                                  max_iters, scratch, (slice(None), slice(None)), dtype, us)
    if keep is not None:
        keep += [volume_np._compose(sides, periodic, state, data, boundary, frames(u), dtype).reshape(shape) for u in us]
    return volume_np._compose(sides, periodic, state, data, boundary, frames(scratch), dtype).reshape(shape), it, rel


def pcg_f32(args, boundary=None, tol=1e-5, max_iters=400, means=None):
    """pcg() in the library's arithmetic: float32 vectors, table and direct solves -- the yardstick of tests/volume_wls_bounds.py"""
    return pcg(args, boundary, tol, max_iters, means, np.float32)


def unpinned_components(sides, periodic, tper, state, weight=None):
    """boolean T x H x W x C: the UNKNOWN pixels of connected components (through spatial and temporal links between UNKNOWN pixels, the
    wrap of periodic time included) that have no KNOWN or Dirichlet neighbour in space, no KNOWN neighbour in time and no positive weight"""
    k = kinds(sides, periodic, state)
    unk = k == UNKNOWN
    big = k.size
    label = np.where(unk, np.arange(k.size).reshape(k.shape), big)

    def around(a, fill):          # a at the six neighbours
        f = np.full((1,) + a.shape[1:], fill, a.dtype)
        time = [np.roll(a, 1, 0), np.roll(a, -1, 0)] if tper else [np.concatenate([f, a[:-1]]), np.concatenate([a[1:], f])]
        return [np.stack([region_np._neighbour(a[t], shift, axis, periodic, fill) for t in range(a.shape[0])]) for shift, axis in region_np._SHIFTS] + time
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
