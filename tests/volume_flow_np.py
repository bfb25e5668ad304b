"""The test side's restatement of the flow volume solve (sc_hip_volume_flow*), numpy only, built on volume_wls_np.

A problem travels as volume_wls_np's tuple args = (sides, periodic, tper, state, weight, sx, sy, smt, tau, data, lap) and, beside it, the
links (fwd, bwd) that match() makes of a flow.  flow is (T - 1) x H x W x 2 -- periodic time: T x H x W x 2 -- of (dx, dy): pixel (x, y)
of frame t is pixel (x + dx, y + dy) of frame t + 1 (of frame 0 behind the last).  fwd and bwd are int64 arrays T x ny x nx over the work
rectangle (the border kind's unknowns) holding work-plane indices (t ny + y) nx + x: fwd the element a pixel's link leads to, bwd the
element whose link arrives, -1: none.

match() is the header's rule: a pixel is a candidate when both components are finite, at most 1e6 in magnitude and its target lies in
the work rectangle (a periodic axis wraps); among the candidates of one target the smallest index holds the link (np.minimum.at).  A
matched link is live when neither end is OUTSIDE and at least one is UNKNOWN; its weight lt = tau * smt and its guidance gt are stored at
its source.  live_links(), divergence(), folded_rhs(), _planes(), block_operator(), residual(), solve_exact(), precond_means() and
pcg_f32() are volume_wls_np's with "the next frame's pixel" read through fwd and "the previous frame's" through bwd; with a flow of
zeros every one returns volume_wls_np's arrays exactly.  The preconditioner is volume_wls_np's, unchanged: straight time links."""
from __future__ import annotations

import numpy as np

import pcg_np
import region_np
import volume_np
import volume_wls_np as vw
import weighted_np

UNKNOWN, KNOWN, OUTSIDE, DIRICHLET = vw.UNKNOWN, vw.KNOWN, vw.OUTSIDE, vw.DIRICHLET
unknowns = vw.unknowns
has_dirichlet = vw.has_dirichlet
kinds = vw.kinds
_thwc, _f32, _frame = vw._thwc, vw._f32, vw._frame
FLOW_LIMIT = 1e6


def match(sides, periodic, tper, shape, flow):
    """(fwd, bwd) of a volume of shape = (T, H, W) under these borders"""
    T, H, W = shape
    rows, cols = unknowns(sides, periodic, H, W)
    ny, nx = rows.stop - rows.start, cols.stop - cols.start
    Tf = T if tper else T - 1
    flow = np.asarray(flow, np.float64)
    assert flow.shape == (Tf, H, W, 2), (flow.shape, (Tf, H, W, 2))
    f = flow[:, rows, cols]
    ok = np.isfinite(f).all(-1)
    ok &= (np.abs(np.where(np.isfinite(f), f, 0.0)) <= FLOW_LIMIT).all(-1)
    d = np.rint(np.where(ok[..., None], f, 0.0)).astype(np.int64)
    t, y, x = np.mgrid[0:Tf, 0:ny, 0:nx]
    tx, ty = x + d[..., 0], y + d[..., 1]
    if "x" in periodic:
        tx %= nx
    if "y" in periodic:
        ty %= ny
    ok &= (tx >= 0) & (tx < nx) & (ty >= 0) & (ty < ny)
    own = (t * ny + y) * nx + x
    target = (((t + 1) % T) * ny + ty) * nx + tx
    big = np.iinfo(np.int64).max
    bwd = np.full(T * ny * nx, big, np.int64)
    np.minimum.at(bwd, target[ok], own[ok])
    fwd = np.full(T * ny * nx, -1, np.int64)
    won = ok & (bwd[np.where(ok, target, 0)] == own)
    fwd[own[won]] = target[won]
    bwd[bwd == big] = -1
    return fwd.reshape(T, ny, nx), bwd.reshape(T, ny, nx)


def _blk(sides, periodic, a):
    """a T x H x W (x ...) array on the work rectangle"""
    return a[(slice(None),) + unknowns(sides, periodic, *a.shape[1:3])]


def _gather(a, idx, fill):
    """a (T x ny x nx x C) at the elements idx names, `fill` where idx is -1"""
    flat = a.reshape((-1,) + a.shape[3:])
    got = flat[np.where(idx >= 0, idx, 0).reshape(-1)].reshape(a.shape)
    return np.where((idx >= 0)[..., None], got, fill)


def _pad(a, T):
    """a temporal array on T frames (a zero frame behind T - 1 of them)"""
    return a if a.shape[0] == T else np.concatenate([a, np.zeros((1,) + a.shape[1:], a.dtype)])


def _held_live(kb, fwd):
    """boolean T x ny x nx x C: the link this pixel holds is live"""
    q = _gather(kb, fwd, OUTSIDE)
    return (fwd >= 0)[..., None] & (kb <= KNOWN) & (q <= KNOWN) & ((kb == UNKNOWN) | (q == UNKNOWN))


def live_links(sides, periodic, tper, state, links):
    """(live_x, live_y, live_t): the elements of sx / gx, sy / gy (T x H x W x C) and smt / gt (their own length) that a call reads"""
    fwd, _ = links
    st = _f32(state)
    lx, ly, _ = vw.live_links(sides, periodic, tper, st)
    k = kinds(sides, periodic, st)
    T, H, W, C = k.shape
    lt = np.zeros(k.shape, bool)
    lt[(slice(None),) + unknowns(sides, periodic, H, W)] = _held_live(_blk(sides, periodic, k), fwd)
    return lx, ly, lt[:T if tper else T - 1]


def _lt(sides, periodic, tper, k, smt, tau, fwd):
    """float32 T x ny x nx x C: lt = tau * smt of the link each pixel holds (one rounded product; smt None: tau) where it is live, else 0"""
    kb = _blk(sides, periodic, k)
    live = _held_live(kb, fwd)
    tau = np.float32(tau)
    if smt is None:
        v = np.full(live.shape, tau, np.float32)
    else:
        v = tau * np.where(live, _pad(_blk(sides, periodic, _f32(smt)), k.shape[0]), np.float32(1))
    assert v.dtype == np.float32
    return np.where(live, v, np.float32(0))


def _time_links(sides, periodic, tper, k, smt, tau, links, dtype):
    """(back, forward) on the work rectangle: the weight of the link that arrives at / is held by every pixel (0: none or dead)"""
    fwd, bwd = links
    lt = _lt(sides, periodic, tper, k, smt, tau, fwd)
    return _gather(lt, bwd, np.float32(0)).astype(dtype), lt.astype(dtype)


def divergence(sides, periodic, tper, state, sx, sy, smt, tau, gx, gy, gt, links):
    """steps 1 and 2 of the right-hand side in float32, T x H x W x C (valid at the UNKNOWN pixels)"""
    fwd, bwd = links
    st, sxf, syf = _f32(state), _f32(sx), _f32(sy)
    gx, gy = _f32(gx), _f32(gy)
    T = st.shape[0]
    div = np.stack([region_np.divergence(sides, periodic, st[t], _frame(sxf, t), _frame(syf, t), gx[t], gy[t]) for t in range(T)])
    k = kinds(sides, periodic, st)
    lt = _lt(sides, periodic, tper, k, smt, tau, fwd)
    if gt is None:
        e = np.zeros(lt.shape, np.float32)
    else:
        g = _pad(_blk(sides, periodic, _f32(gt)), T)
        e = np.where(lt != 0, lt * np.where(lt != 0, g, np.float32(0)), np.float32(0))
    f = _gather(e, bwd, np.float32(0))
    tm = np.zeros(div.shape, np.float32)
    tm[(slice(None),) + unknowns(sides, periodic, *div.shape[1:3])] = e - f
    out = div + tm
    assert out.dtype == np.float32
    return out


def folded_rhs(args, links, boundary=None, dtype=np.float64):
    """b on the unknown blocks [T][ny][nx][C]; lap: steps 1 and 2 (divergence(), or the caller's lap)"""
    sides, periodic, tper, state, weight, sx, sy, smt, tau, data, lap = args
    fwd, bwd = links
    st, d, lap, w, sx, sy, bd = (_f32(a) for a in (state, data, lap, weight, sx, sy, boundary))
    k = kinds(sides, periodic, st)
    T = k.shape[0]
    g = np.stack([region_np.folded_rhs(sides, periodic, st[t], _frame(w, t), _frame(sx, t), _frame(sy, t), d[t], lap[t], _frame(bd, t), dtype)
                  for t in range(T)])
    back, hold = _time_links(sides, periodic, tper, k, smt, tau, links, dtype)
    kb = _blk(sides, periodic, k)
    held = np.where(kb == KNOWN, _blk(sides, periodic, d), np.float32(0)).astype(dtype)
    unk = kb == UNKNOWN
    prev = np.where(unk & (_gather(kb, bwd, OUTSIDE) == KNOWN) & (back != 0), back * _gather(held, bwd, dtype(0)), dtype(0))
    nxt = np.where(unk & (_gather(kb, fwd, OUTSIDE) == KNOWN) & (hold != 0), hold * _gather(held, fwd, dtype(0)), dtype(0))
    g = (g - prev) - nxt
    assert g.dtype == dtype
    return g


def _planes(args, links, dtype):
    """the operator's coefficients on the unknown blocks: (west, east, north, south, back, forward) kept only where both ends are
    UNKNOWN, and the diagonal in the kernel's order; all 0 at a pixel that is not UNKNOWN"""
    sides, periodic, tper, state, weight, sx, sy, smt, tau = args[:9]
    fwd, bwd = links
    st, sx, sy = _f32(state), _f32(sx), _f32(sy)
    k = kinds(sides, periodic, st)
    T, H, W, _ = k.shape
    blk = (slice(None),) + unknowns(sides, periodic, H, W)
    unk = k == UNKNOWN
    full = [np.stack(f) for f in zip(*(region_np._links(sides, periodic, st[t], _frame(sx, t), _frame(sy, t), dtype) for t in range(T)))]
    back, hold = _time_links(sides, periodic, tper, k, smt, tau, links, dtype)
    w = dtype(0) if weight is None else _f32(weight).astype(dtype)[blk]
    ub = unk[blk]
    dg = np.where(ub, (((full[0][blk] + full[1][blk]) + (full[2][blk] + full[3][blk])) + (back + hold)) + np.where(ub, w, dtype(0)), dtype(0))
    out = [np.stack([np.where(unk[t] & (region_np._neighbour(k[t], shift, axis, periodic, OUTSIDE) == UNKNOWN), f[t], dtype(0)) for t in range(T)])[blk]
           for f, (shift, axis) in zip(full, region_np._SHIFTS)]
    out.append(np.where(ub & _gather(ub, bwd, False), back, dtype(0)))
    out.append(np.where(ub & _gather(ub, fwd, False), hold, dtype(0)))
    return tuple(out), dg


def block_operator(coef, dg, u, links):
    """L u on the unknown blocks in u's dtype, in the kernel's order; the temporal neighbours gathered through bwd and fwd"""
    west, east, north, south, back, hold = coef
    fwd, bwd = links
    zero = u.dtype.type(0)
    return (((west * np.roll(u, 1, 2) + east * np.roll(u, -1, 2)) + (north * np.roll(u, 1, 1) + south * np.roll(u, -1, 1)))
            + (back * _gather(u, bwd, zero) + hold * _gather(u, fwd, zero))) - dg * u


def residual(args, links, u, boundary=None):
    """L u - b in float64 on the unknown blocks (0 where the pixel is not UNKNOWN); u: a call's out"""
    sides, periodic, _, state = args[:4]
    coef, dg = _planes(args, links, np.float64)
    kb = _blk(sides, periodic, kinds(sides, periodic, state))
    ub = np.where(kb == UNKNOWN, _blk(sides, periodic, _thwc(np.asarray(u, np.float64))), 0.0)
    return block_operator(coef, dg, ub, links) - folded_rhs(args, links, boundary)


def precond_means(args, links):
    """volume_wls_np.precond_means with the temporal links along the flow: (s-bar, tau-bar, w-bar, (spatial links live in the region,
    live temporal links, UNKNOWN pixels))"""
    sides, periodic, tper, state, weight, sx, sy, smt, tau = args[:9]
    fwd, _ = links
    st, sxf, syf = _f32(state), _f32(sx), _f32(sy)
    k = kinds(sides, periodic, st)
    lx, ly, _ = vw.live_links(sides, periodic, tper, st)
    one = np.ones(k.shape, np.float32)
    sxf, syf = (one if a is None else a for a in (sxf, syf))
    v = np.concatenate([sxf[lx], syf[ly]]).astype(np.float64)
    uk = 0.0
    for live, s, axis in ((lx, sxf, 2), (ly, syf, 1)):
        q = np.stack([region_np._neighbour(k[t], -1, axis - 1, periodic, OUTSIDE) for t in range(k.shape[0])])
        uk += float(s[live & (k + q == KNOWN)].astype(np.float64).sum())
    kb = _blk(sides, periodic, k)
    lt = _lt(sides, periodic, tper, k, smt, tau, fwd)
    tl = _held_live(kb, fwd)
    uk += float(lt[tl & (kb + _gather(kb, fwd, OUTSIDE) == KNOWN)].astype(np.float64).sum())
    unk = k == UNKNOWN
    wsum = 0.0 if weight is None else float(_f32(weight)[unk].astype(np.float64).sum())
    n = int(unk.sum())
    sbar = float(v.mean()) if v.size and sx is not None else 1.0
    tbar = float(lt[tl].astype(np.float64).mean()) if tl.any() and smt is not None else float(np.float32(tau))
    return sbar, tbar, ((wsum + uk) / n if n else 1.0), (v.size, int(tl.sum()), n)


def assemble(args, links, c=0):
    """(A, index): the dense matrix of channel c over its UNKNOWN pixels (A u = b, A = L), and each block element's row (-1: none)"""
    sides, periodic, _, state = args[:4]
    fwd, bwd = links
    coef, dg = _planes(args, links, np.float64)
    kb = _blk(sides, periodic, kinds(sides, periodic, state))
    m = kb[..., c] == UNKNOWN
    n = int(m.sum())
    index = np.full(m.shape, -1)
    index[m] = np.arange(n)
    A = np.zeros((n, n))
    A[np.arange(n), np.arange(n)] = -dg[..., c][m]
    nb = [np.roll(index, s, a) for s, a in ((1, 2), (-1, 2), (1, 1), (-1, 1))]
    nb += [_gather(index[..., None], bwd, -1)[..., 0], _gather(index[..., None], fwd, -1)[..., 0]]
    for l, j in zip(coef, nb):
        v = l[..., c][m]
        ok = v != 0
        np.add.at(A, (np.arange(n)[ok], j[m][ok]), v[ok])
    return A, index


def solve_exact(args, links, boundary=None, dense=None):
    """float64 solution, data's shape, composed like out: LAPACK up to volume_wls_np.DENSE_LIMIT unknowns per channel, else conjugate
    gradients in float64 under the straight-link preconditioner to a relative residual of 1e-13"""
    sides, periodic, tper, state, weight, sx, sy, smt, tau, data, lap = args
    shape = np.asarray(data).shape
    kb = _blk(sides, periodic, kinds(sides, periodic, state))
    T, ny, nx, C = kb.shape
    g = folded_rhs(args, links, boundary)
    coef, dg = _planes(args, links, np.float64)
    u = np.zeros(g.shape)
    M_inv = None
    for c in range(C):
        m = kb[..., c] == UNKNOWN
        n = int(m.sum())
        if not n:
            continue
        if dense if dense is not None else n <= vw.DENSE_LIMIT:
            A, _ = assemble(args, links, c)
            sol = np.zeros(m.shape)
            sol[m] = np.linalg.solve(A, g[..., c][m])
            u[..., c] = sol
            continue
        if M_inv is None:
            sbar, tbar, wbar, _ = precond_means(args, links)
            M_inv = vw._precond_exact(sides, periodic, tper, m.shape, sbar, tbar, wbar)
        lc, dc = tuple(l[..., c:c + 1] for l in coef), dg[..., c:c + 1]
        b = g[..., c:c + 1]
        bn = float(np.sqrt((b * b).sum()))
        x = M_inv(b)
        r = b - block_operator(lc, dc, x, links)
        z = M_inv(r)
        p, rho = z.copy(), float((r * z).sum())
        for _ in range(40000):
            if float(np.sqrt((r * r).sum())) <= 1e-13 * bn:
                break
            q = block_operator(lc, dc, p, links)
            alpha = rho / float((p * q).sum())
            x, r = x + alpha * p, r - alpha * q
            z = M_inv(r)
            rho_new = float((r * z).sum())
            p, rho = z + (rho_new / rho) * p, rho_new
        else:
            raise RuntimeError("volume_flow_np.solve_exact: the float64 conjugate gradients did not reach 1e-13")
        u[..., c] = np.where(m, x[..., 0], 0.0)
    return volume_np._compose(sides, periodic, state, data, boundary, u, np.float64).reshape(shape)


def pcg(args, links, boundary=None, tol=1e-5, max_iters=400, means=None, dtype=np.float32):
    """volume_wls_np.pcg with the flow operator: the library's iteration, the preconditioner unchanged (straight time links, the means
    of precond_means or `means`).  Returns (out, iterations, the worst channel's final ||r|| / ||b||)."""
    sides, periodic, tper, state, weight, sx, sy, smt, tau, data, lap = args
    shape = np.asarray(data).shape
    k = kinds(sides, periodic, state)
    T, H, W, C = k.shape
    coef, dg = _planes(args, links, dtype)
    sbar, tbar, wbar = precond_means(args, links)[:3] if means is None else means
    D = vw.time_table(T, tper).astype(dtype)
    shifts = vw.mode_shifts(T, wbar, tbar, sbar, tper)
    scale = np.float32(1.0 / sbar)
    b = folded_rhs(args, links, boundary, dtype)
    _, ny, nx, _ = b.shape
    tall = lambda a: a.reshape(T * ny, nx, C)
    frames = lambda a: a.reshape(T, ny, nx, C)

    def precond(r):
        X = np.einsum("kt,tyxc->kyxc", D, frames(r))
        Z = np.stack([weighted_np._precond(sides, periodic, shifts[m], X[m], (H, W, C), dtype) for m in range(T)])
        return tall(np.einsum("kt,kyxc->tyxc", D, Z).astype(dtype))

    scratch = np.zeros((T * ny, nx, C), dtype)
    scratch, it, rel = pcg_np.pcg(tall(b), lambda p: tall(block_operator(coef, dg, frames(p), links)), precond, None if scale == 1 else dtype(scale),
                                  tol, max_iters, scratch, (slice(None), slice(None)), dtype, [])
    return volume_np._compose(sides, periodic, state, data, boundary, frames(scratch), dtype).reshape(shape), it, rel


def pcg_f32(args, links, boundary=None, tol=1e-5, max_iters=400, means=None):
    """pcg() in the library's arithmetic -- the yardstick of tests/volume_flow_bounds.py"""
    return pcg(args, links, boundary, tol, max_iters, means, np.float32)


def unpinned_components(args, links):
    """boolean T x H x W x C: the UNKNOWN pixels of connected components (through spatial links and matched temporal links between
    UNKNOWN pixels) that have no KNOWN or Dirichlet neighbour in space, no KNOWN partner along a matched link and no positive weight"""
    sides, periodic, tper, state, weight = args[:5]
    fwd, bwd = links
    k = kinds(sides, periodic, state)
    T, H, W, C = k.shape
    blk = (slice(None),) + unknowns(sides, periodic, H, W)
    kb = k[blk]
    unk = kb == UNKNOWN
    big = kb.size
    label = np.where(unk, np.arange(kb.size).reshape(kb.shape), big)
    kfull = [np.stack([region_np._neighbour(k[t], shift, axis, periodic, OUTSIDE) for t in range(T)])[blk] for shift, axis in region_np._SHIFTS]
    held = np.zeros(kb.shape, bool)
    for q in kfull:
        held |= (q == KNOWN) | (q == DIRICHLET)
    for idx in (fwd, bwd):
        held |= _gather(kb, idx, OUTSIDE) == KNOWN
    if weight is not None:
        held |= np.where(unk, _thwc(np.asarray(weight, np.float32))[blk], np.float32(0)) > 0
    wrapx, wrapy = "x" in periodic, "y" in periodic

    def shifted(a, s, axis, wrap):
        r = np.roll(a, s, axis)
        if not wrap:
            sl = [slice(None)] * a.ndim
            sl[axis] = 0 if s == 1 else -1
            r[tuple(sl)] = big
        return r
    while True:
        new = label
        for q in (shifted(label, 1, 2, wrapx), shifted(label, -1, 2, wrapx), shifted(label, 1, 1, wrapy), shifted(label, -1, 1, wrapy),
                  _gather(label, fwd, big), _gather(label, bwd, big)):
            new = np.minimum(new, q)
        new = np.where(unk, new, big)
        if np.array_equal(new, label):
            break
        label = new
    pinned = np.unique(label[unk & held])
    loose = np.zeros(k.shape, bool)
    loose[blk] = unk & ~np.isin(label, pinned)
    return loose
