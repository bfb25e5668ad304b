"""The test side's restatement of the sub-pixel flow volume solve (sc_hip_volume_subflow*), numpy only, built on volume_flow_np and
volume_wls_np.

A problem travels as volume_wls_np's tuple args = (sides, periodic, tper, state, weight, sx, sy, smt, tau, data, lap) and, beside it, the
links (idx, b) that taps() makes of a flow.  flow is (T - 1) x H x W x 2 -- periodic time: T x H x W x 2 -- of (dx, dy), real-valued:
pixel (x, y) of frame t is the point (x + dx, y + dy) of frame t + 1 (of frame 0 behind the last), read there by bilinear
interpolation.  idx is int64 T x ny x nx x 4 over the work rectangle (the border kind's unknowns) holding work-plane indices
(t ny + y) nx + x of the four taps of the link each pixel holds, -1: the tap is no part of the link (all four -1: no link); b is float32
of the same shape, the taps' weights, 0 where idx is -1.

taps() is the header's rule.  Per component in float32: x0 = floor(dx), ax = dx - x0 (one float32 subtraction); the tap columns x + x0 and one more, the
rows y + y0 and one more; the weights the float32 products (1 - ax)(1 - ay), ax (1 - ay), (1 - ax) ay, ax ay in that order; a tap of
weight exactly 0 is left out.  A pixel is a candidate when both components are finite and at most 1e6 in magnitude and its frame has a
next one; a periodic axis wraps each tap, elsewhere a link with a remaining tap outside the work rectangle is no link.  No matching.

With B the matrix whose row p holds b_k(p) at the taps and -1 at p, and S = diag(lt) over the live links (neither the source nor a tap
OUTSIDE, at least one of the up to five points UNKNOWN; lt = tau * smt and gt stored at the source), the system on the UNKNOWN pixels is
L = A_s - W - B^T S B with sc_hip_volume_wls's spatial part, and b = (the spatial right-hand side) - B^T S gt + B^T S B d_K, d_K data at
the KNOWN pixels and 0 elsewhere.  The preconditioner is volume_wls_np's, unchanged: straight time links."""
from __future__ import annotations

import numpy as np

import pcg_np
import region_np
import volume_flow_np as vf
import volume_np
import volume_wls_np as vw
import weighted_np

UNKNOWN, KNOWN, OUTSIDE, DIRICHLET = vw.UNKNOWN, vw.KNOWN, vw.OUTSIDE, vw.DIRICHLET
unknowns = vw.unknowns
has_dirichlet = vw.has_dirichlet
kinds = vw.kinds
_thwc, _f32, _frame = vw._thwc, vw._f32, vw._frame
_blk, _pad = vf._blk, vf._pad
FLOW_LIMIT = 1e6


def taps(sides, periodic, tper, shape, flow):
    """(idx, b) of a volume of shape = (T, H, W) under these borders"""
    T, H, W = shape
    rows, cols = unknowns(sides, periodic, H, W)
    ny, nx = rows.stop - rows.start, cols.stop - cols.start
    Tf = T if tper else T - 1
    flow = np.asarray(flow, np.float32)
    assert flow.shape == (Tf, H, W, 2), (flow.shape, (Tf, H, W, 2))
    f = flow[:, rows, cols]
    with np.errstate(invalid="ignore"):
        ok = (np.abs(f) <= np.float32(FLOW_LIMIT)).all(-1)          # (NaN and the infinities fail)
    f = np.where(ok[..., None], f, np.float32(0))
    f0 = np.floor(f)
    a = f - f0
    assert a.dtype == np.float32 and (a >= 0).all() and (a <= 1).all()          # (1: a tiny negative value, rounded)
    one = np.float32(1)
    wx, wy = (one - a[..., 0], a[..., 0]), (one - a[..., 1], a[..., 1])
    i0 = f0.astype(np.int64)
    t, y, x = np.mgrid[0:Tf, 0:ny, 0:nx]
    idx = np.full((T, ny, nx, 4), -1, np.int64)
    b = np.zeros((T, ny, nx, 4), np.float32)
    for k in range(4):
        w = wx[k & 1] * wy[k >> 1]
        assert w.dtype == np.float32
        part = ok & (w != 0)
        tx, ty = x + i0[..., 0] + (k & 1), y + i0[..., 1] + (k >> 1)
        if "x" in periodic:
            tx %= nx
        if "y" in periodic:
            ty %= ny
        inside = (tx >= 0) & (tx < nx) & (ty >= 0) & (ty < ny)
        ok &= ~(part & ~inside)
        target = (((t + 1) % T) * ny + ty) * nx + tx
        idx[:Tf, ..., k] = np.where(part & inside, target, -1)
        b[:Tf, ..., k] = np.where(part & inside, w, np.float32(0))
    idx[:Tf][~ok] = -1
    b[:Tf][~ok] = 0
    return idx, b


def _gather(a, idx, fill):
    """a (T x ny x nx x C) at the elements idx (T x ny x nx) names, `fill` where idx is -1"""
    return vf._gather(a, idx, fill)


def _point_kinds(kb, links):
    """the kinds of the four taps of every pixel's link, 4 arrays T x ny x nx x C (OUTSIDE stands in where the tap is no part)"""
    idx, _ = links
    return [np.where((idx[..., k] >= 0)[..., None], _gather(kb, idx[..., k], OUTSIDE), -1) for k in range(4)]


def _held_live(kb, links):
    """boolean T x ny x nx x C: the link this pixel holds is live"""
    idx, _ = links
    has = (idx >= 0).any(-1)[..., None]
    dead = kb == OUTSIDE
    unk = kb == UNKNOWN
    for k, q in enumerate(_point_kinds(kb, links)):
        dead = dead | (q == OUTSIDE)
        unk = unk | (q == UNKNOWN)
    return has & ~dead & unk


def live_links(sides, periodic, tper, state, links):
    """(live_x, live_y, live_t): the elements of sx / gx, sy / gy (T x H x W x C) and smt / gt (their own length) that a call reads"""
    st = _f32(state)
    lx, ly, _ = vw.live_links(sides, periodic, tper, st)
    k = kinds(sides, periodic, st)
    T, H, W, C = k.shape
    lt = np.zeros(k.shape, bool)
    lt[(slice(None),) + unknowns(sides, periodic, H, W)] = _held_live(_blk(sides, periodic, k), links)
    return lx, ly, lt[:T if tper else T - 1]


def _lt(sides, periodic, tper, k, smt, tau, links):
    """float32 T x ny x nx x C: lt = tau * smt of the link each pixel holds (one rounded product; smt None: tau) where it is live, else 0"""
    kb = _blk(sides, periodic, k)
    live = _held_live(kb, links)
    tau = np.float32(tau)
    if smt is None:
        v = np.full(live.shape, tau, np.float32)
    else:
        v = tau * np.where(live, _pad(_blk(sides, periodic, _f32(smt)), k.shape[0]), np.float32(1))
    assert v.dtype == np.float32
    return np.where(live, v, np.float32(0))


def _B(links, v):
    """(B v) per link: sum_k b_k v(q_k) - v(p), in v's dtype, the taps in their order"""
    idx, b = links
    acc = np.zeros_like(v)
    for k in range(4):
        acc = acc + b[..., k, None].astype(v.dtype) * _gather(v, idx[..., k], v.dtype.type(0))
    return acc - v


def _Bt(links, r):
    """(B^T r) per pixel: the sum over the arrivals (source, tap) of b r(source), ascending (source, tap), less r(p)"""
    idx, b = links
    flat = np.zeros((idx[..., 0].size,) + r.shape[3:], r.dtype)
    tgt, wgt = idx.reshape(-1), b.reshape(-1)          # (slot 4 source + tap: already ascending (source, tap))
    rr = np.repeat(r.reshape((-1,) + r.shape[3:]), 4, axis=0)
    ok = tgt >= 0
    np.add.at(flat, tgt[ok], wgt[ok, None].astype(r.dtype) * rr[ok])
    return flat.reshape(r.shape) - r


def divergence(sides, periodic, tper, state, sx, sy, smt, tau, gx, gy, gt, links):
    """steps 1 and 2 of the right-hand side in float32, T x H x W x C (valid at the UNKNOWN pixels): the spatial divergence and -B^T S gt"""
    st, sxf, syf = _f32(state), _f32(sx), _f32(sy)
    gx, gy = _f32(gx), _f32(gy)
    T = st.shape[0]
    div = np.stack([region_np.divergence(sides, periodic, st[t], _frame(sxf, t), _frame(syf, t), gx[t], gy[t]) for t in range(T)])
    k = kinds(sides, periodic, st)
    lt = _lt(sides, periodic, tper, k, smt, tau, links)
    tm = np.zeros(div.shape, np.float32)
    if gt is not None:
        g = _pad(_blk(sides, periodic, _f32(gt)), T)
        e = np.where(lt != 0, lt * np.where(lt != 0, g, np.float32(0)), np.float32(0))
        tm[(slice(None),) + unknowns(sides, periodic, *div.shape[1:3])] = -_Bt(links, e)
    out = div + tm
    assert out.dtype == np.float32
    return out


def _no_links(k, sides, periodic):
    kb = _blk(sides, periodic, k)
    none = np.full(kb.shape[:3], -1, np.int64)
    return none, none


def folded_rhs(args, links, boundary=None, dtype=np.float64):
    """b on the unknown blocks [T][ny][nx][C]; lap: steps 1 and 2 (divergence(), or the caller's lap)"""
    sides, periodic, tper, state, weight, sx, sy, smt, tau, data, lap = args
    st, d, lap, w, sx, sy, bd = (_f32(a) for a in (state, data, lap, weight, sx, sy, boundary))
    k = kinds(sides, periodic, st)
    T = k.shape[0]
    g = np.stack([region_np.folded_rhs(sides, periodic, st[t], _frame(w, t), _frame(sx, t), _frame(sy, t), d[t], lap[t], _frame(bd, t), dtype)
                  for t in range(T)])
    kb = _blk(sides, periodic, k)
    lt = _lt(sides, periodic, tper, k, smt, tau, links).astype(dtype)
    dk = np.where(kb == KNOWN, _blk(sides, periodic, d), np.float32(0)).astype(dtype)
    g = g + np.where(kb == UNKNOWN, _Bt(links, lt * _B(links, dk)), dtype(0))
    assert g.dtype == dtype
    return g


def _planes(args, links, dtype):
    """the operator's parts on the unknown blocks: the spatial coefficients (west, east, north, south) kept only where both ends are
    UNKNOWN, the diagonal of the spatial links and w in the kernel's order, lt of the live links and the mask of the UNKNOWN pixels"""
    sides, periodic, tper, state, weight, sx, sy, smt, tau = args[:9]
    k = kinds(sides, periodic, _f32(state))
    coef, dg = vf._planes(args[:9], _no_links(k, sides, periodic), dtype)
    kb = _blk(sides, periodic, k)
    return coef[:4], dg, _lt(sides, periodic, tper, k, smt, tau, links).astype(dtype), (kb == UNKNOWN).astype(dtype)


def block_operator(planes, u, links):
    """L u on the unknown blocks in u's dtype: the kernel's spatial order, the temporal part in product form -B^T (S (B (mask u)))"""
    (west, east, north, south), dg, lt, mask = planes
    tm = mask * _Bt(links, lt * _B(links, mask * u))
    return (((west * np.roll(u, 1, 2) + east * np.roll(u, -1, 2)) + (north * np.roll(u, 1, 1) + south * np.roll(u, -1, 1))) - tm) - dg * u


def residual(args, links, u, boundary=None):
    """L u - b in float64 on the unknown blocks (0 where the pixel is not UNKNOWN); u: a call's out"""
    sides, periodic, _, state = args[:4]
    kb = _blk(sides, periodic, kinds(sides, periodic, state))
    ub = np.where(kb == UNKNOWN, _blk(sides, periodic, _thwc(np.asarray(u, np.float64))), 0.0)
    return block_operator(_planes(args, links, np.float64), ub, links) - folded_rhs(args, links, boundary)


def precond_means(args, links):
    """volume_wls_np.precond_means with the bilinear links: (s-bar, tau-bar, w-bar, (spatial links live in the region, live temporal
    links, UNKNOWN pixels)); a temporal link's share of w-bar is lt * (1 where its source is KNOWN, else the sum of b over its KNOWN taps)"""
    sides, periodic, tper, state, weight, sx, sy, smt, tau = args[:9]
    _, b = links
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
    lt = _lt(sides, periodic, tper, k, smt, tau, links)
    tl = _held_live(kb, links)
    share = np.zeros(kb.shape, np.float32)
    for kk, q in enumerate(_point_kinds(kb, links)):
        share = share + np.where(q == KNOWN, b[..., kk, None], np.float32(0))
    share = np.where(kb == KNOWN, np.float32(1), share)
    uk += float((lt.astype(np.float64) * share.astype(np.float64))[tl].sum())
    unk = k == UNKNOWN
    wsum = 0.0 if weight is None else float(_f32(weight)[unk].astype(np.float64).sum())
    n = int(unk.sum())
    sbar = float(v.mean()) if v.size and sx is not None else 1.0
    tbar = float(lt[tl].astype(np.float64).mean()) if tl.any() and smt is not None else float(np.float32(tau))
    return sbar, tbar, ((wsum + uk) / n if n else 1.0), (v.size, int(tl.sum()), n)


def assemble(args, links, c=0):
    """(A, index): the dense matrix A_s - W - B^T S B of channel c over its UNKNOWN pixels (A u = b, A = L), and each block element's
    row (-1: none)"""
    sides, periodic, _, state = args[:4]
    idx, b = links
    (west, east, north, south), dg, lt, mask = _planes(args, links, np.float64)
    m = mask[..., c] != 0
    n = int(m.sum())
    index = np.full(m.shape, -1)
    index[m] = np.arange(n)
    A = np.zeros((n, n))
    A[np.arange(n), np.arange(n)] = -dg[..., c][m]
    nb = [np.roll(index, s, a) for s, a in ((1, 2), (-1, 2), (1, 1), (-1, 1))]
    for l, j in zip((west, east, north, south), nb):
        v = l[..., c][m]
        ok = v != 0
        np.add.at(A, (np.arange(n)[ok], j[m][ok]), v[ok])
    # - B^T S B: every live link's up to five points among the unknowns, pair by pair
    live = lt[..., c] != 0
    flat = index.reshape(-1)
    pts = [np.where(idx[..., k] >= 0, flat[np.where(idx[..., k] >= 0, idx[..., k], 0)], -1) for k in range(4)] + [index]
    cfs = [b[..., k].astype(np.float64) for k in range(4)] + [np.full(index.shape, -1.0)]
    for pi, ci in zip(pts, cfs):
        for pj, cj in zip(pts, cfs):
            ok = live & (pi >= 0) & (pj >= 0)
            np.add.at(A, (pi[ok], pj[ok]), -(lt[..., c] * ci * cj)[ok])
    return A, index


def _cg64(planes_c, links, b, M_inv, who):
    bn = float(np.sqrt((b * b).sum()))
    x = M_inv(b)
    r = b - block_operator(planes_c, x, links)
    z = M_inv(r)
    p, rho = z.copy(), float((r * z).sum())
    for _ in range(40000):
        if float(np.sqrt((r * r).sum())) <= 1e-13 * bn:
            return x
        q = block_operator(planes_c, p, links)
        alpha = rho / float((p * q).sum())
        x, r = x + alpha * p, r - alpha * q
        z = M_inv(r)
        rho_new = float((r * z).sum())
        p, rho = z + (rho_new / rho) * p, rho_new
    raise RuntimeError(f"{who}: the float64 conjugate gradients did not reach 1e-13")


def solve_exact(args, links, boundary=None, dense=None):
    """float64 solution, data's shape, composed like out: LAPACK up to volume_wls_np.DENSE_LIMIT unknowns per channel, else conjugate
    gradients in float64 under the straight-link preconditioner to a relative residual of 1e-13"""
    sides, periodic, tper, state, weight, sx, sy, smt, tau, data, lap = args
    shape = np.asarray(data).shape
    kb = _blk(sides, periodic, kinds(sides, periodic, state))
    T, ny, nx, C = kb.shape
    g = folded_rhs(args, links, boundary)
    planes = _planes(args, links, np.float64)
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
        (west, east, north, south), dg, lt, mask = planes
        pc = (tuple(l[..., c:c + 1] for l in (west, east, north, south)), dg[..., c:c + 1], lt[..., c:c + 1], mask[..., c:c + 1])
        x = _cg64(pc, links, g[..., c:c + 1], M_inv, "volume_subflow_np.solve_exact")
        u[..., c] = np.where(m, x[..., 0], 0.0)
    return volume_np._compose(sides, periodic, state, data, boundary, u, np.float64).reshape(shape)


def pcg(args, links, boundary=None, tol=1e-5, max_iters=400, means=None, dtype=np.float32):
    """volume_wls_np.pcg with the product-form operator: the library's iteration, the preconditioner unchanged (straight time links, the
    means of precond_means or `means`).  Returns (out, iterations, the worst channel's final ||r|| / ||b||)."""
    sides, periodic, tper, state, weight, sx, sy, smt, tau, data, lap = args
    shape = np.asarray(data).shape
    k = kinds(sides, periodic, state)
    T, H, W, C = k.shape
    planes = _planes(args, links, dtype)
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

    def op(p):
        q = block_operator(planes, frames(p), links)
        assert q.dtype == dtype
        return tall(q)

    scratch = np.zeros((T * ny, nx, C), dtype)
    scratch, it, rel = pcg_np.pcg(tall(b), op, precond, None if scale == 1 else dtype(scale), tol, max_iters, scratch, (slice(None), slice(None)),
                                  dtype, [])
    return volume_np._compose(sides, periodic, state, data, boundary, frames(scratch), dtype).reshape(shape), it, rel


def pcg_f32(args, links, boundary=None, tol=1e-5, max_iters=400, means=None):
    """pcg() in the library's arithmetic -- the yardstick of tests/volume_subflow_bounds.py"""
    return pcg(args, links, boundary, tol, max_iters, means, np.float32)


def unpinned_components(args, links):
    """boolean T x H x W x C: the UNKNOWN pixels of connected components (through spatial links between UNKNOWN pixels and through live
    bilinear links, which join all their UNKNOWN points) that have no KNOWN or Dirichlet neighbour in space, no live link with a KNOWN
    point and no positive weight"""
    sides, periodic, tper, state, weight = args[:5]
    idx, _ = links
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
    live = _held_live(kb, links)
    pk = _point_kinds(kb, links)
    known_in = live & (kb == KNOWN)
    for q in pk:
        known_in |= live & (q == KNOWN)
    # a live link with a KNOWN point pins every UNKNOWN point of it
    held |= known_in & unk
    chan = np.broadcast_to(np.arange(C), kb.shape)
    hflat = held.reshape(-1, C)
    for kk in range(4):
        ok = known_in & (pk[kk] == UNKNOWN)
        hflat[np.broadcast_to(idx[..., kk, None], kb.shape)[ok], chan[ok]] = True
    held = hflat.reshape(kb.shape)
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
        for q in (shifted(label, 1, 2, wrapx), shifted(label, -1, 2, wrapx), shifted(label, 1, 1, wrapy), shifted(label, -1, 1, wrapy)):
            new = np.minimum(new, q)
        new = np.where(unk, new, big)
        # a live link: the smallest label among its UNKNOWN points goes to all of them
        low = np.where(live, new, big)
        for kk in range(4):
            low = np.minimum(low, np.where(live & (pk[kk] == UNKNOWN), _gather(new, idx[..., kk], big), big))
        new = np.minimum(new, np.where(unk, low, big))
        nflat = new.reshape(-1, C).copy()
        for kk in range(4):
            ok = live & (pk[kk] == UNKNOWN)
            np.minimum.at(nflat, (np.broadcast_to(idx[..., kk, None], kb.shape)[ok], chan[ok]), low[ok])
        new = nflat.reshape(kb.shape)
        if np.array_equal(new, label):
            break
        label = new
    pinned = np.unique(label[unk & held])
    loose = np.zeros(k.shape, bool)
    loose[blk] = unk & ~np.isin(label, pinned)
    return loose
