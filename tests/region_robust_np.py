"""The test side's restatement of the robust region solve (sc_hip_region_robust*), numpy only, on top of tests/region_np.py with the
penalties of tests/robust_np.py and the coupled magnitudes of tests/robust_coupled_np.py.

Per channel the library minimises over the UNKNOWN pixels, with exponents 0 < p, q <= 2,
    sum w phi_q(u - d; eps_d) + sum_live x-links c_x phi_p(dx u - gx; eps_g) + sum_live y-links c_y phi_p(dy u - gy; eps_g),
"live" being region_np.live_links, by iteratively reweighted least squares: round 0 is the region problem with the caller's links and
weights, round k >= 1 the region problem with s = c rho_p(link residual) on every live link and w' = w rho_q(u - d) at round k - 1's
iterate.  coupling is 0, ISO, JOINT or ISO | JOINT (robust_coupled_np's): one magnitude M over the live links that share a penalty -- a
dead link adds nothing to it, under JOINT a link's magnitude sums the channels in which it is live -- and s = c rho_p(M).

A problem travels as a dict: sides, periodic, state, weight (None: no data term), sx, sy (the base links; None: 1), gx, gy, data,
boundary -- region_bounds.make_input's fields -- and the penalties as pen = (p, q, eps_g, eps_d).  An iterate is a full H x W x C array
composed like the library's out: u at UNKNOWN pixels, data at KNOWN (and OUTSIDE) pixels, boundary on the Dirichlet lines; so np.roll
gives the value across every live link, the wrap of a periodic axis included.  Only live links and UNKNOWN pixels enter any result.

reweigh() gives a round's (sx, sy, w'), 1 at every link that is not live; energy() is float64 throughout (a joint form's gradient
energy, one number per image, on channel 0); irls_exact() runs the rounds in float64 with region_np.solve_exact inside; irls_f32() runs
the library's rounds for a chunk of problems: float32 vectors, float64 dot products, round 0 region_np.pcg_f32's cold start, every later
round region_np's float32 iteration started warm from the previous iterate (robust_np._warm_pcg) under that round's own means -- the
yardstick of tests/region_robust_bounds.py.  round_residual() is RES of an iterate in the system its predecessor gives."""
from __future__ import annotations

import numpy as np

import region_np
import robust_coupled_np as rc
import robust_np
import weighted_np
import wls_np

rho, phi = robust_np.rho, robust_np.phi
_hwc = region_np._hwc
UNKNOWN, KNOWN = region_np.UNKNOWN, region_np.KNOWN
ISO, JOINT = rc.ISO, rc.JOINT
COUPLINGS = rc.COUPLINGS


def _head(P):
    return P["sides"], P["periodic"], P["state"]


def _f32(a):
    return None if a is None else _hwc(np.asarray(a, np.float32))


def _ones(a, shape):
    return np.ones(shape, np.float32) if a is None else _f32(a)


def _boundary(P):
    return P["boundary"] if region_np.has_dirichlet(P["sides"], P["periodic"]) else None


def quadratic(pen):
    return pen[0] == 2 and pen[1] == 2


def effective(coupling, pen, C):
    """the coupling that changes anything: none with p = 2, no joint form of one channel"""
    return 0 if pen[0] == 2 else (coupling & ~JOINT if C == 1 else coupling)


def magnitudes(P, u, coupling, dtype=np.float32):
    """(M_x, M_y, has_x, has_y), H x W x C: the magnitude each x-link / y-link shares, in dtype, and whether that magnitude has a live
    link at all (its owner then books its energy)"""
    lx, ly = region_np.live_links(*_head(P))
    C = lx.shape[2]
    with np.errstate(invalid="ignore", over="ignore"):
        tx, ty = robust_np.link_residuals(u, P["gx"], P["gy"], dtype)
        ax, ay = tx * tx, ty * ty
        if P["sx"] is not None:
            ax = _f32(P["sx"]).astype(dtype) * ax
            ay = _f32(P["sy"]).astype(dtype) * ay
    ax = np.where(lx, ax, dtype(0))
    ay = np.where(ly, ay, dtype(0))
    if coupling & ISO:
        mx = my = ax + ay
        hx = hy = lx | ly
    else:
        mx, my, hx, hy = ax, ay, lx, ly
    if coupling & JOINT:
        def over_channels(m):
            s = m[:, :, 0]
            for k in range(1, C):
                s = s + m[:, :, k]
            return np.repeat(s[:, :, None], C, 2)
        mx = over_channels(mx)
        my = mx if coupling & ISO else over_channels(my)
        hx = np.repeat(hx.any(2)[:, :, None], C, 2)
        hy = hx if coupling & ISO else np.repeat(hy.any(2)[:, :, None], C, 2)
    assert mx.dtype == dtype and my.dtype == dtype
    return mx, my, hx, hy


def reweigh(P, pen, u, coupling=0, dtype=np.float32):
    """(s_x, s_y, w') of the round after iterate u, float32 H x W x C; 1 in every link that is not live, w' None without weight"""
    p, q, eg, ed = pen
    k = region_np.kinds(*_head(P))
    lx, ly = region_np.live_links(*_head(P))
    cx, cy = _ones(P["sx"], k.shape), _ones(P["sy"], k.shape)
    coupling = effective(coupling, pen, k.shape[2])
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if coupling:
            mx, my, _, _ = magnitudes(P, u, coupling, dtype)
            rx, ry = rc.rho_of(p, eg, mx, dtype), rc.rho_of(p, eg, my, dtype)
        else:
            tx, ty = robust_np.link_residuals(u, P["gx"], P["gy"], dtype)
            rx, ry = rho(p, eg, tx, dtype), rho(p, eg, ty, dtype)
        sx = (cx.astype(dtype) * rx).astype(np.float32)
        sy = (cy.astype(dtype) * ry).astype(np.float32)
        w2 = None
        if P["weight"] is not None:
            t = _hwc(np.asarray(u, dtype)) - _f32(P["data"]).astype(dtype)
            w2 = (_f32(P["weight"]).astype(dtype) * rho(q, ed, t, dtype)).astype(np.float32)
            w2 = np.where(k == UNKNOWN, w2, np.float32(0))
    one = np.float32(1)
    return np.where(lx, sx, one), np.where(ly, sy, one), w2


def round_args(P, pen=None, u=None, coupling=0, dtype=np.float32):
    """region_np's args (sides .. lap) of one round: the caller's system (u None), or the system that iterate u gives"""
    if u is None:
        sx, sy, w = P["sx"], P["sy"], P["weight"]
    else:
        sx, sy, w = reweigh(P, pen, u, coupling, dtype)
    lap = region_np.divergence(*_head(P), sx, sy, P["gx"], P["gy"])
    return _head(P) + (w, sx, sy, P["data"], lap)


def energy(P, pen, u, coupling=0):
    """the energy of u per channel, float64 [C]; a joint form's gradient term, one number for the image, on channel 0"""
    p, q, eg, ed = pen
    k = region_np.kinds(*_head(P))
    lx, ly = region_np.live_links(*_head(P))
    C = k.shape[2]
    uu = _hwc(np.asarray(u, np.float64))
    coupling = effective(coupling, pen, C)
    with np.errstate(invalid="ignore"):
        if coupling:
            mx, my, hx, hy = magnitudes(P, uu, coupling, np.float64)
            e = np.where(hx, rc._psi(p, eg, mx), 0.0).reshape(-1, C).sum(0)
            if not coupling & ISO:
                e = e + np.where(hy, rc._psi(p, eg, my), 0.0).reshape(-1, C).sum(0)
            if coupling & JOINT:          # every channel holds the image's magnitude: count it once
                e = np.concatenate([e[:1], np.zeros(C - 1)])
        else:
            cx, cy = (_ones(P[n], k.shape).astype(np.float64) for n in ("sx", "sy"))
            tx, ty = robust_np.link_residuals(uu, P["gx"], P["gy"], np.float64)
            e = np.where(lx, cx * phi(p, eg, tx), 0.0).reshape(-1, C).sum(0) + np.where(ly, cy * phi(p, eg, ty), 0.0).reshape(-1, C).sum(0)
        if P["weight"] is not None:
            d = uu - _f32(P["data"]).astype(np.float64)
            e = e + np.where(k == UNKNOWN, _f32(P["weight"]).astype(np.float64) * phi(q, ed, d), 0.0).reshape(-1, C).sum(0)
    return e


def irls_exact(P, pen, rounds, coupling=0):
    """[u_0 .. u_rounds], float64 H x W x C: u_0 the quadratic solve, u_k the exact region solve with the links and weights of u_(k-1)"""
    out = [_hwc(region_np.solve_exact(*round_args(P), _boundary(P)))]
    for _ in range(rounds):
        if quadratic(pen):
            break
        out.append(_hwc(region_np.solve_exact(*round_args(P, pen, out[-1], coupling, np.float64), _boundary(P))))
    return out


def chunk_means(all_args):
    """(s-bar, w-bar) as the library takes them for a chunk of systems (region_np args): every mean over all its members' live links or
    UNKNOWN pixels"""
    m = [region_np.precond_means(*a[:6]) for a in all_args]
    if len(m) == 1:
        return m[0][:2]
    ns, nu = sum(c[2] for c in m), sum(c[3] for c in m)
    sbar = sum(c[0] * c[2] for c in m) / ns if ns and all_args[0][4] is not None else 1.0
    return sbar, (sum(c[1] * c[3] for c in m) / nu if nu else sbar)


def _warm_round(args, boundary, means, u, tol, max_iters):
    """one warm-started float32 solve of the system args from the composed iterate u: (the next composed iterate, iterations)"""
    sides, periodic, state, weight, sx, sy, data, lap = args
    k = region_np.kinds(sides, periodic, state)
    H, W, C = k.shape
    blk = region_np.unknowns(sides, periodic, H, W)
    links, dg = region_np._planes(sides, periodic, state, weight, sx, sy, np.float32)
    sbar, wbar = means
    lam = np.float32(wbar / sbar)
    b = region_np.folded_rhs(sides, periodic, state, weight, sx, sy, data, lap, boundary, np.float32)
    start = np.where(k[blk] == UNKNOWN, _hwc(np.asarray(u, np.float32))[blk], np.float32(0))
    x, it, _ = robust_np._warm_pcg(b, lambda v: wls_np.block_operator(links, dg, v),
                                   lambda r: weighted_np._precond(sides, periodic, lam, r, (H, W, C), np.float32), start, tol, max_iters)
    return _hwc(region_np._compose(sides, periodic, state, data, boundary, x, np.float32)), it


def irls_f32(probs, pen, rounds, coupling=0, tol=1e-5, max_iters=400):
    """The library's rounds in numpy for a chunk of problems (a dict: a chunk of one): per problem ([u_0 .. u_rounds] float32 H x W x C,
    [inner iterations of every round]); every round's means are the chunk's"""
    single = isinstance(probs, dict)
    probs = [probs] if single else list(probs)
    args0 = [round_args(P) for P in probs]
    us, its = [], []
    means = (None, None) if single else chunk_means(args0)          # (a chunk of one: region_np.pcg_f32 takes the problem's own)
    for P, a in zip(probs, args0):
        u0, it, _ = region_np.pcg_f32(*a, _boundary(P), tol=tol, max_iters=max_iters, precond_smooth=means[0], precond_lambda=means[1])
        us.append([_hwc(u0)])
        its.append([it])
    for _ in range(rounds):
        if quadratic(pen):
            break
        args = [round_args(P, pen, u[-1], coupling) for P, u in zip(probs, us)]
        means = chunk_means(args)
        for P, a, u, n in zip(probs, args, us, its):
            nxt, it = _warm_round(a, _boundary(P), means, u[-1], tol, max_iters)
            u.append(nxt)
            n.append(it)
    return (us[0], its[0]) if single else list(zip(us, its))


def _res(P, args, u):
    sides, periodic, state, weight, sx, sy, data, lap = args
    k = region_np.kinds(sides, periodic, state)
    blk = region_np.unknowns(sides, periodic, *k.shape[:2])
    unk = (k == UNKNOWN)[blk]
    b = region_np.folded_rhs(sides, periodic, state, weight, sx, sy, data, lap, _boundary(P))
    r = region_np.residual(sides, periodic, state, weight, sx, sy, u, data, lap, _boundary(P))
    scale = float(np.abs(b[unk]).max()) if unk.any() else 0.0
    return float(np.abs(r[unk]).max()) / scale if scale > 0 else 0.0


def round_residual(P, pen, u_prev, u, coupling=0):
    """RES of u in the region system that u_prev's links and weights give (u_prev None: the caller's system): max |L u - b| / max |b|
    over the UNKNOWN pixels, float64"""
    return _res(P, round_args(P) if u_prev is None else round_args(P, pen, u_prev, coupling), u)
