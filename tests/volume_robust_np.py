"""The test side's restatement of the robust volume solve (sc_hip_volume_robust*), numpy only, on top of tests/volume_wls_np.py with the
penalties of tests/robust_np.py.

Per channel the library minimises over the UNKNOWN pixels of all frames, with exponents 0 < p, r, q <= 2,
    sum w phi_q(u - d; eps_d) + sum_live x-links c_x phi_p(dx u - gx; eps_g) + sum_live y-links c_y phi_p(dy u - gy; eps_g)
                              + sum_live t-links c_t phi_r(u_(t+1) - u_t - gt; eps_t),
c_t = tau * smooth_t rounded once (volume_wls_np's lt), by iteratively reweighted least squares: round 0 is the WLS volume problem with
the caller's links and weights, round k >= 1 the WLS volume problem with s = c rho(link residual) on every live link and w' = w rho_q(u -
d) at round k - 1's iterate.  A round's links go into volume_wls_np as sx, sy, smt with tau = 1: 1 * smt is exact.

A problem travels as a dict: sides, periodic, tper, state, weight (None: no data term), sx, sy, smt (the base links; None: 1), tau, gx,
gy, gt (None: zeros), data, boundary -- volume_wls_bounds.make_input's fields -- and the penalties as pen = (p, r, q, eps_g, eps_t, eps_d).
An iterate is a full T x H x W x C array composed like the library's out: u at UNKNOWN pixels, data at KNOWN (and OUTSIDE) pixels,
boundary on the Dirichlet lines; so np.roll gives the value across every live link, the wrap of a periodic axis and of periodic time
included.  Only live links and UNKNOWN pixels enter any result.

reweigh() gives a round's (sx, sy, smt, w'), 1 at every link that is not live; energy() is float64 throughout; irls_exact() runs the
rounds in float64 with volume_wls_np.solve_exact inside; irls_f32() runs the library's rounds for a chunk of problems: float32 vectors,
float64 dot products, round 0 volume_wls_np.pcg_f32's cold start, every later round volume_wls_np's float32 iteration started warm from
the previous iterate (robust_np._warm_pcg) under that round's own means -- the yardstick of tests/volume_robust_bounds.py.
round_residual() is RES of an iterate in the system its predecessor gives."""
from __future__ import annotations

import numpy as np

import robust_np
import volume_np
import volume_wls_np as vw
import weighted_np

rho, phi = robust_np.rho, robust_np.phi
_thwc = vw._thwc
UNKNOWN, KNOWN = vw.UNKNOWN, vw.KNOWN


def _head(P):
    return P["sides"], P["periodic"], P["tper"], P["state"]


def _f32(a):
    return None if a is None else _thwc(np.asarray(a, np.float32))


def _ones(a, shape):
    return np.ones(shape, np.float32) if a is None else _f32(a)


def link_residuals(P, u, dtype=np.float32):
    """(t_x, t_y, t_t) in dtype: (u_hi - u_lo) - g at every element of gx, gy and of the temporal arrays (what is not live holds whatever
    the wrap gives)"""
    u = _thwc(np.asarray(u, dtype))
    tper = P["tper"]
    tt = vw._next(u, tper) - vw._here(u, tper)
    if P["gt"] is not None:
        tt = tt - _f32(P["gt"]).astype(dtype)
    return (np.roll(u, -1, 2) - u) - _f32(P["gx"]).astype(dtype), (np.roll(u, -1, 1) - u) - _f32(P["gy"]).astype(dtype), tt


def base_links(P):
    """(c_x, c_y, lt) float32: the caller's base links, lt = tau * smooth_t as the library rounds it (0 at a temporal link that is not live)"""
    k = vw.kinds(*_head(P)[:2], P["state"])
    return _ones(P["sx"], k.shape), _ones(P["sy"], k.shape), vw._lt(k, P["tper"], P["smt"], P["tau"])


def reweigh(P, pen, u, dtype=np.float32):
    """(s_x, s_y, s_t, w') of the round after iterate u, float32; 1 in every link that is not live, w' None without weight"""
    p, r, q, eg, et, ed = pen
    lx, ly, lt_live = vw.live_links(*_head(P))
    cx, cy, lt = base_links(P)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        tx, ty, tt = link_residuals(P, u, dtype)
        sx = (cx.astype(dtype) * rho(p, eg, tx, dtype)).astype(np.float32)
        sy = (cy.astype(dtype) * rho(p, eg, ty, dtype)).astype(np.float32)
        st = (lt.astype(dtype) * rho(r, et, tt, dtype)).astype(np.float32)
        w2 = None
        if P["weight"] is not None:
            t = _thwc(np.asarray(u, dtype)) - _f32(P["data"]).astype(dtype)
            w2 = (_f32(P["weight"]).astype(dtype) * rho(q, ed, t, dtype)).astype(np.float32)
            w2 = np.where(vw.kinds(*_head(P)[:2], P["state"]) == UNKNOWN, w2, np.float32(0))
    one = np.float32(1)
    return np.where(lx, sx, one), np.where(ly, sy, one), np.where(lt_live, st, one), w2


def round_args(P, pen=None, u=None, dtype=np.float32):
    """volume_wls_np's args of one round: the caller's system (u None), or the system that iterate u gives"""
    if u is None:
        sx, sy, smt, w, tau = P["sx"], P["sy"], P["smt"], P["weight"], P["tau"]
    else:
        sx, sy, smt, w = reweigh(P, pen, u, dtype)
        tau = 1.0
    lap = vw.divergence(*_head(P), sx, sy, smt, tau, P["gx"], P["gy"], P["gt"])
    data = P["data"] if P["weight"] is not None else np.where(vw.kinds(*_head(P)[:2], P["state"]) == UNKNOWN, np.float32(0), _f32(P["data"]))
    return _head(P) + (w, sx, sy, smt, tau, data, lap)


def _boundary(P):
    return P["boundary"] if vw.has_dirichlet(P["sides"], P["periodic"]) else None


def energy(P, pen, u):
    """the energy of u per channel, float64 [C]"""
    p, r, q, eg, et, ed = pen
    k = vw.kinds(*_head(P)[:2], P["state"])
    lx, ly, lt_live = vw.live_links(*_head(P))
    cx, cy, lt = (a.astype(np.float64) for a in base_links(P))
    uu = _thwc(np.asarray(u, np.float64))
    C = k.shape[3]
    with np.errstate(invalid="ignore"):
        tx, ty, tt = link_residuals(P, uu, np.float64)
        e = np.where(lx, cx * phi(p, eg, tx), 0.0).reshape(-1, C).sum(0) + np.where(ly, cy * phi(p, eg, ty), 0.0).reshape(-1, C).sum(0)
        e = e + np.where(lt_live, lt * phi(r, et, tt), 0.0).reshape(-1, C).sum(0)
        if P["weight"] is not None:
            d = uu - _f32(P["data"]).astype(np.float64)
            e = e + np.where(k == UNKNOWN, _f32(P["weight"]).astype(np.float64) * phi(q, ed, d), 0.0).reshape(-1, C).sum(0)
    return e


def quadratic(pen):
    return pen[0] == 2 and pen[1] == 2 and pen[2] == 2


def irls_exact(P, pen, rounds):
    """[u_0 .. u_rounds], float64 T x H x W x C: u_0 the quadratic solve, u_k the exact WLS volume solve with the links and weights of u_(k-1)"""
    out = [_thwc(vw.solve_exact(round_args(P), _boundary(P)))]
    for _ in range(rounds):
        if quadratic(pen):
            break
        out.append(_thwc(vw.solve_exact(round_args(P, pen, out[-1], np.float64), _boundary(P))))
    return out


def _counts_means(args):
    sbar, tbar, wbar, (ns, nt, nu) = vw.precond_means(*args[:9])
    return sbar, tbar, wbar, ns, nt, nu


def chunk_means(all_args):
    """(s-bar, tau-bar, w-bar) as the library takes them for a chunk of systems (volume_wls_np args): every mean over all its members'
    live links or UNKNOWN pixels"""
    m = [_counts_means(a) for a in all_args]
    if len(m) == 1:
        return m[0][:3]
    ns, nt, nu = (sum(c[3 + i] for c in m) for i in range(3))
    first = all_args[0]
    sbar = sum(c[0] * c[3] for c in m) / ns if ns and first[5] is not None else 1.0
    tbar = sum(c[1] * c[4] for c in m) / nt if nt and first[7] is not None else float(np.float32(first[8]))
    return sbar, tbar, (sum(c[2] * c[5] for c in m) / nu if nu else 1.0)


def _warm_round(args, boundary, means, u, tol, max_iters):
    """one warm-started float32 solve of the system args from the composed iterate u: (the next composed iterate, iterations)"""
    sides, periodic, tper, state, weight, sx, sy, smt, tau, data, lap = args
    k = vw.kinds(sides, periodic, state)
    T, H, W, C = k.shape
    blk = (slice(None),) + vw.unknowns(sides, periodic, H, W)
    links, dg = vw._planes(sides, periodic, tper, state, weight, sx, sy, smt, tau, np.float32)
    sbar, tbar, wbar = means
    D = vw.time_table(T, tper).astype(np.float32)
    shifts = vw.mode_shifts(T, wbar, tbar, sbar, tper)
    b = vw.folded_rhs(*args, boundary, np.float32)
    _, ny, nx, _ = b.shape
    tall = lambda a: a.reshape(T * ny, nx, C)
    frames = lambda a: a.reshape(T, ny, nx, C)

    def precond(r):
        X = np.einsum("kt,tyxc->kyxc", D, frames(r))
        Z = np.stack([weighted_np._precond(sides, periodic, shifts[m], X[m], (H, W, C), np.float32) for m in range(T)])
        return tall(np.einsum("kt,kyxc->tyxc", D, Z).astype(np.float32))

    start = np.where(k[blk] == UNKNOWN, _thwc(np.asarray(u, np.float32))[blk], np.float32(0))
    x, it, _ = robust_np._warm_pcg(tall(b), lambda v: tall(vw.block_operator(links, dg, frames(v))), precond, tall(start), tol, max_iters)
    return _thwc(volume_np._compose(sides, periodic, state, data, boundary, frames(x), np.float32)), it


def irls_f32(probs, pen, rounds, tol=1e-5, max_iters=400):
    """The library's rounds in numpy for a chunk of problems (a dict: a chunk of one): per problem ([u_0 .. u_rounds] float32 T x H x W x C,
    [inner iterations of every round]); every round's means are the chunk's"""
    single = isinstance(probs, dict)
    probs = [probs] if single else list(probs)
    args0 = [round_args(P) for P in probs]
    means = chunk_means(args0)
    us, its = [], []
    for P, a in zip(probs, args0):
        u0, it, _ = vw.pcg_f32(a, _boundary(P), tol=tol, max_iters=max_iters, means=means)
        us.append([_thwc(u0)])
        its.append([it])
    for _ in range(rounds):
        if quadratic(pen):
            break
        args = [round_args(P, pen, u[-1]) for P, u in zip(probs, us)]
        means = chunk_means(args)
        for P, a, u, n in zip(probs, args, us, its):
            nxt, it = _warm_round(a, _boundary(P), means, u[-1], tol, max_iters)
            u.append(nxt)
            n.append(it)
    return (us[0], its[0]) if single else list(zip(us, its))


def round_residual(P, pen, u_prev, u):
    """RES of u in the WLS volume system that u_prev's links and weights give: max |L u - b| / max |b| over the UNKNOWN pixels, float64"""
    args = round_args(P, pen, u_prev)
    k = vw.kinds(*_head(P)[:2], P["state"])
    blk = (slice(None),) + vw.unknowns(P["sides"], P["periodic"], *k.shape[1:3])
    unk = (k == UNKNOWN)[blk]
    b = vw.folded_rhs(*args, _boundary(P))
    r = vw.residual(args, u, _boundary(P))
    scale = float(np.abs(b[unk]).max())
    return float(np.abs(r[unk]).max()) / scale if scale > 0 else 0.0
