"""The test side's restatement of the coupled volume solve (sc_hip_volume_coupled*), numpy only, on top of tests/volume_robust_np.py after
the coupled part of tests/region_robust_np.py.

coupling is a sum of SPACE (one magnitude per pixel over its x- and y-link), TIME (... and its forward temporal link; comes with SPACE and
with p_time = p_grad, eps_time = eps_grad) and CHANNELS (every magnitude is the running sum over the channels in which the link is
live).  A live link's share of a magnitude is a = c t^2, t = (u_hi - u_lo) - g, c the base link (smooth_x, smooth_y: None is 1 without
a multiply; lt = tau * smooth_t rounded once); a dead link adds nothing; within a pixel the sum is (a_x + a_y) + a_t.  The owner of a
link is its low end, so a magnitude sits at the element of the link arrays that the link itself has: frame t owns the link from t to the
next, frame T - 1 the wrapping one, and a pixel of a low Dirichlet line only its one link into the domain.  s = c rho(M); without
CHANNELS and without TIME a temporal link keeps volume_robust_np's own penalty c_t phi_r(t).

A problem and its penalties travel as volume_robust_np's dict and pen = (p, r, q, eps_g, eps_t, eps_d).  effective() is the coupling
that changes anything; with none every function here returns volume_robust_np's arrays themselves.  energy() is float64 throughout (under
CHANNELS the gradient-and-time term is one number per volume, on channel 0); irls_exact() and irls_f32() are volume_robust_np's rounds with
reweigh() of this module inside; round_residual() is RES of an iterate in the system its predecessor gives."""
from __future__ import annotations

import numpy as np

import robust_coupled_np as rc
import volume_robust_np as vr
import volume_wls_np as vw

SPACE, TIME, CHANNELS = 1, 2, 4
LEGAL = (SPACE, SPACE | TIME, CHANNELS, SPACE | CHANNELS, SPACE | TIME | CHANNELS)
NAMES = {0: "none", SPACE: "space", SPACE | TIME: "spacetime", CHANNELS: "channels", SPACE | CHANNELS: "space+channels",
         SPACE | TIME | CHANNELS: "spacetime+channels"}
_thwc, _head, _f32 = vr._thwc, vr._head, vr._f32
rho, phi = vr.rho, vr.phi


def effective(coupling, pen, C):
    """the coupling that changes anything: SPACE and TIME not with p = 2, CHANNELS not on one channel and not with p = r = 2"""
    if coupling & TIME:
        assert coupling & SPACE and pen[0] == pen[1] and pen[3] == pen[4], "TIME comes with SPACE and is one penalty"
    if pen[0] == 2:
        coupling &= ~(SPACE | TIME)
    if C == 1 or (pen[0] == 2 and pen[1] == 2):
        coupling &= ~CHANNELS
    return coupling


def _forward(v, tper):
    """a temporal array at every frame's forward link, T frames (free time: the last frame has none, 0)"""
    return v if tper else np.concatenate([v, np.zeros((1,) + v.shape[1:], v.dtype)])


def _over_channels(m):
    s = m[..., 0]
    for k in range(1, m.shape[-1]):
        s = s + m[..., k]
    return np.repeat(s[..., None], m.shape[-1], -1)


def _any_channel(h):
    return np.repeat(h.any(-1)[..., None], h.shape[-1], -1)


def magnitudes(P, u, coupling, dtype=np.float32):
    """(M_x, M_y, M_t, has_x, has_y, has_t): the magnitude each x-link / y-link (T x H x W x C) and each temporal link (the temporal arrays'
    shape) shares, in dtype, and whether that magnitude has a live link at all (its owner then books its energy).  M_t is None where the
    temporal links keep their own penalty (neither TIME nor CHANNELS)."""
    lx, ly, lt_live = vw.live_links(*_head(P))
    cx, cy, lt = vr.base_links(P)
    tper = P["tper"]
    with np.errstate(invalid="ignore", over="ignore"):
        tx, ty, tt = vr.link_residuals(P, u, dtype)
        ax, ay, at = tx * tx, ty * ty, lt.astype(dtype) * (tt * tt)
        if P["sx"] is not None:
            ax = cx.astype(dtype) * ax
            ay = cy.astype(dtype) * ay
    zero = dtype(0)
    ax, ay, at = np.where(lx, ax, zero), np.where(ly, ay, zero), np.where(lt_live, at, zero)
    if coupling & TIME:
        m = (ax + ay) + _forward(at, tper)
        h = lx | ly | _forward(lt_live, tper)
        if coupling & CHANNELS:
            m, h = _over_channels(m), _any_channel(h)
        out = m, m, vw._here(m, tper), h, h, vw._here(h, tper)
    else:
        if coupling & SPACE:
            mx = my = ax + ay
            hx = hy = lx | ly
        else:
            mx, my, hx, hy = ax, ay, lx, ly
        mt, ht = None, lt_live
        if coupling & CHANNELS:
            mx, hx = _over_channels(mx), _any_channel(hx)
            my, hy = (mx, hx) if coupling & SPACE else (_over_channels(my), _any_channel(hy))
            mt, ht = _over_channels(at), _any_channel(lt_live)
        out = mx, my, mt, hx, hy, ht
    assert all(a is None or a.dtype == dtype for a in out[:3])
    return out


def reweigh(P, pen, u, coupling=0, dtype=np.float32):
    """(s_x, s_y, s_t, w') of the round after iterate u, float32; 1 in every link that is not live, w' None without weight"""
    base = vr.reweigh(P, pen, u, dtype)
    p, r, q, eg, et, ed = pen
    coupling = effective(coupling, pen, vw.kinds(*_head(P)[:2], P["state"]).shape[3])
    if not coupling:
        return base
    lx, ly, lt_live = vw.live_links(*_head(P))
    cx, cy, lt = vr.base_links(P)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        mx, my, mt, _, _, _ = magnitudes(P, u, coupling, dtype)
        sx = (cx.astype(dtype) * rc.rho_of(p, eg, mx, dtype)).astype(np.float32)
        sy = (cy.astype(dtype) * rc.rho_of(p, eg, my, dtype)).astype(np.float32)
        st = base[2] if mt is None else (lt.astype(dtype) * rc.rho_of(*((p, eg) if coupling & TIME else (r, et)), mt, dtype)).astype(np.float32)
    one = np.float32(1)
    return np.where(lx, sx, one), np.where(ly, sy, one), np.where(lt_live, st, one), base[3]


def round_args(P, pen=None, u=None, coupling=0, dtype=np.float32):
    """volume_wls_np's args of one round: the caller's system (u None), or the system that iterate u gives"""
    if u is None:
        return vr.round_args(P)
    sx, sy, smt, w = reweigh(P, pen, u, coupling, dtype)
    lap = vw.divergence(*_head(P), sx, sy, smt, 1.0, P["gx"], P["gy"], P["gt"])
    data = P["data"] if P["weight"] is not None else np.where(vw.kinds(*_head(P)[:2], P["state"]) == vw.UNKNOWN, np.float32(0), _f32(P["data"]))
    return _head(P) + (w, sx, sy, smt, 1.0, data, lap)


def energy(P, pen, u, coupling=0):
    """the energy of u per channel, float64 [C]; under CHANNELS the gradient-and-time term, one number for the volume, on channel 0"""
    p, r, q, eg, et, ed = pen
    k = vw.kinds(*_head(P)[:2], P["state"])
    C = k.shape[3]
    coupling = effective(coupling, pen, C)
    if not coupling:
        return vr.energy(P, pen, u)
    uu = _thwc(np.asarray(u, np.float64))
    per_channel = lambda a: a.reshape(-1, C).sum(0)
    with np.errstate(invalid="ignore"):
        mx, my, mt, hx, hy, ht = magnitudes(P, uu, coupling, np.float64)
        e = per_channel(np.where(hx, rc._psi(p, eg, mx), 0.0))
        if not coupling & SPACE:
            e = e + per_channel(np.where(hy, rc._psi(p, eg, my), 0.0))
        if not coupling & TIME:
            if mt is None:
                _, _, tt = vr.link_residuals(P, uu, np.float64)
                e = e + per_channel(np.where(ht, vr.base_links(P)[2].astype(np.float64) * phi(r, et, tt), 0.0))
            else:
                e = e + per_channel(np.where(ht, rc._psi(r, et, mt), 0.0))
        if coupling & CHANNELS:          # every channel holds the volume's magnitude: count it once
            e = np.concatenate([e[:1], np.zeros(C - 1)])
        if P["weight"] is not None:
            d = uu - _f32(P["data"]).astype(np.float64)
            e = e + per_channel(np.where(k == vw.UNKNOWN, _f32(P["weight"]).astype(np.float64) * phi(q, ed, d), 0.0))
    return e


def irls_exact(P, pen, rounds, coupling=0):
    """[u_0 .. u_rounds], float64 T x H x W x C: u_0 the quadratic solve, u_k the exact WLS volume solve with the links and weights of u_(k-1)"""
    out = [_thwc(vw.solve_exact(round_args(P), vr._boundary(P)))]
    for _ in range(rounds):
        if vr.quadratic(pen):
            break
        out.append(_thwc(vw.solve_exact(round_args(P, pen, out[-1], coupling, np.float64), vr._boundary(P))))
    return out


def irls_f32(probs, pen, rounds, coupling=0, tol=1e-5, max_iters=400):
    """The library's rounds in numpy for a chunk of problems (a dict: a chunk of one): per problem ([u_0 .. u_rounds] float32 T x H x W x C,
    [inner iterations of every round]); every round's means are the chunk's"""
    single = isinstance(probs, dict)
    probs = [probs] if single else list(probs)
    args0 = [round_args(P) for P in probs]
    means = vr.chunk_means(args0)
    us, its = [], []
    for P, a in zip(probs, args0):
        u0, it, _ = vw.pcg_f32(a, vr._boundary(P), tol=tol, max_iters=max_iters, means=means)
        us.append([_thwc(u0)])
        its.append([it])
    for _ in range(rounds):
        if vr.quadratic(pen):
            break
        args = [round_args(P, pen, u[-1], coupling) for P, u in zip(probs, us)]
        means = vr.chunk_means(args)
        for P, a, u, n in zip(probs, args, us, its):
            nxt, it = vr._warm_round(a, vr._boundary(P), means, u[-1], tol, max_iters)
            u.append(nxt)
            n.append(it)
    return (us[0], its[0]) if single else list(zip(us, its))


def round_residual(P, pen, u_prev, u, coupling=0):
    """RES of u in the WLS volume system that u_prev's links and weights give (u_prev None: the caller's system): max |L u - b| / max |b|
    over the UNKNOWN pixels, float64"""
    args = round_args(P) if u_prev is None else round_args(P, pen, u_prev, coupling)
    k = vw.kinds(*_head(P)[:2], P["state"])
    blk = (slice(None),) + vw.unknowns(P["sides"], P["periodic"], *k.shape[1:3])
    unk = (k == vw.UNKNOWN)[blk]
    b = vw.folded_rhs(*args, vr._boundary(P))
    r = vw.residual(args, u, vr._boundary(P))
    scale = float(np.abs(b[unk]).max()) if unk.any() else 0.0
    return float(np.abs(r[unk]).max()) / scale if scale > 0 else 0.0
