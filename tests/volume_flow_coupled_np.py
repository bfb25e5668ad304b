"""The test side's restatement of the coupled flow volume solve (sc_hip_volume_flow_coupled*), numpy only: the magnitudes of
tests/volume_coupled_np.py with every temporal link taken through (fwd, bwd) as tests/volume_flow_robust_np.py takes it, around the
system of tests/volume_flow_np.py.

coupling is volume_coupled_np's sum of SPACE, TIME and CHANNELS.  The owner of a temporal link is its SOURCE, the pixel i that holds the
matched link i -> fwd[i]: its share a_t = lt t^2, t = (u[fwd[i]] - u[i]) - gt(i), lt = tau * smooth_t rounded once, sits at i's own
element.  Under SPACE | TIME a pixel's magnitude is (a_x + a_y) + a_t with a_t of the link it holds; a pixel that holds no live link
(occluded, the loser of a collision, its target off the rectangle, a dead end) has a_t = 0, and a link that arrives at a pixel plays no
part in that pixel's magnitude.  Under CHANNELS a magnitude is the running sum over the channels in which the link is live: the
matching is per volume, liveness per channel.  Without CHANNELS and without TIME a temporal link keeps volume_flow_robust_np's own
penalty c_t phi_r(t).  s = c rho(M); a temporal link's s goes into volume_flow_np as a smooth_t array at its source with tau = 1.

A problem travels as volume_flow_robust_np's dict (flow and links = (fwd, bwd) among its fields), the penalties as pen = (p, r, q,
eps_g, eps_t, eps_d).  Temporal arrays have the shape of smooth_t / gt (T - 1 frames, periodic time: T), a link at its source.  With
no effective coupling every function returns volume_flow_robust_np's arrays themselves; with a flow of zeros every function returns
volume_coupled_np's arrays exactly (tests/test_volume_flow_coupled_host.py)."""
from __future__ import annotations

import numpy as np

import robust_coupled_np as rc
import volume_coupled_np as vc
import volume_flow_np as vf
import volume_flow_robust_np as vfr
import volume_robust_np as vr
import volume_wls_np as vw

SPACE, TIME, CHANNELS = vc.SPACE, vc.TIME, vc.CHANNELS
LEGAL, NAMES, effective = vc.LEGAL, vc.NAMES, vc.effective
_thwc, _head, _f32, _boundary = vr._thwc, vr._head, vr._f32, vr._boundary
rho, phi = vr.rho, vr.phi
_over_channels, _any_channel = vc._over_channels, vc._any_channel


def _channels(P):
    return vw.kinds(*_head(P)[:2], P["state"]).shape[3]


def _embed(P, a, fill):
    """a (T x ny x nx x C, the work rectangle) inside a T x H x W x C array of `fill`"""
    sides, periodic, _, state = _head(P)
    T, H, W, C = vw.kinds(sides, periodic, state).shape
    full = np.full((T, H, W, C), fill, a.dtype)
    full[(slice(None),) + vw.unknowns(sides, periodic, H, W)] = a
    return full


def _temporal(P, full):
    """a T-frame array of values at the links' sources in the temporal arrays' shape (free time: frame T - 1 holds no link)"""
    return full if P["tper"] else full[:-1]


def time_shares(P, u, dtype=np.float32):
    """(a_t, lt, live), T x H x W x C: the share lt t^2 of the link every pixel holds in dtype (0 where it holds no live link), its base
    weight in float32 (0 likewise) and whether it is live"""
    with np.errstate(invalid="ignore", over="ignore"):
        tt, lt, live = vfr._time_residuals(P, u, dtype)
        at = np.where(live, lt.astype(dtype) * (tt * tt), dtype(0))
    return _embed(P, at, dtype(0)), _embed(P, lt, np.float32(0)), _embed(P, live, False)


def magnitudes(P, u, coupling, dtype=np.float32):
    """volume_coupled_np.magnitudes with the temporal links through the matching: (M_x, M_y, M_t, has_x, has_y, has_t), M_t and has_t in
    the temporal arrays' shape with a link at its source; M_t None where the temporal links keep their own penalty"""
    lx, ly, _ = vw.live_links(*_head(P))
    cx, cy, _ = vr.base_links(P)
    with np.errstate(invalid="ignore", over="ignore"):
        tx, ty, _ = vr.link_residuals(P, u, dtype)
        ax, ay = tx * tx, ty * ty
        if P["sx"] is not None:
            ax = cx.astype(dtype) * ax
            ay = cy.astype(dtype) * ay
    at, _, lt_live = time_shares(P, _thwc(np.asarray(u, dtype)), dtype)
    zero = dtype(0)
    ax, ay = np.where(lx, ax, zero), np.where(ly, ay, zero)
    if coupling & TIME:
        m = (ax + ay) + at
        h = lx | ly | lt_live
        if coupling & CHANNELS:
            m, h = _over_channels(m), _any_channel(h)
        out = m, m, _temporal(P, m), h, h, _temporal(P, h)
    else:
        if coupling & SPACE:
            mx = my = ax + ay
            hx = hy = lx | ly
        else:
            mx, my, hx, hy = ax, ay, lx, ly
        mt, ht = None, _temporal(P, lt_live)
        if coupling & CHANNELS:
            mx, hx = _over_channels(mx), _any_channel(hx)
            my, hy = (mx, hx) if coupling & SPACE else (_over_channels(my), _any_channel(hy))
            mt, ht = _over_channels(_temporal(P, at)), _any_channel(_temporal(P, lt_live))
        out = mx, my, mt, hx, hy, ht
    assert all(a is None or a.dtype == dtype for a in out[:3])
    return out


def reweigh(P, pen, u, coupling=0, dtype=np.float32):
    """(s_x, s_y, s_t, w') of the round after iterate u, float32; 1 in every link that is not live (s_t: in smooth_t's shape, a link at
    its source), w' None without weight"""
    base = vfr.reweigh(P, pen, u, dtype)
    p, r, q, eg, et, ed = pen
    coupling = effective(coupling, pen, _channels(P))
    if not coupling:
        return base
    lx, ly, _ = vw.live_links(*_head(P))
    cx, cy, _ = vr.base_links(P)
    _, lt, lt_live = (_temporal(P, a) for a in time_shares(P, _thwc(np.asarray(u, dtype)), dtype))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        mx, my, mt, _, _, _ = magnitudes(P, u, coupling, dtype)
        sx = (cx.astype(dtype) * rc.rho_of(p, eg, mx, dtype)).astype(np.float32)
        sy = (cy.astype(dtype) * rc.rho_of(p, eg, my, dtype)).astype(np.float32)
        st = base[2] if mt is None else (lt.astype(dtype) * rc.rho_of(*((p, eg) if coupling & TIME else (r, et)), mt, dtype)).astype(np.float32)
    one = np.float32(1)
    return np.where(lx, sx, one), np.where(ly, sy, one), np.where(lt_live, st, one), base[3]


def round_args(P, pen=None, u=None, coupling=0, dtype=np.float32):
    """volume_flow_np's args of one round: the caller's system (u None), or the system that iterate u gives"""
    if u is None:
        return vfr.round_args(P)
    sx, sy, smt, w = reweigh(P, pen, u, coupling, dtype)
    lap = vf.divergence(*_head(P), sx, sy, smt, 1.0, P["gx"], P["gy"], P["gt"], P["links"])
    data = P["data"] if P["weight"] is not None else np.where(vw.kinds(*_head(P)[:2], P["state"]) == vw.UNKNOWN, np.float32(0), _f32(P["data"]))
    return _head(P) + (w, sx, sy, smt, 1.0, data, lap)


def energy(P, pen, u, coupling=0):
    """the energy of u per channel, float64 [C]; under CHANNELS the gradient-and-time term, one number for the volume, on channel 0"""
    p, r, q, eg, et, ed = pen
    k = vw.kinds(*_head(P)[:2], P["state"])
    C = k.shape[3]
    coupling = effective(coupling, pen, C)
    if not coupling:
        return vfr.energy(P, pen, u)
    uu = _thwc(np.asarray(u, np.float64))
    per_channel = lambda a: a.reshape(-1, C).sum(0)
    with np.errstate(invalid="ignore"):
        mx, my, mt, hx, hy, ht = magnitudes(P, uu, coupling, np.float64)
        e = per_channel(np.where(hx, rc._psi(p, eg, mx), 0.0))
        if not coupling & SPACE:
            e = e + per_channel(np.where(hy, rc._psi(p, eg, my), 0.0))
        if not coupling & TIME:
            if mt is None:
                tt, lt, live = vfr._time_residuals(P, uu, np.float64)
                own = _embed(P, np.where(live, lt.astype(np.float64) * phi(r, et, tt), 0.0), 0.0)
                e = e + per_channel(_temporal(P, own))
            else:
                e = e + per_channel(np.where(ht, rc._psi(r, et, mt), 0.0))
        if coupling & CHANNELS:          # every channel holds the volume's magnitude: count it once
            e = np.concatenate([e[:1], np.zeros(C - 1)])
        if P["weight"] is not None:
            d = uu - _f32(P["data"]).astype(np.float64)
            e = e + per_channel(np.where(k == vw.UNKNOWN, _f32(P["weight"]).astype(np.float64) * phi(q, ed, d), 0.0))
    return e


def irls_exact(P, pen, rounds, coupling=0):
    """[u_0 .. u_rounds], float64 T x H x W x C: u_0 the quadratic solve, u_k the exact flow volume solve with the links and weights of u_(k-1)"""
    out = [_thwc(vf.solve_exact(round_args(P), P["links"], _boundary(P)))]
    for _ in range(rounds):
        if vr.quadratic(pen):
            break
        out.append(_thwc(vf.solve_exact(round_args(P, pen, out[-1], coupling, np.float64), P["links"], _boundary(P))))
    return out


def irls_f32(probs, pen, rounds, coupling=0, tol=1e-5, max_iters=400, rels=None):
    """The library's rounds in numpy for a chunk of problems (a dict: a chunk of one): per problem ([u_0 .. u_rounds] float32 T x H x W x C,
    [inner iterations of every round]); every round's means are the chunk's, a temporal link counted once at its source.  rels: a list
    that takes every inner solve's final ||r|| / ||b||, round by round and problem by problem."""
    single = isinstance(probs, dict)
    probs = [probs] if single else list(probs)
    links = [P["links"] for P in probs]
    args0 = [round_args(P) for P in probs]
    means = vfr.chunk_means(args0, links)
    us, its = [], []
    for P, a in zip(probs, args0):
        u0, it, rel = vf.pcg_f32(a, P["links"], _boundary(P), tol=tol, max_iters=max_iters, means=means)
        us.append([_thwc(u0)])
        its.append([it])
        if rels is not None:
            rels.append(rel)
    for _ in range(rounds):
        if vr.quadratic(pen):
            break
        args = [round_args(P, pen, u[-1], coupling) for P, u in zip(probs, us)]
        means = vfr.chunk_means(args, links)
        for P, a, u, n in zip(probs, args, us, its):
            nxt, it, rel = vfr._warm_round(a, P["links"], _boundary(P), means, u[-1], tol, max_iters)
            u.append(nxt)
            n.append(it)
            if rels is not None:
                rels.append(rel)
    return (us[0], its[0]) if single else list(zip(us, its))


def round_residual(P, pen, u_prev, u, coupling=0):
    """RES of u in the flow volume system that u_prev's links and weights give (u_prev None: the caller's system): max |L u - b| /
    max |b| over the UNKNOWN pixels, float64"""
    args = round_args(P, pen, u_prev, coupling)
    k = vw.kinds(*_head(P)[:2], P["state"])
    blk = (slice(None),) + vw.unknowns(P["sides"], P["periodic"], *k.shape[1:3])
    unk = (k == vw.UNKNOWN)[blk]
    b = vf.folded_rhs(args, P["links"], _boundary(P))
    r = vf.residual(args, P["links"], u, _boundary(P))
    scale = float(np.abs(b[unk]).max()) if unk.any() else 0.0
    return float(np.abs(r[unk]).max()) / scale if scale > 0 else 0.0
