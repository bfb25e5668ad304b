"""The test side's restatement of the robust sub-pixel flow volume solve (sc_hip_volume_subflow_robust*), numpy only: the rounds of
tests/volume_robust_np.py around the system of tests/volume_subflow_np.py.

Per channel the library minimises over the UNKNOWN pixels of all frames
    sum w phi_q(u - d) + sum_live x-links c_x phi_p(dx u - gx) + sum_live y-links c_y phi_p(dy u - gy)
                       + sum_(live links p) c_t(p) phi_r(sum_k b_k(p) u~(q_k(p)) - u~(p) - gt(p)),
c_t = tau * smooth_t rounded once and gt stored at the link's source p, u~ = u at an UNKNOWN pixel and data at a KNOWN one, by
iteratively reweighted least squares: round 0 is the sub-pixel volume problem with the caller's links and weights, round k >= 1 the
sub-pixel volume problem with s = c rho(link residual) on every live link and w' = w rho_q(u - d) at round k - 1's iterate.

A problem travels as volume_robust_np's dict with two more fields: flow, and links = (idx, b) as volume_subflow_np.taps makes them of
it.  An iterate is composed like the library's out, so its work-rectangle block IS u~ wherever a live link has a point.  The spatial
links and the data weights of a round are volume_robust_np.reweigh's.  The temporal ones are lt * rho_r(t), t = (hi - u~(p)) - gt(p)
with hi = sum_k b_k u~(q_k) accumulated in the iterate's dtype in tap order 0..3 (volume_subflow_np._B: the same operations in the
same order as the kernel's), on the work rectangle where volume_subflow_np._held_live is true; they go into volume_subflow_np as a
smooth_t array (1 wherever no live link has its source) with tau = 1: 1 * smt is exact, and with r = 2 rho is 1 and the array holds
the base weight lt in every round.  A round's system is volume_subflow_np's -- divergence, folded_rhs, _planes, block_operator,
precond_means, assemble -- under the straight-link preconditioner; round 0 is volume_subflow_np.pcg_f32's cold start, every later
round the float32 iteration started warm from the previous iterate (robust_np._warm_pcg) under that round's own means.

With a flow of zeros energy() and the float64 rounds are volume_robust_np's on an input whose temporal links are all straight, to
float64 rounding (tests/test_volume_subflow_robust_host.py)."""
from __future__ import annotations

import numpy as np

import robust_np
import volume_np
import volume_robust_np as vr
import volume_subflow_np as vs
import volume_wls_np as vw
import weighted_np

rho, phi = robust_np.rho, robust_np.phi
_thwc = vw._thwc
UNKNOWN, KNOWN = vw.UNKNOWN, vw.KNOWN
quadratic = vr.quadratic
_head, _f32, _boundary = vr._head, vr._f32, vr._boundary


def _time_residuals(P, u, dtype):
    """(hi - u~) - gt on the work rectangle, T x ny x nx x C in dtype (what holds no live link: whatever the gathers give), the base
    links lt there in float32 (0 where the held link is not live) and where it is live"""
    sides, periodic, tper, state = _head(P)
    k = vw.kinds(sides, periodic, state)
    ub = vs._blk(sides, periodic, _thwc(np.asarray(u, dtype)))
    tt = vs._B(P["links"], ub)
    if P["gt"] is not None:
        tt = tt - vs._pad(vs._blk(sides, periodic, _f32(P["gt"])), k.shape[0]).astype(dtype)
    lt = vs._lt(sides, periodic, tper, k, P["smt"], P["tau"], P["links"])
    return tt, lt, vs._held_live(vs._blk(sides, periodic, k), P["links"])


def reweigh(P, pen, u, dtype=np.float32):
    """(s_x, s_y, s_t, w') of the round after iterate u, float32; 1 in every link that is not live (s_t: in smooth_t's shape, a link at
    its source), w' None without weight"""
    sx, sy, _, w2 = vr.reweigh(P, pen, u, dtype)
    sides, periodic, tper, state = _head(P)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        tt, lt, live = _time_residuals(P, u, dtype)
        st = (lt.astype(dtype) * rho(pen[1], pen[4], tt, dtype)).astype(np.float32)
    T, H, W = sx.shape[:3]
    full = np.ones(sx.shape, np.float32)
    full[(slice(None),) + vw.unknowns(sides, periodic, H, W)] = np.where(live, st, np.float32(1))
    return sx, sy, full[:T if tper else T - 1], w2


def round_args(P, pen=None, u=None, dtype=np.float32):
    """volume_subflow_np's args of one round: the caller's system (u None), or the system that iterate u gives"""
    if u is None:
        sx, sy, smt, w, tau = P["sx"], P["sy"], P["smt"], P["weight"], P["tau"]
    else:
        sx, sy, smt, w = reweigh(P, pen, u, dtype)
        tau = 1.0
    lap = vs.divergence(*_head(P), sx, sy, smt, tau, P["gx"], P["gy"], P["gt"], P["links"])
    data = P["data"] if P["weight"] is not None else np.where(vw.kinds(*_head(P)[:2], P["state"]) == UNKNOWN, np.float32(0), _f32(P["data"]))
    return _head(P) + (w, sx, sy, smt, tau, data, lap)


def energy(P, pen, u):
    """the energy of u per channel, float64 [C]"""
    p, r, q, eg, et, ed = pen
    k = vw.kinds(*_head(P)[:2], P["state"])
    lx, ly, _ = vw.live_links(*_head(P))
    cx, cy, _ = (a.astype(np.float64) for a in vr.base_links(P))
    uu = _thwc(np.asarray(u, np.float64))
    C = k.shape[3]
    with np.errstate(invalid="ignore"):
        tx, ty, _ = vr.link_residuals(P, uu, np.float64)
        tt, lt, live = _time_residuals(P, uu, np.float64)
        e = np.where(lx, cx * phi(p, eg, tx), 0.0).reshape(-1, C).sum(0) + np.where(ly, cy * phi(p, eg, ty), 0.0).reshape(-1, C).sum(0)
        e = e + np.where(live, lt.astype(np.float64) * phi(r, et, tt), 0.0).reshape(-1, C).sum(0)
        if P["weight"] is not None:
            d = uu - _f32(P["data"]).astype(np.float64)
            e = e + np.where(k == UNKNOWN, _f32(P["weight"]).astype(np.float64) * phi(q, ed, d), 0.0).reshape(-1, C).sum(0)
    return e


def irls_exact(P, pen, rounds):
    """[u_0 .. u_rounds], float64 T x H x W x C: u_0 the quadratic solve, u_k the exact sub-pixel volume solve with the links and weights of u_(k-1)"""
    out = [_thwc(vs.solve_exact(round_args(P), P["links"], _boundary(P)))]
    for _ in range(rounds):
        if quadratic(pen):
            break
        out.append(_thwc(vs.solve_exact(round_args(P, pen, out[-1], np.float64), P["links"], _boundary(P))))
    return out


def chunk_means(all_args, all_links):
    """(s-bar, tau-bar, w-bar) as the library takes them for a chunk of systems: every mean over all its members' live links or UNKNOWN pixels"""
    m = [vs.precond_means(a, l) for a, l in zip(all_args, all_links)]
    if len(m) == 1:
        return m[0][:3]
    ns, nt, nu = (sum(c[3][i] for c in m) for i in range(3))
    first = all_args[0]
    sbar = sum(c[0] * c[3][0] for c in m) / ns if ns and first[5] is not None else 1.0
    tbar = sum(c[1] * c[3][1] for c in m) / nt if nt and first[7] is not None else float(np.float32(first[8]))
    return sbar, tbar, (sum(c[2] * c[3][2] for c in m) / nu if nu else 1.0)


def _warm_round(args, links, boundary, means, u, tol, max_iters):
    """one warm-started float32 solve of the system args from the composed iterate u: (the next composed iterate, iterations, rel)"""
    sides, periodic, tper, state, weight, sx, sy, smt, tau, data, lap = args
    k = vw.kinds(sides, periodic, state)
    T, H, W, C = k.shape
    blk = (slice(None),) + vw.unknowns(sides, periodic, H, W)
    planes = vs._planes(args, links, np.float32)
    sbar, tbar, wbar = means
    D = vw.time_table(T, tper).astype(np.float32)
    shifts = vw.mode_shifts(T, wbar, tbar, sbar, tper)
    b = vs.folded_rhs(args, links, boundary, np.float32)
    _, ny, nx, _ = b.shape
    tall = lambda a: a.reshape(T * ny, nx, C)
    frames = lambda a: a.reshape(T, ny, nx, C)

    def precond(r):
        X = np.einsum("kt,tyxc->kyxc", D, frames(r))
        Z = np.stack([weighted_np._precond(sides, periodic, shifts[m], X[m], (H, W, C), np.float32) for m in range(T)])
        return tall(np.einsum("kt,kyxc->tyxc", D, Z).astype(np.float32))

    start = np.where(k[blk] == UNKNOWN, _thwc(np.asarray(u, np.float32))[blk], np.float32(0))
    x, it, rel = robust_np._warm_pcg(tall(b), lambda v: tall(vs.block_operator(planes, frames(v), links)), precond, tall(start), tol, max_iters)
    return _thwc(volume_np._compose(sides, periodic, state, data, boundary, frames(x), np.float32)), it, rel


def irls_f32(probs, pen, rounds, tol=1e-5, max_iters=400, rels=None):
    """The library's rounds in numpy for a chunk of problems (a dict: a chunk of one): per problem ([u_0 .. u_rounds] float32 T x H x W x C,
    [inner iterations of every round]); every round's means are the chunk's.  rels: a list that takes every inner solve's final
    ||r|| / ||b||, round by round and problem by problem."""
    single = isinstance(probs, dict)
    probs = [probs] if single else list(probs)
    links = [P["links"] for P in probs]
    args0 = [round_args(P) for P in probs]
    means = chunk_means(args0, links)
    us, its = [], []
    for P, a in zip(probs, args0):
        u0, it, rel = vs.pcg_f32(a, P["links"], _boundary(P), tol=tol, max_iters=max_iters, means=means)
        us.append([_thwc(u0)])
        its.append([it])
        if rels is not None:
            rels.append(rel)
    for _ in range(rounds):
        if quadratic(pen):
            break
        args = [round_args(P, pen, u[-1]) for P, u in zip(probs, us)]
        means = chunk_means(args, links)
        for P, a, u, n in zip(probs, args, us, its):
            nxt, it, rel = _warm_round(a, P["links"], _boundary(P), means, u[-1], tol, max_iters)
            u.append(nxt)
            n.append(it)
            if rels is not None:
                rels.append(rel)
    return (us[0], its[0]) if single else list(zip(us, its))


def round_residual(P, pen, u_prev, u):
    """RES of u in the sub-pixel volume system that u_prev's links and weights give (u_prev None: the caller's system): max |L u - b| /
    max |b| over the UNKNOWN pixels, float64"""
    args = round_args(P, pen, u_prev)
    k = vw.kinds(*_head(P)[:2], P["state"])
    blk = (slice(None),) + vw.unknowns(P["sides"], P["periodic"], *k.shape[1:3])
    unk = (k == UNKNOWN)[blk]
    b = vs.folded_rhs(args, P["links"], _boundary(P))
    r = vs.residual(args, P["links"], u, _boundary(P))
    scale = float(np.abs(b[unk]).max())
    return float(np.abs(r[unk]).max()) / scale if scale > 0 else 0.0
