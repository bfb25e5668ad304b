"""The test side's restatement of the robust solve (sc_hip_robust*), numpy only, on top of tests/wls_np.py.

Per channel the library minimises, with exponents 0 < p, q <= 2,
    sum_unknowns w phi_q(u - d; eps_d) + sum_live x-links c_x phi_p(u(x+1,y) - u(x,y) - gx; eps_g) + sum_live y-links c_y phi_p(.. gy ..),
    phi_r(t; eps) = (2 / r) (t^2 + eps^2)^(r/2)          (r = 2: t^2, eps unused),
by iteratively reweighted least squares: round 0 is the WLS problem with links c and weights w, round k >= 1 the WLS problem with
    s = c rho_p(link residual),  w' = w rho_q(u - d),      rho_r(t) = (t^2 + eps^2)^((r-2)/2)       (r = 2: 1)
at round k - 1's iterate.  Images here are full H x W x C arrays (H x W accepted) that hold boundary's values on the Dirichlet lines, so
a link to a Dirichlet pixel takes boundary's value and np.roll gives the link across a periodic seam.  Borders are (sides, periodic) as
in wls_np; c_x = c_y = None stands for base links of 1.  Only live links (wls_np.live_links) and unknowns enter any result: the GPU tests
put NaN everywhere else.

rho(dtype=float32) is the library's float32 rule: t * t and eps * eps rounded on their own, then their sum; r = 1: 1 / sqrt of it (both
correctly rounded: the same bits as the device), any other r < 2: power(.., (r - 2) / 2), which may differ from the device's powf in
the last place.  energy() is float64 throughout.  irls_exact() runs the rounds in float64 with wls_np.solve_exact as its inner solve;
irls_f32() runs the library's rounds: float32 vectors, float64 dot products, round 0 from wls_np.pcg_f32's cold start, every later
round started from the previous iterate (r = b - L u, z = M^-1 r, p = z) under that round's own s-bar and w-bar -- the yardstick of
tests/robust_bounds.py."""
from __future__ import annotations

import numpy as np

import direct_np
import wls_np
import weighted_np

_hwc = wls_np._hwc


def rho(r, eps, t, dtype=np.float32):
    """rho_r(t) in dtype, t an array of that dtype"""
    t = np.asarray(t, dtype)
    if r == 2:
        return np.ones_like(t)
    e = dtype(eps)
    q = t * t + e * e
    if r == 1 and dtype == np.float32:
        return np.float32(1) / np.sqrt(q)
    return np.power(q, dtype((dtype(r) - dtype(2)) * dtype(0.5)))


def phi(r, eps, t):
    """phi_r(t; eps) in float64"""
    t = np.asarray(t, np.float64)
    return t * t if r == 2 else (2.0 / r) * np.power(t * t + float(eps) ** 2, r / 2.0)


def _ones_if_none(c, shape):
    return np.ones(shape, np.float32) if c is None else _hwc(np.asarray(c, np.float32))


def link_residuals(u, gx, gy, dtype=np.float32):
    """(t_x, t_y): (u(x+1,y) - u(x,y)) - gx and (u(x,y+1) - u(x,y)) - gy in dtype at every element (what is not live holds whatever the
    wrap gives)"""
    u = _hwc(np.asarray(u, dtype))
    return ((np.roll(u, -1, 1) - u) - _hwc(np.asarray(gx, np.float32)).astype(dtype),
            (np.roll(u, -1, 0) - u) - _hwc(np.asarray(gy, np.float32)).astype(dtype))


def reweigh(sides, periodic, p, q, eps_g, eps_d, weight, cx, cy, gx, gy, data, u, dtype=np.float32):
    """(s_x, s_y, w') of the round after iterate u, float32 H x W x C: NaN in every link that is not live"""
    w = _hwc(np.asarray(weight, np.float32))
    shape = w.shape
    lx, ly = wls_np.live_links(sides, periodic, *shape[:2])
    with np.errstate(invalid="ignore"):
        tx, ty = link_residuals(u, gx, gy, dtype)
        sx = (_ones_if_none(cx, shape).astype(dtype) * rho(p, eps_g, tx, dtype)).astype(np.float32)
        sy = (_ones_if_none(cy, shape).astype(dtype) * rho(p, eps_g, ty, dtype)).astype(np.float32)
        w2 = (w.astype(dtype) * rho(q, eps_d, _hwc(np.asarray(u, dtype)) - _hwc(np.asarray(data, np.float32)).astype(dtype), dtype)).astype(np.float32)
    nan = np.float32(np.nan)
    return np.where(lx[:, :, None], sx, nan), np.where(ly[:, :, None], sy, nan), w2


def energy(sides, periodic, p, q, eps_g, eps_d, weight, cx, cy, gx, gy, data, u):
    """the energy of u per channel, float64 [C]"""
    w = _hwc(np.asarray(weight, np.float32)).astype(np.float64)
    shape = w.shape
    H, W = shape[:2]
    lx, ly = wls_np.live_links(sides, periodic, H, W)
    unk = ~direct_np.dirichlet_mask(sides, periodic, H, W)
    uu = _hwc(np.asarray(u, np.float64))
    with np.errstate(invalid="ignore"):
        tx, ty = link_residuals(uu, gx, gy, np.float64)
        ex = _ones_if_none(cx, shape).astype(np.float64) * phi(p, eps_g, tx)
        ey = _ones_if_none(cy, shape).astype(np.float64) * phi(p, eps_g, ty)
    ed = w * phi(q, eps_d, uu - _hwc(np.asarray(data, np.float32)).astype(np.float64))
    return ed[unk].sum(0) + ex[lx].sum(0) + ey[ly].sum(0)


def _start_image(sides, periodic, boundary, shape):
    if wls_np.has_dirichlet(sides, periodic):
        return _hwc(np.asarray(boundary, np.float32))
    return None


def irls_exact(sides, periodic, p, q, eps_g, eps_d, weight, cx, cy, gx, gy, data, boundary, rounds):
    """[u_0 .. u_rounds], float64 H x W x C: u_0 the quadratic solve, u_k the exact WLS solve with the links and weights of u_(k-1)"""
    w = _hwc(np.asarray(weight, np.float32))
    d = _hwc(np.asarray(data, np.float32))
    b = _start_image(sides, periodic, boundary, w.shape)
    sx, sy, w2 = _ones_if_none(cx, w.shape), _ones_if_none(cy, w.shape), w
    out = []
    for k in range(rounds + 1):
        if k:
            sx, sy, w2 = reweigh(sides, periodic, p, q, eps_g, eps_d, w, cx, cy, gx, gy, d, out[-1], np.float64)
        lap = wls_np.divergence(sides, periodic, sx, sy, gx, gy)
        out.append(_hwc(wls_np.solve_exact(sides, periodic, w2, sx, sy, d, lap, b)))
        if p == 2 and q == 2:
            break
    return out


def _warm_pcg(b, apply, precond, u, tol, max_iters):
    """pcg_np.pcg_f32 started from u instead of M^-1 b: (u, iterations, the worst channel's final ||r|| / ||b||)"""
    dot = lambda a, c: np.einsum("yxc,yxc->c", a.astype(np.float64), c.astype(np.float64))
    bb = dot(b, b)
    rel = lambda r: float(np.sqrt(np.max(np.where(bb > 0, dot(r, r) / np.where(bb > 0, bb, 1.0), 0.0))))
    r = b - apply(u)
    z = precond(r)
    pp = z.copy()
    rz = dot(r, z)
    it = 0
    while rel(r) > tol and it < max_iters:
        qq = apply(pp)
        pq = dot(pp, qq)
        alpha = np.where(pq != 0, rz / np.where(pq != 0, pq, 1.0), 0.0).astype(np.float32)
        u = u + alpha * pp
        r = r - alpha * qq
        z = precond(r)
        rz_new = dot(r, z)
        beta = np.where(rz != 0, rz_new / np.where(rz != 0, rz, 1.0), 0.0).astype(np.float32)
        pp = z + beta * pp
        rz = rz_new
        it += 1
        assert u.dtype == np.float32 and pp.dtype == np.float32
    return u, it, rel(r)


def irls_f32(sides, periodic, p, q, eps_g, eps_d, weight, cx, cy, gx, gy, data, boundary, rounds, tol=1e-5, max_iters=400):
    """The library's rounds in numpy: ([u_0 .. u_rounds] float32 H x W x C, [inner iterations of every round])"""
    w = _hwc(np.asarray(weight, np.float32))
    d = _hwc(np.asarray(data, np.float32))
    H, W, C = w.shape
    b_img = _start_image(sides, periodic, boundary, w.shape)
    blk = wls_np.unknowns(sides, periodic, H, W)
    unk = ~direct_np.dirichlet_mask(sides, periodic, H, W)
    sx, sy = _ones_if_none(cx, w.shape), _ones_if_none(cy, w.shape)
    lap = wls_np.divergence(sides, periodic, sx, sy, gx, gy)
    u0, it, _ = wls_np.pcg_f32(sides, periodic, w, sx, sy, d, lap, b_img, tol=tol, max_iters=max_iters)
    us, its = [_hwc(u0)], [it]
    for k in range(1, rounds + 1):
        if p == 2 and q == 2:
            break
        sx, sy, w2 = reweigh(sides, periodic, p, q, eps_g, eps_d, w, cx, cy, gx, gy, d, us[-1])
        lap = wls_np.divergence(sides, periodic, sx, sy, gx, gy)
        full = wls_np._links(sides, periodic, sx, sy, np.float32)
        dg = (((full[0] + full[1]) + (full[2] + full[3])) + w2)[blk]
        links = tuple(np.where(np.roll(unk, shift, axis)[:, :, None], f, np.float32(0))[blk]
                      for f, shift, axis in zip(full, (1, -1, 1, -1), (1, 1, 0, 0)))
        lam = np.float32(wls_np.mean_weight(sides, periodic, w2) / wls_np.mean_link(sides, periodic, sx, sy))
        rhs = wls_np.folded_rhs(sides, periodic, w2, sx, sy, d, lap, b_img, np.float32)
        u, it, _ = _warm_pcg(rhs, lambda v: wls_np.block_operator(links, dg, v), lambda r: weighted_np._precond(sides, periodic, lam, r, (H, W, C)),
                             us[-1][blk], tol, max_iters)
        nxt = us[-1].copy()
        nxt[blk] = u
        us.append(nxt)
        its.append(it)
    return us, its


def round_residual(sides, periodic, p, q, eps_g, eps_d, weight, cx, cy, gx, gy, data, u_prev, u):
    """RES of u in the WLS system that u_prev's links and weights give: max |L u - rhs| / max |rhs|, float64"""
    sx, sy, w2 = reweigh(sides, periodic, p, q, eps_g, eps_d, weight, cx, cy, gx, gy, data, u_prev)
    lap = wls_np.divergence(sides, periodic, sx, sy, gx, gy)
    f = np.abs(wls_np.rhs(sides, periodic, w2, _hwc(np.asarray(data, np.float32)), lap).astype(np.float64)).max()
    return float(np.abs(wls_np.residual(sides, periodic, w2, sx, sy, _hwc(np.asarray(u)), _hwc(np.asarray(data, np.float32)), lap)).max()) / float(f)
