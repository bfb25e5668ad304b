"""The test side's restatement of the robust solve's coupled gradient terms (SC_ROBUST_ISOTROPIC, SC_ROBUST_JOINT_CHANNELS), numpy only,
on top of tests/robust_np.py and tests/wls_np.py.

coupling is 0, ISO, JOINT or ISO | JOINT.  The owner of a link is its low end: element [y, x] of gx / smooth_x is the x-link that pixel
(x, y) owns, of gy / smooth_y its y-link (the last column / row: the wrapped link of a periodic axis).  With t = (u_hi - u_lo) - g of a
live link on channel k and a = c t^2 (c the base link, 1 without), the gradient term is
    0            sum_links c phi_p(t)                                          robust_np's, to the byte: every function here hands over to it
    ISO          sum_k sum_pixels psi_p(a_x + a_y)
    JOINT        sum_x-links psi_p(sum_k a_x) + sum_y-links psi_p(sum_k a_y)
    ISO | JOINT  sum_pixels psi_p(sum_k (a_x + a_y)),               psi_p(M) = (2 / p) (M + eps^2)^(p/2)      (p = 2: M)
a dead link contributes 0 and a pixel without a live forward link nothing.  The data term is robust_np's.  A round solves the WLS
system with s = c rho_p(M) on every link that shares M, rho_p(M) = (M + eps^2)^((p-2)/2).

magnitudes(dtype=float32) is the library's rule: t t rounded, times c rounded (no base links: no multiply), a_x + a_y within a pixel,
then the running sum over the channels 0 .. C - 1; rho: Q = M + eps eps, 1 / sqrt(Q) for p = 1 (correctly rounded: the device's bits),
power(Q, (p - 2) / 2) otherwise (may differ from the device's powf in the last place); s = c rho rounded.  energy() is float64 and books
a joint form's gradient energy -- one number per image -- on channel 0.  irls_exact / irls_f32 / round_residual are robust_np's with
this module's reweigh."""
from __future__ import annotations

import numpy as np

import direct_np
import robust_np
import weighted_np
import wls_np

ISO, JOINT = 1, 2
COUPLINGS = (0, ISO, JOINT, ISO | JOINT)
NAMES = {0: "aniso", ISO: "iso", JOINT: "joint", ISO | JOINT: "vectorial"}

_hwc = wls_np._hwc


def magnitudes(sides, periodic, cx, cy, gx, gy, u, coupling, dtype=np.float32):
    """(M_x, M_y), H x W x C in dtype: the magnitude that each x-link / y-link shares (what is not live: whatever its live partners give)"""
    u = _hwc(np.asarray(u, dtype))
    H, W, C = u.shape
    lx, ly = wls_np.live_links(sides, periodic, H, W)
    with np.errstate(invalid="ignore"):
        tx, ty = robust_np.link_residuals(u, gx, gy, dtype)
        ax, ay = tx * tx, ty * ty
        if cx is not None:
            ax = _hwc(np.asarray(cx, np.float32)).astype(dtype) * ax
            ay = _hwc(np.asarray(cy, np.float32)).astype(dtype) * ay
    ax = np.where(lx[:, :, None], ax, dtype(0))
    ay = np.where(ly[:, :, None], ay, dtype(0))
    if coupling & ISO:
        mx = my = ax + ay
    else:
        mx, my = ax, ay
    if coupling & JOINT:
        def over_channels(m):
            s = m[:, :, 0]
            for k in range(1, C):
                s = s + m[:, :, k]
            return np.repeat(s[:, :, None], C, 2)
        mx = over_channels(mx)
        my = mx if coupling & ISO else over_channels(my)
    assert mx.dtype == dtype and my.dtype == dtype
    return mx, my


def rho_of(p, eps, m, dtype=np.float32):
    """rho_p(M) in dtype"""
    if p == 2:
        return np.ones_like(m)
    e = dtype(eps)
    q = m + e * e
    if p == 1 and dtype == np.float32:
        return np.float32(1) / np.sqrt(q)
    return np.power(q, dtype((dtype(p) - dtype(2)) * dtype(0.5)))


def reweigh(sides, periodic, p, q, eps_g, eps_d, weight, cx, cy, gx, gy, data, u, coupling=0, dtype=np.float32):
    """(s_x, s_y, w') of the round after iterate u, float32 H x W x C: NaN in every link that is not live"""
    base = robust_np.reweigh(sides, periodic, p, q, eps_g, eps_d, weight, cx, cy, gx, gy, data, u, dtype)
    if not coupling:
        return base
    shape = base[2].shape
    lx, ly = wls_np.live_links(sides, periodic, *shape[:2])
    mx, my = magnitudes(sides, periodic, cx, cy, gx, gy, u, coupling, dtype)
    with np.errstate(invalid="ignore"):
        sx = (robust_np._ones_if_none(cx, shape).astype(dtype) * rho_of(p, eps_g, mx, dtype)).astype(np.float32)
        sy = (robust_np._ones_if_none(cy, shape).astype(dtype) * rho_of(p, eps_g, my, dtype)).astype(np.float32)
    nan = np.float32(np.nan)
    return np.where(lx[:, :, None], sx, nan), np.where(ly[:, :, None], sy, nan), base[2]


def _psi(p, eps, m):
    return m if p == 2 else (2.0 / p) * np.power(m + float(eps) ** 2, p / 2.0)


def energy(sides, periodic, p, q, eps_g, eps_d, weight, cx, cy, gx, gy, data, u, coupling=0):
    """the energy of u, float64 [C]: per channel; a joint form's gradient term, one number for the image, on channel 0"""
    if not coupling:
        return robust_np.energy(sides, periodic, p, q, eps_g, eps_d, weight, cx, cy, gx, gy, data, u)
    w = _hwc(np.asarray(weight, np.float32)).astype(np.float64)
    H, W, C = w.shape
    lx, ly = wls_np.live_links(sides, periodic, H, W)
    unk = ~direct_np.dirichlet_mask(sides, periodic, H, W)
    uu = _hwc(np.asarray(u, np.float64))
    ed = w * robust_np.phi(q, eps_d, uu - _hwc(np.asarray(data, np.float32)).astype(np.float64))
    mx, my = magnitudes(sides, periodic, cx, cy, gx, gy, uu, coupling, np.float64)
    if coupling & ISO:
        eg = _psi(p, eps_g, mx)[lx | ly].sum(0)
    else:
        eg = _psi(p, eps_g, mx)[lx].sum(0) + _psi(p, eps_g, my)[ly].sum(0)
    if coupling & JOINT:          # every channel holds the image's magnitude: count it once
        eg = np.concatenate([eg[:1], np.zeros(C - 1)])
    return ed[unk].sum(0) + eg


def irls_exact(sides, periodic, p, q, eps_g, eps_d, weight, cx, cy, gx, gy, data, boundary, rounds, coupling=0):
    """[u_0 .. u_rounds], float64 H x W x C: u_0 the quadratic solve, u_k the exact WLS solve with the links and weights of u_(k-1)"""
    w = _hwc(np.asarray(weight, np.float32))
    d = _hwc(np.asarray(data, np.float32))
    b = robust_np._start_image(sides, periodic, boundary, w.shape)
    sx, sy, w2 = robust_np._ones_if_none(cx, w.shape), robust_np._ones_if_none(cy, w.shape), w
    out = []
    for k in range(rounds + 1):
        if k:
            sx, sy, w2 = reweigh(sides, periodic, p, q, eps_g, eps_d, w, cx, cy, gx, gy, d, out[-1], coupling, np.float64)
        lap = wls_np.divergence(sides, periodic, sx, sy, gx, gy)
        out.append(_hwc(wls_np.solve_exact(sides, periodic, w2, sx, sy, d, lap, b)))
        if p == 2 and q == 2:
            break
    return out


def irls_f32(sides, periodic, p, q, eps_g, eps_d, weight, cx, cy, gx, gy, data, boundary, rounds, coupling=0, tol=1e-5, max_iters=400):
    """The library's rounds in numpy: ([u_0 .. u_rounds] float32 H x W x C, [inner iterations of every round])"""
    if not coupling:
        return robust_np.irls_f32(sides, periodic, p, q, eps_g, eps_d, weight, cx, cy, gx, gy, data, boundary, rounds, tol, max_iters)
    w = _hwc(np.asarray(weight, np.float32))
    d = _hwc(np.asarray(data, np.float32))
    H, W, C = w.shape
    b_img = robust_np._start_image(sides, periodic, boundary, w.shape)
    blk = wls_np.unknowns(sides, periodic, H, W)
    unk = ~direct_np.dirichlet_mask(sides, periodic, H, W)
    sx, sy = robust_np._ones_if_none(cx, w.shape), robust_np._ones_if_none(cy, w.shape)
    lap = wls_np.divergence(sides, periodic, sx, sy, gx, gy)
    u0, it, _ = wls_np.pcg_f32(sides, periodic, w, sx, sy, d, lap, b_img, tol=tol, max_iters=max_iters)
    us, its = [_hwc(u0)], [it]
    for k in range(1, rounds + 1):
        if p == 2 and q == 2:
            break
        sx, sy, w2 = reweigh(sides, periodic, p, q, eps_g, eps_d, w, cx, cy, gx, gy, d, us[-1], coupling)
        lap = wls_np.divergence(sides, periodic, sx, sy, gx, gy)
        full = wls_np._links(sides, periodic, sx, sy, np.float32)
        dg = (((full[0] + full[1]) + (full[2] + full[3])) + w2)[blk]
        links = tuple(np.where(np.roll(unk, shift, axis)[:, :, None], f, np.float32(0))[blk]
                      for f, shift, axis in zip(full, (1, -1, 1, -1), (1, 1, 0, 0)))
        lam = np.float32(wls_np.mean_weight(sides, periodic, w2) / wls_np.mean_link(sides, periodic, sx, sy))
        rhs = wls_np.folded_rhs(sides, periodic, w2, sx, sy, d, lap, b_img, np.float32)
        u, it, _ = robust_np._warm_pcg(rhs, lambda v: wls_np.block_operator(links, dg, v),
                                       lambda r: weighted_np._precond(sides, periodic, lam, r, (H, W, C)), us[-1][blk], tol, max_iters)
        nxt = us[-1].copy()
        nxt[blk] = u
        us.append(nxt)
        its.append(it)
    return us, its


def round_residual(sides, periodic, p, q, eps_g, eps_d, weight, cx, cy, gx, gy, data, u_prev, u, coupling=0):
    """RES of u in the WLS system that u_prev's links and weights give: max |L u - rhs| / max |rhs|, float64"""
    sx, sy, w2 = reweigh(sides, periodic, p, q, eps_g, eps_d, weight, cx, cy, gx, gy, data, u_prev, coupling)
    lap = wls_np.divergence(sides, periodic, sx, sy, gx, gy)
    d = _hwc(np.asarray(data, np.float32))
    f = np.abs(wls_np.rhs(sides, periodic, w2, d, lap).astype(np.float64)).max()
    return float(np.abs(wls_np.residual(sides, periodic, w2, sx, sy, _hwc(np.asarray(u)), d, lap)).max()) / float(f)
