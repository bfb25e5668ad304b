"""The library's preconditioned conjugate gradients in numpy, once for every family (weighted_np, wls_np): what a family brings is its
right-hand side, its operator, its preconditioner and a factor on the start -- what PcgOperator abstracts in the library.  pcg() is the
iteration with the vectors' dtype as a parameter: float32 is the library's arithmetic (pcg_f32), float64 its twin -- the same start and
the same steps without the vectors' rounding, the yardstick of single iterates (tests/pcg_steps_bounds.py)."""
import numpy as np


def pcg(b, apply, precond, u0_scale, tol, max_iters, out, blk, dtype=np.float32, keep=None):
    """Conjugate gradients on L u = b on the unknown block [ny][nx][C] in dtype with float64 dot products, per channel its own alpha and
    beta: apply(p) = L p, precond(r) = M^-1 r, started from M^-1 b times u0_scale (None: no factor); stops when ||r|| <= tol ||b|| on
    every channel, r the iteration's own residual.  keep: a list that receives u after every iteration.  Returns (out with u written at
    blk, iterations, the worst channel's final ||r|| / ||b||)."""
    dot = lambda a, c: np.einsum("yxc,yxc->c", a.astype(np.float64), c.astype(np.float64))
    bb = dot(b, b)
    rel = lambda r: float(np.sqrt(np.max(np.where(bb > 0, dot(r, r) / np.where(bb > 0, bb, 1.0), 0.0))))
    u = precond(b) if u0_scale is None else precond(b) * u0_scale
    r = b - apply(u)
    assert r.dtype == dtype
    z = precond(r)
    p = z.copy()
    rho = dot(r, z)
    it = 0
    while rel(r) > tol and it < max_iters:
        q = apply(p)
        pq = dot(p, q)
        alpha = np.where(pq != 0, rho / np.where(pq != 0, pq, 1.0), 0.0).astype(dtype)
        u = u + alpha * p
        r = r - alpha * q
        z = precond(r)
        rho_new = dot(r, z)
        beta = np.where(rho != 0, rho_new / np.where(rho != 0, rho, 1.0), 0.0).astype(dtype)
        p = z + beta * p
        rho = rho_new
        it += 1
        assert u.dtype == dtype and p.dtype == dtype
        if keep is not None:
            keep.append(u)
    out[blk] = u
    return out, it, rel(r)


def pcg_f32(b, apply, precond, u0_scale, tol, max_iters, out, blk):
    """pcg() on float32 vectors: the library's iteration"""
    return pcg(b, apply, precond, u0_scale, tol, max_iters, out, blk, np.float32)
