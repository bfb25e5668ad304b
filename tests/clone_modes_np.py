"""Restatement of OpenCV's MIXED_CLONE and MONOCHROME_TRANSFER right-hand sides (OpenCV 3.4.5 modules/photo,
Cloning::normalClone and evaluate), on the reference's thresholded mask (oracle_np.mask_stage).

Only the blended gradient field changes with the mode; the divergence, the Dirichlet fold, the solve and the output are the
NORMAL path's, reused from oracle_np.  Inside the eroded mask (m = 1):
    NORMAL       (Gx, Gy) = the patch's (gx, gy)
    MIXED        per channel: the patch's (gx, gy) where |pgx - pgy| > |dgx - dgy|, else the destination's (a tie picks D)
    MONOCHROME   (gx, gy) of the patch's grey image Y = (1868 B + 9617 G + 4899 R + 8192) >> 14, the same in every channel
and the destination's (gx, gy) outside it.  Every gradient is an integer, so the arithmetic below is exact in any float type.
"""
from __future__ import annotations

import numpy as np

from oracle import oracle_np

NORMAL, MIXED, MONOCHROME = 1, 2, 3


def grey_bgr(img: np.ndarray) -> np.ndarray:
    """cvtColor(BGR2GRAY) for 8-bit data: the fixed-point formula with 14 fractional bits, byte 0 = B."""
    i = img.astype(np.int64)
    return ((1868 * i[..., 0] + 9617 * i[..., 1] + 4899 * i[..., 2] + 8192) >> 14).astype(np.uint8)


def build_rhs(dst: np.ndarray, patch: np.ndarray, geo: dict, mode: int = NORMAL, dtype=np.float32):
    """oracle_np.build_rhs with the clone mode: returns (B, lap, g) in the same layout."""
    if mode not in (NORMAL, MIXED, MONOCHROME):
        raise ValueError("clone mode %r" % (mode,))
    if geo.get("opencv_grey"):
        raise ValueError("grey masks are blended NORMAL only")
    W, H, x0, y0, ltx, lty = (geo[k] for k in ("W", "H", "x0", "y0", "ltx", "lty"))
    if ltx < 0 or lty < 0 or ltx + W > dst.shape[1] or lty + H > dst.shape[0]:
        raise ValueError("ROI falls outside the destination image")
    B = dst[lty:lty + H, ltx:ltx + W, :].astype(dtype)
    Pu8 = patch[y0:y0 + H, x0:x0 + W, :]
    if mode == MONOCHROME:
        Pu8 = np.repeat(grey_bgr(Pu8)[:, :, None], 3, axis=2)
    P = Pu8.astype(dtype)
    m = (geo["M"] != 0)[:, :, None]
    gxb, gyb = oracle_np._fwd_grad_reflect(B)
    gxp, gyp = oracle_np._fwd_grad_reflect(P)
    if mode == MIXED:
        m = m & (np.abs(gxp - gyp) > np.abs(gxb - gyb))
    GX = np.where(m, gxp, gxb)
    GY = np.where(m, gyp, gyb)
    lap = np.zeros((H, W, 3), dtype=dtype)
    lap[1:-1, 1:-1] = (GX[1:-1, 1:-1] - GX[1:-1, :-2]) + (GY[1:-1, 1:-1] - GY[:-2, 1:-1])
    g = lap[1:-1, 1:-1].copy()
    g[:, 0] -= B[1:-1, 0]
    g[0, :] -= B[0, 1:-1]
    g[:, -1] -= B[1:-1, -1]
    g[-1, :] -= B[-1, 1:-1]
    return B, lap, g


def seamless_clone(dst, patch, mask, cx, cy, mode: int = NORMAL, float_tables: bool = True, return_all: bool = False):
    """The whole clone under `mode` with the float64 direct solve (float_tables: the reference's denominators, what the
    library computes by default)."""
    geo = oracle_np.mask_stage(mask, cx, cy)
    B, lap, g = build_rhs(dst, patch, geo, mode, dtype=np.float64)
    u = oracle_np.solve_dst(g, float_tables)
    out = oracle_np.splice(dst, oracle_np.clamp_truncate(u), geo)
    if return_all:
        return out, dict(geo=geo, B=B, lap=lap, g=g, u=u)
    return out
