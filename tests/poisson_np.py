"""The test side's restatement of sc_hip_poisson (include/seamlessclone_hip.h): the divergence of a guidance field in float32 in the
documented order, the frame folded into the right-hand side, and the exact solve of the 5-point system in float64.

    u(x-1,y) + u(x+1,y) + u(x,y-1) + u(x,y+1) - 4 u(x,y) = lap(x,y)   on rows 1..H-2, columns 1..W-2, u = boundary on the frame
    lap(q) = (gx(q) - gx(q - x)) + (gy(q) - gy(q - y))                  (SC_POISSON_GUIDANCE)

Arrays are H x W x C (numpy's image order); H x W is taken as one channel.
"""
from __future__ import annotations

import numpy as np

from oracle import oracle_np


def _hwc(a: np.ndarray) -> np.ndarray:
    return a[:, :, None] if a.ndim == 2 else a


def forward_differences(img: np.ndarray):
    """(gx, gy) of an image in its own dtype: gx(x, y) = I(x+1, y) - I(x, y) on columns 0..W-2, gy likewise on rows 0..H-2, 0 on the
    last column / row (never read)."""
    gx = np.zeros_like(img)
    gy = np.zeros_like(img)
    gx[:, :-1] = img[:, 1:] - img[:, :-1]
    gy[:-1, :] = img[1:, :] - img[:-1, :]
    return gx, gy


def divergence(gx: np.ndarray, gy: np.ndarray) -> np.ndarray:
    """lap on the interior, 0 on the frame, in the arrays' dtype (float32 for the library's contract): (gx(q) - gx(q - x)) +
    (gy(q) - gy(q - y)), in this order."""
    lap = np.zeros_like(gx)
    lap[1:-1, 1:-1] = (gx[1:-1, 1:-1] - gx[1:-1, :-2]) + (gy[1:-1, 1:-1] - gy[:-2, 1:-1])
    return lap


def folded_rhs(boundary: np.ndarray, lap: np.ndarray) -> np.ndarray:
    """float64 right-hand side of the interior unknowns with zero Dirichlet values: lap minus the frame neighbours' values."""
    b = _hwc(boundary).astype(np.float64)
    g = _hwc(lap)[1:-1, 1:-1].astype(np.float64).copy()
    fr = np.zeros_like(b)
    fr[0, :] = b[0, :]
    fr[-1, :] = b[-1, :]
    fr[:, 0] = b[:, 0]
    fr[:, -1] = b[:, -1]
    g -= fr[1:-1, :-2] + fr[1:-1, 2:] + fr[:-2, 1:-1] + fr[2:, 1:-1]
    return g


def solve_exact(boundary: np.ndarray, lap: np.ndarray) -> np.ndarray:
    """The exact solution in float64, boundary's shape: the frame is boundary's, the interior the DST solve of the folded system."""
    u = _hwc(boundary).astype(np.float64).copy()
    u[1:-1, 1:-1] = oracle_np.solve_dst(folded_rhs(boundary, lap), float_tables=False)
    return u.reshape(boundary.shape)


def solve_guidance(boundary: np.ndarray, gx: np.ndarray, gy: np.ndarray) -> np.ndarray:
    """solve_exact with the float32 divergence of (gx, gy), as the library forms it."""
    return solve_exact(boundary, divergence(gx.astype(np.float32), gy.astype(np.float32)))
