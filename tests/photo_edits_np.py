"""Restatement of OpenCV 3.4.5's whole-image gradient edits (modules/photo, "Seamless Cloning": cv::colorChange,
cv::illuminationChange, cv::textureFlattening) as the library computes them (sc_hip_edit).

PARITY UNPINNED: OpenCV is not available to this project and the reference has no fixture of these functions.  This module
restates the rules the kernels follow; the GPU tests check the library against it (class and edge maps, eroded mask and the
right-hand side of colorChange / textureFlattening bit for bit, illuminationChange's within powf's error, whole edits within one
grey level).

    domain     the whole image: unknowns are rows 1..H-2, columns 1..W-2; the frame is src's own (Dirichlet data)
    mask       7 x 7 minimum filter ignoring pixels outside the image; m = M (1/255f), mi = (255 - M)(1/255f)
    P          forward differences (gx, gy) of src, per channel (float32)
    P'         colour        (P m) k_c, k = (blue_mul, green_mul, red_mul) for channels 0, 1, 2
               illumination  Q = P m, (Q powf(alpha, beta)) |Q|^-beta, NaN -> 0 (cv::patchNaNs)
               texture       (P if edge(q) else 0) m, edge = Canny of the whole src
    G          (gx, gy) mi + P'
    lap        (Gx(q) - Gx(q - x)) + (Gy(q) - Gy(q - y)), then the reference's float-table Poisson solve

Canny (cv::Canny, L2gradient = false): thresholds swapped when low > high and floored; per channel Sobel dx, dy of the aperture
with replicated borders, int32 sums saturated once to int16; per pixel the channel of the largest |dx| + |dy| (the first on a tie);
magnitudes outside the image are 0; non-maximum suppression with TG22 = 13573 evaluated in 64-bit integers (OpenCV's int32 form
can overflow only at aperture 7, where |dx| reaches 32768 and |dx| << 16 leaves int32); strong above `high`; hysteresis keeps the
weak pixels 8-connected to a strong one through weak pixels (scipy.ndimage.label, 3 x 3 structure).
"""
from __future__ import annotations

import numpy as np
from scipy import ndimage

from oracle import oracle_np

F32 = np.float32
COLOR, ILLUMINATION, TEXTURE = 1, 2, 3
TG22 = 13573
SOBEL = {3: ([1, 2, 1], [-1, 0, 1]),
         5: ([1, 4, 6, 4, 1], [-1, -2, 0, 2, 1]),
         7: ([1, 6, 15, 20, 15, 6, 1], [-1, -4, -5, 0, 5, 4, 1])}
DEFAULTS = {COLOR: dict(red_mul=1.0, green_mul=1.0, blue_mul=1.0),
            ILLUMINATION: dict(alpha=0.2, beta=0.4),
            TEXTURE: dict(low_threshold=30.0, high_threshold=45.0, kernel_size=3)}


def grey_bgr(img: np.ndarray) -> np.ndarray:
    """cvtColor(BGR2GRAY) for 8-bit data (what the Python wrappers apply to a three-channel mask)."""
    i = img.astype(np.int64)
    return ((1868 * i[..., 0] + 9617 * i[..., 1] + 4899 * i[..., 2] + 8192) >> 14).astype(np.uint8)


def erode_whole(mask: np.ndarray) -> np.ndarray:
    """Three 3 x 3 erodes of the whole mask = one 7 x 7 minimum filter; pixels outside the image are ignored."""
    return ndimage.minimum_filter(mask.astype(np.uint8), size=7, mode="constant", cval=255)


def canny_thresholds(low: float, high: float):
    low, high = float(np.float32(low)), float(np.float32(high))
    if low > high:
        low, high = high, low
    return int(np.floor(low)), int(np.floor(high))


def sobel(plane: np.ndarray, k: int):
    """(dx, dy) of one channel: correlation with the separable kernels, replicated borders, int32 sums saturated to int16."""
    s, d = SOBEL[k]
    r = k // 2
    P = np.pad(plane.astype(np.int64), r, mode="edge")
    H, W = plane.shape
    dx = np.zeros((H, W), np.int64)
    dy = np.zeros((H, W), np.int64)
    for j in range(k):
        for i in range(k):
            win = P[j:j + H, i:i + W]
            dx += s[j] * d[i] * win
            dy += d[j] * s[i] * win
    return np.clip(dx, -32768, 32767), np.clip(dy, -32768, 32767)


def canny_classes(src: np.ndarray, low: float, high: float, k: int = 3):
    """Class map after non-maximum suppression: 0 none, 1 weak, 2 strong (uint8 H x W)."""
    if k not in SOBEL:
        raise ValueError("kernel_size must be 3, 5 or 7")
    lo, hi = canny_thresholds(low, high)
    H, W = src.shape[:2]
    per = [sobel(src[:, :, c], k) for c in range(3)]
    mags = np.stack([np.abs(dx) + np.abs(dy) for dx, dy in per])
    best = np.argmax(mags, axis=0)                      # the first channel on a tie
    dx = np.choose(best, [p[0] for p in per])
    dy = np.choose(best, [p[1] for p in per])
    mag = np.choose(best, list(mags))
    mp = np.pad(mag, 1)                                 # 0 outside the image

    def nb(ox, oy):
        return mp[1 + oy:1 + oy + H, 1 + ox:1 + ox + W]

    xs, ys = np.abs(dx), np.abs(dy)
    tg22x = xs * TG22
    yy = ys << 15
    horiz = yy < tg22x
    vert = ~horiz & (yy > tg22x + (xs << 16))
    diag = ~horiz & ~vert
    s = np.where((dx ^ dy) < 0, -1, 1)
    keep_h = (mag > nb(-1, 0)) & (mag >= nb(1, 0))
    keep_v = (mag > nb(0, -1)) & (mag >= nb(0, 1))
    yi, xi = np.mgrid[0:H, 0:W]
    a = mp[yi - 1 + 1, xi - s + 1]
    b = mp[yi + 1 + 1, xi + s + 1]
    keep_d = (mag > a) & (mag > b)
    keep = (mag > lo) & np.where(horiz, keep_h, np.where(vert, keep_v, keep_d))
    cls = np.zeros((H, W), np.uint8)
    cls[keep] = 1
    cls[keep & (mag > hi)] = 2
    return cls


def hysteresis(cls: np.ndarray) -> np.ndarray:
    """Edge map (bool): strong pixels and the weak ones 8-connected to a strong pixel through weak pixels."""
    labels, _ = ndimage.label(cls > 0, structure=np.ones((3, 3), int))
    strong = np.unique(labels[cls == 2])
    return np.isin(labels, strong[strong > 0])


def canny(src: np.ndarray, low: float, high: float, k: int = 3):
    """(class map, edge map as 0 / 255 bytes)."""
    cls = canny_classes(src, low, high, k)
    return cls, hysteresis(cls).astype(np.uint8) * 255


def _params(op: int, params: dict) -> dict:
    if op not in DEFAULTS:
        raise ValueError("op %r" % (op,))
    p = dict(DEFAULTS[op])
    p.update(params)
    return p


def patch_field(op: int, gx, gy, m, src=None, **params):
    """P' = (Px, Py) per channel (float32 arrays H x W x 3)."""
    p = _params(op, params)
    if op == COLOR:
        k = np.array([p["blue_mul"], p["green_mul"], p["red_mul"]], F32)
        return (gx * m) * k, (gy * m) * k
    if op == ILLUMINATION:
        ab = np.power(F32(p["alpha"]), F32(p["beta"]))
        qx, qy = gx * m, gy * m
        mag = np.sqrt(qx * qx + qy * qy)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            w = np.power(mag, F32(-F32(p["beta"])))
            px, py = (qx * ab) * w, (qy * ab) * w
        return np.where(np.isnan(px), F32(0), px), np.where(np.isnan(py), F32(0), py)
    edge = hysteresis(canny_classes(src, p["low_threshold"], p["high_threshold"], int(p["kernel_size"])))[:, :, None]
    z = F32(0)
    return np.where(edge, gx, z) * m, np.where(edge, gy, z) * m


def build_rhs(src: np.ndarray, mask: np.ndarray, op: int, **params):
    """(eroded mask M, lap [3][H][W] float32 with 0 on the frame, field (Gx, Gy) H x W x 3) of an edit."""
    I = src.astype(F32)
    H, W = I.shape[:2]
    M = erode_whole(mask)
    m = (M.astype(F32) * F32(1.0 / 255.0))[:, :, None]
    mi = ((255 - M.astype(np.int32)).astype(F32) * F32(1.0 / 255.0))[:, :, None]
    gx, gy = oracle_np._fwd_grad_reflect(I)
    px, py = patch_field(op, gx, gy, m, src=src, **params)
    GX = gx * mi + px
    GY = gy * mi + py
    lap = np.zeros((H, W, 3), F32)
    lap[1:-1, 1:-1] = (GX[1:-1, 1:-1] - GX[1:-1, :-2]) + (GY[1:-1, 1:-1] - GY[:-2, 1:-1])
    return M, np.ascontiguousarray(lap.transpose(2, 0, 1)), (GX, GY)


def solve(src: np.ndarray, lap: np.ndarray) -> np.ndarray:
    """The Poisson solve of a planar right-hand side with src's frame as Dirichlet data (the reference's float tables), output
    clamped and truncated; the frame stays src's."""
    B = src.astype(np.float64)
    g = lap.transpose(1, 2, 0)[1:-1, 1:-1].astype(np.float64)
    g[:, 0] -= B[1:-1, 0]
    g[0, :] -= B[0, 1:-1]
    g[:, -1] -= B[1:-1, -1]
    g[-1, :] -= B[-1, 1:-1]
    u = oracle_np.solve_dst(g, float_tables=True)
    out = src.copy()
    out[1:-1, 1:-1] = oracle_np.clamp_truncate(u)
    return out


def edit(src: np.ndarray, mask: np.ndarray, op: int, **params) -> np.ndarray:
    """The whole edit: a new H x W x 3 image."""
    _, lap, _ = build_rhs(src, mask, op, **params)
    return solve(src, lap)


def color_change(src, mask, red_mul=1.0, green_mul=1.0, blue_mul=1.0):
    return edit(src, mask, COLOR, red_mul=red_mul, green_mul=green_mul, blue_mul=blue_mul)


def illumination_change(src, mask, alpha=0.2, beta=0.4):
    return edit(src, mask, ILLUMINATION, alpha=alpha, beta=beta)


def texture_flattening(src, mask, low_threshold=30.0, high_threshold=45.0, kernel_size=3):
    return edit(src, mask, TEXTURE, low_threshold=low_threshold, high_threshold=high_threshold, kernel_size=kernel_size)
