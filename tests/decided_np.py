"""Decided channels: the output bytes that must equal the float-table solve EXACTLY.

The library promises the reference's answer: OpenCV's float-table DST solve, clamped to [0, 255] and truncated to bytes
(oracle/sc_oracle.c sco_finish).  Clamp-then-truncate gives byte b for every value in [b, b + 1) (b = 1 ... 254), 0 below 1 and
255 from 255 on: the byte changes at the integers 1 ... 255 and nowhere else (0 is not a boundary: -0.3 and 0.3 both give 0).

Every path reaches that answer only to within some error delta of its own (the multigrid default's stop rule, early
correction and node interpolation; the direct paths' transform rounding).  A channel whose float-table value u_ref lies more than
delta from every boundary is DECIDED at delta: any value within delta of u_ref truncates to the same byte, so the byte is known and
must match exactly.  The statistical checks the end-to-end tests used before (max <= 1, a small share of channels off) accept an
error of 0.3 grey levels over a whole 8 x 8 cell -- a few thousand flipped channels; this check does not (self-test in
tests/test_decided_host.py).

Channels within delta of a boundary are undecided; a GPU byte that differs there implies |u_gpu - u_ref| >= the distance from u_ref
to the boundary the byte crossed.  The largest such lower bound is returned so that tests can print it and later changes can
tighten delta."""
from __future__ import annotations

import numpy as np

# ---- delta per path, from the documented error budget (sc_multigrid.cpp stop rule, sc_lowmode.hip lowmode_early_kind)
# multigrid default and its flag variants (a converged solve plus the float-table correction):
#   stop rule: predicted error <= 0.1 x update_tol = 0.025 (default update_tol 0.25)
#   early correction (that of the iterate one cycle earlier): <= max_ratio x 4.9 x update_tol, accepted only <= 0.049 (kind 1 and 3)
#   node interpolation and K-mode truncation of the correction: < 0.002
#   16-bit fixed-point fields two cycles before the output: ~1e-4
#   0.025 + 0.049 + 0.002 + 0.0001 = 0.0761  ->  0.08
DELTA_MG = 0.08
# direct solves with double transforms (SC_METHOD_AUTO -> FFT fp64, SC_METHOD_DST).  They keep double between the float input and the
# float output; the C port stores float32 between its 1-D transform passes (as OpenCV does), and that storage is the larger term:
# the port differs from a float64 solve of the same right-hand side by 2.0e-4 at 700 x 500 and 3.8e-4 at 1030 x 1000 (growing with the
# size: the rounding of the transform's intermediates is divided by the smallest denominators, ~(pi / n)^2), and the GPU from the
# port by up to 6e-4 at 2048^2.  Plus 4 float32 ulps of the output (tests/test_gpu_direct_lengths.py F64_ULPS: 4 x 2^-15 = 1.2e-4 for
# |u| < 256):  6e-4 + 1.2e-4 = 7.2e-4  ->  1e-3, for ROIs up to 2048^2
DELTA_DIRECT = 1e-3
# float32 transforms (SC_METHOD_FFT): tests/test_gpu_direct_lengths.py F32_FACTOR / F32_FLOOR: the scaled error stays within
# max(4 x the port's own float32 transforms' error, 4e-4) (scale = max(1, max|u| / 500)); computed per case, delta_fft32()
F32_FACTOR, F32_FLOOR = 4.0, 4e-4


def boundary_distance(u):
    """distance from u to the nearest byte boundary (the integers 1 ... 255)"""
    u = np.asarray(u, np.float64)
    return np.abs(u - np.clip(np.rint(u), 1.0, 255.0))


def to_bytes(u):
    """clamp, then truncate toward zero: sco_finish"""
    return np.clip(np.asarray(u, np.float32), 0.0, 255.0).astype(np.uint8)


def crossed_bound(u, b):
    """least |v - u| over the values v that give byte b: the distance from u to [b, b + 1) (b = 0: (-inf, 1), b = 255: [255, inf))"""
    u = np.asarray(u, np.float64)
    b = np.asarray(b, np.float64)
    lo = np.where(b > 0, b, -np.inf)
    hi = np.where(b < 255, b + 1.0, np.inf)
    return np.maximum(np.maximum(lo - u, u - hi), 0.0)


class Case:
    """One solve to judge: the destination (H x W x 3 bytes), the ROI box in it (W, H, ltx, lty: ring included) and the float-table
    solution u_ref of the interior (3 x (H - 2) x (W - 2) float32, the oracle's float32 answer)."""

    def __init__(self, dst, W, H, ltx, lty, u_ref, g=None):
        self.dst = np.asarray(dst, np.uint8)
        self.W, self.H, self.ltx, self.lty = int(W), int(H), int(ltx), int(lty)
        self.u = np.asarray(u_ref, np.float32)
        assert self.u.shape == (3, self.H - 2, self.W - 2), (self.u.shape, self.W, self.H)
        self.g = g                      # the folded right-hand side (for the float32-transform bound)
        self._e32 = None

    def want(self):
        out = self.dst.copy()
        out[self.lty + 1:self.lty + self.H - 1, self.ltx + 1:self.ltx + self.W - 1] = np.moveaxis(to_bytes(self.u), 0, 2)
        return out

    def delta_fft32(self, oc, nthreads):
        """delta for SC_METHOD_FFT (float32 transforms) on this case: max(F32_FACTOR x the port's float32 error, F32_FLOOR) x scale"""
        if self._e32 is None:
            u32 = oc.solve_dst(self.g, nthreads, exact_den=False, internals="f32")
            scale = max(1.0, float(np.abs(self.u).max()) / 500.0)
            self._e32 = (max(F32_FACTOR * float(np.abs(u32.astype(np.float64) - self.u).max()) / scale, F32_FLOOR)) * scale
        return self._e32


def rhs_case(oc, dst, W, H, ltx, lty, B, lap, nthreads=1):
    """Case from a planar right-hand side (B: Dirichlet ring, lap: divergence; 3 x H x W float32) through the C oracle's float-table
    direct solve (oracle_c.solve_dst, exact_den=False: the reference's arithmetic)."""
    g = oc.fold(np.ascontiguousarray(B, np.float32), np.ascontiguousarray(lap, np.float32))
    return Case(dst, W, H, ltx, lty, oc.solve_dst(g, nthreads, exact_den=False), g)


def clone_case(oc, dst, patch, mask, cx, cy, nthreads=1):
    """Case of a NORMAL_CLONE through the C oracle (its mask stage, right-hand side, fold and float-table solve)."""
    geo, M = oc.mask_stage(mask, cx, cy)
    B, lap = oc.build_rhs(dst, patch, geo, M)
    return rhs_case(oc, dst, geo[2], geo[3], geo[4], geo[5], B, lap, nthreads)


def check(case, got, delta, label=""):
    """Asserts that every channel decided at delta equals the oracle's byte and that every byte outside the ROI interior equals the
    destination.  Returns (undecided share, mismatches, worst lower bound on |u_gpu - u_ref| the mismatches imply)."""
    got = np.asarray(got)
    assert got.shape == case.dst.shape and got.dtype == np.uint8, (label, got.shape, case.dst.shape)
    y0, x0 = case.lty + 1, case.ltx + 1
    h, w = case.H - 2, case.W - 2
    inner = np.zeros(case.dst.shape[:2], bool)
    inner[y0:y0 + h, x0:x0 + w] = True
    outside = ~inner
    n_out = int((got[outside] != case.dst[outside]).sum())
    assert n_out == 0, "%s: %d bytes outside the ROI interior differ from the destination" % (label, n_out)
    gb = np.moveaxis(got[y0:y0 + h, x0:x0 + w], 2, 0)             # 3 x h x w, the layout of u_ref
    wb = to_bytes(case.u)
    dist = boundary_distance(case.u)
    decided = dist > delta
    diff = gb != wb
    bound = float(crossed_bound(case.u[diff], gb[diff]).max()) if diff.any() else 0.0
    bad = diff & decided
    undecided = float(1.0 - decided.mean())
    if bad.any():
        c, y, x = (int(v[0]) for v in np.nonzero(bad))
        raise AssertionError("%s: %d decided channels (delta %.3g) differ from the float-table bytes; first at channel %d, image (%d, %d): "
                             "u_ref %.4f, oracle %d, got %d; worst implied |u_gpu - u_ref| >= %.4f; %d mismatches, %.3g %% undecided"
                             % (label, int(bad.sum()), delta, c, y + y0, x + x0, float(case.u[c, y, x]), int(wb[c, y, x]), int(gb[c, y, x]),
                                bound, int(diff.sum()), 100.0 * undecided))
    return undecided, int(diff.sum()), bound
