"""ctypes binding of libseamlessclone_hip.so -- the C ABI declared in include/seamlessclone_hip.h.

There is no CPU fallback: if the HIP library is missing or does not load this module raises,
and every compute entry point needs a visible MI355X.
"""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_PKG)
LIB_PATH = os.path.join(_PKG, "libseamlessclone_hip.so")
HEADER_PATH = os.path.join(_ROOT, "include", "seamlessclone_hip.h")
TESTING_HEADER_PATH = os.path.join(_ROOT, "include", "seamlessclone_hip_testing.h")      # test and measurement hooks, same library

SC_OK = 0
SC_ERR_BAD_ARG = -1
SC_ERR_BAD_SIZE = -2
SC_ERR_EMPTY_MASK = -3
SC_ERR_ROI_OOB = -4
SC_ERR_HIP = -5
SC_ERR_NOT_CONVERGED = -6

# clone modes: OpenCV's flag values (cv2.NORMAL_CLONE, cv2.MIXED_CLONE, cv2.MONOCHROME_TRANSFER); Instance.set_clone_mode
SC_NORMAL_CLONE = 1
SC_MIXED_CLONE = 2
SC_MONOCHROME_TRANSFER = 3
CLONE_MODES = (SC_NORMAL_CLONE, SC_MIXED_CLONE, SC_MONOCHROME_TRANSFER)

# whole-image gradient edits (sc_hip_edit): cv::colorChange, cv::illuminationChange, cv::textureFlattening; Instance.edit
SC_EDIT_COLOR_CHANGE = 1
SC_EDIT_ILLUMINATION_CHANGE = 2
SC_EDIT_TEXTURE_FLATTENING = 3
EDIT_OPS = (SC_EDIT_COLOR_CHANGE, SC_EDIT_ILLUMINATION_CHANGE, SC_EDIT_TEXTURE_FLATTENING)

SC_METHOD_JACOBI = 0
SC_METHOD_RBGS = 1
SC_METHOD_SOR = 2
SC_METHOD_MULTIGRID = 3
SC_METHOD_DST = 4
SC_METHOD_AUTO = 5      # default: the FFT-form direct solve (double transforms) up to SC_AUTO_DIRECT_MAX unknowns per side, MULTIGRID above
SC_METHOD_FFT = 6       # the reference's default back-end: FFT-based direct solve, float32, O(n^2 log n)
SC_AUTO_DIRECT_MAX = 720
SC_AUTO_DIRECT_AREA = 450000
SC_AUTO_NARROW_MAX = 140
SC_AUTO_THIN_MAX = 4
SC_AUTO_THIN_LONG_MAX = 4096

SC_FLAG_NO_SPECULATE = 1 << 0
SC_FLAG_FLOAT_RHS = 1 << 1
SC_FLAG_FLOAT_U0 = 1 << 2
SC_FLAG_NO_COMPOSE_L1 = 1 << 3
SC_FLAG_VCYCLE_BOTTOM = 1 << 4
SC_FLAG_EXACT_TABLES = 1 << 5
SC_FLAG_LEGACY_PATHS = 1 << 6      # run the superseded launch forms named in SolverOpts.legacy_paths (SC_LEGACY_* bits)
SC_LEGACY_SEPARATE_RESTRICT, SC_LEGACY_BOTTOM_F32, SC_LEGACY_SEPARATE_TAIL, SC_LEGACY_UNPACKED_TILES = 1, 2, 4, 8
SC_LEGACY_SPLICE_LAUNCH = 16       # same-size groups: the judged cycle leaves planar bytes and a splice launch interleaves them, always
SC_FORCE_INTERLEAVED_OUT = 32      # ... the judged launch writes the interleaved bytes itself wherever that form exists, whatever the threshold
SC_LEGACY_U0_PLANES = 64           # same-size groups: the pre-process stores the float16 initial field and the first level-0 launch reads it, always
SC_FORCE_U0_BYTES = 128            # ... the first launch reads the destinations' bytes wherever that form exists, whatever the threshold
SC_FLAG_KEEP_FIELD = 1 << 7
SC_FLAG_FFT_FP64 = 1 << 8
SC_FLAG_OPENCV_GREY_MASK = 1 << 9
SC_FLAG_FLOAT_L1 = 1 << 10
SC_FLAG_FLOAT_FIELD = 1 << 11
SC_FLAG_NO_STAGE_MARKS = 1 << 12
SC_FLAG_ROWS_RETURN = 1 << 13     # host-image call, opt-in: whole destination rows come back as one linear copy (default: ROI bytes only)
SC_FLAG_POISON_ARENA = 1 << 14    # testing: blocks handed out without zeroing are filled with 0xFF (NaN) first

def auto_takes_direct(w: int, h: int) -> bool:
    """SC_METHOD_AUTO's choice for ONE clone with w x h unknowns (sc_solver.cpp effective_method): True = the direct solve (SC_METHOD_FFT,
    double transforms), False = multigrid.  (A group of clones always takes the cycles; tol > 0 too.)"""
    if w <= SC_AUTO_DIRECT_MAX and h <= SC_AUTO_DIRECT_MAX:
        return True
    if max(w, h) <= SC_AUTO_THIN_LONG_MAX and (w * h <= SC_AUTO_DIRECT_AREA or min(w, h) <= SC_AUTO_NARROW_MAX):
        return True
    return False


ERR_NAMES = {
    SC_ERR_BAD_ARG: "SC_ERR_BAD_ARG", SC_ERR_BAD_SIZE: "SC_ERR_BAD_SIZE", SC_ERR_EMPTY_MASK: "SC_ERR_EMPTY_MASK",
    SC_ERR_ROI_OOB: "SC_ERR_ROI_OOB", SC_ERR_HIP: "SC_ERR_HIP", SC_ERR_NOT_CONVERGED: "SC_ERR_NOT_CONVERGED",
}


class SolverOpts(C.Structure):
    _fields_ = [("method", C.c_int), ("max_sweeps", C.c_int), ("tol", C.c_float), ("check_every", C.c_int),
                ("omega", C.c_float), ("sweeps_per_launch", C.c_int), ("reference_warmup", C.c_int),
                ("mg_pre", C.c_int), ("mg_post", C.c_int), ("update_tol", C.c_float), ("flags", C.c_int), ("jacobi_tile_rows", C.c_int), ("mg_level1_sweeps", C.c_int), ("mg_direct_max", C.c_int), ("legacy_paths", C.c_int)]


class RunInfo(C.Structure):
    _fields_ = [("x0", C.c_int), ("y0", C.c_int), ("W", C.c_int), ("H", C.c_int), ("ltx", C.c_int), ("lty", C.c_int),
                ("sweeps", C.c_int), ("converged", C.c_int), ("rel_residual", C.c_double),
                ("ms_h2d", C.c_float), ("ms_mask", C.c_float), ("ms_pre", C.c_float), ("ms_solve", C.c_float),
                ("ms_post", C.c_float), ("ms_d2h", C.c_float), ("ms_device_total", C.c_float),
                ("sweep_launches", C.c_int), ("last_update", C.c_float), ("device_bytes", C.c_size_t), ("method", C.c_int),
                ("device", C.c_int), ("ms_call", C.c_float), ("field_retry", C.c_int), ("new_size", C.c_int),
                ("group_members", C.c_int), ("group_ragged", C.c_int)]


class BatchJob(C.Structure):
    _fields_ = [("face", C.c_void_p), ("face_cols", C.c_int), ("face_rows", C.c_int), ("face_step", C.c_int),
                ("body", C.c_void_p), ("body_cols", C.c_int), ("body_rows", C.c_int), ("body_step", C.c_int),
                ("mask", C.c_void_p), ("mask_cols", C.c_int), ("mask_rows", C.c_int), ("mask_step", C.c_int),
                ("centerX", C.c_int), ("centerY", C.c_int), ("body_restore", C.c_void_p), ("rc", C.c_int)]


class EditParams(C.Structure):
    _fields_ = [("op", C.c_int), ("red_mul", C.c_float), ("green_mul", C.c_float), ("blue_mul", C.c_float),
                ("alpha", C.c_float), ("beta", C.c_float), ("low_threshold", C.c_float), ("high_threshold", C.c_float),
                ("kernel_size", C.c_int)]


class EditJob(C.Structure):
    _fields_ = [("src", C.c_void_p), ("cols", C.c_int), ("rows", C.c_int), ("src_step", C.c_int),
                ("mask", C.c_void_p), ("mask_step", C.c_int),
                ("dst", C.c_void_p), ("dst_step", C.c_int), ("rc", C.c_int)]


# the Poisson solver on float32 images with caller guidance fields (sc_hip_poisson*): Instance.poisson / poisson_device
SC_POISSON_GUIDANCE = 1
SC_POISSON_LAPLACIAN = 2
SC_POISSON_NEUMANN = 1 << 8          # or'ed into either kind: reflecting border, every pixel an unknown
SC_POISSON_FREE_LEFT = 1 << 12       # or'ed into either kind: that side has no Dirichlet line, its outermost pixels are unknowns
SC_POISSON_FREE_RIGHT = 1 << 13      # (all four: the Neumann problem)
SC_POISSON_FREE_TOP = 1 << 14
SC_POISSON_FREE_BOTTOM = 1 << 15
SC_POISSON_FREE_ALL = SC_POISSON_FREE_LEFT | SC_POISSON_FREE_RIGHT | SC_POISSON_FREE_TOP | SC_POISSON_FREE_BOTTOM
_FREE_SIDE_BITS = {"l": SC_POISSON_FREE_LEFT, "r": SC_POISSON_FREE_RIGHT, "t": SC_POISSON_FREE_TOP, "b": SC_POISSON_FREE_BOTTOM}


def free_side_bits(free_sides="", neumann=False) -> int:
    """The SC_POISSON_FREE_* bits of a string over the letters "lrtb" (left, right, top, bottom; order and repeats do not matter).
    neumann=True is "lrtb" and reads SC_POISSON_NEUMANN.  Anything else raises ValueError."""
    if not isinstance(free_sides, str):
        raise ValueError('free_sides must be a string over the letters "lrtb"')
    bits = 0
    for ch in free_sides:
        if ch not in _FREE_SIDE_BITS:
            raise ValueError(f'free_sides: {ch!r} is none of the letters "lrtb"')
        bits |= _FREE_SIDE_BITS[ch]
    return SC_POISSON_NEUMANN if neumann else bits
SC_POISSON_PERIODIC_X = 1 << 17      # or'ed into either kind: the x axis wraps (column cols-1 is column 0's left neighbour)
SC_POISSON_PERIODIC_Y = 1 << 18      # ... the y axis (row rows-1 is row 0's upper neighbour); bit 16 is not a kind
SC_POISSON_PERIODIC_ALL = SC_POISSON_PERIODIC_X | SC_POISSON_PERIODIC_Y
_PERIODIC_BITS = {"x": SC_POISSON_PERIODIC_X, "y": SC_POISSON_PERIODIC_Y}


def periodic_bits(periodic="") -> int:
    """The SC_POISSON_PERIODIC_* bits of "x", "y", "xy" or "" (order and repeats do not matter).  Anything else raises ValueError."""
    if not isinstance(periodic, str):
        raise ValueError('periodic must be a string over the letters "xy"')
    bits = 0
    for ch in periodic:
        if ch not in _PERIODIC_BITS:
            raise ValueError(f'periodic: {ch!r} is neither "x" nor "y"')
        bits |= _PERIODIC_BITS[ch]
    return bits


def border_bits(free_sides="", neumann=False, periodic="") -> int:
    """free_side_bits | periodic_bits of one call's borders.  ValueError for periodic together with neumann=True or with a free side on
    the same axis: an axis wraps or reflects, not both."""
    per = periodic_bits(periodic)
    if per and neumann:
        raise ValueError("periodic excludes neumann=True: name the free sides of the other axis with free_sides")
    free = free_side_bits(free_sides, neumann)
    if (per & SC_POISSON_PERIODIC_X) and (free & (SC_POISSON_FREE_LEFT | SC_POISSON_FREE_RIGHT)):
        raise ValueError('periodic "x" excludes the free sides "l" and "r"')
    if (per & SC_POISSON_PERIODIC_Y) and (free & (SC_POISSON_FREE_TOP | SC_POISSON_FREE_BOTTOM)):
        raise ValueError('periodic "y" excludes the free sides "t" and "b"')
    return free | per


def no_dirichlet(kind: int) -> bool:
    """No side of a kind keeps a Dirichlet line (each axis periodic or free at both ends): the unscreened system is singular, boundary
    gives only the mean and may be None; a screened solve does not use it."""
    if kind & SC_POISSON_NEUMANN:
        return True
    x = (kind & SC_POISSON_PERIODIC_X) or (kind & SC_POISSON_FREE_LEFT and kind & SC_POISSON_FREE_RIGHT)
    y = (kind & SC_POISSON_PERIODIC_Y) or (kind & SC_POISSON_FREE_TOP and kind & SC_POISSON_FREE_BOTTOM)
    return bool(x and y)


SC_POISSON_MAX_PLANES = 192


class PoissonLayout(C.Structure):
    _fields_ = [("cols", C.c_int), ("rows", C.c_int), ("channels", C.c_int),
                ("col_stride", C.c_longlong), ("row_stride", C.c_longlong), ("channel_stride", C.c_longlong)]


class PoissonParams(C.Structure):
    _fields_ = [("kind", C.c_int), ("tol", C.c_float)]


class PoissonJob(C.Structure):
    _fields_ = [("gx", C.c_void_p), ("gy", C.c_void_p), ("lap", C.c_void_p), ("boundary", C.c_void_p), ("out", C.c_void_p),
                ("rc", C.c_int)]


# screened Poisson solves (sc_hip_screened*): Instance.screened / screened_device
class ScreenedParams(C.Structure):
    _fields_ = [("kind", C.c_int), ("lam", C.c_float)]        # (the C field is `lambda`)


class ScreenedJob(C.Structure):
    _fields_ = [("gx", C.c_void_p), ("gy", C.c_void_p), ("lap", C.c_void_p), ("data", C.c_void_p), ("boundary", C.c_void_p),
                ("out", C.c_void_p), ("rc", C.c_int)]


# weighted solves (sc_hip_weighted*): Instance.weighted / weighted_device
SC_WEIGHTED_POLL = 4        # iterations between an iteration and the host's read of its norms (seamlessclone_hip.h)


class WeightedParams(C.Structure):
    _fields_ = [("kind", C.c_int), ("tol", C.c_float), ("max_iters", C.c_int), ("precond_lambda", C.c_float)]


class WeightedJob(C.Structure):
    _fields_ = [("gx", C.c_void_p), ("gy", C.c_void_p), ("lap", C.c_void_p), ("data", C.c_void_p), ("weight", C.c_void_p),
                ("boundary", C.c_void_p), ("out", C.c_void_p), ("rc", C.c_int)]


# WLS solves (sc_hip_wls*): Instance.wls / wls_device
class WlsParams(C.Structure):
    _fields_ = [("kind", C.c_int), ("tol", C.c_float), ("max_iters", C.c_int), ("precond_lambda", C.c_float), ("precond_smooth", C.c_float)]


class WlsJob(C.Structure):
    _fields_ = [("gx", C.c_void_p), ("gy", C.c_void_p), ("lap", C.c_void_p), ("data", C.c_void_p), ("weight", C.c_void_p),
                ("smooth_x", C.c_void_p), ("smooth_y", C.c_void_p), ("boundary", C.c_void_p), ("out", C.c_void_p), ("rc", C.c_int)]


# region solves (sc_hip_region*): Instance.region / region_device -- the values of a state array (float32 0.0, 1.0, 2.0 on the device)
SC_REGION_UNKNOWN = 0       # solved for
SC_REGION_KNOWN = 1         # u = data there, exactly
SC_REGION_OUTSIDE = 2       # not part of the domain: its links do not exist


class RegionParams(C.Structure):
    _fields_ = [("kind", C.c_int), ("tol", C.c_float), ("max_iters", C.c_int), ("precond_lambda", C.c_float), ("precond_smooth", C.c_float)]


class RegionJob(C.Structure):
    _fields_ = [("gx", C.c_void_p), ("gy", C.c_void_p), ("lap", C.c_void_p), ("data", C.c_void_p), ("state", C.c_void_p),
                ("weight", C.c_void_p), ("smooth_x", C.c_void_p), ("smooth_y", C.c_void_p), ("boundary", C.c_void_p), ("out", C.c_void_p),
                ("rc", C.c_int)]


# bounded solves (sc_hip_bounded*): Instance.bounded / bounded_device -- region solves under lower <= u <= upper at the UNKNOWN pixels;
# bounded_trace() reports the rounds
class BoundedParams(C.Structure):
    _fields_ = [("kind", C.c_int), ("tol", C.c_float), ("max_iters", C.c_int), ("precond_lambda", C.c_float), ("precond_smooth", C.c_float),
                ("lower", C.c_float), ("upper", C.c_float), ("max_rounds", C.c_int)]


class BoundedJob(C.Structure):
    _fields_ = [("gx", C.c_void_p), ("gy", C.c_void_p), ("lap", C.c_void_p), ("data", C.c_void_p), ("state", C.c_void_p),
                ("weight", C.c_void_p), ("smooth_x", C.c_void_p), ("smooth_y", C.c_void_p), ("boundary", C.c_void_p), ("lower", C.c_void_p),
                ("upper", C.c_void_p), ("out", C.c_void_p), ("rc", C.c_int)]


# volume solves (sc_hip_volume*): Instance.volume / volume_device -- region solves on frame stacks with temporal links
class VolumeParams(C.Structure):
    _fields_ = [("kind", C.c_int), ("frames", C.c_int), ("frame_stride", C.c_longlong), ("tau", C.c_float), ("tol", C.c_float),
                ("max_iters", C.c_int), ("precond_lambda", C.c_float)]


class VolumeJob(C.Structure):
    _fields_ = [("gx", C.c_void_p), ("gy", C.c_void_p), ("gt", C.c_void_p), ("lap", C.c_void_p), ("data", C.c_void_p), ("state", C.c_void_p),
                ("weight", C.c_void_p), ("boundary", C.c_void_p), ("out", C.c_void_p), ("rc", C.c_int)]


# WLS volume solves (sc_hip_volume_wls*): Instance.volume_wls / volume_wls_device -- volume solves with per-link weights in space and
# time and, if asked, periodic time
class VolumeWlsParams(C.Structure):
    _fields_ = [("kind", C.c_int), ("frames", C.c_int), ("frame_stride", C.c_longlong), ("tau", C.c_float), ("time_periodic", C.c_int),
                ("tol", C.c_float), ("max_iters", C.c_int), ("precond_lambda", C.c_float), ("precond_smooth", C.c_float), ("precond_tau", C.c_float)]


class VolumeWlsJob(C.Structure):
    _fields_ = [("gx", C.c_void_p), ("gy", C.c_void_p), ("gt", C.c_void_p), ("lap", C.c_void_p), ("data", C.c_void_p), ("state", C.c_void_p),
                ("weight", C.c_void_p), ("smooth_x", C.c_void_p), ("smooth_y", C.c_void_p), ("smooth_t", C.c_void_p), ("boundary", C.c_void_p),
                ("out", C.c_void_p), ("rc", C.c_int)]


# flow volume solves (sc_hip_volume_flow*): Instance.volume_flow / volume_flow_device -- VolumeWlsParams themselves; temporal links along a flow
class VolumeFlowJob(C.Structure):
    _fields_ = [("gx", C.c_void_p), ("gy", C.c_void_p), ("gt", C.c_void_p), ("lap", C.c_void_p), ("data", C.c_void_p), ("state", C.c_void_p),
                ("weight", C.c_void_p), ("smooth_x", C.c_void_p), ("smooth_y", C.c_void_p), ("smooth_t", C.c_void_p), ("flow_x", C.c_void_p),
                ("flow_y", C.c_void_p), ("boundary", C.c_void_p), ("out", C.c_void_p), ("rc", C.c_int)]


# robust solves (sc_hip_robust*): Instance.robust / robust_device / robust_trace
SC_ROBUST_ISOTROPIC = 1 << 20        # or'ed into RobustParams.kind only: one penalty per pixel over its two forward links
SC_ROBUST_JOINT_CHANNELS = 1 << 21   # ... one penalty over all channels of a job (both: vectorial TV)


def robust_coupling_bits(isotropic=False, joint_channels=False) -> int:
    return (SC_ROBUST_ISOTROPIC if isotropic else 0) | (SC_ROBUST_JOINT_CHANNELS if joint_channels else 0)


def robust_penalties(**terms):
    """What every robust call asks of its penalties, name=(exponent, eps): an exponent in (0, 2], an eps finite and > 0 wherever its
    exponent is not 2."""
    for name, (r, eps) in terms.items():
        if not (np.isfinite(r) and 0 < r <= 2):
            raise ValueError(f"p_{name} must lie in (0, 2]")
        if r != 2 and not (np.isfinite(eps) and eps > 0):
            raise ValueError(f"eps_{name} must be finite and > 0")


class RobustParams(C.Structure):
    _fields_ = [("kind", C.c_int), ("p_grad", C.c_float), ("eps_grad", C.c_float), ("p_data", C.c_float), ("eps_data", C.c_float),
                ("max_rounds", C.c_int), ("round_tol", C.c_float), ("tol", C.c_float), ("max_iters", C.c_int)]


def robust_params(kind, p_grad=1.0, eps_grad=1e-3, p_data=2.0, eps_data=1e-3, max_rounds=0, round_tol=0.0, tol=0.0, max_iters=0) -> RobustParams:
    return RobustParams(int(kind), float(p_grad), float(eps_grad), float(p_data), float(eps_data), int(max_rounds), float(round_tol), float(tol),
                        int(max_iters))


class RobustJob(C.Structure):
    _fields_ = [("gx", C.c_void_p), ("gy", C.c_void_p), ("data", C.c_void_p), ("weight", C.c_void_p), ("smooth_x", C.c_void_p),
                ("smooth_y", C.c_void_p), ("boundary", C.c_void_p), ("out", C.c_void_p), ("rc", C.c_int)]


# robust region solves (sc_hip_region_robust*): Instance.region_robust / region_robust_device -- RobustParams themselves (the coupling bits
# included) on a RegionJob without lap; robust_trace() reports the rounds
class RegionRobustJob(C.Structure):
    _fields_ = [("gx", C.c_void_p), ("gy", C.c_void_p), ("data", C.c_void_p), ("state", C.c_void_p), ("weight", C.c_void_p),
                ("smooth_x", C.c_void_p), ("smooth_y", C.c_void_p), ("boundary", C.c_void_p), ("out", C.c_void_p), ("rc", C.c_int)]


# robust volume solves (sc_hip_volume_robust*): Instance.volume_robust / volume_robust_device -- Lp penalties in space, time and data on
# frame stacks; robust_trace() reports the rounds
class VolumeRobustParams(C.Structure):
    _fields_ = [("kind", C.c_int), ("frames", C.c_int), ("frame_stride", C.c_longlong), ("tau", C.c_float), ("time_periodic", C.c_int),
                ("p_grad", C.c_float), ("eps_grad", C.c_float), ("p_time", C.c_float), ("eps_time", C.c_float), ("p_data", C.c_float),
                ("eps_data", C.c_float), ("max_rounds", C.c_int), ("round_tol", C.c_float), ("tol", C.c_float), ("max_iters", C.c_int)]


class VolumeRobustJob(C.Structure):
    _fields_ = [("gx", C.c_void_p), ("gy", C.c_void_p), ("gt", C.c_void_p), ("data", C.c_void_p), ("state", C.c_void_p), ("weight", C.c_void_p),
                ("smooth_x", C.c_void_p), ("smooth_y", C.c_void_p), ("smooth_t", C.c_void_p), ("boundary", C.c_void_p), ("out", C.c_void_p),
                ("rc", C.c_int)]


# robust flow volume solves (sc_hip_volume_flow_robust*): Instance.volume_flow_robust / volume_flow_robust_device -- VolumeRobustParams
# themselves; every temporal link, its penalty included, along a flow
class VolumeFlowRobustJob(C.Structure):
    _fields_ = [("gx", C.c_void_p), ("gy", C.c_void_p), ("gt", C.c_void_p), ("data", C.c_void_p), ("state", C.c_void_p), ("weight", C.c_void_p),
                ("smooth_x", C.c_void_p), ("smooth_y", C.c_void_p), ("smooth_t", C.c_void_p), ("flow_x", C.c_void_p), ("flow_y", C.c_void_p),
                ("boundary", C.c_void_p), ("out", C.c_void_p), ("rc", C.c_int)]


# robust sub-pixel flow volume solves (sc_hip_volume_subflow_robust*): Instance.volume_subflow_robust / volume_subflow_robust_device --
# VolumeRobustParams and VolumeFlowRobustJob themselves; the flow's values as they are, every temporal link a bilinear stencil


# coupled volume solves (sc_hip_volume_coupled*): Instance.volume_coupled / volume_coupled_device -- VolumeRobustParams and VolumeRobustJob
# themselves, the coupling beside them; along a flow (sc_hip_volume_flow_coupled*): Instance.volume_flow_coupled /
# volume_flow_coupled_device, with VolumeFlowRobustJob
SC_VOLUME_COUPLE_SPACE = 1           # one penalty per pixel over its x- and y-link (per frame isotropic TV)
SC_VOLUME_COUPLE_TIME = 2            # ... and its forward temporal link in the same magnitude (space-time TV); comes with SPACE
SC_VOLUME_COUPLE_CHANNELS = 4        # every magnitude sums over the channels of a volume (vectorial TV)


def volume_coupling(isotropic=False, spacetime=False, joint_channels=False) -> int:
    """the coupling of sc_hip_volume_coupled: spacetime implies isotropic"""
    return ((SC_VOLUME_COUPLE_SPACE if isotropic or spacetime else 0) | (SC_VOLUME_COUPLE_TIME if spacetime else 0) |
            (SC_VOLUME_COUPLE_CHANNELS if joint_channels else 0))


class SeamlessCloneError(RuntimeError):
    def __init__(self, code, msg=""):
        self.code = code
        super().__init__(f"{ERR_NAMES.get(code, code)}: {msg}")


u8p = C.POINTER(C.c_uint8)
f32p = C.POINTER(C.c_float)
i32p = C.POINTER(C.c_int)
f64p = C.POINTER(C.c_double)
_IMG = [C.c_void_p, C.c_int, C.c_int, C.c_int]

_lib = None


def declared_symbols(header: str | None = None) -> list[str]:
    """Every function name `header` declares; by default both headers, the drop-in one and the testing one (used by the CPU-side
    ABI test)."""
    txt = "".join(open(h).read() for h in ([header] if header else [HEADER_PATH, TESTING_HEADER_PATH]))
    return sorted(set(re.findall(r"SC_API[^;(]*?\b((?:my_seamlessclone_api_imp_|sc_hip_)\w+)\s*\(", txt)))


def build(verbose: bool = False) -> str:
    """hipcc --offload-arch=gfx950 build of the in-tree shared library (no GPU needed)."""
    cmd = ["make", "-C", os.path.join(_PKG, "csrc"), "-j4"]
    if not verbose:
        cmd.append("-s")
    subprocess.check_call(cmd)
    return LIB_PATH


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc, gfx950). There is no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    L.my_seamlessclone_api_imp_create_instance.argtypes = [C.c_int]
    L.my_seamlessclone_api_imp_create_instance.restype = C.c_void_p
    L.my_seamlessclone_api_imp_run.argtypes = [C.c_void_p] + _IMG * 3 + [C.c_int, C.c_int, C.c_int, C.c_bool]
    L.my_seamlessclone_api_imp_run.restype = C.c_int
    L.my_seamlessclone_api_imp_destroy.argtypes = [C.c_void_p]
    L.my_seamlessclone_api_imp_destroy.restype = None
    L.my_seamlessclone_api_imp_sync.argtypes = [C.c_void_p]
    L.my_seamlessclone_api_imp_sync.restype = None
    L.sc_hip_default_opts.argtypes = [C.POINTER(SolverOpts)]
    L.sc_hip_default_opts.restype = None
    L.sc_hip_set_solver.argtypes = [C.c_void_p, C.POINTER(SolverOpts)]
    L.sc_hip_set_solver.restype = C.c_int
    L.sc_hip_get_solver.argtypes = [C.c_void_p, C.POINTER(SolverOpts)]
    L.sc_hip_get_solver.restype = C.c_int
    L.sc_hip_get_info.argtypes = [C.c_void_p, C.POINTER(RunInfo)]
    L.sc_hip_get_info.restype = C.c_int
    L.sc_hip_last_error.argtypes = [C.c_void_p]
    L.sc_hip_last_error.restype = C.c_char_p
    L.sc_hip_set_clone_mode.argtypes = [C.c_void_p, C.c_int]
    L.sc_hip_set_clone_mode.restype = C.c_int
    L.sc_hip_get_clone_mode.argtypes = [C.c_void_p]
    L.sc_hip_get_clone_mode.restype = C.c_int
    L.sc_hip_pool_set_clone_mode.argtypes = [C.c_void_p, C.c_int]
    L.sc_hip_pool_set_clone_mode.restype = C.c_int
    L.sc_hip_run_device.argtypes = [C.c_void_p] + _IMG * 3 + [C.c_int, C.c_int, C.c_bool]
    L.sc_hip_run_device.restype = C.c_int
    L.sc_hip_malloc.argtypes = [C.c_void_p, C.c_size_t]
    L.sc_hip_malloc.restype = C.c_void_p
    L.sc_hip_free.argtypes = [C.c_void_p, C.c_void_p]
    L.sc_hip_free.restype = None
    L.sc_hip_host_alloc.argtypes = [C.c_void_p, C.c_size_t]
    L.sc_hip_host_alloc.restype = C.c_void_p
    L.sc_hip_host_free.argtypes = [C.c_void_p, C.c_void_p]
    L.sc_hip_host_free.restype = None
    L.sc_hip_memcpy_h2d.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    L.sc_hip_memcpy_h2d.restype = C.c_int
    L.sc_hip_memcpy_d2h.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    L.sc_hip_memcpy_d2h.restype = C.c_int
    L.sc_hip_memcpy_d2d_async.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    L.sc_hip_memcpy_d2d_async.restype = C.c_int
    L.sc_hip_device_count.argtypes = []
    L.sc_hip_device_count.restype = C.c_int
    L.sc_hip_device_pci_bus_id.argtypes = [C.c_int, C.c_char_p, C.c_int]
    L.sc_hip_device_pci_bus_id.restype = C.c_int
    L.sc_hip_mask_stage.argtypes = [C.c_void_p] + _IMG + [C.c_int, C.c_int, i32p, u8p, C.c_size_t]
    L.sc_hip_mask_stage.restype = C.c_int
    L.sc_hip_build_rhs.argtypes = [C.c_void_p] + _IMG * 3 + [C.c_int, C.c_int, i32p, f32p, f32p, C.c_size_t]
    L.sc_hip_build_rhs.restype = C.c_int
    L.sc_hip_front_end_device.argtypes = [C.c_void_p, C.POINTER(BatchJob), C.c_int, C.c_int, C.c_int, i32p, i32p, i32p, i32p, u8p, f32p, f32p, C.c_size_t]
    L.sc_hip_front_end_device.restype = C.c_int
    L.sc_hip_field_load.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, f32p, f32p]
    L.sc_hip_field_load.restype = C.c_int
    L.sc_hip_field_sweep.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_int]
    L.sc_hip_field_sweep.restype = C.c_int
    L.sc_hip_field_residual.argtypes = [C.c_void_p, f64p]
    L.sc_hip_field_residual.restype = C.c_int
    L.sc_hip_field_solve.argtypes = [C.c_void_p]
    L.sc_hip_field_solve.restype = C.c_int
    L.sc_hip_bytes_writer.argtypes = [C.c_void_p]
    L.sc_hip_bytes_writer.restype = C.c_int
    L.sc_hip_u0_reader.argtypes = [C.c_void_p]
    L.sc_hip_u0_reader.restype = C.c_int
    L.sc_hip_u0_bytes_fetch.argtypes = [C.c_void_p, C.c_int, C.c_int, i32p]
    L.sc_hip_u0_bytes_fetch.restype = C.c_int
    L.sc_hip_field_shape.argtypes = [C.c_void_p, i32p]
    L.sc_hip_field_shape.restype = C.c_int
    L.sc_hip_field_store.argtypes = [C.c_void_p, f32p, C.c_size_t]
    L.sc_hip_field_store.restype = C.c_int
    L.sc_hip_field_finish.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    L.sc_hip_field_finish.restype = C.c_int
    L.sc_hip_field_lowmode.argtypes = [C.c_void_p]
    L.sc_hip_field_lowmode.restype = C.c_int
    L.sc_hip_field_time_sweeps.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.POINTER(C.c_float)]
    L.sc_hip_field_time_sweeps.restype = C.c_int
    L.sc_hip_pool_create.argtypes = [C.c_int, C.c_int]
    L.sc_hip_pool_create.restype = C.c_void_p
    L.sc_hip_pool_destroy.argtypes = [C.c_void_p]
    L.sc_hip_pool_destroy.restype = None
    L.sc_hip_pool_size.argtypes = [C.c_void_p]
    L.sc_hip_pool_size.restype = C.c_int
    L.sc_hip_pool_instance.argtypes = [C.c_void_p, C.c_int]
    L.sc_hip_pool_instance.restype = C.c_void_p
    L.sc_hip_pool_set_solver.argtypes = [C.c_void_p, C.POINTER(SolverOpts)]
    L.sc_hip_pool_set_solver.restype = C.c_int
    L.sc_hip_pool_run.argtypes = [C.c_void_p, C.POINTER(BatchJob), C.c_int, C.c_int]
    L.sc_hip_pool_run.restype = C.c_int
    L.sc_hip_pool_set_group.argtypes = [C.c_void_p, C.c_int]
    L.sc_hip_pool_set_group.restype = C.c_int
    L.sc_hip_run_device_batch.argtypes = [C.c_void_p, C.POINTER(BatchJob), C.c_int]
    L.sc_hip_run_device_batch.restype = C.c_int
    L.sc_hip_time_cycle0.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_float)]
    L.sc_hip_time_cycle0.restype = C.c_int
    L.sc_hip_time_coarse_chain.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_int)]
    L.sc_hip_time_coarse_chain.restype = C.c_int
    L.sc_hip_time_tail_phases.argtypes = [C.c_void_p, C.POINTER(C.c_ulonglong)]
    L.sc_hip_time_tail_phases.restype = C.c_int
    L.sc_hip_time_cycle0_form.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float)]
    L.sc_hip_time_cycle0_form.restype = C.c_int
    L.sc_hip_reference_tables_singular.argtypes = [C.c_int, C.c_int]
    L.sc_hip_reference_tables_singular.restype = C.c_int
    L.sc_hip_selftest_host.argtypes = []
    L.sc_hip_selftest_host.restype = C.c_int
    L.sc_hip_cycle0_form.argtypes = [i32p, C.c_int, i32p]
    L.sc_hip_cycle0_form.restype = C.c_int
    L.sc_hip_coarse_tile_plan.argtypes = [i32p, i32p]
    L.sc_hip_coarse_tile_plan.restype = C.c_int
    L.sc_hip_cycle0_plan.argtypes = [i32p, i32p, C.c_int]
    L.sc_hip_cycle0_plan.restype = C.c_int
    L.sc_hip_pcg_plan.argtypes = [C.c_int] * 4 + [C.POINTER(C.c_longlong)]
    L.sc_hip_pcg_plan.restype = C.c_int
    L.sc_hip_fused_schedule.argtypes = [i32p, i32p, C.c_int, i32p, C.c_int]
    L.sc_hip_fused_schedule.restype = C.c_int
    L.sc_hip_restore_spans.argtypes = [C.c_longlong] + [C.c_int] * 5 + [C.POINTER(C.c_longlong), C.c_int]
    L.sc_hip_restore_spans.restype = C.c_int
    L.sc_hip_plan_groups.argtypes = [i32p, C.c_int, C.c_int, C.POINTER(SolverOpts), i32p, i32p]
    L.sc_hip_plan_groups.restype = C.c_int
    L.sc_hip_plan_size.argtypes = [C.c_int, C.c_int, C.POINTER(SolverOpts), i32p]
    L.sc_hip_plan_groups_pool.argtypes = [i32p, C.c_int, C.c_int, C.c_int, C.POINTER(SolverOpts), i32p, i32p]
    L.sc_hip_plan_groups_pool.restype = C.c_int
    L.sc_hip_plan_prepare.argtypes = [i32p, C.c_int, C.POINTER(SolverOpts)]
    L.sc_hip_plan_prepare.restype = C.c_int
    L.sc_hip_plan_cache_clear.argtypes = []
    L.sc_hip_plan_cache_clear.restype = None
    L.sc_hip_plan_size.restype = C.c_int
    L.sc_hip_default_edit_params.argtypes = [C.POINTER(EditParams), C.c_int]
    L.sc_hip_default_edit_params.restype = None
    L.sc_hip_edit.argtypes = [C.c_void_p, C.POINTER(EditParams)] + _IMG + [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    L.sc_hip_edit.restype = C.c_int
    L.sc_hip_edit_device.argtypes = [C.c_void_p, C.POINTER(EditParams)] + _IMG + [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_bool]
    L.sc_hip_edit_device.restype = C.c_int
    L.sc_hip_edit_device_batch.argtypes = [C.c_void_p, C.POINTER(EditParams), C.POINTER(EditJob), C.c_int]
    L.sc_hip_edit_device_batch.restype = C.c_int
    L.sc_hip_pool_edit.argtypes = [C.c_void_p, C.POINTER(EditParams), C.POINTER(EditJob), C.c_int, C.c_int]
    L.sc_hip_pool_edit.restype = C.c_int
    L.sc_hip_plan_edit_groups_pool.argtypes = [i32p, C.c_int, C.c_int, C.c_int, i32p]
    L.sc_hip_plan_edit_groups_pool.restype = C.c_int
    L.sc_hip_edit_rhs.argtypes = [C.c_void_p, C.POINTER(EditParams)] + _IMG + [C.c_void_p, C.c_int, u8p, f32p, C.c_size_t]
    L.sc_hip_edit_rhs.restype = C.c_int
    L.sc_hip_canny.argtypes = [C.c_void_p] + _IMG + [C.c_float, C.c_float, C.c_int, u8p, u8p, i32p]
    L.sc_hip_canny.restype = C.c_int
    L.sc_hip_edit_counts.argtypes = [C.c_void_p, i32p]
    L.sc_hip_edit_counts.restype = C.c_int
    L.sc_hip_poisson_check.argtypes = [C.POINTER(PoissonParams), C.POINTER(PoissonLayout)]
    L.sc_hip_poisson_check.restype = C.c_int
    L.sc_hip_poisson_device.argtypes = [C.c_void_p, C.POINTER(PoissonParams), C.POINTER(PoissonLayout), C.POINTER(PoissonJob), C.c_int,
                                        C.c_bool]
    L.sc_hip_poisson_device.restype = C.c_int
    L.sc_hip_poisson.argtypes = [C.c_void_p, C.POINTER(PoissonParams), C.POINTER(PoissonLayout)] + [C.c_void_p] * 5
    L.sc_hip_poisson.restype = C.c_int
    L.sc_hip_screened_check.argtypes = [C.POINTER(ScreenedParams), C.POINTER(PoissonLayout)]
    L.sc_hip_screened_check.restype = C.c_int
    L.sc_hip_screened_device.argtypes = [C.c_void_p, C.POINTER(ScreenedParams), C.POINTER(PoissonLayout), C.POINTER(ScreenedJob), C.c_int,
                                         C.c_bool]
    L.sc_hip_screened_device.restype = C.c_int
    L.sc_hip_screened.argtypes = [C.c_void_p, C.POINTER(ScreenedParams), C.POINTER(PoissonLayout)] + [C.c_void_p] * 6
    L.sc_hip_screened.restype = C.c_int
    L.sc_hip_weighted_check.argtypes = [C.POINTER(WeightedParams), C.POINTER(PoissonLayout)]
    L.sc_hip_weighted_check.restype = C.c_int
    L.sc_hip_weighted_device.argtypes = [C.c_void_p, C.POINTER(WeightedParams), C.POINTER(PoissonLayout), C.POINTER(WeightedJob), C.c_int,
                                         C.c_bool]
    L.sc_hip_weighted_device.restype = C.c_int
    L.sc_hip_weighted.argtypes = [C.c_void_p, C.POINTER(WeightedParams), C.POINTER(PoissonLayout)] + [C.c_void_p] * 7
    L.sc_hip_weighted.restype = C.c_int
    L.sc_hip_wls_check.argtypes = [C.POINTER(WlsParams), C.POINTER(PoissonLayout)]
    L.sc_hip_wls_check.restype = C.c_int
    L.sc_hip_wls_device.argtypes = [C.c_void_p, C.POINTER(WlsParams), C.POINTER(PoissonLayout), C.POINTER(WlsJob), C.c_int, C.c_bool]
    L.sc_hip_wls_device.restype = C.c_int
    L.sc_hip_wls.argtypes = [C.c_void_p, C.POINTER(WlsParams), C.POINTER(PoissonLayout)] + [C.c_void_p] * 9
    L.sc_hip_wls.restype = C.c_int
    L.sc_hip_region_check.argtypes = [C.POINTER(RegionParams), C.POINTER(PoissonLayout)]
    L.sc_hip_region_check.restype = C.c_int
    L.sc_hip_region_device.argtypes = [C.c_void_p, C.POINTER(RegionParams), C.POINTER(PoissonLayout), C.POINTER(RegionJob), C.c_int, C.c_bool]
    L.sc_hip_region_device.restype = C.c_int
    L.sc_hip_region.argtypes = [C.c_void_p, C.POINTER(RegionParams), C.POINTER(PoissonLayout)] + [C.c_void_p] * 10
    L.sc_hip_region.restype = C.c_int
    L.sc_hip_volume_check.argtypes = [C.POINTER(VolumeParams), C.POINTER(PoissonLayout)]
    L.sc_hip_volume_check.restype = C.c_int
    L.sc_hip_volume_device.argtypes = [C.c_void_p, C.POINTER(VolumeParams), C.POINTER(PoissonLayout), C.POINTER(VolumeJob), C.c_int, C.c_bool]
    L.sc_hip_volume_device.restype = C.c_int
    L.sc_hip_volume.argtypes = [C.c_void_p, C.POINTER(VolumeParams), C.POINTER(PoissonLayout)] + [C.c_void_p] * 9
    L.sc_hip_volume.restype = C.c_int
    L.sc_hip_volume_wls_check.argtypes = [C.POINTER(VolumeWlsParams), C.POINTER(PoissonLayout)]
    L.sc_hip_volume_wls_check.restype = C.c_int
    L.sc_hip_volume_wls_device.argtypes = [C.c_void_p, C.POINTER(VolumeWlsParams), C.POINTER(PoissonLayout), C.POINTER(VolumeWlsJob), C.c_int,
                                           C.c_bool]
    L.sc_hip_volume_wls_device.restype = C.c_int
    L.sc_hip_volume_wls.argtypes = [C.c_void_p, C.POINTER(VolumeWlsParams), C.POINTER(PoissonLayout)] + [C.c_void_p] * 12
    L.sc_hip_volume_wls.restype = C.c_int
    L.sc_hip_volume_flow_check.argtypes = [C.POINTER(VolumeWlsParams), C.POINTER(PoissonLayout)]
    L.sc_hip_volume_flow_check.restype = C.c_int
    L.sc_hip_volume_flow_device.argtypes = [C.c_void_p, C.POINTER(VolumeWlsParams), C.POINTER(PoissonLayout), C.POINTER(VolumeFlowJob), C.c_int,
                                            C.c_bool]
    L.sc_hip_volume_flow_device.restype = C.c_int
    L.sc_hip_volume_flow.argtypes = [C.c_void_p, C.POINTER(VolumeWlsParams), C.POINTER(PoissonLayout)] + [C.c_void_p] * 14
    L.sc_hip_volume_flow.restype = C.c_int
    L.sc_hip_volume_subflow_check.argtypes = [C.POINTER(VolumeWlsParams), C.POINTER(PoissonLayout)]
    L.sc_hip_volume_subflow_check.restype = C.c_int
    L.sc_hip_volume_subflow_device.argtypes = [C.c_void_p, C.POINTER(VolumeWlsParams), C.POINTER(PoissonLayout), C.POINTER(VolumeFlowJob), C.c_int,
                                               C.c_bool]
    L.sc_hip_volume_subflow_device.restype = C.c_int
    L.sc_hip_volume_subflow.argtypes = [C.c_void_p, C.POINTER(VolumeWlsParams), C.POINTER(PoissonLayout)] + [C.c_void_p] * 14
    L.sc_hip_volume_subflow.restype = C.c_int
    L.sc_hip_volume_robust_check.argtypes = [C.POINTER(VolumeRobustParams), C.POINTER(PoissonLayout)]
    L.sc_hip_volume_robust_check.restype = C.c_int
    L.sc_hip_volume_robust_device.argtypes = [C.c_void_p, C.POINTER(VolumeRobustParams), C.POINTER(PoissonLayout), C.POINTER(VolumeRobustJob),
                                              C.c_int, C.c_bool]
    L.sc_hip_volume_robust_device.restype = C.c_int
    L.sc_hip_volume_robust.argtypes = [C.c_void_p, C.POINTER(VolumeRobustParams), C.POINTER(PoissonLayout)] + [C.c_void_p] * 11
    L.sc_hip_volume_robust.restype = C.c_int
    L.sc_hip_volume_flow_robust_check.argtypes = [C.POINTER(VolumeRobustParams), C.POINTER(PoissonLayout)]
    L.sc_hip_volume_flow_robust_check.restype = C.c_int
    L.sc_hip_volume_flow_robust_device.argtypes = [C.c_void_p, C.POINTER(VolumeRobustParams), C.POINTER(PoissonLayout),
                                                   C.POINTER(VolumeFlowRobustJob), C.c_int, C.c_bool]
    L.sc_hip_volume_flow_robust_device.restype = C.c_int
    L.sc_hip_volume_flow_robust.argtypes = [C.c_void_p, C.POINTER(VolumeRobustParams), C.POINTER(PoissonLayout)] + [C.c_void_p] * 13
    L.sc_hip_volume_flow_robust.restype = C.c_int
    L.sc_hip_volume_subflow_robust_check.argtypes = [C.POINTER(VolumeRobustParams), C.POINTER(PoissonLayout)]
    L.sc_hip_volume_subflow_robust_check.restype = C.c_int
    L.sc_hip_volume_subflow_robust_device.argtypes = [C.c_void_p, C.POINTER(VolumeRobustParams), C.POINTER(PoissonLayout),
                                                      C.POINTER(VolumeFlowRobustJob), C.c_int, C.c_bool]
    L.sc_hip_volume_subflow_robust_device.restype = C.c_int
    L.sc_hip_volume_subflow_robust.argtypes = [C.c_void_p, C.POINTER(VolumeRobustParams), C.POINTER(PoissonLayout)] + [C.c_void_p] * 13
    L.sc_hip_volume_subflow_robust.restype = C.c_int
    L.sc_hip_volume_coupled_check.argtypes = [C.POINTER(VolumeRobustParams), C.c_int, C.POINTER(PoissonLayout)]
    L.sc_hip_volume_coupled_check.restype = C.c_int
    L.sc_hip_volume_coupled_device.argtypes = [C.c_void_p, C.POINTER(VolumeRobustParams), C.c_int, C.POINTER(PoissonLayout),
                                               C.POINTER(VolumeRobustJob), C.c_int, C.c_bool]
    L.sc_hip_volume_coupled_device.restype = C.c_int
    L.sc_hip_volume_coupled.argtypes = [C.c_void_p, C.POINTER(VolumeRobustParams), C.c_int, C.POINTER(PoissonLayout)] + [C.c_void_p] * 11
    L.sc_hip_volume_coupled.restype = C.c_int
    L.sc_hip_volume_flow_coupled_check.argtypes = [C.POINTER(VolumeRobustParams), C.c_int, C.POINTER(PoissonLayout)]
    L.sc_hip_volume_flow_coupled_check.restype = C.c_int
    L.sc_hip_volume_flow_coupled_device.argtypes = [C.c_void_p, C.POINTER(VolumeRobustParams), C.c_int, C.POINTER(PoissonLayout),
                                                    C.POINTER(VolumeFlowRobustJob), C.c_int, C.c_bool]
    L.sc_hip_volume_flow_coupled_device.restype = C.c_int
    L.sc_hip_volume_flow_coupled.argtypes = [C.c_void_p, C.POINTER(VolumeRobustParams), C.c_int, C.POINTER(PoissonLayout)] + [C.c_void_p] * 13
    L.sc_hip_volume_flow_coupled.restype = C.c_int
    L.sc_hip_region_robust_check.argtypes = [C.POINTER(RobustParams), C.POINTER(PoissonLayout)]
    L.sc_hip_region_robust_check.restype = C.c_int
    L.sc_hip_region_robust_device.argtypes = [C.c_void_p, C.POINTER(RobustParams), C.POINTER(PoissonLayout), C.POINTER(RegionRobustJob), C.c_int,
                                              C.c_bool]
    L.sc_hip_region_robust_device.restype = C.c_int
    L.sc_hip_region_robust.argtypes = [C.c_void_p, C.POINTER(RobustParams), C.POINTER(PoissonLayout)] + [C.c_void_p] * 9
    L.sc_hip_region_robust.restype = C.c_int
    L.sc_hip_robust_check.argtypes = [C.POINTER(RobustParams), C.POINTER(PoissonLayout)]
    L.sc_hip_robust_check.restype = C.c_int
    L.sc_hip_robust_device.argtypes = [C.c_void_p, C.POINTER(RobustParams), C.POINTER(PoissonLayout), C.POINTER(RobustJob), C.c_int, C.c_bool]
    L.sc_hip_robust_device.restype = C.c_int
    L.sc_hip_robust.argtypes = [C.c_void_p, C.POINTER(RobustParams), C.POINTER(PoissonLayout)] + [C.c_void_p] * 8
    L.sc_hip_robust.restype = C.c_int
    L.sc_hip_robust_trace.argtypes = [C.c_void_p, f64p, i32p, C.c_int]
    L.sc_hip_robust_trace.restype = C.c_int
    L.sc_hip_bounded_check.argtypes = [C.POINTER(BoundedParams), C.POINTER(PoissonLayout)]
    L.sc_hip_bounded_check.restype = C.c_int
    L.sc_hip_bounded_device.argtypes = [C.c_void_p, C.POINTER(BoundedParams), C.POINTER(PoissonLayout), C.POINTER(BoundedJob), C.c_int, C.c_bool]
    L.sc_hip_bounded_device.restype = C.c_int
    L.sc_hip_bounded.argtypes = [C.c_void_p, C.POINTER(BoundedParams), C.POINTER(PoissonLayout)] + [C.c_void_p] * 12
    L.sc_hip_bounded.restype = C.c_int
    L.sc_hip_bounded_trace.argtypes = [C.c_void_p, i32p, i32p, i32p, C.c_int]
    L.sc_hip_bounded_trace.restype = C.c_int
    _lib = L
    return L


def _img(a: np.ndarray):
    """numpy HxW[x3] uint8 (row-contiguous, arbitrary row stride) -> (ptr, cols, rows, step)."""
    if a.dtype != np.uint8:
        raise TypeError("images must be uint8")
    if a.ndim == 3 and a.shape[2] == 1:
        a = a[:, :, 0]
    ch = 1 if a.ndim == 2 else a.shape[2]
    if a.strides[-1] != 1 or (a.ndim == 3 and a.strides[1] != ch):
        raise ValueError("image rows must be contiguous (cv::Mat layout)")
    return a.ctypes.data, a.shape[1], a.shape[0], a.strides[0]


def poisson_layout_of(a: np.ndarray) -> PoissonLayout:
    """The PoissonLayout of a float32 array of shape H x W or H x W x C (numpy's strides, in floats)."""
    if a.dtype != np.float32:
        raise TypeError("Poisson arrays must be float32")
    if a.ndim not in (2, 3):
        raise ValueError("Poisson arrays are H x W or H x W x C")
    if any(s % 4 for s in a.strides):
        raise ValueError("strides must be whole floats")
    H, W = a.shape[:2]
    Cn = a.shape[2] if a.ndim == 3 else 1
    rs, cs = a.strides[0] // 4, a.strides[1] // 4
    chs = a.strides[2] // 4 if a.ndim == 3 else 1
    return PoissonLayout(W, H, Cn, cs, rs, chs)


def _layout_key(l: PoissonLayout):
    return (l.cols, l.rows, l.channels, l.col_stride, l.row_stride, l.channel_stride)


def _check_call(fn, params, layout, **fields) -> int:
    """A host-only sc_hip_*_check: the layout as a PoissonLayout or as keyword fields."""
    if layout is None:
        layout = PoissonLayout(*(int(fields[name]) for name, _ in PoissonLayout._fields_))
    return int(getattr(load(), fn)(C.byref(params), C.byref(layout)))


def _same_shape_f32(name, a, ref):
    """a is a float32 numpy array of ref's shape, or the families' TypeError / ValueError."""
    if not isinstance(a, np.ndarray) or a.dtype != np.float32:
        raise TypeError(f"{name} must be a float32 numpy array")
    if a.shape != ref.shape:
        raise ValueError(f"{name} has shape {a.shape}, the problem {ref.shape}")


def poisson_check(kind: int = SC_POISSON_GUIDANCE, tol: float = 0.0, layout: "PoissonLayout | None" = None, *, cols=None, rows=None,
                  channels=None, col_stride=None, row_stride=None, channel_stride=None) -> int:
    """Host-only sc_hip_poisson_check: SC_OK or the code a call with this kind, tol and layout returns before it runs anything.  The
    layout as a PoissonLayout or as keyword fields."""
    return _check_call("sc_hip_poisson_check", PoissonParams(int(kind), float(tol)), layout, cols=cols, rows=rows, channels=channels,
                       col_stride=col_stride, row_stride=row_stride, channel_stride=channel_stride)


def poisson_arrays(boundary, gx=None, gy=None, lap=None, out=None, neumann=False, free_sides="", periodic=""):
    """Checks a Poisson problem's numpy arrays before any device is touched: (kind, layout, boundary, gx, gy, lap, out) with every array
    float32 and of boundary's shape.  The layout is numpy's strides when all arrays share them; otherwise the arrays are made
    contiguous (out then stays the caller's and is written back by the caller: see Instance.poisson).  neumann: the kind carries
    SC_POISSON_NEUMANN and boundary may be None (the shape is then gx's or lap's).  free_sides: the sides without a Dirichlet line,
    a string over "lrtb" (free_side_bits); all four are the Neumann problem, with fewer boundary is required.  periodic: the axes
    that wrap, "x", "y" or "xy" (periodic_bits; border_bits' ValueErrors); boundary may be None exactly when no side keeps a
    Dirichlet line (no_dirichlet)."""
    free = border_bits(free_sides, neumann, periodic)
    neumann = no_dirichlet(free)
    if (gx is None) != (gy is None):
        raise ValueError("gx and gy go together")
    if (gx is None) == (lap is None):
        raise ValueError("give either gx and gy or lap")
    kind = SC_POISSON_LAPLACIAN if lap is not None else SC_POISSON_GUIDANCE
    kind |= free
    if boundary is None and not neumann:
        raise ValueError("boundary may be None only for a Neumann problem (neumann=True) or when no side keeps a Dirichlet line")
    arrays = {"boundary": boundary, "gx": gx, "gy": gy, "lap": lap, "out": out}
    first = boundary if boundary is not None else (lap if lap is not None else gx)
    for name, a in arrays.items():
        if a is None:
            continue
        if not isinstance(a, np.ndarray) or a.dtype != np.float32:
            raise TypeError(f"{name} must be a float32 numpy array")
        if not isinstance(first, np.ndarray):
            raise TypeError("Poisson arrays must be float32 numpy arrays")
        if a.shape != first.shape:
            raise ValueError(f"{name} has shape {a.shape}, the problem {first.shape}")
    if first.ndim not in (2, 3) or (first.ndim == 3 and not 1 <= first.shape[2] <= 4):
        raise ValueError("Poisson arrays are H x W or H x W x C with C in 1..4")
    if out is not None and not out.flags.writeable:
        raise ValueError("out must be writeable")
    return kind, boundary, gx, gy, lap, out


def screened_check(kind: int = SC_POISSON_GUIDANCE, lam: float = 1.0, layout: "PoissonLayout | None" = None, *, cols=None, rows=None,
                   channels=None, col_stride=None, row_stride=None, channel_stride=None) -> int:
    """Host-only sc_hip_screened_check: SC_OK or the code a screened call with this kind, lambda and layout returns before it runs
    anything.  The layout as a PoissonLayout or as keyword fields."""
    return _check_call("sc_hip_screened_check", ScreenedParams(int(kind), float(lam)), layout, cols=cols, rows=rows, channels=channels,
                       col_stride=col_stride, row_stride=row_stride, channel_stride=channel_stride)


def screened_arrays(data, gx=None, gy=None, lap=None, lam=None, boundary=None, out=None, neumann=False, free_sides="", periodic=""):
    """Checks a screened problem's numpy arrays and lambda before any device is touched: (kind, data, gx, gy, lap, boundary, out), every
    array float32 and of data's shape (poisson_arrays' rules).  A Dirichlet problem (neumann=False) needs boundary; a Neumann one
    ignores it.  free_sides, periodic: as poisson_arrays'; with a Dirichlet line left on any side boundary is required, without one it
    is ignored."""
    all_free = no_dirichlet(border_bits(free_sides, neumann, periodic))
    if data is None:
        raise ValueError("a screened solve needs its data term")
    if lam is None or not np.isfinite(lam) or not lam > 0:
        raise ValueError("lam must be finite and > 0")
    if all_free:
        boundary = None
    elif boundary is None:
        raise ValueError("a Dirichlet screened solve needs boundary (neumann=True: none)")
    kind, _, gx, gy, lap, out = poisson_arrays(data, gx, gy, lap, out, neumann, free_sides, periodic)
    if boundary is not None:
        _same_shape_f32("boundary", boundary, data)
    return kind, data, gx, gy, lap, boundary, out


def weighted_check(kind: int = SC_POISSON_GUIDANCE, tol: float = 0.0, max_iters: int = 0, precond_lambda: float = 0.0,
                   layout: "PoissonLayout | None" = None, *, cols=None, rows=None, channels=None, col_stride=None, row_stride=None,
                   channel_stride=None) -> int:
    """Host-only sc_hip_weighted_check: SC_OK or the code a weighted call with these parameters and this layout returns before it runs
    anything.  The layout as a PoissonLayout or as keyword fields."""
    p = WeightedParams(int(kind), float(tol), int(max_iters), float(precond_lambda))
    return _check_call("sc_hip_weighted_check", p, layout, cols=cols, rows=rows, channels=channels, col_stride=col_stride,
                       row_stride=row_stride, channel_stride=channel_stride)


def weighted_arrays(data, weight, gx=None, gy=None, lap=None, boundary=None, out=None, neumann=False, free_sides="", periodic=""):
    """Checks a weighted problem's numpy arrays before any device is touched: (kind, data, weight, gx, gy, lap, boundary, out), every
    array float32 and of data's shape, except that a 2-D weight beside 3-D data is broadcast over the channels.  Neither gx, gy nor lap:
    zero guidance (lap = 0).  boundary is required when a side keeps a Dirichlet line and ignored otherwise."""
    all_free = no_dirichlet(border_bits(free_sides, neumann, periodic))
    if data is None or weight is None:
        raise ValueError("a weighted solve needs its data term and its weights")
    _same_shape_f32("data", data, data)
    if isinstance(weight, np.ndarray) and weight.ndim == 2 and data.ndim == 3 and weight.shape == data.shape[:2]:
        weight = np.ascontiguousarray(np.broadcast_to(weight[:, :, None], data.shape))
    _same_shape_f32("weight", weight, data)
    if gx is None and gy is None and lap is None:
        lap = np.zeros(data.shape, np.float32)
    if all_free:
        boundary = None
    elif boundary is None:
        raise ValueError("a weighted solve with a Dirichlet line needs boundary")
    kind, _, gx, gy, lap, out = poisson_arrays(data, gx, gy, lap, out, neumann, free_sides, periodic)
    if boundary is not None:
        _same_shape_f32("boundary", boundary, data)
    return kind, data, weight, gx, gy, lap, boundary, out


def wls_check(kind: int = SC_POISSON_GUIDANCE, tol: float = 0.0, max_iters: int = 0, precond_lambda: float = 0.0, precond_smooth: float = 0.0,
              layout: "PoissonLayout | None" = None, *, cols=None, rows=None, channels=None, col_stride=None, row_stride=None,
              channel_stride=None) -> int:
    """Host-only sc_hip_wls_check: SC_OK or the code a WLS call with these parameters and this layout returns before it runs anything.
    The layout as a PoissonLayout or as keyword fields."""
    p = WlsParams(int(kind), float(tol), int(max_iters), float(precond_lambda), float(precond_smooth))
    return _check_call("sc_hip_wls_check", p, layout, cols=cols, rows=rows, channels=channels, col_stride=col_stride,
                       row_stride=row_stride, channel_stride=channel_stride)


def border_unknowns(kind: int, H: int, W: int):
    """Boolean H x W: the pixels a call of this kind calls unknowns (everything but its Dirichlet lines) -- where a region call reads state."""
    px, py = bool(kind & SC_POISSON_PERIODIC_X), bool(kind & SC_POISSON_PERIODIC_Y)
    neu = bool(kind & SC_POISSON_NEUMANN)
    u = np.ones((H, W), bool)
    if not px:
        u[:, 0] &= neu or bool(kind & SC_POISSON_FREE_LEFT)
        u[:, -1] &= neu or bool(kind & SC_POISSON_FREE_RIGHT)
    if not py:
        u[0] &= neu or bool(kind & SC_POISSON_FREE_TOP)
        u[-1] &= neu or bool(kind & SC_POISSON_FREE_BOTTOM)
    return u


def live_links(kind: int, H: int, W: int):
    """(live_x, live_y), boolean H x W: the elements of smooth_x / smooth_y that a WLS call of this kind reads -- the links with at least
    one end among the unknowns; the last column / row holds the wrapping link of a periodic axis and is not live otherwise."""
    px, py = bool(kind & SC_POISSON_PERIODIC_X), bool(kind & SC_POISSON_PERIODIC_Y)
    unknown = border_unknowns(kind, H, W)
    lx = unknown | np.roll(unknown, -1, 1)
    ly = unknown | np.roll(unknown, -1, 0)
    if not px:
        lx[:, -1] = False
    if not py:
        ly[-1] = False
    return lx, ly


def wls_arrays(data, weight, smooth_x, smooth_y, gx=None, gy=None, lap=None, boundary=None, out=None, neumann=False, free_sides="",
               periodic=""):
    """Checks a WLS problem's numpy arrays before any device is touched: (kind, data, weight, smooth_x, smooth_y, gx, gy, lap, boundary,
    out), weighted_arrays' rules for all but the link weights.  smooth_x, smooth_y: float32, of data's shape or H x W (broadcast over
    the channels), finite and > 0 on every live link (live_links); what is not live may hold anything."""
    if smooth_x is None or smooth_y is None:
        raise ValueError("a WLS solve needs its link weights smooth_x and smooth_y")
    kind, data, weight, gx, gy, lap, boundary, out = weighted_arrays(data, weight, gx, gy, lap, boundary, out, neumann, free_sides, periodic)
    lx, ly = live_links(kind, *data.shape[:2])
    links = []
    for name, a, live in (("smooth_x", smooth_x, lx), ("smooth_y", smooth_y, ly)):
        if isinstance(a, np.ndarray) and a.ndim == 2 and data.ndim == 3 and a.shape == data.shape[:2]:
            a = np.ascontiguousarray(np.broadcast_to(a[:, :, None], data.shape))
        _same_shape_f32(name, a, data)
        v = a[live]
        if not (np.isfinite(v).all() and (v > 0).all()):
            raise ValueError(f"{name} must be finite and > 0 on every live link")
        links.append(a)
    return kind, data, weight, links[0], links[1], gx, gy, lap, boundary, out


def region_check(kind: int = SC_POISSON_GUIDANCE, tol: float = 0.0, max_iters: int = 0, precond_lambda: float = 0.0, precond_smooth: float = 0.0,
                 layout: "PoissonLayout | None" = None, *, cols=None, rows=None, channels=None, col_stride=None, row_stride=None,
                 channel_stride=None) -> int:
    """Host-only sc_hip_region_check: SC_OK or the code a region call with these parameters and this layout returns before it runs
    anything.  The layout as a PoissonLayout or as keyword fields."""
    p = RegionParams(int(kind), float(tol), int(max_iters), float(precond_lambda), float(precond_smooth))
    return _check_call("sc_hip_region_check", p, layout, cols=cols, rows=rows, channels=channels, col_stride=col_stride,
                       row_stride=row_stride, channel_stride=channel_stride)


def region_unpinned(kind: int, state, weight=None):
    """Boolean array of state's shape (H x W or H x W x C): the UNKNOWN pixels of connected components that nothing pins -- no KNOWN
    neighbour, no Dirichlet line of the kind next to them and no positive weight (weight None: no data term).  A flood fill in numpy from
    the pinned pixels through the links between UNKNOWN pixels; a region call does not detect such components (its result there is
    some constant in the guidance form)."""
    st = np.asarray(state)
    st3 = st[:, :, None] if st.ndim == 2 else st
    H, W = st3.shape[:2]
    px, py = bool(kind & SC_POISSON_PERIODIC_X), bool(kind & SC_POISSON_PERIODIC_Y)
    inside = border_unknowns(kind, H, W)[:, :, None]
    unk = (st3 == SC_REGION_UNKNOWN) & inside
    # a Dirichlet pixel acts as a KNOWN one
    fixed = ((st3 == SC_REGION_KNOWN) & inside) | np.broadcast_to(~inside, st3.shape)

    def neighbours(a):          # the four shifted copies of a: a's value at the pixel across each link, False where there is none
        out = []
        for axis, wraps in ((1, px), (0, py)):
            for step in (1, -1):
                r = np.roll(a, step, axis).copy()
                if not wraps:
                    edge = [slice(None)] * 3
                    edge[axis] = 0 if step == 1 else -1
                    r[tuple(edge)] = False
                out.append(r)
        return out

    pinned = unk & np.logical_or.reduce(neighbours(fixed))
    if weight is not None:
        w = np.asarray(weight)
        pinned |= unk & ((w[:, :, None] if w.ndim == 2 else w) > 0)
    while True:
        grown = pinned | (unk & np.logical_or.reduce(neighbours(pinned)))
        if (grown == pinned).all():
            break
        pinned = grown
    loose = unk & ~pinned
    return loose[:, :, 0] if st.ndim == 2 else loose


def region_arrays(data, state, weight=None, smooth_x=None, smooth_y=None, gx=None, gy=None, lap=None, boundary=None, out=None, neumann=False,
                  free_sides="", periodic=""):
    """Checks a region problem's numpy arrays before any device is touched: (kind, data, state, weight, smooth_x, smooth_y, gx, gy, lap,
    boundary, out).  data: float32, H x W or H x W x C.  state: of data's shape or H x W (broadcast over the channels); float32, an
    integer type or bool, holding SC_REGION_UNKNOWN (0, False), SC_REGION_KNOWN (1, True) or SC_REGION_OUTSIDE (2) at every pixel the
    borders call an unknown (border_unknowns; elsewhere it is not read) -- returned as float32.  weight: None (no data term) or as
    weighted_arrays'.  smooth_x, smooth_y: both None (every link 1) or as wls_arrays', judged on the device where they are live in the
    region.  Neither gx, gy nor lap: zero guidance (lap = 0).  boundary is required when a side keeps a Dirichlet line."""
    all_free = no_dirichlet(border_bits(free_sides, neumann, periodic))
    if data is None or state is None:
        raise ValueError("a region solve needs data and state")
    _same_shape_f32("data", data, data)
    if not isinstance(state, np.ndarray):
        raise TypeError("state must be a numpy array (float32, an integer type or bool)")
    if state.dtype != np.float32 and state.dtype != np.bool_ and not np.issubdtype(state.dtype, np.integer):
        raise TypeError("state must be float32, an integer type or bool")
    if (smooth_x is None) != (smooth_y is None):
        raise ValueError("smooth_x and smooth_y go together (both None: every link 1)")

    def broadcast(name, a):
        if a.ndim == 2 and data.ndim == 3 and a.shape == data.shape[:2]:
            a = np.ascontiguousarray(np.broadcast_to(a[:, :, None], data.shape))
        if a.shape != data.shape:
            raise ValueError(f"{name} has shape {a.shape}, the problem {data.shape}")
        return a

    state = broadcast("state", state.astype(np.float32))
    if gx is None and gy is None and lap is None:
        lap = np.zeros(data.shape, np.float32)
    if all_free:
        boundary = None
    elif boundary is None:
        raise ValueError("a region solve with a Dirichlet line needs boundary")
    kind, _, gx, gy, lap, out = poisson_arrays(data, gx, gy, lap, out, neumann, free_sides, periodic)
    read = border_unknowns(kind, *data.shape[:2])
    if not np.isin(state[read], (0.0, 1.0, 2.0)).all():
        raise ValueError("state must hold 0 (unknown), 1 (known) or 2 (outside) at every pixel the borders call an unknown")
    if boundary is not None:
        _same_shape_f32("boundary", boundary, data)
    if weight is not None:
        if not isinstance(weight, np.ndarray):
            raise TypeError("weight must be a float32 numpy array")
        weight = broadcast("weight", weight)
        _same_shape_f32("weight", weight, data)
    if smooth_x is not None:
        links = []
        for name, a in (("smooth_x", smooth_x), ("smooth_y", smooth_y)):
            if not isinstance(a, np.ndarray):
                raise TypeError(f"{name} must be a float32 numpy array")
            a = broadcast(name, a)
            _same_shape_f32(name, a, data)
            links.append(a)
        smooth_x, smooth_y = links
    return kind, data, state, weight, smooth_x, smooth_y, gx, gy, lap, boundary, out


def bounded_check(kind: int = SC_POISSON_GUIDANCE, lower: float = -np.inf, upper: float = np.inf, max_rounds: int = 0, tol: float = 0.0,
                  max_iters: int = 0, precond_lambda: float = 0.0, precond_smooth: float = 0.0, layout: "PoissonLayout | None" = None, *,
                  cols=None, rows=None, channels=None, col_stride=None, row_stride=None, channel_stride=None) -> int:
    """Host-only sc_hip_bounded_check: SC_OK or the code a bounded call with these parameters and this layout returns before it runs
    anything.  The layout as a PoissonLayout or as keyword fields."""
    p = BoundedParams(int(kind), float(tol), int(max_iters), float(precond_lambda), float(precond_smooth), float(lower), float(upper),
                      int(max_rounds))
    return _check_call("sc_hip_bounded_check", p, layout, cols=cols, rows=rows, channels=channels, col_stride=col_stride,
                       row_stride=row_stride, channel_stride=channel_stride)


def bounded_arrays(data, state, lower=None, upper=None, weight=None, smooth_x=None, smooth_y=None, gx=None, gy=None, lap=None, boundary=None,
                   out=None, neumann=False, free_sides="", periodic=""):
    """Checks a bounded problem's numpy arrays and bounds before any device is touched: (kind, data, state, weight, smooth_x, smooth_y,
    gx, gy, lap, boundary, out, lower scalar, upper scalar, lower array, upper array), region_arrays' rules for all but the bounds.
    lower, upper: None (no bound on that side), a number, or a float32 array of data's shape or H x W (broadcast over the channels);
    an array stands in for the scalar, which then reads -inf / +inf.  No bound may be NaN, and lower <= upper must hold at every
    UNKNOWN pixel the borders call an unknown (elsewhere the bounds are not read)."""
    kind, data, state, weight, sx, sy, gx, gy, lap, boundary, out = region_arrays(data, state, weight, smooth_x, smooth_y, gx, gy, lap, boundary,
                                                                                  out, neumann, free_sides, periodic)
    read = border_unknowns(kind, *data.shape[:2])
    read = (read if data.ndim == 2 else read[:, :, None]) & (state == SC_REGION_UNKNOWN)
    scalars, arrays = [], []
    for name, b, none in (("lower", lower, -np.inf), ("upper", upper, np.inf)):
        if isinstance(b, np.ndarray) and b.ndim:
            if b.ndim == 2 and data.ndim == 3 and b.shape == data.shape[:2]:
                b = np.ascontiguousarray(np.broadcast_to(b[:, :, None], data.shape))
            _same_shape_f32(name, b, data)
            if np.isnan(b[read]).any():
                raise ValueError(f"{name} must not be NaN at an UNKNOWN pixel")
            scalars.append(none)
            arrays.append(b)
        else:
            b = none if b is None else float(b)
            if b != b:
                raise ValueError(f"{name} must not be NaN")
            scalars.append(float(np.float32(b)))
            arrays.append(None)
    lo = arrays[0][read] if arrays[0] is not None else scalars[0]
    hi = arrays[1][read] if arrays[1] is not None else scalars[1]
    if np.any(np.asarray(lo) > np.asarray(hi)):
        raise ValueError("lower must not exceed upper at an UNKNOWN pixel")
    return (kind, data, state, weight, sx, sy, gx, gy, lap, boundary, out, *scalars, *arrays)


def volume_check(kind: int = SC_POISSON_GUIDANCE, frames: int = 2, frame_stride: int = 0, tau: float = 1.0, tol: float = 0.0, max_iters: int = 0,
                 precond_lambda: float = 0.0, layout: "PoissonLayout | None" = None, *, cols=None, rows=None, channels=None, col_stride=None,
                 row_stride=None, channel_stride=None) -> int:
    """Host-only sc_hip_volume_check: SC_OK or the code a volume call with these parameters and this layout returns before it runs
    anything.  The layout (of one frame) as a PoissonLayout or as keyword fields."""
    p = VolumeParams(int(kind), int(frames), int(frame_stride), float(tau), float(tol), int(max_iters), float(precond_lambda))
    return _check_call("sc_hip_volume_check", p, layout, cols=cols, rows=rows, channels=channels, col_stride=col_stride,
                       row_stride=row_stride, channel_stride=channel_stride)


def volume_arrays(data, state, weight=None, gx=None, gy=None, gt=None, lap=None, boundary=None, tau=1.0, neumann=False, free_sides="",
                  periodic=""):
    """Checks a volume problem's numpy arrays before any device is touched: (kind, data, state, weight, gx, gy, gt, lap, boundary), every
    array C-contiguous float32.  data: float32, T x H x W or T x H x W x C with T >= 2 and T * C <= 192.  state: of data's shape or
    T x H x W (broadcast over the channels), region_arrays' types and values.  weight: None or of data's shape (or T x H x W).  gx, gy: of
    data's shape, together; gt: (T - 1) x H x W (x C), only beside gx and gy; lap: of data's shape, instead of the three.  None of them:
    zero guidance.  boundary: of data's shape, required when a side keeps a Dirichlet line.  tau: finite and > 0."""
    all_free = no_dirichlet(border_bits(free_sides, neumann, periodic))
    if data is None or state is None:
        raise ValueError("a volume solve needs data and state")
    if not isinstance(data, np.ndarray) or data.dtype != np.float32:
        raise TypeError("data must be a float32 numpy array")
    if data.ndim not in (3, 4) or (data.ndim == 4 and not 1 <= data.shape[3] <= 4):
        raise ValueError("volume arrays are T x H x W or T x H x W x C with C in 1..4")
    T, Cn = data.shape[0], (data.shape[3] if data.ndim == 4 else 1)
    if T < 2:
        raise ValueError("a volume has at least 2 frames")
    if T * Cn > 192:
        raise ValueError("frames x channels must be at most 192")
    if not (np.isfinite(tau) and tau > 0):
        raise ValueError("tau must be finite and > 0")
    if not isinstance(state, np.ndarray):
        raise TypeError("state must be a numpy array (float32, an integer type or bool)")
    if state.dtype != np.float32 and state.dtype != np.bool_ and not np.issubdtype(state.dtype, np.integer):
        raise TypeError("state must be float32, an integer type or bool")

    def shaped(name, a, shape, broadcast=False):
        if not isinstance(a, np.ndarray) or a.dtype != np.float32:
            raise TypeError(f"{name} must be a float32 numpy array")
        if broadcast and a.ndim == 3 and len(shape) == 4 and a.shape == shape[:3]:
            a = np.broadcast_to(a[:, :, :, None], shape)
        if a.shape != shape:
            raise ValueError(f"{name} has shape {a.shape}, the problem {shape}")
        return np.ascontiguousarray(a)

    data = np.ascontiguousarray(data)
    state = shaped("state", state.astype(np.float32), data.shape, True)
    if (gx is None) != (gy is None):
        raise ValueError("gx and gy go together")
    if lap is not None and (gx is not None or gt is not None):
        raise ValueError("either guidance (gx, gy and, if wanted, gt) or lap, not both")
    if gt is not None and gx is None:
        raise ValueError("gt goes with gx and gy")
    if gx is None and lap is None:
        lap = np.zeros(data.shape, np.float32)
    kind = (SC_POISSON_LAPLACIAN if lap is not None else SC_POISSON_GUIDANCE) | border_bits(free_sides, neumann, periodic)
    gx, gy, lap = (None if a is None else shaped(n, a, data.shape) for n, a in (("gx", gx), ("gy", gy), ("lap", lap)))
    if gt is not None:
        gt = shaped("gt", gt, (T - 1,) + data.shape[1:])
    if all_free:
        boundary = None
    elif boundary is None:
        raise ValueError("a volume solve with a Dirichlet line needs boundary")
    else:
        boundary = shaped("boundary", boundary, data.shape)
    if weight is not None:
        weight = shaped("weight", weight, data.shape, True)
    read = border_unknowns(kind, *data.shape[1:3])
    if not np.isin(state[:, read], (0.0, 1.0, 2.0)).all():
        raise ValueError("state must hold 0 (unknown), 1 (known) or 2 (outside) at every pixel the borders call an unknown")
    return kind, data, state, weight, gx, gy, gt, lap, boundary


def volume_wls_check(kind: int = SC_POISSON_GUIDANCE, frames: int = 2, frame_stride: int = 0, tau: float = 1.0, time_periodic: int = 0,
                     tol: float = 0.0, max_iters: int = 0, precond_lambda: float = 0.0, precond_smooth: float = 0.0, precond_tau: float = 0.0,
                     layout: "PoissonLayout | None" = None, *, cols=None, rows=None, channels=None, col_stride=None, row_stride=None,
                     channel_stride=None) -> int:
    """Host-only sc_hip_volume_wls_check: SC_OK or the code a WLS volume call with these parameters and this layout returns before it
    runs anything.  The layout (of one frame) as a PoissonLayout or as keyword fields."""
    p = VolumeWlsParams(int(kind), int(frames), int(frame_stride), float(tau), int(time_periodic), float(tol), int(max_iters),
                        float(precond_lambda), float(precond_smooth), float(precond_tau))
    return _check_call("sc_hip_volume_wls_check", p, layout, cols=cols, rows=rows, channels=channels, col_stride=col_stride,
                       row_stride=row_stride, channel_stride=channel_stride)


def volume_wls_arrays(data, state, weight=None, smooth_x=None, smooth_y=None, smooth_t=None, gx=None, gy=None, gt=None, lap=None, boundary=None,
                      tau=1.0, loop=False, neumann=False, free_sides="", periodic=""):
    """Checks a WLS volume problem's numpy arrays before any device is touched: (kind, data, state, weight, smooth_x, smooth_y, smooth_t,
    gx, gy, gt, lap, boundary), every array C-contiguous float32.  volume_arrays' rules for all but the link weights and the temporal
    arrays' length: gt and smooth_t hold T - 1 frames, with loop (periodic time, T >= 3) T frames, the last of them the link from frame
    T - 1 to frame 0.  smooth_x, smooth_y: together, of data's shape or T x H x W (broadcast over the channels); smooth_t likewise at its
    own length.  Their values are judged on the device where their links are live."""
    if not isinstance(data, np.ndarray) or data.dtype != np.float32:
        raise TypeError("data must be a float32 numpy array")
    if data.ndim not in (3, 4):
        raise ValueError("volume arrays are T x H x W or T x H x W x C with C in 1..4")
    T = data.shape[0]
    if loop and T < 3:
        raise ValueError("a looping volume has at least 3 frames")
    if (smooth_x is None) != (smooth_y is None):
        raise ValueError("smooth_x and smooth_y go together (both None: every spatial link 1)")
    tshape = ((T if loop else T - 1),) + data.shape[1:]

    def shaped(name, a, shape):
        if not isinstance(a, np.ndarray) or a.dtype != np.float32:
            raise TypeError(f"{name} must be a float32 numpy array")
        if a.ndim == 3 and len(shape) == 4 and a.shape == shape[:3]:
            a = np.broadcast_to(a[:, :, :, None], shape)
        if a.shape != shape:
            raise ValueError(f"{name} has shape {a.shape}, the problem {shape}")
        return np.ascontiguousarray(a)

    if gt is not None and loop:          # (volume_arrays checks gt at T - 1 frames: the wrapping frame is checked here)
        if gx is None or lap is not None:
            raise ValueError("gt goes with gx and gy")
        gt_full = shaped("gt", gt, tshape)
        gt = gt_full[:T - 1]
    else:
        gt_full = None
    kind, data, state, weight, gx, gy, gt, lap, boundary = volume_arrays(data, state, weight, gx, gy, gt, lap, boundary, tau, neumann, free_sides,
                                                                         periodic)
    if gt_full is not None:
        gt = gt_full
    if smooth_x is not None:
        smooth_x, smooth_y = shaped("smooth_x", smooth_x, data.shape), shaped("smooth_y", smooth_y, data.shape)
    if smooth_t is not None:
        smooth_t = shaped("smooth_t", smooth_t, tshape)
    return kind, data, state, weight, smooth_x, smooth_y, smooth_t, gx, gy, gt, lap, boundary


def volume_flow_check(kind: int = SC_POISSON_GUIDANCE, frames: int = 2, frame_stride: int = 0, tau: float = 1.0, time_periodic: int = 0,
                      tol: float = 0.0, max_iters: int = 0, precond_lambda: float = 0.0, precond_smooth: float = 0.0, precond_tau: float = 0.0,
                      layout: "PoissonLayout | None" = None, *, cols=None, rows=None, channels=None, col_stride=None, row_stride=None,
                      channel_stride=None) -> int:
    """Host-only sc_hip_volume_flow_check: volume_wls_check's codes -- the flow call takes the WLS volume call's parameters unchanged."""
    p = VolumeWlsParams(int(kind), int(frames), int(frame_stride), float(tau), int(time_periodic), float(tol), int(max_iters),
                        float(precond_lambda), float(precond_smooth), float(precond_tau))
    return _check_call("sc_hip_volume_flow_check", p, layout, cols=cols, rows=rows, channels=channels, col_stride=col_stride,
                       row_stride=row_stride, channel_stride=channel_stride)


def volume_flow_shape(flow, frames: int, rows: int, cols: int, loop: bool = False) -> None:
    """volume_flow_planes' refusals of a flow's type and shape alone: nothing is converted"""
    if not isinstance(flow, np.ndarray) or not (np.issubdtype(flow.dtype, np.floating) or np.issubdtype(flow.dtype, np.integer)):
        raise TypeError("flow must be a numpy array of real numbers")
    want = ((frames if loop else frames - 1), rows, cols, 2)
    if flow.shape != want:
        raise ValueError(f"flow has shape {flow.shape}, the problem {want}: (dx, dy) per pixel of every frame that has a next one")


def volume_flow_planes(flow, frames: int, rows: int, cols: int, loop: bool = False):
    """A flow for a volume of `frames` frames of rows x cols pixels as the C layer wants it: (flow_x, flow_y), two C-contiguous float32
    arrays of shape (frames - 1) x rows x cols -- with loop `frames` of them, the last from the last frame onto frame 0.  flow: a real
    array of that shape x 2 holding (dx, dy): pixel (x, y) of frame t is pixel (x + dx, y + dy) of frame t + 1.  Values are rounded to
    whole numbers (np.rint); NaN and the infinities are kept: "no link here" (an occlusion)."""
    volume_flow_shape(flow, frames, rows, cols, loop)
    f = np.rint(flow.astype(np.float32))
    return np.ascontiguousarray(f[..., 0]), np.ascontiguousarray(f[..., 1])


def volume_subflow_check(kind: int = SC_POISSON_GUIDANCE, frames: int = 2, frame_stride: int = 0, tau: float = 1.0, time_periodic: int = 0,
                         tol: float = 0.0, max_iters: int = 0, precond_lambda: float = 0.0, precond_smooth: float = 0.0, precond_tau: float = 0.0,
                         layout: "PoissonLayout | None" = None, *, cols=None, rows=None, channels=None, col_stride=None, row_stride=None,
                         channel_stride=None) -> int:
    """Host-only sc_hip_volume_subflow_check: volume_flow_check's codes -- the sub-pixel call takes the flow call's parameters unchanged."""
    p = VolumeWlsParams(int(kind), int(frames), int(frame_stride), float(tau), int(time_periodic), float(tol), int(max_iters),
                        float(precond_lambda), float(precond_smooth), float(precond_tau))
    return _check_call("sc_hip_volume_subflow_check", p, layout, cols=cols, rows=rows, channels=channels, col_stride=col_stride,
                       row_stride=row_stride, channel_stride=channel_stride)


def volume_subflow_planes(flow, frames: int, rows: int, cols: int, loop: bool = False):
    """volume_flow_planes without the rounding: (flow_x, flow_y) as float32, the values as they are (sc_hip_volume_subflow takes a
    real-valued flow); NaN and the infinities are kept: "no link here"."""
    volume_flow_shape(flow, frames, rows, cols, loop)
    f = flow.astype(np.float32)
    return np.ascontiguousarray(f[..., 0]), np.ascontiguousarray(f[..., 1])


def volume_robust_params(kind, frames, frame_stride, tau=1.0, loop=False, p_grad=1.0, eps_grad=1e-3, p_time=1.0, eps_time=1e-3, p_data=2.0,
                         eps_data=1e-3, max_rounds=0, round_tol=0.0, tol=0.0, max_iters=0) -> VolumeRobustParams:
    return VolumeRobustParams(int(kind), int(frames), int(frame_stride), float(tau), 1 if loop else 0, float(p_grad), float(eps_grad), float(p_time),
                              float(eps_time), float(p_data), float(eps_data), int(max_rounds), float(round_tol), float(tol), int(max_iters))


def volume_robust_check(kind: int = SC_POISSON_GUIDANCE, frames: int = 2, frame_stride: int = 0, tau: float = 1.0, time_periodic: int = 0,
                        p_grad: float = 1.0, eps_grad: float = 1e-3, p_time: float = 1.0, eps_time: float = 1e-3, p_data: float = 2.0,
                        eps_data: float = 1e-3, max_rounds: int = 0, round_tol: float = 0.0, tol: float = 0.0, max_iters: int = 0,
                        layout: "PoissonLayout | None" = None, *, cols=None, rows=None, channels=None, col_stride=None, row_stride=None,
                        channel_stride=None) -> int:
    """Host-only sc_hip_volume_robust_check: SC_OK or the code a robust volume call with these parameters and this layout returns before
    it runs anything.  The layout (of one frame) as a PoissonLayout or as keyword fields."""
    p = VolumeRobustParams(int(kind), int(frames), int(frame_stride), float(tau), int(time_periodic), float(p_grad), float(eps_grad), float(p_time),
                           float(eps_time), float(p_data), float(eps_data), int(max_rounds), float(round_tol), float(tol), int(max_iters))
    return _check_call("sc_hip_volume_robust_check", p, layout, cols=cols, rows=rows, channels=channels, col_stride=col_stride,
                       row_stride=row_stride, channel_stride=channel_stride)


def volume_flow_robust_check(kind: int = SC_POISSON_GUIDANCE, frames: int = 2, frame_stride: int = 0, tau: float = 1.0, time_periodic: int = 0,
                             p_grad: float = 1.0, eps_grad: float = 1e-3, p_time: float = 1.0, eps_time: float = 1e-3, p_data: float = 2.0,
                             eps_data: float = 1e-3, max_rounds: int = 0, round_tol: float = 0.0, tol: float = 0.0, max_iters: int = 0,
                             layout: "PoissonLayout | None" = None, *, cols=None, rows=None, channels=None, col_stride=None, row_stride=None,
                             channel_stride=None) -> int:
    """Host-only sc_hip_volume_flow_robust_check: volume_robust_check's codes, then the flow call's refusal of a volume whose unknowns
    32 bits cannot index (SC_ERR_BAD_SIZE)."""
    p = VolumeRobustParams(int(kind), int(frames), int(frame_stride), float(tau), int(time_periodic), float(p_grad), float(eps_grad), float(p_time),
                           float(eps_time), float(p_data), float(eps_data), int(max_rounds), float(round_tol), float(tol), int(max_iters))
    return _check_call("sc_hip_volume_flow_robust_check", p, layout, cols=cols, rows=rows, channels=channels, col_stride=col_stride,
                       row_stride=row_stride, channel_stride=channel_stride)


def volume_subflow_robust_check(kind: int = SC_POISSON_GUIDANCE, frames: int = 2, frame_stride: int = 0, tau: float = 1.0, time_periodic: int = 0,
                                p_grad: float = 1.0, eps_grad: float = 1e-3, p_time: float = 1.0, eps_time: float = 1e-3, p_data: float = 2.0,
                                eps_data: float = 1e-3, max_rounds: int = 0, round_tol: float = 0.0, tol: float = 0.0, max_iters: int = 0,
                                layout: "PoissonLayout | None" = None, *, cols=None, rows=None, channels=None, col_stride=None, row_stride=None,
                                channel_stride=None) -> int:
    """Host-only sc_hip_volume_subflow_robust_check: volume_flow_robust_check's codes -- the robust sub-pixel call takes the robust flow
    call's parameters unchanged."""
    p = VolumeRobustParams(int(kind), int(frames), int(frame_stride), float(tau), int(time_periodic), float(p_grad), float(eps_grad), float(p_time),
                           float(eps_time), float(p_data), float(eps_data), int(max_rounds), float(round_tol), float(tol), int(max_iters))
    return _check_call("sc_hip_volume_subflow_robust_check", p, layout, cols=cols, rows=rows, channels=channels, col_stride=col_stride,
                       row_stride=row_stride, channel_stride=channel_stride)


def volume_robust_arrays(gx, gy, data, state, weight=None, smooth_x=None, smooth_y=None, smooth_t=None, gt=None, boundary=None, tau=1.0, loop=False,
                         neumann=False, free_sides="", periodic="", p_grad=1.0, eps_grad=1e-3, p_time=1.0, eps_time=1e-3, p_data=2.0, eps_data=1e-3):
    """Checks a robust volume problem's numpy arrays and penalties before any device is touched: (kind, data, state, weight, smooth_x,
    smooth_y, smooth_t, gx, gy, gt, boundary), volume_wls_arrays' rules.  gx and gy are required: the residual of a link needs the
    guidance itself (there is no lap).  Exponents in (0, 2]; an eps finite and > 0 wherever its exponent is not 2."""
    if gx is None or gy is None:
        raise ValueError("a robust volume solve needs the guidance gx and gy (there is no Laplacian form)")
    robust_penalties(grad=(p_grad, eps_grad), time=(p_time, eps_time), data=(p_data, eps_data))
    kind, data, state, weight, sx, sy, smt, gx, gy, gt, _, boundary = volume_wls_arrays(data, state, weight, smooth_x, smooth_y, smooth_t, gx, gy, gt,
                                                                                       None, boundary, tau, loop, neumann, free_sides, periodic)
    return kind, data, state, weight, sx, sy, smt, gx, gy, gt, boundary


def volume_coupled_check(coupling: int, kind: int = SC_POISSON_GUIDANCE, frames: int = 2, frame_stride: int = 0, tau: float = 1.0, time_periodic: int = 0,
                         p_grad: float = 1.0, eps_grad: float = 1e-3, p_time: float = 1.0, eps_time: float = 1e-3, p_data: float = 2.0,
                         eps_data: float = 1e-3, max_rounds: int = 0, round_tol: float = 0.0, tol: float = 0.0, max_iters: int = 0,
                         layout: "PoissonLayout | None" = None, *, cols=None, rows=None, channels=None, col_stride=None, row_stride=None,
                         channel_stride=None) -> int:
    """Host-only sc_hip_volume_coupled_check: SC_OK or the code a coupled volume call with this coupling (SC_VOLUME_COUPLE_*), these
    parameters (volume_robust_check's) and this layout returns before it runs anything."""
    p = VolumeRobustParams(int(kind), int(frames), int(frame_stride), float(tau), int(time_periodic), float(p_grad), float(eps_grad), float(p_time),
                           float(eps_time), float(p_data), float(eps_data), int(max_rounds), float(round_tol), float(tol), int(max_iters))
    if layout is None:
        layout = PoissonLayout(*(int(v) for v in (cols, rows, channels, col_stride, row_stride, channel_stride)))
    return int(load().sc_hip_volume_coupled_check(C.byref(p), int(coupling), C.byref(layout)))


def volume_flow_coupled_check(coupling: int, kind: int = SC_POISSON_GUIDANCE, frames: int = 2, frame_stride: int = 0, tau: float = 1.0,
                              time_periodic: int = 0, p_grad: float = 1.0, eps_grad: float = 1e-3, p_time: float = 1.0, eps_time: float = 1e-3,
                              p_data: float = 2.0, eps_data: float = 1e-3, max_rounds: int = 0, round_tol: float = 0.0, tol: float = 0.0,
                              max_iters: int = 0, layout: "PoissonLayout | None" = None, *, cols=None, rows=None, channels=None, col_stride=None,
                              row_stride=None, channel_stride=None) -> int:
    """Host-only sc_hip_volume_flow_coupled_check: volume_coupled_check's codes, then the flow call's refusal of a volume whose unknowns
    32 bits cannot index (SC_ERR_BAD_SIZE)."""
    p = VolumeRobustParams(int(kind), int(frames), int(frame_stride), float(tau), int(time_periodic), float(p_grad), float(eps_grad), float(p_time),
                           float(eps_time), float(p_data), float(eps_data), int(max_rounds), float(round_tol), float(tol), int(max_iters))
    if layout is None:
        layout = PoissonLayout(*(int(v) for v in (cols, rows, channels, col_stride, row_stride, channel_stride)))
    return int(load().sc_hip_volume_flow_coupled_check(C.byref(p), int(coupling), C.byref(layout)))


def robust_check(kind: int = SC_POISSON_GUIDANCE, p_grad: float = 1.0, eps_grad: float = 1e-3, p_data: float = 2.0, eps_data: float = 1e-3,
                 max_rounds: int = 0, round_tol: float = 0.0, tol: float = 0.0, max_iters: int = 0, layout: "PoissonLayout | None" = None, *,
                 cols=None, rows=None, channels=None, col_stride=None, row_stride=None, channel_stride=None, isotropic=False,
                 joint_channels=False) -> int:
    """Host-only sc_hip_robust_check: SC_OK or the code a robust call with these parameters and this layout returns before it runs
    anything.  The layout as a PoissonLayout or as keyword fields.  isotropic, joint_channels: SC_ROBUST_ISOTROPIC and
    SC_ROBUST_JOINT_CHANNELS or'ed into kind (which may carry them itself)."""
    p = robust_params(int(kind) | robust_coupling_bits(isotropic, joint_channels), p_grad, eps_grad, p_data, eps_data, max_rounds, round_tol, tol, max_iters)
    return _check_call("sc_hip_robust_check", p, layout, cols=cols, rows=rows, channels=channels, col_stride=col_stride,
                       row_stride=row_stride, channel_stride=channel_stride)


def robust_arrays(gx, gy, data, weight, smooth_x=None, smooth_y=None, boundary=None, out=None, neumann=False, free_sides="", periodic="",
                  p_grad=1.0, eps_grad=1e-3, p_data=2.0, eps_data=1e-3, isotropic=False, joint_channels=False):
    """Checks a robust problem's numpy arrays and penalties before any device is touched: (kind, gx, gy, data, weight, smooth_x, smooth_y,
    boundary, out), weighted_arrays' rules for data, weight and boundary and wls_arrays' for the base links, which come both or not at
    all (None: all 1).  gx and gy are required: the residual of a link needs the guidance itself.  Exponents in (0, 2]; an eps finite
    and > 0 wherever its exponent is not 2.  isotropic, joint_channels: kind carries SC_ROBUST_ISOTROPIC, SC_ROBUST_JOINT_CHANNELS."""
    if gx is None or gy is None:
        raise ValueError("a robust solve needs the guidance gx and gy (there is no Laplacian form)")
    if (smooth_x is None) != (smooth_y is None):
        raise ValueError("smooth_x and smooth_y go together (both None: all base links 1)")
    robust_penalties(grad=(p_grad, eps_grad), data=(p_data, eps_data))
    if smooth_x is None:
        kind, data, weight, gx, gy, _, boundary, out = weighted_arrays(data, weight, gx, gy, None, boundary, out, neumann, free_sides, periodic)
    else:
        kind, data, weight, smooth_x, smooth_y, gx, gy, _, boundary, out = wls_arrays(data, weight, smooth_x, smooth_y, gx, gy, None, boundary,
                                                                                     out, neumann, free_sides, periodic)
    return kind | robust_coupling_bits(isotropic, joint_channels), gx, gy, data, weight, smooth_x, smooth_y, boundary, out


def region_robust_check(kind: int = SC_POISSON_GUIDANCE, p_grad: float = 1.0, eps_grad: float = 1e-3, p_data: float = 2.0, eps_data: float = 1e-3,
                        max_rounds: int = 0, round_tol: float = 0.0, tol: float = 0.0, max_iters: int = 0, layout: "PoissonLayout | None" = None, *,
                        cols=None, rows=None, channels=None, col_stride=None, row_stride=None, channel_stride=None, isotropic=False,
                        joint_channels=False) -> int:
    """Host-only sc_hip_region_robust_check: SC_OK or the code a robust region call with these parameters and this layout returns before
    it runs anything.  The layout as a PoissonLayout or as keyword fields.  isotropic, joint_channels: SC_ROBUST_ISOTROPIC and
    SC_ROBUST_JOINT_CHANNELS or'ed into kind (which may carry them itself)."""
    p = robust_params(int(kind) | robust_coupling_bits(isotropic, joint_channels), p_grad, eps_grad, p_data, eps_data, max_rounds, round_tol, tol, max_iters)
    return _check_call("sc_hip_region_robust_check", p, layout, cols=cols, rows=rows, channels=channels, col_stride=col_stride,
                       row_stride=row_stride, channel_stride=channel_stride)


def region_robust_arrays(gx, gy, data, state, weight=None, smooth_x=None, smooth_y=None, boundary=None, out=None, neumann=False, free_sides="",
                         periodic="", p_grad=1.0, eps_grad=1e-3, p_data=2.0, eps_data=1e-3, isotropic=False, joint_channels=False):
    """Checks a robust region problem's numpy arrays and penalties before any device is touched: (kind, gx, gy, data, state, weight,
    smooth_x, smooth_y, boundary, out), region_arrays' rules.  gx and gy are required: the residual of a link needs the guidance itself
    (there is no lap).  Exponents in (0, 2]; an eps finite and > 0 wherever its exponent is not 2 (p_data and eps_data are checked with
    weight None as well, and then unused).  isotropic, joint_channels: kind carries SC_ROBUST_ISOTROPIC, SC_ROBUST_JOINT_CHANNELS."""
    if gx is None or gy is None:
        raise ValueError("a robust region solve needs the guidance gx and gy (there is no Laplacian form)")
    robust_penalties(grad=(p_grad, eps_grad), data=(p_data, eps_data))
    kind, data, state, weight, sx, sy, gx, gy, _, boundary, out = region_arrays(data, state, weight, smooth_x, smooth_y, gx, gy, None, boundary, out,
                                                                                neumann, free_sides, periodic)
    return kind | robust_coupling_bits(isotropic, joint_channels), gx, gy, data, state, weight, sx, sy, boundary, out


class Instance:
    """Thin RAII wrapper over one library instance (one GPU, one stream)."""

    def __init__(self, gpu_id: int = 0):
        self.L = load()
        self.h = self.L.my_seamlessclone_api_imp_create_instance(int(gpu_id))
        if not self.h:
            raise SeamlessCloneError(SC_ERR_HIP, f"cannot create an instance on GPU {gpu_id} "
                                     "(no MI355X visible? there is no CPU fallback)")
        self.gpu_id = gpu_id

    # ---- lifetime
    def destroy(self):
        if getattr(self, "h", None):
            self.L.my_seamlessclone_api_imp_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass

    def sync(self):
        self.L.my_seamlessclone_api_imp_sync(self.h)

    def _check(self, rc, allow=()):
        if rc != SC_OK and rc not in allow:
            raise SeamlessCloneError(rc, (self.L.sc_hip_last_error(self.h) or b"").decode())
        return rc

    # ---- options / info
    def default_opts(self) -> SolverOpts:
        o = SolverOpts()
        self.L.sc_hip_default_opts(C.byref(o))
        return o

    def set_solver(self, **kw) -> SolverOpts:
        o = self.get_solver()
        for k, v in kw.items():
            if not hasattr(o, k):
                raise AttributeError(k)
            setattr(o, k, v)
        self._check(self.L.sc_hip_set_solver(self.h, C.byref(o)))
        return o

    def get_solver(self) -> SolverOpts:
        o = SolverOpts()
        self._check(self.L.sc_hip_get_solver(self.h, C.byref(o)))
        return o

    def set_clone_mode(self, mode: int) -> None:
        """SC_NORMAL_CLONE (default), SC_MIXED_CLONE or SC_MONOCHROME_TRANSFER for the next runs; set_solver leaves it alone."""
        self._check(self.L.sc_hip_set_clone_mode(self.h, int(mode)))

    @property
    def clone_mode(self) -> int:
        return self._check(self.L.sc_hip_get_clone_mode(self.h), allow=CLONE_MODES)

    def info(self) -> RunInfo:
        i = RunInfo()
        self._check(self.L.sc_hip_get_info(self.h, C.byref(i)))
        return i

    # ---- the clone
    def run(self, face, body, mask, cx, cy, sync=False, allow_not_converged=False):
        """In place on `body` (reference semantics).  Returns the C return code.  The call is complete when it returns
        either way; sync = the reference's bSync: True also prints its two timing lines on stdout (the reference's
        Python binding passes False, SeamlessClone.cpp:63)."""
        if not body.flags.writeable:
            raise ValueError("body must be writeable: the clone is in place")
        f, b, m = _img(face), _img(body), _img(mask)
        rc = self.L.my_seamlessclone_api_imp_run(self.h, *f, *b, *m, int(cx), int(cy), self.gpu_id, bool(sync))
        return self._check(rc, allow=(SC_ERR_NOT_CONVERGED,) if allow_not_converged else ())

    # ---- whole-image edits
    def edit_params(self, op: int, **kw) -> EditParams:
        """OpenCV's defaults for `op` (sc_hip_default_edit_params), with the fields named in kw replaced."""
        p = EditParams()
        self.L.sc_hip_default_edit_params(C.byref(p), int(op))
        for k, v in kw.items():
            if not hasattr(p, k):
                raise AttributeError(k)
            setattr(p, k, v)
        return p

    def edit(self, params: EditParams, src, mask, dst=None, allow_not_converged=False):
        """sc_hip_edit on host images: src H x W x 3, mask H x W (uint8).  dst: an array of src's shape to write (may be src
        itself), default a new one.  Returns dst."""
        if dst is None:
            dst = np.empty_like(src)
        s, m, d = _img(src), _img(mask), _img(dst)
        if m[1:3] != s[1:3] or d[1:3] != s[1:3]:
            raise ValueError("src, mask and dst must have one size")
        rc = self.L.sc_hip_edit(self.h, C.byref(params), *s, m[0], m[3], d[0], d[3])
        self._check(rc, allow=(SC_ERR_NOT_CONVERGED,) if allow_not_converged else ())
        return dst

    def edit_device(self, params: EditParams, d_src, shape, d_mask, d_dst, src_step=None, mask_step=None, dst_step=None,
                    sync=True, allow_not_converged=False):
        """sc_hip_edit_device: device images of shape (rows, cols); steps default to dense rows."""
        rows, cols = shape[0], shape[1]
        rc = self.L.sc_hip_edit_device(self.h, C.byref(params), d_src, cols, rows, src_step or 3 * cols, d_mask,
                                       mask_step or cols, d_dst, dst_step or 3 * cols, bool(sync))
        return self._check(rc, allow=(SC_ERR_NOT_CONVERGED,) if allow_not_converged else ())

    @staticmethod
    def make_edit_jobs(n: int):
        return (EditJob * n)()

    def edit_device_batch(self, params: EditParams, jobs, sync=True, allow_job_errors=False):
        """sc_hip_edit_device_batch: jobs is an EditJob array (make_edit_jobs) of device images, one op and parameter set for all.
        Jobs of one image size are solved as one field of 3n channels; per-job codes in jobs[i].rc.  Returns the worst code:
        SC_ERR_NOT_CONVERGED is returned, other failures raise unless allow_job_errors (then they are returned as well)."""
        rc = self.L.sc_hip_edit_device_batch(self.h, C.byref(params), jobs, len(jobs))
        if sync:
            self.sync()
        if allow_job_errors and rc != SC_ERR_HIP:
            return rc
        return self._check(rc, allow=(SC_ERR_NOT_CONVERGED,))

    def edit_rhs(self, params: EditParams, src, mask):
        """(eroded mask H x W, un-folded right-hand side [3][H][W]) of an edit (test hook)."""
        s, m = _img(src), _img(mask)
        W, H = s[1], s[2]
        M = np.zeros((H, W), np.uint8)
        lap = np.zeros((3, H, W), np.float32)
        self._check(self.L.sc_hip_edit_rhs(self.h, C.byref(params), *s, m[0], m[3], M.ctypes.data_as(u8p), lap.ctypes.data_as(f32p),
                                           W * H))
        return M, lap

    def canny(self, src, low, high, kernel_size=3):
        """(class map before hysteresis: 0 / 1 weak / 2 strong, edge map 0 / 255, (hysteresis launches, mailbox reads))."""
        s = _img(src)
        W, H = s[1], s[2]
        cls = np.zeros((H, W), np.uint8)
        edges = np.zeros((H, W), np.uint8)
        counts = np.zeros(2, np.int32)
        self._check(self.L.sc_hip_canny(self.h, *s, float(low), float(high), int(kernel_size), cls.ctypes.data_as(u8p),
                                        edges.ctypes.data_as(u8p), counts.ctypes.data_as(i32p)))
        return cls, edges, (int(counts[0]), int(counts[1]))

    def edit_counts(self):
        """(hysteresis launches, mailbox reads) of the last edit."""
        counts = np.zeros(2, np.int32)
        self._check(self.L.sc_hip_edit_counts(self.h, counts.ctypes.data_as(i32p)))
        return int(counts[0]), int(counts[1])

    # ---- the Poisson solver on float32 arrays
    def poisson(self, boundary, gx=None, gy=None, lap=None, out=None, tol=0.0, allow_not_converged=False, neumann=False, free_sides="",
                periodic=""):
        """sc_hip_poisson on numpy float32 arrays of shape H x W or H x W x C (C 1..4): solve lap(u) = div (gx, gy) (or = lap) with
        u = boundary on the frame; boundary's interior is the initial guess of the iterative methods.  out: an array of boundary's
        shape to write (may be boundary itself), default a new one.  Returns out.
        neumann: the reflecting problem on every pixel (SC_POISSON_NEUMANN); mean(out) = mean(boundary) per channel, boundary may be
        None (mean zero; shape and layout then come from gx / lap).
        free_sides: the sides without a Dirichlet line, a string over "lrtb" (SC_POISSON_FREE_*): their outermost pixels are unknowns,
        the other sides' outermost rows and columns keep boundary's values; a direct solve, tol unused.
        periodic: the axes that wrap, "x", "y" or "xy" (SC_POISSON_PERIODIC_*): no Dirichlet line there, the pixel beyond either end is
        the one at the other end, and gx's last column / gy's last row hold the difference across the seam.  Without a Dirichlet line
        on the other axis either, boundary gives only the mean and may be None, as for neumann."""
        kind, boundary, gx, gy, lap, out = poisson_arrays(boundary, gx, gy, lap, out, neumann, free_sides, periodic)
        first = boundary if boundary is not None else (lap if lap is not None else gx)
        return self._host_call("sc_hip_poisson", PoissonParams(kind, float(tol)), (gx, gy, lap, boundary), out, first,
                               (SC_ERR_NOT_CONVERGED,) if allow_not_converged else (), in_place=3)

    def _host_call(self, fn, params, arrays, out, first, allow, in_place=None):
        """One host call of a float32 family: arrays in the C entry's order (None: absent), out or None (a new array of first's shape).
        One layout per call: numpy's strides when all arrays share them and they are positive, else contiguous copies and a
        contiguous out that is copied back.  in_place: the index of the array an `out is arrays[in_place]` call keeps as its out
        through the copies.  Returns the caller's out."""
        target = out = np.empty_like(first) if out is None else out
        lays = [poisson_layout_of(a) for a in (*arrays, out) if a is not None]
        if len({_layout_key(l) for l in lays}) != 1 or any(l.col_stride <= 0 or l.row_stride <= 0 or l.channel_stride <= 0 for l in lays):
            same = in_place is not None and out is arrays[in_place]
            arrays = [None if a is None else np.ascontiguousarray(a) for a in arrays]
            out = arrays[in_place] if same and arrays[in_place] is target else np.empty(first.shape, np.float32)
        layout = poisson_layout_of(out)
        rc = getattr(self.L, fn)(self.h, C.byref(params), C.byref(layout), *(None if a is None else a.ctypes.data for a in arrays),
                                 out.ctypes.data)
        self._check(rc, allow=allow)
        if out is not target:
            target[...] = out
        return target

    def _device_call(self, fn, params, layout, jobs, sync, allow_job_errors, allow):
        """One device call of a float32 family: bSync and a wait for the stream when sync; the worst code, raised unless it is in
        allow or allow_job_errors lets it through (SC_ERR_HIP always raises)."""
        rc = getattr(self.L, fn)(self.h, C.byref(params), C.byref(layout), jobs, len(jobs), bool(sync))
        if sync:
            self.sync()
        if allow_job_errors and rc != SC_ERR_HIP:
            return rc
        return self._check(rc, allow=allow)

    @staticmethod
    def make_poisson_jobs(n: int):
        return (PoissonJob * n)()

    def poisson_device(self, params: PoissonParams, layout: PoissonLayout, jobs, sync=True, allow_job_errors=False):
        """sc_hip_poisson_device: jobs is a PoissonJob array (make_poisson_jobs) of device pointers, one layout for all.  sync: bSync
        (stage times) and a wait for the stream.  Per-job codes in jobs[i].rc; returns the worst code: SC_ERR_NOT_CONVERGED is
        returned, other failures raise unless allow_job_errors (then they are returned as well)."""
        return self._device_call("sc_hip_poisson_device", params, layout, jobs, sync, allow_job_errors, (SC_ERR_NOT_CONVERGED,))

    # ---- screened Poisson solves on float32 arrays
    def screened(self, data, gx=None, gy=None, lap=None, lam=None, boundary=None, neumann=False, out=None, free_sides="", periodic=""):
        """sc_hip_screened on numpy float32 arrays of shape H x W or H x W x C (C 1..4): minimise lam sum (u - data)^2 +
        sum |grad u - (gx, gy)|^2 (or with the divergence given as lap), with u = boundary on the frame, or, neumann, reflected at the
        border (boundary then unused).  out: an array of data's shape to write (may be data or boundary), default a new one.
        free_sides, periodic: as poisson's (boundary is read on the remaining Dirichlet lines).  Returns out."""
        kind, data, gx, gy, lap, boundary, out = screened_arrays(data, gx, gy, lap, lam, boundary, out, neumann, free_sides, periodic)
        return self._host_call("sc_hip_screened", ScreenedParams(kind, float(lam)), (gx, gy, lap, data, boundary), out, data, ())

    @staticmethod
    def make_screened_jobs(n: int):
        return (ScreenedJob * n)()

    def screened_device(self, params: ScreenedParams, layout: PoissonLayout, jobs, sync=True, allow_job_errors=False):
        """sc_hip_screened_device: jobs is a ScreenedJob array (make_screened_jobs) of device pointers, one layout for all.  sync: bSync
        (stage times) and a wait for the stream.  Per-job codes in jobs[i].rc; failures raise unless allow_job_errors (then the worst
        code is returned)."""
        return self._device_call("sc_hip_screened_device", params, layout, jobs, sync, allow_job_errors, ())

    # ---- weighted solves on float32 arrays
    def weighted(self, data, weight, gx=None, gy=None, lap=None, boundary=None, neumann=False, out=None, free_sides="", periodic="",
                 tol=0.0, max_iters=0, precond_lambda=0.0, allow_not_converged=False):
        """sc_hip_weighted on numpy float32 arrays of shape H x W or H x W x C (C 1..4): minimise sum weight (u - data)^2 +
        sum |grad u - (gx, gy)|^2 (or with the divergence given as lap; neither: zero guidance) under the borders of poisson()
        (neumann, free_sides, periodic; boundary on the remaining Dirichlet lines).  weight >= 0, of data's shape or H x W (broadcast
        over the channels).  tol, max_iters, precond_lambda: sc_weighted_params' (0: the defaults).  out: an array of data's shape
        to write (may be data or boundary), default a new one.  Returns out; info() has the iterations and the final residual."""
        kind, data, weight, gx, gy, lap, boundary, out = weighted_arrays(data, weight, gx, gy, lap, boundary, out, neumann, free_sides,
                                                                         periodic)
        p = WeightedParams(kind, float(tol), int(max_iters), float(precond_lambda))
        return self._host_call("sc_hip_weighted", p, (gx, gy, lap, data, weight, boundary), out, data,
                               (SC_ERR_NOT_CONVERGED,) if allow_not_converged else ())

    @staticmethod
    def make_weighted_jobs(n: int):
        return (WeightedJob * n)()

    def weighted_device(self, params: WeightedParams, layout: PoissonLayout, jobs, sync=True, allow_job_errors=False):
        """sc_hip_weighted_device: jobs is a WeightedJob array (make_weighted_jobs) of device pointers, one layout for all.  sync: bSync
        and a wait for the stream.  Per-job codes in jobs[i].rc; returns the worst code: SC_ERR_NOT_CONVERGED is returned, other
        failures raise unless allow_job_errors (then they are returned as well)."""
        return self._device_call("sc_hip_weighted_device", params, layout, jobs, sync, allow_job_errors, (SC_ERR_NOT_CONVERGED,))

    # ---- WLS solves on float32 arrays
    def wls(self, data, weight, smooth_x, smooth_y, gx=None, gy=None, lap=None, boundary=None, neumann=False, out=None, free_sides="",
            periodic="", tol=0.0, max_iters=0, precond_lambda=0.0, precond_smooth=0.0, allow_not_converged=False):
        """sc_hip_wls on numpy float32 arrays of shape H x W or H x W x C (C 1..4): minimise sum weight (u - data)^2 +
        sum smooth_x (d_x u - gx)^2 + sum smooth_y (d_y u - gy)^2 (or with div(smooth g) given as lap; neither: zero guidance) under the
        borders of poisson().  smooth_x[y, x] weighs the link (x, y) - (x + 1, y), smooth_y[y, x] the link (x, y) - (x, y + 1); > 0 on
        every live link (live_links), of data's shape or H x W.  tol, max_iters, precond_lambda, precond_smooth: sc_wls_params' (0: the
        defaults).  Returns out; info() has the iterations and the final residual."""
        kind, data, weight, sx, sy, gx, gy, lap, boundary, out = wls_arrays(data, weight, smooth_x, smooth_y, gx, gy, lap, boundary, out,
                                                                            neumann, free_sides, periodic)
        p = WlsParams(kind, float(tol), int(max_iters), float(precond_lambda), float(precond_smooth))
        return self._host_call("sc_hip_wls", p, (gx, gy, lap, data, weight, sx, sy, boundary), out, data,
                               (SC_ERR_NOT_CONVERGED,) if allow_not_converged else ())

    @staticmethod
    def make_wls_jobs(n: int):
        return (WlsJob * n)()

    def wls_device(self, params: WlsParams, layout: PoissonLayout, jobs, sync=True, allow_job_errors=False):
        """sc_hip_wls_device: jobs is a WlsJob array (make_wls_jobs) of device pointers, one layout for all.  sync: bSync and a wait for
        the stream.  Per-job codes in jobs[i].rc; returns the worst code: SC_ERR_NOT_CONVERGED is returned, other failures raise unless
        allow_job_errors (then they are returned as well)."""
        return self._device_call("sc_hip_wls_device", params, layout, jobs, sync, allow_job_errors, (SC_ERR_NOT_CONVERGED,))

    # ---- region solves on float32 arrays
    def region(self, data, state, weight=None, smooth_x=None, smooth_y=None, gx=None, gy=None, lap=None, boundary=None, neumann=False,
               out=None, free_sides="", periodic="", tol=0.0, max_iters=0, precond_lambda=0.0, precond_smooth=0.0, allow_not_converged=False):
        """sc_hip_region on numpy float32 arrays of shape H x W or H x W x C (C 1..4): wls()'s problem on a domain of any shape.
        state (region_arrays' types; of data's shape or H x W) says of every pixel inside the borders whether it is solved for
        (SC_REGION_UNKNOWN), held at data's value (SC_REGION_KNOWN) or not part of the domain (SC_REGION_OUTSIDE: no link reaches it).
        weight None: no data term; smooth_x, smooth_y None: every link 1.  Returns out: the solution at UNKNOWN pixels, data at KNOWN
        and OUTSIDE ones, boundary on the Dirichlet lines; info() has the iterations and the final residual."""
        kind, data, state, weight, sx, sy, gx, gy, lap, boundary, out = region_arrays(data, state, weight, smooth_x, smooth_y, gx, gy, lap,
                                                                                      boundary, out, neumann, free_sides, periodic)
        p = RegionParams(kind, float(tol), int(max_iters), float(precond_lambda), float(precond_smooth))
        return self._host_call("sc_hip_region", p, (gx, gy, lap, data, state, weight, sx, sy, boundary), out, data,
                               (SC_ERR_NOT_CONVERGED,) if allow_not_converged else ())

    @staticmethod
    def make_region_jobs(n: int):
        return (RegionJob * n)()

    def region_device(self, params: RegionParams, layout: PoissonLayout, jobs, sync=True, allow_job_errors=False):
        """sc_hip_region_device: jobs is a RegionJob array (make_region_jobs) of device pointers, one layout for all.  sync: bSync and a
        wait for the stream.  Per-job codes in jobs[i].rc; returns the worst code: SC_ERR_NOT_CONVERGED is returned, other failures
        raise unless allow_job_errors (then they are returned as well)."""
        return self._device_call("sc_hip_region_device", params, layout, jobs, sync, allow_job_errors, (SC_ERR_NOT_CONVERGED,))

    # ---- bounded solves on float32 arrays
    def bounded(self, data, state, lower=None, upper=None, weight=None, smooth_x=None, smooth_y=None, gx=None, gy=None, lap=None, boundary=None,
                neumann=False, out=None, free_sides="", periodic="", max_rounds=0, tol=0.0, max_iters=0, precond_lambda=0.0,
                precond_smooth=0.0, allow_not_converged=False):
        """sc_hip_bounded on numpy float32 arrays of shape H x W or H x W x C (C 1..4): region()'s problem under lower <= u <= upper at
        every UNKNOWN pixel, by the primal-dual active set method on the device.  lower, upper: None (no bound on that side), a number,
        or a float32 array of data's shape or H x W (bounded_arrays).  Returns out as region() composes it, the UNKNOWN pixels inside
        their bounds; info() has the total of the inner iterations and whether the active set stopped changing within max_rounds
        (0: 30), bounded_trace() the rounds."""
        kind, data, state, weight, sx, sy, gx, gy, lap, boundary, out, lo, hi, lo_a, hi_a = bounded_arrays(
            data, state, lower, upper, weight, smooth_x, smooth_y, gx, gy, lap, boundary, out, neumann, free_sides, periodic)
        p = BoundedParams(kind, float(tol), int(max_iters), float(precond_lambda), float(precond_smooth), lo, hi, int(max_rounds))
        return self._host_call("sc_hip_bounded", p, (gx, gy, lap, data, state, weight, sx, sy, boundary, lo_a, hi_a), out, data,
                               (SC_ERR_NOT_CONVERGED,) if allow_not_converged else ())

    @staticmethod
    def make_bounded_jobs(n: int):
        return (BoundedJob * n)()

    def bounded_device(self, params: BoundedParams, layout: PoissonLayout, jobs, sync=True, allow_job_errors=False):
        """sc_hip_bounded_device: jobs is a BoundedJob array (make_bounded_jobs) of device pointers, one layout for all.  sync: bSync and
        a wait for the stream.  Per-job codes in jobs[i].rc; returns the worst code: SC_ERR_NOT_CONVERGED is returned, other failures
        raise unless allow_job_errors (then they are returned as well)."""
        return self._device_call("sc_hip_bounded_device", params, layout, jobs, sync, allow_job_errors, (SC_ERR_NOT_CONVERGED,))

    def bounded_trace(self):
        """(changed, active, iters) of the last bounded call's last chunk: int32 arrays with one entry per round -- the pixels whose set
        changed in the mark behind that round's solve, the pixels active after it, the solve's inner iterations."""
        n = int(self.L.sc_hip_bounded_trace(self.h, None, None, None, 0))
        changed, active, iters = (np.zeros(n, np.int32) for _ in range(3))
        if n:
            self.L.sc_hip_bounded_trace(self.h, changed.ctypes.data_as(i32p), active.ctypes.data_as(i32p), iters.ctypes.data_as(i32p), n)
        return changed, active, iters

    # ---- robust region solves on float32 arrays
    def region_robust(self, gx, gy, data, state, weight=None, smooth_x=None, smooth_y=None, boundary=None, neumann=False, out=None, free_sides="",
                      periodic="", p_grad=1.0, eps_grad=1e-3, p_data=2.0, eps_data=1e-3, max_rounds=0, round_tol=0.0, tol=0.0, max_iters=0,
                      allow_not_converged=False, isotropic=False, joint_channels=False):
        """sc_hip_region_robust on numpy float32 arrays of shape H x W or H x W x C (C 1..4): region()'s problem with the penalties of
        robust() in place of the squares -- over the UNKNOWN pixels minimise sum weight phi_q(u - data) + sum smooth_x phi_p(d_x u - gx) +
        sum smooth_y phi_p(d_y u - gy) over the links live in the region, p = p_grad, q = p_data -- by reweighted region solves on the
        device.  state as region()'s; weight None: no data term; smooth_x, smooth_y None: every base link 1.  isotropic, joint_channels:
        robust()'s coupled forms on the live links.  max_rounds, round_tol, tol, max_iters: sc_robust_params' (0: the defaults; round_tol
        < 0: never stop early).  Returns out as region() composes it; info() has the total of the inner iterations and whether the round
        rule was met, robust_trace() the rounds."""
        kind, gx, gy, data, state, weight, sx, sy, boundary, out = region_robust_arrays(gx, gy, data, state, weight, smooth_x, smooth_y, boundary, out,
                                                                                        neumann, free_sides, periodic, p_grad, eps_grad, p_data,
                                                                                        eps_data, isotropic, joint_channels)
        p = robust_params(kind, p_grad, eps_grad, p_data, eps_data, max_rounds, round_tol, tol, max_iters)
        return self._host_call("sc_hip_region_robust", p, (gx, gy, data, state, weight, sx, sy, boundary), out, data,
                               (SC_ERR_NOT_CONVERGED,) if allow_not_converged else ())

    @staticmethod
    def make_region_robust_jobs(n: int):
        return (RegionRobustJob * n)()

    def region_robust_device(self, params: RobustParams, layout: PoissonLayout, jobs, sync=True, allow_job_errors=False):
        """sc_hip_region_robust_device: jobs is a RegionRobustJob array (make_region_robust_jobs) of device pointers, one layout for all.
        sync: bSync and a wait for the stream.  Per-job codes in jobs[i].rc; returns the worst code: SC_ERR_NOT_CONVERGED is returned,
        other failures raise unless allow_job_errors (then they are returned as well)."""
        return self._device_call("sc_hip_region_robust_device", params, layout, jobs, sync, allow_job_errors, (SC_ERR_NOT_CONVERGED,))

    # ---- volume solves on float32 arrays
    def volume(self, data, state, weight=None, gx=None, gy=None, gt=None, lap=None, boundary=None, tau=1.0, neumann=False, free_sides="",
               periodic="", tol=0.0, max_iters=0, precond_lambda=0.0, allow_not_converged=False):
        """sc_hip_volume on numpy float32 arrays of shape T x H x W or T x H x W x C (volume_arrays' rules): region()'s problem with unit
        links on every frame, the frames joined by temporal links of weight tau; gt ((T - 1) x H x W (x C), or None: zeros) is the wanted
        difference from a frame to the next.  Returns a NEW array: the solution at UNKNOWN pixels, data at KNOWN and OUTSIDE ones,
        boundary on the Dirichlet lines of every frame; info() has the iterations and the final residual."""
        kind, data, state, weight, gx, gy, gt, lap, boundary = volume_arrays(data, state, weight, gx, gy, gt, lap, boundary, tau, neumann,
                                                                             free_sides, periodic)
        layout = poisson_layout_of(data[0])
        p = VolumeParams(kind, data.shape[0], data[0].size, float(tau), float(tol), int(max_iters), float(precond_lambda))
        out = np.empty_like(data)
        rc = self.L.sc_hip_volume(self.h, C.byref(p), C.byref(layout), *(None if a is None else a.ctypes.data for a in
                                  (gx, gy, gt, lap, data, state, weight, boundary)), out.ctypes.data)
        self._check(rc, allow=(SC_ERR_NOT_CONVERGED,) if allow_not_converged else ())
        return out

    @staticmethod
    def make_volume_jobs(n: int):
        return (VolumeJob * n)()

    def volume_device(self, params: VolumeParams, layout: PoissonLayout, jobs, sync=True, allow_job_errors=False):
        """sc_hip_volume_device: jobs is a VolumeJob array (make_volume_jobs) of device pointers, one frame layout and one frame stride
        for all.  sync: bSync and a wait for the stream.  Per-job codes in jobs[i].rc; returns the worst code: SC_ERR_NOT_CONVERGED is
        returned, other failures raise unless allow_job_errors (then they are returned as well)."""
        return self._device_call("sc_hip_volume_device", params, layout, jobs, sync, allow_job_errors, (SC_ERR_NOT_CONVERGED,))

    # ---- WLS volume solves on float32 arrays
    def volume_wls(self, data, state, weight=None, smooth_x=None, smooth_y=None, smooth_t=None, gx=None, gy=None, gt=None, lap=None, boundary=None,
                   tau=1.0, loop=False, neumann=False, free_sides="", periodic="", tol=0.0, max_iters=0, precond_lambda=0.0, precond_smooth=0.0,
                   precond_tau=0.0, allow_not_converged=False):
        """sc_hip_volume_wls on numpy float32 arrays of shape T x H x W or T x H x W x C (volume_wls_arrays' rules): volume()'s problem with
        the spatial links smooth_x, smooth_y (None: 1) and the temporal links tau * smooth_t (None: tau); loop: periodic time -- frame
        T - 1 is linked to frame 0, gt and smooth_t hold T frames.  Returns a NEW array composed as volume()'s; info() has the iterations
        and the final residual."""
        kind, data, state, weight, sx, sy, smt, gx, gy, gt, lap, boundary = volume_wls_arrays(data, state, weight, smooth_x, smooth_y, smooth_t,
                                                                                              gx, gy, gt, lap, boundary, tau, loop, neumann,
                                                                                              free_sides, periodic)
        layout = poisson_layout_of(data[0])
        p = VolumeWlsParams(kind, data.shape[0], data[0].size, float(tau), 1 if loop else 0, float(tol), int(max_iters), float(precond_lambda),
                            float(precond_smooth), float(precond_tau))
        out = np.empty_like(data)
        rc = self.L.sc_hip_volume_wls(self.h, C.byref(p), C.byref(layout), *(None if a is None else a.ctypes.data for a in
                                      (gx, gy, gt, lap, data, state, weight, sx, sy, smt, boundary)), out.ctypes.data)
        self._check(rc, allow=(SC_ERR_NOT_CONVERGED,) if allow_not_converged else ())
        return out

    @staticmethod
    def make_volume_wls_jobs(n: int):
        return (VolumeWlsJob * n)()

    def volume_wls_device(self, params: VolumeWlsParams, layout: PoissonLayout, jobs, sync=True, allow_job_errors=False):
        """sc_hip_volume_wls_device: jobs is a VolumeWlsJob array (make_volume_wls_jobs) of device pointers, one frame layout and one
        frame stride for all.  sync: bSync and a wait for the stream.  Per-job codes in jobs[i].rc; returns the worst code:
        SC_ERR_NOT_CONVERGED is returned, other failures raise unless allow_job_errors (then they are returned as well)."""
        return self._device_call("sc_hip_volume_wls_device", params, layout, jobs, sync, allow_job_errors, (SC_ERR_NOT_CONVERGED,))

    # ---- flow volume solves on float32 arrays
    def volume_flow(self, data, state, flow, weight=None, smooth_x=None, smooth_y=None, smooth_t=None, gx=None, gy=None, gt=None, lap=None,
                    boundary=None, tau=1.0, loop=False, neumann=False, free_sides="", periodic="", tol=0.0, max_iters=0, precond_lambda=0.0,
                    precond_smooth=0.0, precond_tau=0.0, allow_not_converged=False):
        """sc_hip_volume_flow on numpy float32 arrays (volume_wls_arrays' rules): volume_wls()'s problem with every temporal link along
        `flow` ((T - 1) x H x W x 2, with loop T x H x W x 2, holding (dx, dy); volume_flow_planes' rules: rounded, NaN = no link).  gt and
        smooth_t stay stored at a link's source pixel.  flow None: volume_wls() itself.  Returns a NEW array composed as volume()'s."""
        kind, data, state, weight, sx, sy, smt, gx, gy, gt, lap, boundary = volume_wls_arrays(data, state, weight, smooth_x, smooth_y, smooth_t,
                                                                                              gx, gy, gt, lap, boundary, tau, loop, neumann,
                                                                                              free_sides, periodic)
        fx, fy = (None, None) if flow is None else volume_flow_planes(flow, data.shape[0], data.shape[1], data.shape[2], loop)
        layout = poisson_layout_of(data[0])
        p = VolumeWlsParams(kind, data.shape[0], data[0].size, float(tau), 1 if loop else 0, float(tol), int(max_iters), float(precond_lambda),
                            float(precond_smooth), float(precond_tau))
        out = np.empty_like(data)
        rc = self.L.sc_hip_volume_flow(self.h, C.byref(p), C.byref(layout), *(None if a is None else a.ctypes.data for a in
                                       (gx, gy, gt, lap, data, state, weight, sx, sy, smt, fx, fy, boundary)), out.ctypes.data)
        self._check(rc, allow=(SC_ERR_NOT_CONVERGED,) if allow_not_converged else ())
        return out

    @staticmethod
    def make_volume_flow_jobs(n: int):
        return (VolumeFlowJob * n)()

    def volume_flow_device(self, params: VolumeWlsParams, layout: PoissonLayout, jobs, sync=True, allow_job_errors=False):
        """sc_hip_volume_flow_device: jobs is a VolumeFlowJob array (make_volume_flow_jobs) of device pointers; flow_x, flow_y are dense
        W x H x (T - 1; periodic time: T) float32 whatever the layout.  Codes as volume_wls_device."""
        return self._device_call("sc_hip_volume_flow_device", params, layout, jobs, sync, allow_job_errors, (SC_ERR_NOT_CONVERGED,))

    # ---- sub-pixel flow volume solves on float32 arrays
    def volume_subflow(self, data, state, flow, weight=None, smooth_x=None, smooth_y=None, smooth_t=None, gx=None, gy=None, gt=None, lap=None,
                       boundary=None, tau=1.0, loop=False, neumann=False, free_sides="", periodic="", tol=0.0, max_iters=0, precond_lambda=0.0,
                       precond_smooth=0.0, precond_tau=0.0, allow_not_converged=False):
        """sc_hip_volume_subflow on numpy float32 arrays: volume_flow()'s arguments and result with `flow` taken as it is -- a temporal link
        joins a pixel to the bilinear interpolation of the next frame at (x + dx, y + dy) (volume_subflow_planes' rules: float32, not
        rounded, NaN = no link).  gt and smooth_t stay stored at a link's source pixel.  flow None: volume_wls() itself."""
        kind, data, state, weight, sx, sy, smt, gx, gy, gt, lap, boundary = volume_wls_arrays(data, state, weight, smooth_x, smooth_y, smooth_t,
                                                                                              gx, gy, gt, lap, boundary, tau, loop, neumann,
                                                                                              free_sides, periodic)
        fx, fy = (None, None) if flow is None else volume_subflow_planes(flow, data.shape[0], data.shape[1], data.shape[2], loop)
        layout = poisson_layout_of(data[0])
        p = VolumeWlsParams(kind, data.shape[0], data[0].size, float(tau), 1 if loop else 0, float(tol), int(max_iters), float(precond_lambda),
                            float(precond_smooth), float(precond_tau))
        out = np.empty_like(data)
        rc = self.L.sc_hip_volume_subflow(self.h, C.byref(p), C.byref(layout), *(None if a is None else a.ctypes.data for a in
                                          (gx, gy, gt, lap, data, state, weight, sx, sy, smt, fx, fy, boundary)), out.ctypes.data)
        self._check(rc, allow=(SC_ERR_NOT_CONVERGED,) if allow_not_converged else ())
        return out

    def volume_subflow_device(self, params: VolumeWlsParams, layout: PoissonLayout, jobs, sync=True, allow_job_errors=False):
        """sc_hip_volume_subflow_device: volume_flow_device()'s jobs (make_volume_flow_jobs) with flow_x, flow_y real-valued.  Codes as
        volume_wls_device."""
        return self._device_call("sc_hip_volume_subflow_device", params, layout, jobs, sync, allow_job_errors, (SC_ERR_NOT_CONVERGED,))

    # ---- robust volume solves on float32 arrays
    def volume_robust(self, gx, gy, data, state, weight=None, smooth_x=None, smooth_y=None, smooth_t=None, gt=None, boundary=None, tau=1.0,
                      loop=False, neumann=False, free_sides="", periodic="", p_grad=1.0, eps_grad=1e-3, p_time=1.0, eps_time=1e-3, p_data=2.0,
                      eps_data=1e-3, max_rounds=0, round_tol=0.0, tol=0.0, max_iters=0, allow_not_converged=False):
        """sc_hip_volume_robust on numpy float32 arrays of shape T x H x W or T x H x W x C (volume_robust_arrays' rules): volume_wls()'s
        problem with the penalties of robust() in place of the squares -- phi_p (p_grad, eps_grad) on the spatial links, phi_r (p_time,
        eps_time) on the temporal ones, phi_q (p_data, eps_data) on the data term -- by reweighted WLS volume solves on the device.
        max_rounds, round_tol, tol, max_iters: sc_volume_robust_params' (0: the defaults; round_tol < 0: never stop early).  Returns a
        NEW array composed as volume()'s; info() has the total of the inner iterations and whether the round rule was met,
        robust_trace() the rounds."""
        kind, data, state, weight, sx, sy, smt, gx, gy, gt, boundary = volume_robust_arrays(gx, gy, data, state, weight, smooth_x, smooth_y, smooth_t,
                                                                                            gt, boundary, tau, loop, neumann, free_sides, periodic,
                                                                                            p_grad, eps_grad, p_time, eps_time, p_data, eps_data)
        layout = poisson_layout_of(data[0])
        p = volume_robust_params(kind, data.shape[0], data[0].size, tau, loop, p_grad, eps_grad, p_time, eps_time, p_data, eps_data, max_rounds,
                                 round_tol, tol, max_iters)
        out = np.empty_like(data)
        rc = self.L.sc_hip_volume_robust(self.h, C.byref(p), C.byref(layout), *(None if a is None else a.ctypes.data for a in
                                         (gx, gy, gt, data, state, weight, sx, sy, smt, boundary)), out.ctypes.data)
        self._check(rc, allow=(SC_ERR_NOT_CONVERGED,) if allow_not_converged else ())
        return out

    @staticmethod
    def make_volume_robust_jobs(n: int):
        return (VolumeRobustJob * n)()

    def volume_robust_device(self, params: VolumeRobustParams, layout: PoissonLayout, jobs, sync=True, allow_job_errors=False):
        """sc_hip_volume_robust_device: jobs is a VolumeRobustJob array (make_volume_robust_jobs) of device pointers, one frame layout and
        one frame stride for all.  sync: bSync and a wait for the stream.  Per-job codes in jobs[i].rc; returns the worst code:
        SC_ERR_NOT_CONVERGED is returned, other failures raise unless allow_job_errors (then they are returned as well)."""
        return self._device_call("sc_hip_volume_robust_device", params, layout, jobs, sync, allow_job_errors, (SC_ERR_NOT_CONVERGED,))

    # ---- robust flow volume solves on float32 arrays
    def volume_flow_robust(self, gx, gy, data, state, flow, weight=None, smooth_x=None, smooth_y=None, smooth_t=None, gt=None, boundary=None, tau=1.0,
                           loop=False, neumann=False, free_sides="", periodic="", p_grad=1.0, eps_grad=1e-3, p_time=1.0, eps_time=1e-3, p_data=2.0,
                           eps_data=1e-3, max_rounds=0, round_tol=0.0, tol=0.0, max_iters=0, allow_not_converged=False):
        """sc_hip_volume_flow_robust on numpy float32 arrays: volume_robust()'s problem, keywords and result with every temporal link --
        its weight, its gt, its penalty phi_r -- along `flow` ((T - 1) x H x W x 2, with loop T x H x W x 2, holding (dx, dy);
        volume_flow_planes' rules: rounded, NaN = no link).  gt and smooth_t stay stored at a link's source pixel.  flow None:
        volume_robust() itself."""
        kind, data, state, weight, sx, sy, smt, gx, gy, gt, boundary = volume_robust_arrays(gx, gy, data, state, weight, smooth_x, smooth_y, smooth_t,
                                                                                            gt, boundary, tau, loop, neumann, free_sides, periodic,
                                                                                            p_grad, eps_grad, p_time, eps_time, p_data, eps_data)
        fx, fy = (None, None) if flow is None else volume_flow_planes(flow, data.shape[0], data.shape[1], data.shape[2], loop)
        layout = poisson_layout_of(data[0])
        p = volume_robust_params(kind, data.shape[0], data[0].size, tau, loop, p_grad, eps_grad, p_time, eps_time, p_data, eps_data, max_rounds,
                                 round_tol, tol, max_iters)
        out = np.empty_like(data)
        rc = self.L.sc_hip_volume_flow_robust(self.h, C.byref(p), C.byref(layout), *(None if a is None else a.ctypes.data for a in
                                              (gx, gy, gt, data, state, weight, sx, sy, smt, fx, fy, boundary)), out.ctypes.data)
        self._check(rc, allow=(SC_ERR_NOT_CONVERGED,) if allow_not_converged else ())
        return out

    @staticmethod
    def make_volume_flow_robust_jobs(n: int):
        return (VolumeFlowRobustJob * n)()

    def volume_flow_robust_device(self, params: VolumeRobustParams, layout: PoissonLayout, jobs, sync=True, allow_job_errors=False):
        """sc_hip_volume_flow_robust_device: jobs is a VolumeFlowRobustJob array (make_volume_flow_robust_jobs) of device pointers; flow_x,
        flow_y are dense W x H x (T - 1; periodic time: T) float32 whatever the layout.  Codes as volume_robust_device."""
        return self._device_call("sc_hip_volume_flow_robust_device", params, layout, jobs, sync, allow_job_errors, (SC_ERR_NOT_CONVERGED,))

    # ---- robust sub-pixel flow volume solves on float32 arrays
    def volume_subflow_robust(self, gx, gy, data, state, flow, weight=None, smooth_x=None, smooth_y=None, smooth_t=None, gt=None, boundary=None,
                              tau=1.0, loop=False, neumann=False, free_sides="", periodic="", p_grad=1.0, eps_grad=1e-3, p_time=1.0, eps_time=1e-3,
                              p_data=2.0, eps_data=1e-3, max_rounds=0, round_tol=0.0, tol=0.0, max_iters=0, allow_not_converged=False):
        """sc_hip_volume_subflow_robust on numpy float32 arrays: volume_flow_robust()'s problem, keywords and result with `flow` taken as it
        is -- a temporal link, its penalty phi_r included, joins a pixel to the bilinear interpolation of the next frame at (x + dx,
        y + dy) (volume_subflow_planes' rules: float32, not rounded, NaN = no link).  gt and smooth_t stay stored at a link's source
        pixel.  flow None: volume_robust() itself."""
        kind, data, state, weight, sx, sy, smt, gx, gy, gt, boundary = volume_robust_arrays(gx, gy, data, state, weight, smooth_x, smooth_y, smooth_t,
                                                                                            gt, boundary, tau, loop, neumann, free_sides, periodic,
                                                                                            p_grad, eps_grad, p_time, eps_time, p_data, eps_data)
        fx, fy = (None, None) if flow is None else volume_subflow_planes(flow, data.shape[0], data.shape[1], data.shape[2], loop)
        layout = poisson_layout_of(data[0])
        p = volume_robust_params(kind, data.shape[0], data[0].size, tau, loop, p_grad, eps_grad, p_time, eps_time, p_data, eps_data, max_rounds,
                                 round_tol, tol, max_iters)
        out = np.empty_like(data)
        rc = self.L.sc_hip_volume_subflow_robust(self.h, C.byref(p), C.byref(layout), *(None if a is None else a.ctypes.data for a in
                                                 (gx, gy, gt, data, state, weight, sx, sy, smt, fx, fy, boundary)), out.ctypes.data)
        self._check(rc, allow=(SC_ERR_NOT_CONVERGED,) if allow_not_converged else ())
        return out

    def volume_subflow_robust_device(self, params: VolumeRobustParams, layout: PoissonLayout, jobs, sync=True, allow_job_errors=False):
        """sc_hip_volume_subflow_robust_device: volume_flow_robust_device()'s jobs (make_volume_flow_robust_jobs) with flow_x, flow_y
        real-valued.  Codes as volume_robust_device."""
        return self._device_call("sc_hip_volume_subflow_robust_device", params, layout, jobs, sync, allow_job_errors, (SC_ERR_NOT_CONVERGED,))

    # ---- coupled volume solves on float32 arrays
    def volume_coupled(self, coupling, gx, gy, data, state, weight=None, smooth_x=None, smooth_y=None, smooth_t=None, gt=None, boundary=None, tau=1.0,
                       loop=False, neumann=False, free_sides="", periodic="", p_grad=1.0, eps_grad=1e-3, p_time=1.0, eps_time=1e-3, p_data=2.0,
                       eps_data=1e-3, max_rounds=0, round_tol=0.0, tol=0.0, max_iters=0, allow_not_converged=False):
        """sc_hip_volume_coupled on numpy float32 arrays: volume_robust()'s problem, arguments and result with one penalty over several
        links -- coupling: SC_VOLUME_COUPLE_SPACE (per pixel over its x- and y-link: isotropic TV), | SC_VOLUME_COUPLE_TIME (and its forward
        temporal link: space-time TV; p_time = p_grad and eps_time = eps_grad), | SC_VOLUME_COUPLE_CHANNELS (every magnitude over the
        channels: vectorial TV); 0: volume_robust()'s bytes."""
        kind, data, state, weight, sx, sy, smt, gx, gy, gt, boundary = volume_robust_arrays(gx, gy, data, state, weight, smooth_x, smooth_y, smooth_t,
                                                                                            gt, boundary, tau, loop, neumann, free_sides, periodic,
                                                                                            p_grad, eps_grad, p_time, eps_time, p_data, eps_data)
        layout = poisson_layout_of(data[0])
        p = volume_robust_params(kind, data.shape[0], data[0].size, tau, loop, p_grad, eps_grad, p_time, eps_time, p_data, eps_data, max_rounds,
                                 round_tol, tol, max_iters)
        out = np.empty_like(data)
        rc = self.L.sc_hip_volume_coupled(self.h, C.byref(p), int(coupling), C.byref(layout), *(None if a is None else a.ctypes.data for a in
                                          (gx, gy, gt, data, state, weight, sx, sy, smt, boundary)), out.ctypes.data)
        self._check(rc, allow=(SC_ERR_NOT_CONVERGED,) if allow_not_converged else ())
        return out

    def volume_coupled_device(self, params: VolumeRobustParams, coupling: int, layout: PoissonLayout, jobs, sync=True, allow_job_errors=False):
        """sc_hip_volume_coupled_device: volume_robust_device() with a coupling (SC_VOLUME_COUPLE_*); jobs from make_volume_robust_jobs."""
        rc = self.L.sc_hip_volume_coupled_device(self.h, C.byref(params), int(coupling), C.byref(layout), jobs, len(jobs), bool(sync))
        if sync:
            self.sync()
        if allow_job_errors and rc != SC_ERR_HIP:
            return rc
        return self._check(rc, allow=(SC_ERR_NOT_CONVERGED,))

    # ---- coupled flow volume solves on float32 arrays
    def volume_flow_coupled(self, coupling, gx, gy, data, state, flow, weight=None, smooth_x=None, smooth_y=None, smooth_t=None, gt=None,
                            boundary=None, tau=1.0, loop=False, neumann=False, free_sides="", periodic="", p_grad=1.0, eps_grad=1e-3, p_time=1.0,
                            eps_time=1e-3, p_data=2.0, eps_data=1e-3, max_rounds=0, round_tol=0.0, tol=0.0, max_iters=0, allow_not_converged=False):
        """sc_hip_volume_flow_coupled on numpy float32 arrays: volume_coupled()'s problem, coupling, keywords and result with every temporal
        link -- its weight, its gt, its share of a magnitude -- along `flow` ((T - 1) x H x W x 2, with loop T x H x W x 2, holding (dx,
        dy); volume_flow_planes' rules: rounded, NaN = no link).  A temporal link belongs to its source pixel: gt, smooth_t and, under
        SC_VOLUME_COUPLE_TIME, its place in a magnitude.  flow None: volume_coupled() itself; coupling 0: volume_flow_robust()'s bytes."""
        if flow is None:
            return self.volume_coupled(coupling, gx, gy, data, state, weight, smooth_x, smooth_y, smooth_t, gt, boundary, tau, loop, neumann,
                                       free_sides, periodic, p_grad, eps_grad, p_time, eps_time, p_data, eps_data, max_rounds, round_tol, tol,
                                       max_iters, allow_not_converged)
        kind, data, state, weight, sx, sy, smt, gx, gy, gt, boundary = volume_robust_arrays(gx, gy, data, state, weight, smooth_x, smooth_y, smooth_t,
                                                                                            gt, boundary, tau, loop, neumann, free_sides, periodic,
                                                                                            p_grad, eps_grad, p_time, eps_time, p_data, eps_data)
        fx, fy = volume_flow_planes(flow, data.shape[0], data.shape[1], data.shape[2], loop)
        layout = poisson_layout_of(data[0])
        p = volume_robust_params(kind, data.shape[0], data[0].size, tau, loop, p_grad, eps_grad, p_time, eps_time, p_data, eps_data, max_rounds,
                                 round_tol, tol, max_iters)
        out = np.empty_like(data)
        rc = self.L.sc_hip_volume_flow_coupled(self.h, C.byref(p), int(coupling), C.byref(layout), *(None if a is None else a.ctypes.data for a in
                                               (gx, gy, gt, data, state, weight, sx, sy, smt, fx, fy, boundary)), out.ctypes.data)
        self._check(rc, allow=(SC_ERR_NOT_CONVERGED,) if allow_not_converged else ())
        return out

    def volume_flow_coupled_device(self, params: VolumeRobustParams, coupling: int, layout: PoissonLayout, jobs, sync=True, allow_job_errors=False):
        """sc_hip_volume_flow_coupled_device: volume_flow_robust_device() with a coupling (SC_VOLUME_COUPLE_*); jobs from
        make_volume_flow_robust_jobs."""
        rc = self.L.sc_hip_volume_flow_coupled_device(self.h, C.byref(params), int(coupling), C.byref(layout), jobs, len(jobs), bool(sync))
        if sync:
            self.sync()
        if allow_job_errors and rc != SC_ERR_HIP:
            return rc
        return self._check(rc, allow=(SC_ERR_NOT_CONVERGED,))

    # ---- robust solves on float32 arrays
    def robust(self, gx, gy, data, weight, smooth_x=None, smooth_y=None, boundary=None, neumann=False, out=None, free_sides="", periodic="",
               p_grad=1.0, eps_grad=1e-3, p_data=2.0, eps_data=1e-3, max_rounds=0, round_tol=0.0, tol=0.0, max_iters=0,
               allow_not_converged=False, isotropic=False, joint_channels=False):
        """sc_hip_robust on numpy float32 arrays of shape H x W or H x W x C (C 1..4): minimise sum weight phi_q(u - data) +
        sum smooth_x phi_p(d_x u - gx) + sum smooth_y phi_p(d_y u - gy), phi_r(t) = (2 / r) (t^2 + eps^2)^(r/2), p = p_grad, q = p_data, by
        reweighted WLS solves on the device, under the borders of poisson().  smooth_x, smooth_y: the base links as in wls(), or None
        (all 1).  isotropic: one penalty per pixel over its two forward links (SC_ROBUST_ISOTROPIC); joint_channels: one penalty over
        all channels (SC_ROBUST_JOINT_CHANNELS); both: vectorial TV.  max_rounds, round_tol, tol, max_iters: sc_robust_params' (0: the defaults; round_tol < 0: never stop early).  Returns
        out; info() has the total of the inner iterations and whether the round rule was met, robust_trace() the rounds."""
        kind, gx, gy, data, weight, sx, sy, boundary, out = robust_arrays(gx, gy, data, weight, smooth_x, smooth_y, boundary, out, neumann,
                                                                          free_sides, periodic, p_grad, eps_grad, p_data, eps_data, isotropic,
                                                                          joint_channels)
        p = robust_params(kind, p_grad, eps_grad, p_data, eps_data, max_rounds, round_tol, tol, max_iters)
        return self._host_call("sc_hip_robust", p, (gx, gy, data, weight, sx, sy, boundary), out, data,
                               (SC_ERR_NOT_CONVERGED,) if allow_not_converged else ())

    @staticmethod
    def make_robust_jobs(n: int):
        return (RobustJob * n)()

    def robust_device(self, params: RobustParams, layout: PoissonLayout, jobs, sync=True, allow_job_errors=False):
        """sc_hip_robust_device: jobs is a RobustJob array (make_robust_jobs) of device pointers, one layout for all.  sync: bSync and a
        wait for the stream.  Per-job codes in jobs[i].rc; returns the worst code: SC_ERR_NOT_CONVERGED is returned, other failures
        raise unless allow_job_errors (then they are returned as well)."""
        return self._device_call("sc_hip_robust_device", params, layout, jobs, sync, allow_job_errors, (SC_ERR_NOT_CONVERGED,))

    def robust_trace(self):
        """(energy, iters) of the last robust call's last chunk (robust, region_robust, volume_robust, volume_coupled, volume_flow_robust, volume_subflow_robust or volume_flow_coupled, whichever ran last): float64 and int32 arrays with one entry per round, the quadratic one
        included -- the energy (summed over the chunk's planes) of the iterate that round produced and its inner iterations."""
        n = int(self.L.sc_hip_robust_trace(self.h, None, None, 0))
        energy, iters = np.zeros(n, np.float64), np.zeros(n, np.int32)
        if n:
            self.L.sc_hip_robust_trace(self.h, energy.ctypes.data_as(f64p), iters.ctypes.data_as(i32p), n)
        return energy, iters

    # ---- device-resident images
    def malloc(self, nbytes):
        p = self.L.sc_hip_malloc(self.h, nbytes)
        if not p:
            raise SeamlessCloneError(SC_ERR_HIP, f"hipMalloc({nbytes}) failed")
        return p

    def free(self, p):
        self.L.sc_hip_free(self.h, p)

    def pinned_array(self, shape, dtype=np.uint8):
        """numpy array over page-locked host memory (hipHostMalloc).  Returns (array, handle); release the memory with
        free_pinned(handle) after the last use of the array."""
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = self.L.sc_hip_host_alloc(self.h, n)
        if not p:
            raise SeamlessCloneError(SC_ERR_HIP, f"hipHostMalloc({n}) failed")
        buf = (C.c_uint8 * n).from_address(p)
        return np.frombuffer(buf, dtype=dtype).reshape(shape), p

    def free_pinned(self, handle):
        self.L.sc_hip_host_free(self.h, handle)

    def to_device(self, a: np.ndarray):
        a = np.ascontiguousarray(a)
        p = self.malloc(a.nbytes)
        self._check(self.L.sc_hip_memcpy_h2d(self.h, p, a.ctypes.data, a.nbytes))
        return p

    def from_device(self, p, shape, dtype=np.uint8):
        out = np.empty(shape, dtype)
        self._check(self.L.sc_hip_memcpy_d2h(self.h, out.ctypes.data, p, out.nbytes))
        return out

    def copy_d2d_async(self, dst, src, nbytes):
        self._check(self.L.sc_hip_memcpy_d2d_async(self.h, dst, src, nbytes))

    def run_device(self, d_face, fshape, d_body, bshape, d_mask, mshape, cx, cy, sync=True,
                   allow_not_converged=False, face_step=None, body_step=None, mask_step=None):
        """shapes are (rows, cols); rows are dense (step = cols * channels) unless a step is given."""
        rc = self.L.sc_hip_run_device(self.h, d_face, fshape[1], fshape[0], face_step or 3 * fshape[1],
                                      d_body, bshape[1], bshape[0], body_step or 3 * bshape[1],
                                      d_mask, mshape[1], mshape[0], mask_step or mshape[1], int(cx), int(cy), bool(sync))
        return self._check(rc, allow=(SC_ERR_NOT_CONVERGED,) if allow_not_converged else ())

    def run_device_batch(self, jobs, sync=True):
        """jobs: a BatchJob array (Pool.make_jobs) of device-resident clones.  Members whose ROIs have one size are solved
        as one field of 3n channels through one set of launches (sc_hip_run_device_batch); per-member codes in jobs[i].rc."""
        rc = self.L.sc_hip_run_device_batch(self.h, jobs, len(jobs))
        if sync:
            self.sync()
        return self._check(rc, allow=(SC_ERR_NOT_CONVERGED,))

    # ---- stage hooks
    def mask_stage(self, mask, cx, cy):
        m = _img(mask)
        geo = np.zeros(6, np.int32)
        M = np.zeros(m[1] * m[2], np.uint8)
        self._check(self.L.sc_hip_mask_stage(self.h, *m, int(cx), int(cy), geo.ctypes.data_as(i32p),
                                             M.ctypes.data_as(u8p), M.size))
        W, H = int(geo[2]), int(geo[3])
        return geo, M[:W * H].reshape(H, W).copy()

    def build_rhs(self, face, body, mask, cx, cy):
        f, b, m = _img(face), _img(body), _img(mask)
        geo = np.zeros(6, np.int32)
        cap = m[1] * m[2]
        B = np.zeros(3 * cap, np.float32)
        lap = np.zeros(3 * cap, np.float32)
        self._check(self.L.sc_hip_build_rhs(self.h, *f, *b, *m, int(cx), int(cy), geo.ctypes.data_as(i32p),
                                            B.ctypes.data_as(f32p), lap.ctypes.data_as(f32p), cap))
        W, H = int(geo[2]), int(geo[3])
        return geo, B[:3 * W * H].reshape(3, H, W).copy(), lap[:3 * W * H].reshape(3, H, W).copy()

    def front_end_device(self, jobs, form, storage=0, guess=None, fields=True, allow=()):
        """sc_hip_front_end_device on a BatchJob array of device-resident images at the caller's bases and steps.  Returns one dict per
        member: rect_dev, rect_host (the raw rectangle, device copy and pinned mailbox), rc, geo, and with `fields` M, B (None when
        storage bit 2 is set), lap of the ROI the launches ran on.  allow: codes of the call that do not raise."""
        n = len(jobs)
        cap = max(int(j.mask_cols) for j in jobs) * max(int(j.mask_rows) for j in jobs) if fields else 0
        rd, rh, geo = np.zeros((n, 4), np.int32), np.zeros((n, 4), np.int32), np.zeros((n, 6), np.int32)
        M = np.zeros((n, cap), np.uint8) if fields else None
        B = np.zeros((n, 3 * cap), np.float32) if fields else None
        lap = np.zeros((n, 3 * cap), np.float32) if fields else None
        g = None if guess is None else np.ascontiguousarray(guess, np.int32).reshape(n, 4)
        rc = self.L.sc_hip_front_end_device(self.h, jobs, n, int(form), int(storage), None if g is None else g.ctypes.data_as(i32p),
                                            rd.ctypes.data_as(i32p), rh.ctypes.data_as(i32p), geo.ctypes.data_as(i32p),
                                            M.ctypes.data_as(u8p) if fields else None, B.ctypes.data_as(f32p) if fields else None,
                                            lap.ctypes.data_as(f32p) if fields else None, cap)
        self._check(rc, allow=allow)
        out = []
        for i in range(n):
            W, H = int(geo[i, 2]), int(geo[i, 3])
            d = dict(rect_dev=tuple(int(v) for v in rd[i]), rect_host=tuple(int(v) for v in rh[i]), rc=int(jobs[i].rc), geo=geo[i].copy(), M=None, B=None, lap=None)
            if fields and rc == SC_OK and W > 0 and jobs[i].rc == SC_OK:
                d["M"] = M[i, :W * H].reshape(H, W).copy()
                d["lap"] = lap[i, :3 * W * H].reshape(3, H, W).copy()
                if not storage & 4:
                    d["B"] = B[i, :3 * W * H].reshape(3, H, W).copy()
            out.append(d)
        return out

    def field_load(self, U, lap):
        U = np.ascontiguousarray(U, np.float32)
        lap = np.ascontiguousarray(lap, np.float32)
        assert U.shape == lap.shape and U.ndim == 3
        Cc, H, W = U.shape
        self._check(self.L.sc_hip_field_load(self.h, W, H, Cc, U.ctypes.data_as(f32p), lap.ctypes.data_as(f32p)))

    def bytes_writer(self):
        """Who wrote the judged cycles' bytes since the last call of this (which clears it): bit 0 a splice launch, bit 1 the judged launch itself, interleaved."""
        return int(self.L.sc_hip_bytes_writer(self.h))

    def u0_reader(self):
        """Where the first level-0 launches read their initial field since the last call of this (which clears it): bit 0 float16 planes,
        bit 1 the destinations' bytes, bit 2 planes a safety-net launch filled."""
        return int(self.L.sc_hip_u0_reader(self.h))

    def field_shape(self):
        whc = np.zeros(3, np.int32)
        self._check(self.L.sc_hip_field_shape(self.h, whc.ctypes.data_as(i32p)))
        return int(whc[2]), int(whc[1]), int(whc[0])

    def field_sweep(self, method, sweeps, omega=1.0, sweeps_per_launch=1):
        self._check(self.L.sc_hip_field_sweep(self.h, int(method), int(sweeps), float(omega), int(sweeps_per_launch)))

    def field_residual(self):
        out = np.zeros(2, np.float64)
        self._check(self.L.sc_hip_field_residual(self.h, out.ctypes.data_as(f64p)))
        return float(out[0]), float(out[1])

    def field_solve(self, allow_not_converged=False):
        rc = self.L.sc_hip_field_solve(self.h)
        return self._check(rc, allow=(SC_ERR_NOT_CONVERGED,) if allow_not_converged else ())

    def field_store(self):
        out = np.zeros(self.field_shape(), np.float32)
        self._check(self.L.sc_hip_field_store(self.h, out.ctypes.data_as(f32p), out.size))
        return out

    def field_finish(self, body, ltx, lty):
        """Post-process alone: the field on the device -> clamp, truncate, interleave into `body` (in place)."""
        b = _img(body)
        self._check(self.L.sc_hip_field_finish(self.h, *b, int(ltx), int(lty)))

    def field_lowmode(self):
        """Float-table correction alone on the field on the device (result += correction)."""
        self._check(self.L.sc_hip_field_lowmode(self.h))

    def field_time_sweeps(self, method, launches, sweeps_per_launch=1, omega=1.0) -> float:
        ms = C.c_float(0)
        self._check(self.L.sc_hip_field_time_sweeps(self.h, int(method), int(launches), int(sweeps_per_launch),
                                                    float(omega), C.byref(ms)))
        return float(ms.value)

    def time_cycle0(self, launches: int = 100) -> float:
        ms = C.c_float(0)
        self._check(self.L.sc_hip_time_cycle0(self.h, int(launches), C.byref(ms)))
        return float(ms.value)

    def time_cycle0_form(self, form: int, launches: int = 100) -> float:
        ms = C.c_float(0)
        self._check(self.L.sc_hip_time_cycle0_form(self.h, int(form), int(launches), C.byref(ms)))
        return float(ms.value)

    def time_coarse_chain(self, reps: int = 50):
        """(ms per pass as plain launches, ms per pass as HIP-graph replays, dependent launches per pass)"""
        a, b, n = C.c_float(0), C.c_float(0), C.c_int(0)
        self._check(self.L.sc_hip_time_coarse_chain(self.h, int(reps), C.byref(a), C.byref(b), C.byref(n)))
        return float(a.value), float(b.value), int(n.value)

    def time_tail_phases(self):
        """shader-clock differences between the eleven phase boundaries of one k_mg_tail launch (ten numbers)"""
        buf = (C.c_ulonglong * 11)()
        self._check(self.L.sc_hip_time_tail_phases(self.h, buf))
        return [int(buf[i + 1]) - int(buf[i]) for i in range(10)]


class _Borrowed(Instance):
    """An instance owned by a native pool: same methods, no destroy."""

    def __init__(self, L, handle, gpu_id):          # noqa: D401 - no create call
        self.L, self.h, self.gpu_id = L, handle, gpu_id

    def destroy(self):
        self.h = None


class Pool:
    """The library's native batch driver (csrc/sc_pool.cpp): K instances = K HIP streams on one GPU,
    one C++ worker thread each, jobs pulled from a shared counter."""

    def __init__(self, gpu_id: int = 0, streams: int = 4, group: int = 1, clone_mode: int = SC_NORMAL_CLONE, **solver):
        self.L = load()
        self.h = self.L.sc_hip_pool_create(int(gpu_id), int(streams))
        if not self.h:
            raise SeamlessCloneError(SC_ERR_HIP, f"cannot create a pool on GPU {gpu_id} (no CPU fallback)")
        self.gpu_id = gpu_id
        self.instances = [_Borrowed(self.L, self.L.sc_hip_pool_instance(self.h, k), gpu_id)
                          for k in range(self.L.sc_hip_pool_size(self.h))]
        if group != 1 and self.L.sc_hip_pool_set_group(self.h, int(group)) != SC_OK:
            raise SeamlessCloneError(SC_ERR_BAD_ARG, f"bad group size {group}")
        self.group = group
        if solver:
            o = self.instances[0].get_solver()
            for k, v in solver.items():
                setattr(o, k, v)
            rc = self.L.sc_hip_pool_set_solver(self.h, C.byref(o))
            if rc != SC_OK:
                raise SeamlessCloneError(rc, "bad solver options")
        if clone_mode != SC_NORMAL_CLONE:
            self.set_clone_mode(clone_mode)

    @staticmethod
    def make_jobs(n: int):
        return (BatchJob * n)()

    def set_solver(self, **solver):
        """The same options on every instance of the pool (between batches)."""
        o = self.instances[0].get_solver()
        for k, v in solver.items():
            if not hasattr(o, k):
                raise AttributeError(k)
            setattr(o, k, v)
        rc = self.L.sc_hip_pool_set_solver(self.h, C.byref(o))
        if rc != SC_OK:
            raise SeamlessCloneError(rc, "bad solver options")

    def set_clone_mode(self, mode: int) -> None:
        """The same clone mode on every instance of the pool (between batches)."""
        rc = self.L.sc_hip_pool_set_clone_mode(self.h, int(mode))
        if rc != SC_OK:
            raise SeamlessCloneError(rc, f"bad clone mode {mode}")

    def run(self, jobs, device_resident: bool):
        rc = self.L.sc_hip_pool_run(self.h, jobs, len(jobs), 1 if device_resident else 0)
        if rc != SC_OK:
            raise SeamlessCloneError(rc, "a batch job failed (see jobs[i].rc)")

    def run_host(self, items):
        """items: (face, body, mask, cx, cy) numpy tuples; bodies are blended in place."""
        jobs = self.make_jobs(len(items))
        for j, (face, body, mask, cx, cy) in zip(jobs, items):
            f, b, m = _img(face), _img(body), _img(mask)
            (j.face, j.face_cols, j.face_rows, j.face_step) = f
            (j.body, j.body_cols, j.body_rows, j.body_step) = b
            (j.mask, j.mask_cols, j.mask_rows, j.mask_step) = m
            j.centerX, j.centerY, j.body_restore = int(cx), int(cy), None
        self.run(jobs, device_resident=False)

    def edit(self, params: EditParams, jobs, device_resident: bool):
        """sc_hip_pool_edit: an EditJob array (Instance.make_edit_jobs), one op and parameter set for all.  Device-resident jobs go
        in chunks of one image size through sc_hip_edit_device_batch, host images one sc_hip_edit per job."""
        rc = self.L.sc_hip_pool_edit(self.h, C.byref(params), jobs, len(jobs), 1 if device_resident else 0)
        if rc not in (SC_OK, SC_ERR_NOT_CONVERGED):
            raise SeamlessCloneError(rc, "an edit job failed (see jobs[i].rc)")

    def edit_host(self, params: EditParams, items):
        """items: (src, mask, dst) numpy tuples (H x W x 3, H x W, H x W x 3 uint8; dst may be src); dst is written."""
        jobs = Instance.make_edit_jobs(len(items))
        for j, (src, mask, dst) in zip(jobs, items):
            s, m, d = _img(src), _img(mask), _img(dst)
            if m[1:3] != s[1:3] or d[1:3] != s[1:3]:
                raise ValueError("src, mask and dst must have one size")
            (j.src, j.cols, j.rows, j.src_step) = s
            j.mask, j.mask_step = m[0], m[3]
            j.dst, j.dst_step = d[0], d[3]
        self.edit(params, jobs, device_resident=False)
        return jobs

    def close(self):
        if getattr(self, "h", None):
            self.L.sc_hip_pool_destroy(self.h)
            self.h = None
            self.instances = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def plan_size(W: int, H: int, opts: "SolverOpts | None" = None) -> dict:
    """Host-only: what decides the size class of a W x H ROI (ring included)."""
    out = np.zeros(12, np.int32)
    load().sc_hip_plan_size(int(W), int(H), C.byref(opts) if opts is not None else None, out.ctypes.data_as(i32p))
    keys = ("eligible", "levels", "tail_level", "pad_x", "pad_y", "Kxp", "Kyp", "column_tiles", "row_splits", "direct_nx_ny", "solo_differs", "conditional")
    return dict(zip(keys, out.tolist()))


def plan_groups_pool(sizes, group: int = 0, streams: int = 2, opts: "SolverOpts | None" = None):
    """Host-only: plan_groups as a Pool(streams, group) forms its groups (group 0 = SC_POOL_GROUP_AUTO; jobs largest first)."""
    wh = np.ascontiguousarray(np.asarray(sizes, np.int32).reshape(-1, 2))
    n = wh.shape[0]
    g = np.zeros(n, np.int32); k = np.zeros(n, np.int32)
    rc = load().sc_hip_plan_groups_pool(wh.ctypes.data_as(i32p), n, int(group), int(streams), C.byref(opts) if opts is not None else None,
                                        g.ctypes.data_as(i32p), k.ctypes.data_as(i32p))
    if rc < 0:
        raise SeamlessCloneError(rc, "sc_hip_plan_groups_pool")
    return g.tolist(), k.tolist()


SC_POOL_GROUP_AUTO = 0


def plan_edit_groups_pool(sizes, group: int = 0, streams: int = 2):
    """Host-only: the chunks a Pool(streams, group) forms for device-resident edits of images of these sizes [(W, H), ...]:
    group_of per job (group 0 = SC_POOL_GROUP_AUTO)."""
    wh = np.ascontiguousarray(np.asarray(sizes, np.int32).reshape(-1, 2))
    n = wh.shape[0]
    g = np.zeros(n, np.int32)
    rc = load().sc_hip_plan_edit_groups_pool(wh.ctypes.data_as(i32p), n, int(group), int(streams), g.ctypes.data_as(i32p))
    if rc < 0:
        raise SeamlessCloneError(rc, "sc_hip_plan_edit_groups_pool")
    return g.tolist()


def plan_prepare(sizes, opts: "SolverOpts | None" = None) -> int:
    """Host-only: memoise the plans and per-size host tables of these ROI sizes ahead of the calls that will meet them; returns how
    many can join a size class."""
    wh = np.ascontiguousarray(np.asarray(sizes, np.int32).reshape(-1, 2))
    return int(load().sc_hip_plan_prepare(wh.ctypes.data_as(i32p), wh.shape[0], C.byref(opts) if opts is not None else None))


def plan_cache_clear() -> None:
    load().sc_hip_plan_cache_clear()


CYCLE0_FACTS = ("sweeps", "prolong", "f_half", "u_half", "q16_in", "q16_out", "final_cycle", "out_bytes", "composed", "l1_half", "timing",
                "bands", "rag")


def cycle0_form(**facts):
    """Host-only: (T, PRO, TAG) of the k_cycle0 instantiation the level-0 launcher picks for these facts of a launch descriptor
    (CYCLE0_FACTS; those left out are 0 / false), or -1 where the library has no such form (csrc/sc_cycle0.hip)."""
    if facts.pop("out_interleaved", 0):      # travels as bit 1 of out_bytes (sc_hip_cycle0_form)
        facts["out_bytes"] = int(bool(facts.get("out_bytes", 0))) | 2
    if facts.pop("in_bytes", 0):             # ... and as bit 1 of u_half
        facts["u_half"] = int(bool(facts.get("u_half", 0))) | 2
    f = (C.c_int * len(CYCLE0_FACTS))(*[int(facts.pop(k, 0)) for k in CYCLE0_FACTS])
    if facts:
        raise TypeError("cycle0_form: no such fact: %s" % sorted(facts))
    out = (C.c_int * 3)()
    return tuple(out) if load().sc_hip_cycle0_form(f, 0, out) == 0 else -1


def u0_bytes_fetch(buf, offset, W, xw):
    """Host-only: what the first launch that reads destination bytes fetches for the 64 lanes of a wave whose lane 0 serves column xw, of
    one ROI row (csrc/sc_u0_bytes.h): the row starts `offset` bytes into the uint8 array `buf`.  Returns an int32 array [64, 16]:
    offset of the first dword from the row, shift, mask of dwords read, unguarded, then the four values of each of the three channels."""
    out = np.empty((64, 16), np.int32)
    rc = load().sc_hip_u0_bytes_fetch(C.c_void_p(buf.ctypes.data + offset), W, xw, out.ctypes.data_as(i32p))
    if rc:
        raise ValueError("sc_hip_u0_bytes_fetch: %d" % rc)
    return out


def coarse_tile_plan(W, H, C_, useful, halo, rows, size_class=False, unpacked=False, lanes=False):
    """Host-only: the column tiling of a coarse-level multigrid launch: (full column tiles, lanes per slot, planes per packed
    workgroup, workgroups).  lanes=True: also, per workgroup, (row tile [n], lanes per slot [n], plane [n, 64], first column [n, 64])."""
    f = (C.c_int * 10)(W, H, C_, useful, halo, rows, int(size_class), int(unpacked), 0, 0)
    head = np.zeros(4, np.int32)
    rc = load().sc_hip_coarse_tile_plan(f, head.ctypes.data_as(i32p))
    if rc != 0:
        raise SeamlessCloneError(rc, "coarse_tile_plan")
    if not lanes:
        return tuple(int(v) for v in head)
    n = int(head[3])
    f[9] = n
    out = np.zeros(4 + 130 * n, np.int32)
    rc = load().sc_hip_coarse_tile_plan(f, out.ctypes.data_as(i32p))
    if rc != 0:
        raise SeamlessCloneError(rc, "coarse_tile_plan")
    t = out[4:].reshape(n, 130)
    return tuple(int(v) for v in head), (t[:, 0], t[:, 1], t[:, 2::2], t[:, 3::2])


CYCLE0_PLAN = ("nbx", "nby", "xstep", "ystep", "hx", "hy", "waves", "rows", "levels", "bottom", "tail", "composes", "n1x", "n1y", "n2x", "n2y")
CYCLE0_INNER = ("inner", "x_first", "x_last", "y_first", "y_last", "l1_x", "l1_y_first", "l1_y_last", "l2_x", "l2_y")


def cycle0_plan(W, H, sweeps, prolong=False, composed=False):
    """Host-only: the tiling of a level-0 multigrid launch with `sweeps` sweeps on a W x H field (ring included) and what the kernel's
    wave-uniform `inner` test answers for each of its waves (sc_hip_cycle0_plan): a dict of CYCLE0_PLAN (the last eight: the library's
    own ladder for the size) plus "inner": int array [nby, nbx, waves], an index into CYCLE0_INNER (0: the mask-free forms)."""
    f = (C.c_int * 5)(int(W), int(H), int(sweeps), int(bool(prolong)), int(bool(composed)))
    n = len(CYCLE0_PLAN)
    head = np.zeros(n, np.int32)
    rc = load().sc_hip_cycle0_plan(f, head.ctypes.data_as(i32p), n)
    if rc != 0:
        raise SeamlessCloneError(rc, "cycle0_plan")
    waves = int(head[0]) * int(head[1]) * int(head[6])
    out = np.zeros(n + waves, np.int32)
    rc = load().sc_hip_cycle0_plan(f, out.ctypes.data_as(i32p), n + waves)
    if rc != 0:
        raise SeamlessCloneError(rc, "cycle0_plan")
    plan = dict(zip(CYCLE0_PLAN, (int(v) for v in out[:n])))
    plan["inner"] = out[n:].reshape(int(head[1]), int(head[0]), int(head[6])).copy()
    return plan


PCG_PLAN = ("nx", "ny", "x0", "y0", "cg", "bands", "rows", "eparts", "egroups", "stride")


def pcg_plan(cols, rows, kind, frames=1):
    """Host-only: the tiling of the work planes a conjugate-gradient call (weighted, WLS, robust, region; frames > 1: a volume call)
    runs with on cols x rows pixels under the border word `kind` (sc_hip_pcg_plan): a dict of PCG_PLAN."""
    out = (C.c_longlong * len(PCG_PLAN))()
    rc = load().sc_hip_pcg_plan(int(cols), int(rows), int(kind), int(frames), out)
    if rc != 0:
        raise SeamlessCloneError(rc, "pcg_plan")
    return dict(zip(PCG_PLAN, (int(v) for v in out)))


FUSED_FACTS = ("pre", "post", "budget", "tol", "out_wanted", "q16", "u_half", "composed", "separate_restrict", "early_kind", "bytes_form", "small")
FUSED_ROW = ("kind", "sweeps", "prolong", "final_cycle", "out_bytes", "u_half", "q16_in", "q16_out", "composed", "bands", "lm", "nodes", "judged",
             "coarse_first", "sat", "bands_asked", "early_asked", "cycle")


def fused_schedule(verdicts=(), **facts):
    """Host-only: the level-0 launches of a fused multigrid solve with these facts (FUSED_FACTS; defaults: the default clone's) whose
    judged launches meet `verdicts` (sc_hip_fused_schedule): ([one dict of FUSED_ROW per launch], sweeps, sweep_launches, code)."""
    d = dict(pre=2, post=2, budget=30, tol=0, out_wanted=1, q16=1, u_half=1, composed=1, separate_restrict=0, early_kind=1, bytes_form=1, small=1)
    unknown = sorted(set(facts) - set(d))
    if unknown:
        raise TypeError("fused_schedule: no such fact: %s" % unknown)
    d.update(facts)
    f = (C.c_int * len(FUSED_FACTS))(*[int(d[k]) for k in FUSED_FACTS])
    v = (C.c_int * max(1, len(verdicts)))(*[int(x) for x in verdicts])
    cap = len(FUSED_ROW) * (3 * int(d["budget"]) + 2) + 3
    out = (C.c_int * cap)()
    n = load().sc_hip_fused_schedule(f, v, len(verdicts), out, cap)
    if n < 0:
        raise SeamlessCloneError(n, "fused_schedule")
    k = len(FUSED_ROW)
    return [dict(zip(FUSED_ROW, out[k * i:k * i + k])) for i in range(n)], out[k * n], out[k * n + 1], out[k * n + 2]


def restore_spans(step, rows, ltx, lty, W, H):
    """Host-only: the byte spans [(begin, end), ...] a grouped member's frame-only restore copies (sc_hip_restore_spans)."""
    cap = max(2, int(H))
    out = (C.c_longlong * (2 * cap))()
    n = load().sc_hip_restore_spans(int(step), int(rows), int(ltx), int(lty), int(W), int(H), out, cap)
    if n < 0:
        raise SeamlessCloneError(n, "restore_spans")
    return [(out[2 * k], out[2 * k + 1]) for k in range(n)]


def cycle0_forms():
    """Host-only: every (T, PRO, TAG) in the library's table of instantiated level-0 forms."""
    out = (C.c_int * 3)()
    return [tuple(out) for i in range(load().sc_hip_cycle0_form(None, -1, out)) if load().sc_hip_cycle0_form(None, i, out)]


def plan_groups(sizes, cap: int = 0, opts: "SolverOpts | None" = None):
    """Host-only: how a batch whose members have these ROI sizes [(W, H), ...] (ring included) is partitioned into sets of launches:
    (group_of, kind_of) per member -- kind 0 alone, 1 a same-size group, 2 a size class (csrc/sc_ragged.cpp)."""
    L = load()
    wh = np.ascontiguousarray(np.asarray(sizes, np.int32).reshape(-1, 2))
    n = wh.shape[0]
    g = np.zeros(n, np.int32); k = np.zeros(n, np.int32)
    rc = L.sc_hip_plan_groups(wh.ctypes.data_as(i32p), n, int(cap), C.byref(opts) if opts is not None else None,
                              g.ctypes.data_as(i32p), k.ctypes.data_as(i32p))
    if rc < 0:
        raise SeamlessCloneError(rc, "plan_groups")
    return g.tolist(), k.tolist()


def source_fingerprint() -> str:
    """sha256 (16 hex digits) over the library's sources (csrc/*.hip, *.cpp, *.h and both headers).  Profiles under
    profiles/ record it; bench.py refuses to quote counter figures captured from other sources (traffic_stale)."""
    import glob
    import hashlib
    h = hashlib.sha256()
    files = sorted(glob.glob(os.path.join(_PKG, "csrc", "*.hip")) + glob.glob(os.path.join(_PKG, "csrc", "*.cpp")) +
                   glob.glob(os.path.join(_PKG, "csrc", "*.h")) + [HEADER_PATH, TESTING_HEADER_PATH])
    for f in files:
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def device_count() -> int:
    return int(load().sc_hip_device_count())


def device_pci_bus_id(gpu_id: int) -> str | None:
    """'0000:c1:00.0' of HIP device gpu_id, or None (no such device)."""
    buf = C.create_string_buffer(64)
    if load().sc_hip_device_pci_bus_id(int(gpu_id), buf, 64) != SC_OK:
        return None
    return buf.value.decode() or None
