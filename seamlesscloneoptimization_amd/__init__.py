"""MI355X-native seamless clone (Poisson image editing, NORMAL_CLONE).

Product code only: the HIP shared library (csrc/ -> libseamlessclone_hip.so), its ctypes
binding (capi), the reference-shaped Python class (seamless_clone), OpenCV-yml/BMP I/O (ymlio)
and the vs.py-equivalent checker (compare).  Nothing here imports torch or the CPU oracle.
"""
from . import capi, compare, ymlio  # noqa: F401
from .seamless_clone import (SeamlessClone, colorChange, edit_batch, gradient_filter, illuminationChange,  # noqa: F401
                             interpolate_constraints, make_tileable, poisson_solve, poisson_solve_batch, screened_solve, screened_solve_batch, seamlessClone,
                             textureFlattening, weighted_solve, weighted_solve_batch, wls_filter, wls_solve, wls_solve_batch, robust_solve,
                             robust_solve_batch, tv_denoise, integrate_gradients, region_solve, region_solve_batch, inpaint, poisson_clone, volume_solve, inpaint_video,
                             poisson_clone_video, volume_wls_solve, wls_filter_video, interpolate_constraints_video, make_loop,
                             volume_robust_solve, volume_flow_coupled_solve, tv_denoise_video, tv_denoise_video_along_flow, tv_inpaint_video, integrate_gradients_video, region_robust_solve, region_robust_solve_batch,
                             tv_inpaint, integrate_gradients_masked, bounded_solve, bounded_solve_batch, poisson_clone_in_range,
                             interpolate_in_range)

__all__ = ["capi", "compare", "ymlio", "SeamlessClone", "seamlessClone", "colorChange", "illuminationChange", "textureFlattening",
           "edit_batch", "poisson_solve", "poisson_solve_batch", "screened_solve", "screened_solve_batch", "gradient_filter",
           "make_tileable", "weighted_solve", "weighted_solve_batch", "interpolate_constraints", "wls_solve",
           "wls_solve_batch", "wls_filter", "robust_solve", "robust_solve_batch", "tv_denoise", "integrate_gradients",
           "region_solve", "region_solve_batch", "inpaint", "poisson_clone", "volume_solve", "inpaint_video", "poisson_clone_video",
           "volume_wls_solve", "wls_filter_video", "interpolate_constraints_video", "make_loop",
           "volume_robust_solve", "volume_flow_coupled_solve", "tv_denoise_video", "tv_denoise_video_along_flow", "tv_inpaint_video", "integrate_gradients_video", "region_robust_solve", "region_robust_solve_batch",
           "tv_inpaint", "integrate_gradients_masked", "bounded_solve", "bounded_solve_batch", "poisson_clone_in_range",
           "interpolate_in_range"]
