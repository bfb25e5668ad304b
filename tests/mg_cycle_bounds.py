"""The yardstick of the multigrid cycle walk and its bounds (tests/test_gpu_mg_cycles.py, tests/test_mg_cycles_host.py; the shapes:
tests/mg_cycle_cases.py).  Nothing here is tuned on the device: every number comes from oracle/mg_np.py.

A solve with max_sweeps = n, update_tol = 1e-30 and tol = 0 leaves iterate n.  Per shape, plane and budget n:

    u64      the float64 TWIN of the cycle (mg_np.solve(dtype=float64)): the same schedule, coefficients and format roundings, the rest in double
    u32      the float32 restatement that rounds where the kernels round (residual_f32: float32, level 0 in difference form; direct_f32: the
             direct level as four float32 products)
    D(x)     max over the interior of |x - u64|

Float routes -- the field hooks (fused and sweeps_per_launch = 1) and the kept field of a clone under SC_FLAG_FLOAT_L1:

    D(gpu) <= STEP_FACTOR x D(u32)

STEP_FACTOR = 7 is pcg_steps_bounds': the project's margin for "device float32 against its float32 restatement, both against the float64
twin".  The field hooks also keep the absolute caps of test_multigrid_cycles_follow_the_spec against the default spec (ABS_CAP), so the walk
is never looser than that test.

Format routes -- the kept field of a default clone (float16 right-hand side, initial field and level 1 on the composed schedule) and its
bytes (the 16-bit field between the first launches besides): the twin carries the same formats (u64f), and between the device and the
twin a stored code may round the other way.  The allowance for that is the reference's own: E_fmt = max |u64f - u64|, every rounding
of the formats at once:

    max |gpu - u64f| <= E_fmt + STEP_FACTOR x D(u32)              (bytes: decided_np.crossed_bound(u64f, bytes) in place of the difference)

The two terms ADD.  A code flips where the device's float32 value and the twin's double value lie on either side of a rounding point, so
the flips are caused by the float32 error (at most STEP_FACTOR x D(u32), which the SC_FLAG_FLOAT_L1 run asserts) and sized by the format's
step (what E_fmt measures); the device carries its float32 error besides.  max() of the two would hold only if one of them were absent.
From the second cycle on both are present: the values a format rounds carry the 4e-5 float32 noise of a field of magnitude 255 while the
format's step at their own magnitude has shrunk (level 1's correction is ~1 in the second cycle: a float16 step of 1e-3; ~100 in the
first, whose values are dyadic and exact in either precision), so a few percent of the codes of ANY float32 evaluation round the other way
than the twin's.  The float32 restatement with the formats does so on the CPU: 2.1e-4 .. 4.8e-4 from u64f at n = 2 where E_fmt is
2.9e-4 .. 5.3e-4 and D(u32) 4e-5; the host test holds it to this same bound.

The tight bound of the FLOAT_L1 run catches seam defects; this one a wrong float16 or 16-bit load or store (tests/test_mg_cycles_host.py: a
store that truncates misses it at every budget).  Where the shape's ladder does
not compose level 1 the library runs no format beyond the float16 right-hand side and initial field, which hold a clone's integers
exactly: u64f is u64 and E_fmt is 0."""
import functools

import numpy as np

import mg_cycle_cases as cases
from pcg_steps_bounds import STEP_FACTOR

ABS_CAP = {1: 2e-2, 3: 2e-3}            # test_multigrid_cycles_follow_the_spec's, against the default spec
# the float-table node correction on the device against oracle/lowmode_np.correction: the bound of tests/test_gpu_decided_channels.py and
# test_gpu_round2.py::test_float_table_correction_alone -- CORR_REL x max(1, max |correction|) + CORR_ABS
CORR_REL, CORR_ABS = 3e-4, 1e-4


def interior_max(a):
    return float(np.abs(np.asarray(a, np.float64))[..., 1:-1, 1:-1].max())


def plane(name, route, c):
    """(U0 with its ring, F) of one plane: route "fields" (the noise fields, c = 0) or "clone" (channel c of the clone's B, lap)"""
    if route == "fields":
        U, F = cases.noise_fields(name)
        return U[c], F[c]
    B, lap = cases.clone_inputs(name)[5:7]
    return B[c], lap[c]


@functools.lru_cache(maxsize=None)
def solve(name, route, c, n, kind, fused=True):
    """One restatement of iterate n, computed once per process and never written into.  kind: "spec" (the default float32 spec), "u32"
    (rounded where the kernels round), "u64" (the twin), "u64_half" (the twin with float16 level 1), "u64_fast" (... and the 16-bit field),
    "u32_half", "u32_fast" (the float32 restatement with the formats)."""
    from oracle import mg_np
    U0, F = plane(name, route, c)
    kw = dict(cycles=n, fused=fused)
    if kind.endswith("_half") or kind.endswith("_fast"):
        kw.update(level1_half=True, field_q16=kind.endswith("_fast"))
    if kind.startswith("u64"):
        kw.update(dtype=np.float64)
    elif kind.startswith("u32"):
        kw.update(residual_f32=True, direct_f32=True)
    u = mg_np.solve(U0, F, **kw)
    u.setflags(write=False)
    return u


def yardstick(name, route, c, n, fused=True):
    """D(u32) of the plane at budget n"""
    return interior_max(solve(name, route, c, n, "u32", fused) - solve(name, route, c, n, "u64", fused))


def float_bound(name, route, c, n, fused=True):
    return STEP_FACTOR * yardstick(name, route, c, n, fused)


def e_fmt(name, c, n, fast):
    """E_fmt of a clone's plane: the twin with the formats against the twin without"""
    return interior_max(solve(name, "clone", c, n, "u64_fast" if fast else "u64_half") - solve(name, "clone", c, n, "u64"))


def format_bound(name, c, n, fast):
    return e_fmt(name, c, n, fast) + float_bound(name, "clone", c, n)


def distance(u, name, route, c, n, kind="u64", fused=True):
    """D of a device field (one plane, ring included) against the twin `kind`"""
    return interior_max(np.asarray(u, np.float64) - solve(name, route, c, n, kind, fused))


@functools.lru_cache(maxsize=None)
def table_correction(name, c, n, kind):
    """(the float-table correction of the twin's iterate n of a clone's plane, interior only -- what the default tables add to the output --,
    the allowance for the device's evaluation of it)"""
    from oracle import lowmode_np
    corr = lowmode_np.correction(solve(name, "clone", c, n, kind)[1:-1, 1:-1])
    corr.setflags(write=False)
    return corr, CORR_REL * max(1.0, float(np.abs(corr).max())) + CORR_ABS
