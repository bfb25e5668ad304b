"""The two quantities the Neumann GPU tests hold the solver to, and their bounds (shared by tests/test_gpu_neumann.py,
tests/test_gpu_neumann_lengths.py and tests/test_neumann_lengths_host.py).

    RES  max |A u - (lap - mean lap)| / max |lap - mean lap|      A: the reflecting operator, in float64 (neumann_np.residual)
    ERR  max |u - solve_exact| / R,  R = max |solve_exact|

RES is not amplified by 1 / lambda_min: the float32 restatement (neumann_np.solve_f32) stays within 2.5e-8 .. 5.5e-7 from 2 x 2 to
8192 x 64 where its ERR varies a thousandfold, so a wrong coefficient at any but the lowest few k shows in it at full size.

Float32 transforms:  measured <= max(FACTOR x the same quantity for solve_f32 on the same input, FLOOR).  The four constants come
from one MI355X run of tests/test_gpu_neumann_lengths.py (DESIGN.md section 4 holds the table, profiles/neumann_lengths.txt the
record): each factor is the worst ratio to the restatement over the inputs with more than 3 pixels along the walked side, times 2,
rounded up to one digit; each floor twice the worst absolute value at 2 or 3 pixels, where the restatement is unusually exact.
Double transforms (SC_FLAG_FFT_FP64):  ERR within F64_ULPS float32 ulps of max |want| (the result is stored in float32: half an ulp,
and the mean's addition another); RES <= 1e-6 on rough inputs only (five terms of size <= R rounded to 6e-8 each, against max |lap|
>~ R on a rough input; a smooth input's max |lap| ~ R lambda is as small as one likes)."""
import numpy as np

import neumann_np

RES_FACTOR, RES_FLOOR = 8.0, 1.5e-6           # measured: worst ratio 3.6 (8192 x 64), worst value at 2 or 3 pixels 7.1e-7
ERR_FACTOR, ERR_FLOOR = 60.0, 1.3e-6          # measured: worst ratio 29.8 (2048 x 9, random guidance), worst value at 2 or 3 pixels 6.2e-7
F64_ULPS, F64_RES = 4, 1e-6


def err_and_res(u, lap, want):
    """(ERR, RES) of u for the right-hand side lap against want = solve_exact(lap, mean)"""
    lap64 = np.asarray(lap, np.float64)
    rhs = float(np.abs(lap64 - lap64.mean(axis=(0, 1), keepdims=True)).max())
    return (float(np.abs(np.asarray(u, np.float64) - want).max()) / float(np.abs(want).max()),
            float(np.abs(neumann_np.residual(u, lap)).max()) / rhs)


class Yardstick:
    """One input's references: want = solve_exact, and the float32 restatement's (ERR, RES) on it."""

    def __init__(self, lap, mean=None):
        self.lap = lap
        self.want = neumann_np.solve_exact(lap, mean)
        self.R = float(np.abs(self.want).max())
        self.err32, self.res32 = err_and_res(neumann_np.solve_f32(lap, mean), lap, self.want)

    def check(self, out, fp64, rough=True):
        """[(quantity, measured, bound)] that fail, and the measured (ERR, RES).  rough: RES is asserted as well -- float32: every
        input but the smooth ones; double: the white-noise reconstruction only (the solution of a random guidance field is a random
        walk, R ~ 10 max |lap| along a strip of 4096: the float32 rounding of the stored result alone leaves RES 1.9e-6 there)."""
        err, res = err_and_res(out, self.lap, self.want)
        if fp64:
            ulps = err * self.R / float(np.spacing(np.float32(self.R)))
            bad = [("ERR ulps", ulps, F64_ULPS)] if not ulps <= F64_ULPS else []
            if rough and not res <= F64_RES:
                bad.append(("RES", res, F64_RES))
        else:
            eb, rb = max(ERR_FACTOR * self.err32, ERR_FLOOR), max(RES_FACTOR * self.res32, RES_FLOOR)
            bad = ([("ERR", err, eb)] if not err <= eb else []) + ([("RES", res, rb)] if rough and not res <= rb else [])
        return bad, err, res
