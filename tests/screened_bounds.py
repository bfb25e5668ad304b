"""The two quantities the screened GPU tests hold the Neumann float32 solve to, and their bounds (tests/test_gpu_screened.py), after
the pattern of tests/neumann_bounds.py, for the screened operator A - lam:

    RES  max |(A - lam) u - rhs| / max |rhs|        rhs = lap - lam d in the library's float32 order, the rest in float64
    ERR  max |u - solve_exact| / R,  R = max |solve_exact|

Float32 transforms:  measured <= max(FACTOR x the same quantity for screened_np.solve_f32 on the same input, FLOOR).  The four
constants come from one MI355X run of tools/screened_probe.py --lengths over the length walk (DESIGN.md section 4 holds the table,
profiles/screened_lengths.txt the record): each factor is the worst ratio to the restatement over the inputs with more than 3 pixels
along the walked side, times 2, rounded up to one digit; each floor twice the worst absolute value at 2 or 3 pixels, where the
restatement is unusually exact.
Double transforms (SC_FLAG_FFT_FP64):  ERR within F64_ULPS float32 ulps of max |want| (the result is stored in float32)."""
import numpy as np

import screened_np

RES_FACTOR, RES_FLOOR = 7.0, 3.3e-6           # measured: worst ratio 3.19 (6 x 9, lam 1e-3), worst value at 2 or 3 pixels 1.62e-6 (3 x 7, lam 0.1)
ERR_FACTOR, ERR_FLOOR = 40.0, 1.8e-5          # measured: worst ratio 16.5 (33 x 7, lam 1e-3), worst value at 2 or 3 pixels 8.8e-6 (2 x 7, lam 1e-3)
F64_ULPS = 4


def err_and_res(kind, lam, u, data, lap, want):
    """(ERR, RES) of u against want = solve_exact of the same input"""
    f = np.abs(screened_np.rhs(kind, lam, data, lap).astype(np.float64)).max()
    return (float(np.abs(np.asarray(u, np.float64) - want).max()) / float(np.abs(want).max()),
            float(np.abs(screened_np.residual(kind, lam, u, data, lap)).max()) / float(f))


class Yardstick:
    """One Neumann input's references: want = solve_exact, and the float32 restatement's (ERR, RES) on it."""

    def __init__(self, lam, data, lap):
        self.kind, self.lam, self.data, self.lap = screened_np.NEUMANN, lam, data, lap
        self.want = screened_np.solve_exact(self.kind, lam, data, lap)
        self.R = float(np.abs(self.want).max())
        self.err32, self.res32 = err_and_res(self.kind, lam, screened_np.solve_f32(self.kind, lam, data, lap), data, lap, self.want)

    def measure(self, out):
        return err_and_res(self.kind, self.lam, out, self.data, self.lap, self.want)

    def check(self, out, fp64):
        """[(quantity, measured, bound)] that fail, and the measured (ERR, RES)"""
        err, res = self.measure(out)
        if fp64:
            ulps = err * self.R / float(np.spacing(np.float32(self.R)))
            bad = [("ERR ulps", ulps, F64_ULPS)] if not ulps <= F64_ULPS else []
        else:
            eb, rb = max(ERR_FACTOR * self.err32, ERR_FLOOR), max(RES_FACTOR * self.res32, RES_FLOOR)
            bad = ([("ERR", err, eb)] if not err <= eb else []) + ([("RES", res, rb)] if not res <= rb else [])
        return bad, err, res
