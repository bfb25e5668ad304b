"""GPU tests of the front end the float32 families share (sc_hip_poisson*, sc_hip_screened*, sc_hip_weighted*): host staging and job
intake, per family and border kind.

1. host-call aliases, through the raw C entry (capi's contiguous fallback cannot step in): 9 x 7 pixels of 2 channels under a frame, the
   Neumann border, a free left side and a periodic x axis.  Every alias the family allows -- out a fresh array, out is data, out is
   boundary, boundary is data, boundary is data with out is data -- gives the bytes of the call on separate arrays of the same values.
2. device intake: 5 jobs of 9 x 7 x 1, job 1 with a null lap, job 3 with lap two bytes off.  Both read SC_ERR_BAD_ARG and keep their
   sentinel, the call returns SC_ERR_BAD_ARG with the first reason, jobs 0, 2 and 4 read SC_OK and equal their solo solves: bit for bit
   for the direct solves; for the weighted family each side within tests/weighted_bounds.py's ERR bound of the exact solution (the
   batch member's under the chunk's mean weight, as test_gpu_weighted.py's batch test), so the two within the sum of both."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from seamlesscloneoptimization_amd import capi

import weighted_bounds as wb

pytestmark = pytest.mark.gpu

H, W = 9, 7
SENTINEL = -7.25
FAMILIES = ["poisson", "screened", "weighted"]
# (name, neumann, free_sides, periodic)
BORDERS = [("frame", False, "", ""), ("neumann", True, "", ""), ("free_l", False, "l", ""), ("periodic_x", False, "", "x")]


@pytest.fixture(scope="module")
def inst():
    i = capi.Instance(0)
    yield i
    i.destroy()


def configure(inst, method):
    d = inst.default_opts()
    inst.set_solver(**{k: getattr(d, k) for k, _ in capi.SolverOpts._fields_})
    inst.set_solver(method=method)


def params_of(family, kind):
    return {"poisson": capi.PoissonParams(kind, 0.0), "screened": capi.ScreenedParams(kind, 0.75),
            "weighted": capi.WeightedParams(kind, 0.0, 0, 0.0)}[family]


def host_call(inst, family, kind, gx, gy, data, weight, boundary, out):
    """the raw C entry on numpy arrays as they are: (code, out)"""
    ptr = lambda a: None if a is None else a.ctypes.data
    extra = {"poisson": [], "screened": [data], "weighted": [data, weight]}[family]
    fn = getattr(inst.L, "sc_hip_" + family)
    rc = fn(inst.h, C.byref(params_of(family, kind)), C.byref(capi.poisson_layout_of(out)), ptr(gx), ptr(gy), None,
            *[ptr(a) for a in extra], ptr(boundary), ptr(out))
    return rc, out


# ---- 1. host-call aliases -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("border", BORDERS, ids=[b[0] for b in BORDERS])
@pytest.mark.parametrize("family", FAMILIES)
def test_host_call_aliases(inst, family, border):
    _, neumann, sides, periodic = border
    kind = capi.SC_POISSON_GUIDANCE | capi.border_bits(sides, neumann, periodic)
    rng = np.random.default_rng(H * 100 + W + len(family))
    gx, gy, data, boundary = (rng.standard_normal((H, W, 2)).astype(np.float32) for _ in range(4))
    weight = (0.5 + rng.random((H, W, 2))).astype(np.float32)
    configure(inst, capi.SC_METHOD_AUTO)

    def run(data, boundary, out):
        rc, got = host_call(inst, family, kind, gx, gy, data, weight, boundary, out)
        assert rc == capi.SC_OK, (rc, inst.L.sc_hip_last_error(inst.h))
        return got

    fresh = lambda: np.full((H, W, 2), SENTINEL, np.float32)
    want = run(data.copy(), boundary.copy(), fresh())
    assert not (want == SENTINEL).any()
    b = boundary.copy()
    assert run(data.copy(), b, b).tobytes() == want.tobytes(), "out is boundary"
    if family == "poisson":
        return
    d = data.copy()
    assert run(d, boundary.copy(), d).tobytes() == want.tobytes(), "out is data"
    want_bd = run(data.copy(), data.copy(), fresh())           # the problem whose boundary has data's values, on separate arrays
    d = data.copy()
    assert run(d, d, fresh()).tobytes() == want_bd.tobytes(), "boundary is data"
    d = data.copy()
    assert run(d, d, d).tobytes() == want_bd.tobytes(), "boundary is data, out is data"


# ---- 2. device intake -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
def test_device_intake_bad_jobs(inst, family):
    n, kind = 5, capi.SC_POISSON_LAPLACIAN
    rng = np.random.default_rng(31 + len(family))
    probs = []
    for _ in range(n):
        data, boundary = (rng.standard_normal((H, W, 1)).astype(np.float32) for _ in range(2))
        lap = (0.1 * rng.standard_normal((H, W, 1))).astype(np.float32)
        probs.append((lap, data, (0.5 + rng.random((H, W, 1))).astype(np.float32), boundary))
    configure(inst, capi.SC_METHOD_FFT)       # the direct solve: a member's bits do not depend on its chunk
    lay = capi.poisson_layout_of(probs[0][0])
    jobs = getattr(capi.Instance, f"make_{family}_jobs")(n)
    dev = []
    try:
        for j, (lap, data, weight, boundary) in zip(jobs, probs):
            ptrs = [inst.to_device(a) for a in (lap, data, weight, boundary, np.full((H, W, 1), SENTINEL, np.float32))]
            dev += ptrs
            j.lap, j.boundary, j.out = ptrs[0], ptrs[3], ptrs[4]
            if family != "poisson":
                j.data = ptrs[1]
            if family == "weighted":
                j.weight = ptrs[2]
        jobs[1].lap = None
        jobs[3].lap = jobs[3].lap + 2           # not 4-byte aligned
        rc = getattr(inst, family + "_device")(params_of(family, kind), lay, jobs, allow_job_errors=True)
        why = (inst.L.sc_hip_last_error(inst.h) or b"").decode()
        outs = [inst.from_device(j.out, (H, W, 1), np.float32) for j in jobs]
    finally:
        for p in dev:
            inst.free(p)
    assert rc == capi.SC_ERR_BAD_ARG
    assert why == "null array pointer"
    assert [j.rc for j in jobs] == [capi.SC_OK, capi.SC_ERR_BAD_ARG, capi.SC_OK, capi.SC_ERR_BAD_ARG, capi.SC_OK]
    for k in (1, 3):
        assert (outs[k] == SENTINEL).all(), k
    # the chunk's preconditioner constant: the mean weight over the unknowns of the jobs that ran
    lam = np.float32(np.mean([probs[k][2][1:-1, 1:-1].astype(np.float64).mean() for k in (0, 2, 4)]))
    for k in (0, 2, 4):
        lap, data, weight, boundary = probs[k]
        if family == "poisson":
            solo = inst.poisson(boundary, lap=lap)
        elif family == "screened":
            solo = inst.screened(data, lap=lap, lam=0.75, boundary=boundary)
        else:
            solo = inst.weighted(data, weight, lap=lap, boundary=boundary)
        if family != "weighted":
            assert outs[k].tobytes() == solo.tobytes(), k
            continue
        in_batch, alone = wb.Yardstick("", "", weight, data, lap, boundary, precond_lambda=lam), wb.Yardstick("", "", weight, data, lap, boundary)
        eb = [max(wb.ERR_FACTOR * y.err32, wb.ERR_FLOOR) for y in (in_batch, alone)]
        err = [in_batch.measure(outs[k])[0], alone.measure(solo)[0]]
        apart = float(np.abs(outs[k].astype(np.float64) - solo).max()) / float(np.abs(alone.want).max())
        print(f"FRONT END weighted job {k}: ERR in the batch {err[0]:.3g} (bound {eb[0]:.3g}), alone {err[1]:.3g} (bound {eb[1]:.3g}), "
              f"apart {apart:.3g}")
        assert err[0] <= eb[0] and err[1] <= eb[1] and apart <= eb[0] + eb[1], (k, err, eb, apart)
