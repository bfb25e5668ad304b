"""CPU tests of the weighted solve: sc_hip_weighted_check's codes, the numpy restatement (tests/weighted_np.py) against the screened
one and against itself, and the entry points' presence in the library."""
from __future__ import annotations

import numpy as np
import pytest

from seamlesscloneoptimization_amd import capi

import direct_np
import weighted_bounds as wb
import weighted_np

G, L = capi.SC_POISSON_GUIDANCE, capi.SC_POISSON_LAPLACIAN
NEU, PX, PY = capi.SC_POISSON_NEUMANN, capi.SC_POISSON_PERIODIC_X, capi.SC_POISSON_PERIODIC_Y
HWC = dict(cols=33, rows=47, channels=3, col_stride=3, row_stride=99, channel_stride=1)


def test_entry_points_are_exported():
    lib = capi.load()
    for name in ("sc_hip_weighted_check", "sc_hip_weighted_device", "sc_hip_weighted"):
        assert name in capi.declared_symbols()
        assert hasattr(lib, name), name


def test_check_accepts_every_border_kind():
    for bits in (0, NEU, capi.SC_POISSON_FREE_LEFT | capi.SC_POISSON_FREE_TOP, PX, PX | PY, PY | capi.SC_POISSON_FREE_LEFT):
        for base in (G, L):
            assert capi.weighted_check(base | bits, **HWC) == capi.SC_OK, (base, bits)
    assert capi.weighted_check(L | NEU, tol=1e-6, max_iters=50, precond_lambda=0.5, **HWC) == capi.SC_OK
    assert capi.weighted_check(L | NEU, tol=-1.0, max_iters=-3, precond_lambda=-2.0, **HWC) == capi.SC_OK      # <= 0: the defaults


def test_check_codes():
    bad_arg, bad_size = capi.SC_ERR_BAD_ARG, capi.SC_ERR_BAD_SIZE
    # kinds, as the screened call's
    assert capi.weighted_check(0, **HWC) == bad_arg
    assert capi.weighted_check(NEU, **HWC) == bad_arg
    assert capi.weighted_check(L | NEU | PX, **HWC) == bad_arg
    assert capi.weighted_check(L | PX | capi.SC_POISSON_FREE_LEFT, **HWC) == bad_arg
    assert capi.weighted_check(L | PY | capi.SC_POISSON_FREE_BOTTOM, **HWC) == bad_arg
    for kind in (G, L | NEU, L | PX):
        assert capi.screened_check(kind, 1.0, **HWC) == capi.weighted_check(kind, **HWC)
    # parameters
    assert capi.weighted_check(L | NEU, tol=float("nan"), **HWC) == bad_arg
    assert capi.weighted_check(L | NEU, tol=float("inf"), **HWC) == bad_arg
    assert capi.weighted_check(L | NEU, precond_lambda=float("nan"), **HWC) == bad_arg
    assert capi.weighted_check(L | NEU, precond_lambda=float("inf"), **HWC) == bad_arg
    # sizes: the direct solves' limits
    big = lambda cols, rows: dict(cols=cols, rows=rows, channels=1, col_stride=1, row_stride=cols, channel_stride=cols * rows)
    assert capi.weighted_check(L | NEU, **big(8192, 2)) == capi.SC_OK
    assert capi.weighted_check(L | NEU, **big(8193, 2)) == bad_size
    assert capi.weighted_check(L, **big(8194, 3)) == capi.SC_OK
    assert capi.weighted_check(L, **big(8195, 3)) == bad_size
    assert capi.weighted_check(L, **big(2, 7)) == bad_size
    assert capi.weighted_check(L | NEU, **big(1, 7)) == bad_size
    assert capi.weighted_check(L | PX, **big(8193, 3)) == bad_size
    # layouts
    assert capi.weighted_check(L | NEU, cols=33, rows=47, channels=5, col_stride=5, row_stride=165, channel_stride=1) == bad_arg
    assert capi.weighted_check(L | NEU, cols=33, rows=47, channels=3, col_stride=3, row_stride=98, channel_stride=1) == bad_arg      # rows overlap
    assert capi.weighted_check(L | NEU, cols=33, rows=47, channels=3, col_stride=2, row_stride=99, channel_stride=1) == bad_arg      # channels overlap columns
    assert capi.weighted_check(L | NEU, cols=33, rows=47, channels=3, col_stride=0, row_stride=99, channel_stride=1) == bad_arg


@pytest.mark.parametrize("border", [b[0] for b in wb.BORDERS])
def test_constant_weight_is_the_screened_solve(border):
    _, sides, periodic = next(b for b in wb.BORDERS if b[0] == border)
    H, W = 19, 13
    data, _, lap, boundary = wb.make_input(H, W, 2, "constant")
    lam = np.float32(0.3)
    weight = np.full((H, W, 2), lam, np.float32)
    b = boundary if weighted_np.has_dirichlet(sides, periodic) else None
    got = weighted_np.solve_exact(sides, periodic, weight, data, lap, b)
    want = direct_np.solve_exact(sides, periodic, lam, data, lap, b)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    assert np.array_equal(weighted_np.rhs(sides, periodic, weight, data, lap), direct_np.rhs(sides, periodic, lam, data, lap))


@pytest.mark.parametrize("border", [b[0] for b in wb.BORDERS])
def test_exact_solve_leaves_no_residual(border):
    """one of each axis kind among the five borders: free-free, Dirichlet-Dirichlet, free-Dirichlet, periodic"""
    _, sides, periodic = next(b for b in wb.BORDERS if b[0] == border)
    H, W = 21, 16
    data, weight, lap, boundary = wb.make_input(H, W, 2, "sparse", seed=2)
    assert (weight.reshape(-1, 2).sum(0) > 0).all()
    b = boundary if weighted_np.has_dirichlet(sides, periodic) else None
    u = weighted_np.solve_exact(sides, periodic, weight, data, lap, b)
    f = np.abs(weighted_np.rhs(sides, periodic, weight, data, lap)).max()
    assert np.abs(weighted_np.residual(sides, periodic, weight, u, data, lap)).max() <= 1e-12 * f
    if b is not None:
        m = direct_np.dirichlet_mask(sides, periodic, H, W)
        assert np.array_equal(u[m], boundary[m].astype(np.float64))


@pytest.mark.parametrize("wkind", wb.WEIGHTS)
@pytest.mark.parametrize("border", ["neumann", "free_lt", "periodic_xy"])
def test_reference_iteration_converges(border, wkind):
    """pcg_f32 reaches 1e-5 within 20 iterations at 33 x 47 on the weights the GPU tests use; a constant weight needs one at most"""
    _, sides, periodic = next(b for b in wb.BORDERS if b[0] == border)
    H, W = 47, 33
    data, weight, lap, boundary = wb.make_input(H, W, 3, wkind)
    b = boundary if weighted_np.has_dirichlet(sides, periodic) else None
    u, iters, rel = weighted_np.pcg_f32(sides, periodic, weight, data, lap, b, tol=1e-5)
    assert rel <= 1e-5 and iters <= (1 if wkind == "constant" else 20), (iters, rel)
    want = weighted_np.solve_exact(sides, periodic, weight, data, lap, b)
    assert np.abs(u - want).max() <= 1e-4 * np.abs(want).max()


def test_numpy_side_refuses_what_the_library_refuses():
    data = np.zeros((5, 6, 3), np.float32)
    with pytest.raises(ValueError):
        capi.weighted_arrays(data, np.zeros((5, 7), np.float32), neumann=True)
    with pytest.raises(ValueError):
        capi.weighted_arrays(data, np.zeros((5, 6, 3), np.float32), neumann=False)          # a Dirichlet line needs boundary
    kind, d, w, gx, gy, lap, b, out = capi.weighted_arrays(data, np.ones((5, 6), np.float32), neumann=True)
    assert w.shape == data.shape and lap is not None and not lap.any() and kind == (L | NEU)
