"""CPU tests of the region solve's host side: sc_hip_region_check's codes, the numpy restatement (tests/region_np.py) against wls_np and
against its own dense solve on every input of the GPU tests, the fairness of those inputs (no UNKNOWN component that nothing pins), and
the Python wrappers' argument handling -- nothing here touches a GPU."""
from __future__ import annotations

import numpy as np
import pytest

from seamlesscloneoptimization_amd import capi, seamless_clone

import region_bounds as rb
import region_np
import wls_bounds as lb
import wls_np

G, L, N = capi.SC_POISSON_GUIDANCE, capi.SC_POISSON_LAPLACIAN, capi.SC_POISSON_NEUMANN
BORDERS = {b[0]: b[1:] for b in rb.BORDERS}


def test_region_check_codes():
    ok = dict(cols=640, rows=480, channels=3, col_stride=3, row_stride=1920, channel_stride=1)
    assert capi.region_check(G, **ok) == capi.SC_OK
    assert capi.region_check(L | N, 1e-6, 50, 0.5, 2.0, **ok) == capi.SC_OK
    assert capi.region_check(L | capi.SC_POISSON_PERIODIC_X | capi.SC_POISSON_PERIODIC_Y, cols=2, rows=2, channels=4, col_stride=4,
                             row_stride=8, channel_stride=1) == capi.SC_OK
    for bad in (dict(tol=float("nan")), dict(tol=float("inf")), dict(precond_lambda=float("nan")), dict(precond_smooth=float("-inf"))):
        assert capi.region_check(L | N, **bad, **ok) == capi.SC_ERR_BAD_ARG, bad
    assert capi.region_check(0, **ok) == capi.SC_ERR_BAD_ARG
    assert capi.region_check(L | N | capi.SC_POISSON_PERIODIC_X, **ok) == capi.SC_ERR_BAD_ARG
    assert capi.region_check(L | capi.SC_ROBUST_ISOTROPIC, **ok) == capi.SC_ERR_BAD_ARG          # the robust call's bits are its own
    assert capi.region_check(L, cols=2, rows=7, channels=1, col_stride=1, row_stride=2, channel_stride=14) == capi.SC_ERR_BAD_SIZE
    assert capi.region_check(L, cols=8194, rows=3, channels=1, col_stride=1, row_stride=8194, channel_stride=24582) == capi.SC_OK
    assert capi.region_check(L, cols=8195, rows=3, channels=1, col_stride=1, row_stride=8195, channel_stride=24585) == capi.SC_ERR_BAD_SIZE
    assert capi.region_check(L | N, **dict(ok, row_stride=1919)) == capi.SC_ERR_BAD_ARG
    assert capi.region_check(L | N, **dict(ok, channels=5)) == capi.SC_ERR_BAD_ARG
    lib = capi.load()
    assert lib.sc_hip_region_check(None, None) == capi.SC_ERR_BAD_ARG
    # the same verdicts as the WLS call's, whatever they are
    for kind in (G, L, L | N, G | capi.SC_POISSON_FREE_LEFT, L | capi.SC_POISSON_PERIODIC_Y):
        for cols, rows in ((2, 2), (3, 3), (2, 9), (8193, 2), (300, 9)):
            lay = dict(cols=cols, rows=rows, channels=1, col_stride=1, row_stride=cols, channel_stride=cols * rows)
            assert capi.region_check(kind, **lay) == capi.wls_check(kind, **lay), (kind, cols, rows)


@pytest.mark.parametrize("border", list(BORDERS))
def test_every_state_unknown_is_the_wls_restatement(border):
    sides, periodic = BORDERS[border]
    H, W = 12, 9
    data, weight, sx, sy, lap, boundary = lb.make_input(H, W, 2, "sparse", "loguniform")
    st = np.zeros((H, W, 2), np.float32)
    b = boundary if wls_np.has_dirichlet(sides, periodic) else None
    lx, ly = wls_np.live_links(sides, periodic, H, W)
    rx, ry = region_np.live_links(sides, periodic, st)
    assert np.array_equal(rx, np.broadcast_to(lx[:, :, None], rx.shape)) and np.array_equal(ry, np.broadcast_to(ly[:, :, None], ry.shape))
    for dt in (np.float32, np.float64):
        assert wls_np.folded_rhs(sides, periodic, weight, sx, sy, data, lap, b, dt).tobytes() == \
            region_np.folded_rhs(sides, periodic, st, weight, sx, sy, data, lap, b, dt).tobytes()
    rng = np.random.default_rng(3)
    gx, gy = (0.1 * rng.standard_normal((2, H, W, 2))).astype(np.float32)
    blk = wls_np.unknowns(sides, periodic, H, W)
    assert wls_np.divergence(sides, periodic, sx, sy, gx, gy)[blk].tobytes() == region_np.divergence(sides, periodic, st, sx, sy, gx, gy)[blk].tobytes()
    u1, i1, r1 = wls_np.pcg_f32(sides, periodic, weight, sx, sy, data, lap, b)
    u2, i2, r2 = region_np.pcg_f32(sides, periodic, st, weight, sx, sy, data, lap, b)
    if b is None:          # (wls_np leaves 0 where there is no Dirichlet line; the region's out holds data where it is not UNKNOWN: nowhere here)
        assert u1.tobytes() == u2.tobytes()
    else:
        assert u1[blk].tobytes() == u2[blk].tobytes()
    assert (i1, r1) == (i2, r2)
    e1 = wls_np.solve_exact(sides, periodic, weight, sx, sy, data, lap, b)
    e2 = region_np.solve_exact(sides, periodic, st, weight, sx, sy, data, lap, b)
    assert np.abs(e1[blk] - e2[blk]).max() <= 1e-12 * np.abs(e1).max()


_CASES = rb.matrix()
_IDS = [f"{b}-{W}x{H}x{C}-{p}-{wk}-{sk}-{f}" for b, H, W, C, p, wk, sk, f in _CASES]


@pytest.mark.parametrize("case", _CASES, ids=_IDS)
def test_inputs_are_fair_and_the_reference_iteration_meets_the_exact_solve(case):
    """every generated input: no UNKNOWN component that nothing pins (with NaN in every unread element: the restatement reads none of
    them), every channel has an UNKNOWN pixel, and pcg_f32 converges well inside the budget to the dense solve.  1e-3: a hundred times
    the stop rule's 1e-5, for the conditioning of the small masked systems (the sharp bounds are the GPU tests')."""
    border, H, W, C, pattern, wk, sk, form = case
    p = rb.nan_unread(rb.make_input(border, H, W, C, pattern, wk, sk))
    k = region_np.kinds(p["sides"], p["periodic"], p["state"])
    assert (k == region_np.UNKNOWN).reshape(-1, C).any(0).all()
    assert not region_np.unpinned_components(p["sides"], p["periodic"], p["state"], p["weight"]).any()
    kind = capi.border_bits(p["sides"], False, p["periodic"]) | L
    assert not capi.region_unpinned(kind, np.where(np.isnan(p["state"]), 0, p["state"]), p["weight"]).any(), "the wrapper's flood fill agrees"
    y = rb.Yardstick(p, form)
    assert np.isfinite(y.want).all()
    assert y.rel32 <= 1e-5 and y.iters32 <= rb.MAX_ITERS // 2, (y.rel32, y.iters32)
    assert y.err32 <= 1e-3 and y.res32 <= 1e-3, (y.err32, y.res32)


def test_unpinned_components_finds_an_island():
    st = np.ones((9, 11, 1), np.float32)
    st[1:4, 1:4] = 0                      # held by the KNOWN pixels around it
    st[5:8, 6:10] = 0                     # an island inside a ring of OUTSIDE pixels
    st[4, 5:11] = st[8, 5:11] = st[4:9, 5] = st[4:9, 10] = 2
    loose = region_np.unpinned_components("lrtb", "", st)
    assert loose[5:8, 6:10].all() and loose.sum() == 12
    w = np.zeros((9, 11, 1), np.float32)
    w[6, 7] = 0.5
    assert not region_np.unpinned_components("lrtb", "", st, w).any()
    assert np.array_equal(capi.region_unpinned(L | N, st), loose)
    # across a periodic seam the component reaches a Dirichlet-free KNOWN pixel
    st = np.zeros((4, 6, 1), np.float32)
    st[:, 2] = 2
    st[:, 4] = 2
    st[1, 5] = 1
    assert region_np.unpinned_components("lrtb", "", st)[:, :2].all()
    assert not region_np.unpinned_components("tb", "x", st)[:, :2].any()


def test_python_argument_handling():
    H, W = 6, 7
    data = np.arange(H * W * 3, dtype=np.float32).reshape(H, W, 3)
    mask = np.zeros((H, W), bool)
    mask[2, 3] = True
    kind, d, st, w, sx, sy, gx, gy, lap, b, out = capi.region_arrays(data, mask, neumann=True)
    assert st.dtype == np.float32 and st.shape == data.shape and st[2, 3].tolist() == [1.0] * 3 and st.sum() == 3
    assert w is None and sx is None and sy is None and b is None and gx is None and lap is not None and not lap.any()
    assert kind == L | N
    st8 = np.zeros((H, W, 3), np.uint8)
    st8[0, 0] = 2
    st8[1, 1] = 1
    assert capi.region_arrays(data, st8, neumann=True)[2][0, 0, 0] == 2.0
    with pytest.raises(ValueError):
        capi.region_arrays(data, np.full((H, W), 3, np.uint8), neumann=True)
    with pytest.raises(ValueError):
        capi.region_arrays(data, np.full((H, W), 0.5, np.float32), neumann=True)
    # state is not read on the Dirichlet lines: anything may stand there
    edge = np.zeros((H, W), np.float32)
    edge[0] = edge[-1] = edge[:, 0] = edge[:, -1] = np.nan
    capi.region_arrays(data, edge, boundary=data)
    with pytest.raises(ValueError):
        capi.region_arrays(data, edge, neumann=True)
    with pytest.raises(TypeError):
        capi.region_arrays(data, mask.astype(np.float64), neumann=True)
    with pytest.raises(ValueError):
        capi.region_arrays(data, mask[:, :-1], neumann=True)
    with pytest.raises(ValueError):
        capi.region_arrays(data, mask, smooth_x=np.ones((H, W), np.float32), neumann=True)
    with pytest.raises(ValueError):
        capi.region_arrays(data, mask)                      # a frame needs boundary
    with pytest.raises(ValueError):
        capi.region_arrays(data, mask, gx=data, neumann=True)
    w2 = np.ones((H, W), np.float32)
    assert capi.region_arrays(data, mask, weight=w2, smooth_x=w2, smooth_y=w2, neumann=True)[3].shape == data.shape
    with pytest.raises(ValueError):
        seamless_clone.region_solve_batch([data], [mask], smooth_xs=[w2])
    with pytest.raises(ValueError):
        seamless_clone.region_solve_batch([data, data], [mask])


def test_validate_raises_on_an_islanded_component():
    """validate=True: before any device is touched"""
    st = np.ones((9, 11), np.uint8)
    st[5:8, 6:10] = 0
    st[4, 5:11] = st[8, 5:11] = st[4:9, 5] = st[4:9, 10] = 2
    data = np.zeros((9, 11), np.float32)
    with pytest.raises(ValueError, match="nothing pins"):
        seamless_clone.region_solve(data, st, validate=True)
    with pytest.raises(ValueError, match="nothing pins"):
        seamless_clone.region_solve_batch([data], [st], validate=True)
    for fn, args in ((seamless_clone.inpaint, (data, np.ones((9, 11), bool))),
                     (seamless_clone.poisson_clone, (data, data, np.ones((9, 11), bool)))):
        with pytest.raises(ValueError):
            fn(*args)
    with pytest.raises(TypeError):
        seamless_clone.inpaint(data.astype(np.float64), st == 0)
    with pytest.raises(ValueError):
        seamless_clone.poisson_clone(data, data[:-1], st == 0)
