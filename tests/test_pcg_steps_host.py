"""The test side of the steps yardstick (tests/pcg_steps_bounds.py), on the CPU:

1. the reference iteration with its vectors' dtype as a parameter (pcg_np.pcg) is, at float32, the iteration it was: every family's
   pcg_f32 returns the bytes it returns with the earlier function in pcg_np's place.
2. the float64 twin is the same iteration: run on, it reaches the exact solve far below float32's floor, and its first iterates are
   pcg_f32's to float32's rounding.
3. the exact solves' sparse form (above DENSE_LIMIT unknowns) gives the dense form's answer.
4. the sharpness condition of the committed bound: pcg_f32 with lambda-bar, s-bar or tau-bar off by 1 % misses it by a factor of 10
   at least, at every shape up to 521 x 521.
5. region_np.unpinned_components by labelled components (what makes the inputs of 1025 x 1025 affordable) finds what label propagation
   finds, wraps included."""
from __future__ import annotations

import numpy as np
import pytest

import pcg_np
import pcg_steps_bounds as sb
import region_bounds as rb
import region_np
import volume_bounds as vb
import volume_np
import volume_wls_bounds as vwb
import volume_wls_np as vw
import weighted_bounds as wb
import weighted_np
import wls_bounds as lb
import wls_np


def pcg_f32_before(b, apply, precond, u0_scale, tol, max_iters, out, blk):
    """pcg_np.pcg_f32 as it stood before the dtype became a parameter, statement for statement"""
    dot = lambda a, c: np.einsum("yxc,yxc->c", a.astype(np.float64), c.astype(np.float64))
    bb = dot(b, b)
    rel = lambda r: float(np.sqrt(np.max(np.where(bb > 0, dot(r, r) / np.where(bb > 0, bb, 1.0), 0.0))))
    u = precond(b) if u0_scale is None else precond(b) * u0_scale
    r = b - apply(u)
    assert r.dtype == np.float32
    z = precond(r)
    p = z.copy()
    rho = dot(r, z)
    it = 0
    while rel(r) > tol and it < max_iters:
        q = apply(p)
        pq = dot(p, q)
        alpha = np.where(pq != 0, rho / np.where(pq != 0, pq, 1.0), 0.0).astype(np.float32)
        u = u + alpha * p
        r = r - alpha * q
        z = precond(r)
        rho_new = dot(r, z)
        beta = np.where(rho != 0, rho_new / np.where(rho != 0, rho, 1.0), 0.0).astype(np.float32)
        p = z + beta * p
        rho = rho_new
        it += 1
        assert u.dtype == np.float32 and p.dtype == np.float32
    out[blk] = u
    return out, it, rel(r)


def _family_runs():
    """per family one input under free left + top (a Dirichlet line on either axis): name -> a call of its pcg_f32"""
    H, W = 23, 17
    d, w, lap, b = wb.make_input(H, W, 3, "sparse")
    d2, w2, sx, sy, lap2, b2 = lb.make_input(H, W, 3, "sparse", "loguniform")
    pr = rb.make_input("free_lt", H, W, 3, "scatter", "sparse", "loguniform")
    pv = vb.make_input("free_lt", 9, 7, 2, 3, 1.0, "scatter", "sparse")
    runs = {"weighted": lambda: weighted_np.pcg_f32("lt", "", w, d, lap, b),
            "wls": lambda: wls_np.pcg_f32("lt", "", w2, sx, sy, d2, lap2, b2),
            "region": lambda: region_np.pcg_f32(*rb.np_args(pr), pr["boundary"]),
            "volume": lambda: volume_np.pcg_f32(*vb.np_args(pv), pv["boundary"])}
    for time in vwb.TIMES:
        pw = vwb.make_input("free_lt", 9, 7, 2, 3, 1.0, "scatter", "sparse", "xyt", time)
        runs["volume_wls_" + time] = lambda pw=pw: vw.pcg_f32(vwb.np_args(pw), pw["boundary"])
    return runs


@pytest.mark.parametrize("family", sb.FAMILIES)
def test_pcg_f32_returns_the_bytes_it_returned(family, monkeypatch):
    run = _family_runs()[family]
    u, it, rel = run()
    monkeypatch.setattr(pcg_np, "pcg", lambda *a: pcg_f32_before(*a[:8]))          # (dtype and keep: float32, no list)
    u0, it0, rel0 = run()
    assert it > 3 and u.dtype == np.float32
    assert (it, rel) == (it0, rel0) and u.tobytes() == u0.tobytes()


@pytest.mark.parametrize("family", sb.FAMILIES)
def test_the_float64_twin_is_the_same_iteration(family):
    """long_time / three_groups under free left + top: 200 float64 iterations at tol 1e-13 land on the exact solve to 1e-9 (float32 stops
    near 1e-5), the first three iterates differ from pcg_f32's by a few float32 roundings, and `keep` holds what a call with that
    budget returns"""
    shape = "long_time" if family in sb.VOLUME_FAMILIES else "three_groups"
    c = sb.case(family, shape, "free_lt")
    m = c.solved()
    want = np.asarray(c.yardstick().want).reshape(m.shape)
    run = c.iterates(200, np.float64, tol=1e-13)
    assert len(run) < 200 and run[-1].dtype == np.float64
    assert float(np.abs(run[-1].reshape(m.shape) - want)[m].max()) <= 1e-9 * float(np.abs(want[m]).max())
    ref, ran = sb.steps(family, shape, "free_lt")
    assert ran > max(sb.STEPS) + sb.POLL
    for k in sb.STEPS:
        assert np.array_equal(ref[k][0], run[k - 1]) and np.array_equal(ref[k][0], c.iterates(k, np.float64)[-1])
        assert 0 < ref[k][1] <= 2e-6, (k, ref[k][1])


@pytest.mark.parametrize("border", list(sb.BORDERS))
def test_sparse_and_dense_exact_solves_agree(border):
    sides, periodic = sb.BORDERS[border]
    H, W = 47, 33
    close = lambda a, b: float(np.abs(a - b).max()) <= 1e-10 * float(np.abs(b).max())
    d, w, lap, b = wb.make_input(H, W, 3, "sparse")
    assert close(weighted_np.solve_exact(sides, periodic, w, d, lap, b, dense=False), weighted_np.solve_exact(sides, periodic, w, d, lap, b, dense=True))
    d, w, sx, sy, lap, b = lb.make_input(H, W, 3, "sparse", "loguniform")
    assert close(wls_np.solve_exact(sides, periodic, w, sx, sy, d, lap, b, dense=False), wls_np.solve_exact(sides, periodic, w, sx, sy, d, lap, b, dense=True))
    p = rb.make_input(border, H, W, 3, "scatter", "sparse", "loguniform")
    assert close(region_np.solve_exact(*rb.np_args(p), p["boundary"], dense=False), region_np.solve_exact(*rb.np_args(p), p["boundary"], dense=True))
    assert H * W <= weighted_np.DENSE_LIMIT == wls_np.DENSE_LIMIT, "the families' own tests keep their dense solves"


SHARP = [c for c in sb.cases() if np.prod(sb.SHAPES[c[1]]) <= sb.SHARP_LIMIT]


@pytest.mark.parametrize("family,shape,border", SHARP, ids=[" ".join(c) for c in SHARP])
def test_a_preconditioner_off_by_one_percent_misses_the_bound(family, shape, border):
    """each of the preconditioner's constants the family has, times 1.01, in pcg_f32: D of every step at least 10 x the bound the GPU
    test holds the library to"""
    c = sb.case(family, shape, border)
    ref, _ = sb.steps(family, shape, border)
    for i, (name, mean) in enumerate(zip(("lambda-bar", "s-bar", "tau-bar"), c.means())):
        if mean is None:
            continue
        off = tuple(1.01 if j == i else 1.0 for j in range(3))
        for k, u in zip(sb.STEPS, c.iterates(max(sb.STEPS), np.float32, off=off)):
            d, bound = c.distance(u, ref[k][0]), max(sb.STEP_FACTOR * ref[k][1], sb.STEP_FLOOR)
            assert d >= 10.0 * bound, (name, k, d, bound)


def _unpinned_by_propagation(sides, periodic, state, weight):
    """region_np.unpinned_components as label propagation: every UNKNOWN pixel takes the smallest label among itself and its UNKNOWN
    neighbours until nothing changes; a component is pinned by a KNOWN or Dirichlet neighbour or a positive weight"""
    k = region_np.kinds(sides, periodic, state)
    unk = k == region_np.UNKNOWN
    big = k.size
    label = np.where(unk, np.arange(k.size).reshape(k.shape), big)
    while True:
        new = label
        for shift, axis in region_np._SHIFTS:
            new = np.minimum(new, region_np._neighbour(label, shift, axis, periodic, big))
        new = np.where(unk, new, big)
        if np.array_equal(new, label):
            break
        label = new
    held = np.zeros(k.shape, bool)
    for shift, axis in region_np._SHIFTS:
        q = region_np._neighbour(k, shift, axis, periodic, region_np.OUTSIDE)
        held |= (q == region_np.KNOWN) | (q == region_np.DIRICHLET)
    if weight is not None:
        held |= np.where(unk, weight, np.float32(0)) > 0
    return unk & ~np.isin(label, np.unique(label[unk & held]))


@pytest.mark.parametrize("border", list(sb.BORDERS))
def test_unpinned_components_by_labels_and_by_propagation(border):
    sides, periodic = sb.BORDERS[border]
    rng = np.random.default_rng(7)
    found = 0
    for H, W in ((9, 13), (5, 16), (12, 4)):
        for density in (0.05, 0.3, 0.6):
            # UNKNOWN islands in OUTSIDE water, few KNOWN pixels, a weight on a few: many components, some of them loose, some across a wrap
            st = np.where(rng.random((H, W, 2)) < density, 2.0, 0.0).astype(np.float32)
            st[rng.random((H, W, 2)) < 0.03] = 1.0
            w = (rng.random((H, W, 2)) < 0.03).astype(np.float32)
            for weight in (None, w):
                got = region_np.unpinned_components(sides, periodic, st, weight)
                assert np.array_equal(got, _unpinned_by_propagation(sides, periodic, st, weight)), (H, W, density)
                found += int(got.any())
    assert found >= 6, "the inputs must have loose components"
