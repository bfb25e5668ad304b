"""CPU tests of the robust region solve's host side (sc_hip_region_robust*): the declarations, the ctypes struct, every verdict of
sc_hip_region_robust_check against sc_hip_robust_check and sc_hip_region_check, the wrappers' argument checks, the numpy restatement
(tests/region_robust_np.py) against robust_np / robust_coupled_np / region_np and against itself, the coverage of the GPU tests' inputs
(tests/region_robust_bounds.py) and the two behaviour problems in float64."""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

from seamlesscloneoptimization_amd import capi

import region_np
import region_robust_bounds as rb
import region_robust_np as rr
import robust_coupled_np as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G, L, N = capi.SC_POISSON_GUIDANCE, capi.SC_POISSON_LAPLACIAN, capi.SC_POISSON_NEUMANN
HWC = dict(cols=33, rows=47, channels=3, col_stride=3, row_stride=99, channel_stride=1)
BITS = (0, capi.SC_ROBUST_ISOTROPIC, capi.SC_ROBUST_JOINT_CHANNELS, capi.SC_ROBUST_ISOTROPIC | capi.SC_ROBUST_JOINT_CHANNELS)


def test_entry_points_are_declared_and_exported():
    lib = capi.load()
    for name in ("sc_hip_region_robust_check", "sc_hip_region_robust_device", "sc_hip_region_robust"):
        assert name in capi.declared_symbols(capi.HEADER_PATH)
        assert hasattr(lib, name), name
    import seamlesscloneoptimization_amd as pkg
    for name in ("region_robust_solve", "region_robust_solve_batch", "tv_inpaint", "integrate_gradients_masked"):
        assert name in pkg.__all__ and callable(getattr(pkg, name))
    for name in ("region_robust", "make_region_robust_jobs", "region_robust_device"):
        assert callable(getattr(capi.Instance, name))
    assert callable(capi.region_robust_check) and callable(capi.region_robust_arrays)


def test_job_struct_matches_the_header_layout(tmp_path):
    import ctypes
    cname, cls = "sc_region_robust_job", capi.RegionRobustJob
    lines = [f'printf("{cname} %zu\\n", sizeof({cname}));']
    for fname, _ in cls._fields_:
        lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "seamlessclone_hip.h"\nint main(void) {\n' + "\n".join(lines) +
                   "\nreturn 0; }\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out[cname]) == ctypes.sizeof(cls)
    for fname, _ in cls._fields_:
        assert int(out[f"{cname}.{fname}"]) == getattr(cls, fname).offset, fname
    # sc_region_job without lap, in its order
    assert [f for f, _ in cls._fields_] == [f for f, _ in capi.RegionJob._fields_ if f != "lap"]


def test_check_verdicts_are_the_robust_and_the_region_calls():
    bad_arg = capi.SC_ERR_BAD_ARG
    chk = capi.region_robust_check
    nan, inf = float("nan"), float("inf")
    assert chk(G | N, **HWC) == capi.SC_OK
    assert chk(G, 0.5, 1e-2, 1.0, 1e-3, 3, -1.0, 1e-6, 50, **HWC) == capi.SC_OK
    assert chk(G | N, p_grad=2.0, eps_grad=0.0, p_data=2.0, eps_data=nan, **HWC) == capi.SC_OK          # exponent 2: eps unused
    assert capi.load().sc_hip_region_robust_check(None, None) == bad_arg
    # the coupling bits are accepted and change no verdict
    for bits in BITS[1:]:
        assert chk(G | N | bits, **HWC) == capi.SC_OK
        assert chk(G | N, isotropic=bool(bits & capi.SC_ROBUST_ISOTROPIC), joint_channels=bool(bits & capi.SC_ROBUST_JOINT_CHANNELS), **HWC) == capi.SC_OK
    # every verdict against sc_hip_robust_check on the same inputs: exponents, eps, tol, round_tol, a Laplacian base, kinds, layouts
    params = [dict()]
    params += [{name: v} for name in ("p_grad", "p_data") for v in (0.0, -1.0, 2.5, nan, 2.0, 0.3)]
    params += [{p: 1.0, e: v} for p, e in (("p_grad", "eps_grad"), ("p_data", "eps_data")) for v in (0.0, -1.0, nan, inf, 1e-6)]
    params += [dict(tol=nan), dict(tol=inf), dict(tol=-1.0), dict(round_tol=nan), dict(round_tol=inf), dict(round_tol=-1.0), dict(max_rounds=-3),
               dict(max_iters=-1)]
    kinds = (G, G | N, L, L | N, 0, G | capi.SC_POISSON_FREE_LEFT | capi.SC_POISSON_FREE_TOP, G | capi.SC_POISSON_PERIODIC_X,
             G | capi.SC_POISSON_PERIODIC_X | capi.SC_POISSON_PERIODIC_Y, G | N | capi.SC_POISSON_PERIODIC_X,
             G | capi.SC_POISSON_PERIODIC_Y | capi.SC_POISSON_FREE_TOP)
    layouts = [HWC, dict(HWC, row_stride=98), dict(HWC, channels=5, col_stride=5, row_stride=165)]
    layouts += [dict(cols=c, rows=r, channels=1, col_stride=1, row_stride=c, channel_stride=c * r)
                for c, r in ((2, 2), (3, 3), (2, 7), (2, 9), (8194, 3), (8195, 3), (8193, 2), (8192, 2), (300, 9))]
    seen = set()
    for kind in kinds:
        for bits in BITS:
            for lay in layouts:
                for prm in (params if lay is HWC else params[:1]):
                    want = capi.robust_check(kind | bits, **prm, **lay)
                    assert chk(kind | bits, **prm, **lay) == want, (kind, bits, prm, lay)
                    seen.add(want)
                # on a guidance base with valid penalties: the region call's verdict for layout and kind
                if (kind & 3) == G:
                    assert chk(kind | bits, **lay) == capi.region_check(kind, **lay), (kind, lay)
    assert seen == {capi.SC_OK, bad_arg, capi.SC_ERR_BAD_SIZE}
    assert chk(L | N, **HWC) == bad_arg and chk(L, **HWC) == bad_arg


def test_region_robust_arrays_argument_handling():
    H, W = 6, 7
    data = np.arange(H * W * 3, dtype=np.float32).reshape(H, W, 3)
    mask = np.zeros((H, W), bool)
    g = np.ones_like(data)
    out = capi.region_robust_arrays(g, g, data, mask, neumann=True)
    assert len(out) == 10 and out[0] == G | N and out[4].shape == data.shape and out[4].dtype == np.float32 and out[5] is None
    out = capi.region_robust_arrays(g, g, data, mask, weight=g, smooth_x=g, smooth_y=g, neumann=True, isotropic=True, joint_channels=True)
    assert out[0] == G | N | capi.SC_ROBUST_ISOTROPIC | capi.SC_ROBUST_JOINT_CHANNELS and out[6] is not None
    for bad in (dict(gx=None), dict(gy=None), dict(p_grad=0.0), dict(p_grad=2.5), dict(p_data=float("nan")), dict(p_grad=1.0, eps_grad=0.0),
                dict(p_data=1.0, eps_data=-1.0), dict(smooth_x=g), dict(state=np.full((H, W), 3, np.uint8)), dict(neumann=False)):
        a = dict(gx=g, gy=g, data=data, state=mask, neumann=True)
        a.update(bad)
        with pytest.raises(ValueError):
            capi.region_robust_arrays(**a)
    with pytest.raises(TypeError):
        capi.region_robust_arrays(g, g, data, [[0]], neumann=True)


def test_wrappers_refuse_bad_arguments_before_any_device():
    import seamlesscloneoptimization_amd as pkg
    img = np.zeros((6, 7), np.float32)
    hole = np.zeros((6, 7), bool)
    with pytest.raises(TypeError):
        pkg.tv_inpaint(img.astype(np.float64), hole)
    with pytest.raises(ValueError):
        pkg.tv_inpaint(img, np.ones((6, 7), bool))
    with pytest.raises(ValueError):
        pkg.tv_inpaint(img, np.zeros((5, 7), bool))
    with pytest.raises(TypeError):
        pkg.integrate_gradients_masked(img.astype(np.float64), img, hole)
    with pytest.raises(ValueError):
        pkg.integrate_gradients_masked(img, img, hole)                                          # valid is empty
    with pytest.raises(ValueError):
        pkg.integrate_gradients_masked(img, img, ~hole, known=hole)                             # known without values
    with pytest.raises(ValueError):
        pkg.integrate_gradients_masked(img, img, ~hole, known=hole, values=img)                 # known is empty
    with pytest.raises(ValueError):
        pkg.integrate_gradients_masked(img, img, ~hole, anchor=0.0)
    with pytest.raises(ValueError):
        pkg.region_robust_solve_batch([img], [img], [img], [hole], smooth_xs=[img])


def test_matrix_covers_every_value_under_every_border_and_size():
    m = rb.matrix()
    # at most the 2-wide sizes under the frame border may drop
    assert rb.dropped() == [("frame", 7, 2)]
    assert len(m) == rb.REPEATS * (len(rb.BORDERS) * len(rb.SIZES) - len(rb.dropped()))
    axes = {3: rb.CHANNELS, 4: rb.PATTERNS, 5: rb.WEIGHTS, 6: rb.LINKS, 7: rb.COUPLINGS, 8: rb.EXPONENTS, 9: rb.EPS}
    for col, values in axes.items():
        for border, _, _ in rb.BORDERS:
            assert {c[col] for c in m if c[0] == border} == set(values), (col, border)
        for H, W in rb.SIZES:
            assert {c[col] for c in m if (c[1], c[2]) == (H, W)} == set(values), (col, H, W)
    assert set(rb.SIZES) == {(5, 260), (12, 19), (7, 2), (5, 16), (33, 47)} and set(rb.COUPLINGS) == {0, 1, 2, 3}
    assert set(rb.EXPONENTS) == {(1.0, 2.0), (1.0, 1.0), (1.5, 2.0), (0.8, 2.0)} and rb.EPS == [1e-2, 1e-3] and rb.ROUNDS == 4
    # every joint form meets three channels, and every input has an UNKNOWN pixel in every channel and no loose component
    assert {c[7] for c in m if c[3] == 3} == {0, 1, 2, 3}
    for c in m:
        p = rb.make_input(*c[:7])
        k = region_np.kinds(p["sides"], p["periodic"], p["state"])
        assert (k == region_np.UNKNOWN).reshape(-1, c[3]).any(0).all(), c
        assert not region_np.unpinned_components(p["sides"], p["periodic"], p["state"], p["weight"]).any(), c
        if c[4] == "zero":
            assert (p["state"] == 0).all() or (c[5] is None and (p["state"] != 0).sum() == c[3]), c


@pytest.mark.parametrize("coupling", rr.COUPLINGS)
@pytest.mark.parametrize("links", [None, "loguniform"])
def test_every_state_zero_is_the_robust_restatement(coupling, links):
    for border, exps in (("neumann", (1.0, 2.0)), ("frame", (0.8, 1.0)), ("periodic_x", (1.5, 2.0))):
        p = rb.make_input(border, 9, 11, 3, "zero", "sparse", links)
        pen = rb.penalties(p, exps, 1e-2)
        old = (p["sides"], p["periodic"], pen[0], pen[1], pen[2], pen[3], p["weight"], p["sx"], p["sy"], p["gx"], p["gy"], p["data"])
        b = rr._boundary(p)
        want, its = rc.irls_f32(*old, b, 3, coupling)
        got, gits = rr.irls_f32(p, pen, 3, coupling)
        assert gits == its
        for a, c in zip(got, want):
            assert np.array_equal(a, c)
        for a, c in zip(rr.irls_exact(p, pen, 2, coupling), rc.irls_exact(*old, b, 2, coupling)):
            assert np.abs(a - c).max() <= 1e-12 * p["range"]
        assert np.allclose(rr.energy(p, pen, got[-1], coupling), rc.energy(*old, got[-1], coupling), rtol=1e-13, atol=0)


def test_quadratic_exponents_are_the_region_solve():
    p = rb.make_input("free_lt", 12, 19, 3, "scatter", "sparse", "loguniform")
    pen = (2.0, 2.0, 0.0, 0.0)
    args = rr.round_args(p)
    for coupling in rr.COUPLINGS:
        exact = rr.irls_exact(p, pen, 3, coupling)
        assert len(exact) == 1 and np.array_equal(exact[0], region_np._hwc(region_np.solve_exact(*args, rr._boundary(p))))
        us, its = rr.irls_f32(p, pen, 3, coupling)
        u, it, _ = region_np.pcg_f32(*args, rr._boundary(p))
        assert len(us) == 1 and its == [it] and np.array_equal(us[0], region_np._hwc(u))
    # with p = 2 alone the coupling changes nothing either, and the joint bit nothing on one channel
    pen = rb.penalties(p, (2.0, 1.0), 1e-2)
    base = rr.irls_f32(p, pen, 2, 0)[0]
    for coupling in rr.COUPLINGS[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(rr.irls_f32(p, pen, 2, coupling)[0], base))
    p1 = rb.make_input("neumann", 12, 19, 1, "ellipse", None, None)
    pen = rb.penalties(p1, (1.0, 2.0), 1e-2)
    assert all(np.array_equal(a, b) for a, b in zip(rr.irls_f32(p1, pen, 2, rr.JOINT)[0], rr.irls_f32(p1, pen, 2, 0)[0]))
    assert all(np.array_equal(a, b) for a, b in zip(rr.irls_f32(p1, pen, 2, rr.ISO | rr.JOINT)[0], rr.irls_f32(p1, pen, 2, rr.ISO)[0]))


@pytest.mark.parametrize("i", range(len(rb.matrix())))
def test_restatement_on_the_matrix(i):
    """the energy does not rise from round to round; a round's system keeps the zero condition; the NaN copy spoils nothing that is read;
    irls_f32 stays within the stop rule's error of irls_exact"""
    p, pen, coupling, y = rb.matrix_case(i)
    energies = [y.energy(u).sum() for u in y.exact]
    for a, b in zip(energies, energies[1:]):
        assert b <= a * (1 + 1e-12), (rb.matrix()[i], energies)
    args = rr.round_args(p, pen, y.u32[-1], coupling)
    k = region_np.kinds(p["sides"], p["periodic"], p["state"])
    blk = region_np.unknowns(p["sides"], p["periodic"], *k.shape[:2])
    other = (k != region_np.UNKNOWN)[blk]
    links, dg = region_np._planes(*args[:6], np.float32)
    b = region_np.folded_rhs(*args, rr._boundary(p), np.float32)
    assert not b[other].any() and not dg[other].any() and not any(l[other].any() for l in links)
    q = rb.nan_unread(p)
    assert np.array_equal(rr.energy(q, pen, y.exact[-1], coupling), y.energy(y.exact[-1]))
    assert all(np.array_equal(a, c) for a, c in zip(rr.reweigh(q, pen, y.u32[-1], coupling)[:2], rr.reweigh(p, pen, y.u32[-1], coupling)[:2]))
    # the stop rule: ||r||_2 <= tol ||b||_2 per plane, so max |r| <= tol sqrt(n) max |b| over a plane's n UNKNOWN pixels (twice that: the
    # recursion's residual is not the true one to the last float32 bit); the iterate then lies within the system's conditioning times
    # tol of the exact rounds -- a hundred times tol of the data's range covers these systems of at most 1551 unknowns per plane
    n = int((k == region_np.UNKNOWN).reshape(-1, k.shape[2]).sum(0).max())
    assert y.res32 <= 2 * 1e-5 * np.sqrt(n), (rb.matrix()[i], y.res32)
    assert y.err32 <= 100 * 1e-5, (rb.matrix()[i], y.err32)


def test_float64_tv_fill_keeps_the_step_where_the_membrane_does_not():
    img, hole = rb.step_hole()
    state = np.where(hole, 0, 1).astype(np.float32)
    zero = np.zeros_like(img)
    p = dict(sides="lrtb", periodic="", state=state, weight=None, sx=None, sy=None, gx=zero, gy=zero, data=img, boundary=img, range=1.0)
    us = rr.irls_exact(p, (1.0, 2.0, 1e-2, 1e-2), 15, rr.ISO)
    membrane, tv = us[0][:, :, 0], us[-1][:, :, 0]
    assert np.abs(membrane - img)[hole].max() > 0.2          # the membrane blurs the edge inside the hole
    assert np.abs(tv - img)[hole].max() < 0.1                # the TV fill runs it through: every pixel within a tenth of the step of its side


def test_float64_masked_integration_ignores_the_outliers():
    gx, gy, valid, known, values, truth = rb.annulus_problem()
    state = np.where(valid, np.where(known, 1, 0), 2).astype(np.float32)
    data = np.where(valid, values, 0).astype(np.float32)
    p = dict(sides="lrtb", periodic="", state=state, weight=None, sx=None, sy=None, gx=gx, gy=gy, data=data, boundary=data,
             range=float(truth[valid].max() - truth[valid].min()))
    us = rr.irls_exact(p, (1.0, 2.0, 1e-3, 1e-3), 8)
    unk = valid & ~known
    err = lambda u: rb.error_up_to_a_constant(u, truth, unk, p["range"])
    assert err(us[-1]) * 20 <= err(us[0]), (err(us[0]), err(us[-1]))
    lx, ly = region_np.live_links("lrtb", "", state[:, :, None])
    wrong = (np.abs(gx - (np.roll(truth, -1, 1) - truth)) > 0.5)[lx[:, :, 0]].sum() + (np.abs(gy - (np.roll(truth, -1, 0) - truth)) > 0.5)[ly[:, :, 0]].sum()
    assert 0.045 <= wrong / (lx.sum() + ly.sum()) <= 0.06           # 5 to 6 % of the live links
