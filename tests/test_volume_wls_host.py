"""CPU tests of the WLS volume solve's host side (sc_hip_volume_wls*): the declarations, the ctypes structs, every code of
sc_hip_volume_wls_check, what volume_wls_arrays and the four wrappers refuse, the numpy restatement (tests/volume_wls_np.py) against
volume_np and against itself, and the fairness of the GPU tests' inputs (tests/volume_wls_bounds.py)."""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

from seamlesscloneoptimization_amd import capi, seamless_clone

import volume_bounds as vb
import volume_np
import volume_wls_bounds as wb
import volume_wls_np as vw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G, L, N = capi.SC_POISSON_GUIDANCE, capi.SC_POISSON_LAPLACIAN, capi.SC_POISSON_NEUMANN
HWC = dict(cols=33, rows=47, channels=3, col_stride=3, row_stride=99, channel_stride=1)
SPAN = 33 * 47 * 3          # of one HWC frame


def test_entry_points_are_declared_and_exported():
    lib = capi.load()
    for name in ("sc_hip_volume_wls_check", "sc_hip_volume_wls_device", "sc_hip_volume_wls"):
        assert name in capi.declared_symbols(capi.HEADER_PATH)
        assert hasattr(lib, name), name
    import seamlesscloneoptimization_amd as pkg
    for name in ("volume_wls_solve", "wls_filter_video", "interpolate_constraints_video", "make_loop"):
        assert name in pkg.__all__ and callable(getattr(pkg, name))
    for name in ("volume_wls", "make_volume_wls_jobs", "volume_wls_device"):
        assert callable(getattr(capi.Instance, name))


@pytest.mark.parametrize("cname,pyname", [("sc_volume_wls_params", "VolumeWlsParams"), ("sc_volume_wls_job", "VolumeWlsJob")])
def test_structs_match_the_header_layout(tmp_path, cname, pyname):
    import ctypes
    cls = getattr(capi, pyname)
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


def test_check_codes():
    bad_arg, bad_size = capi.SC_ERR_BAD_ARG, capi.SC_ERR_BAD_SIZE
    chk = capi.volume_wls_check
    assert chk(G | N, 2, SPAN, **HWC) == capi.SC_OK
    assert chk(L, 8, SPAN + 1000, 0.1, 1, 1e-6, 50, 0.5, 2.0, 3.0, **HWC) == capi.SC_OK
    assert chk(G | N, 3, SPAN, 1.0, 1, **HWC) == capi.SC_OK
    assert chk(G | N, 2, SPAN, precond_lambda=-1.0, precond_smooth=-1.0, precond_tau=-1.0, **HWC) == capi.SC_OK          # <= 0: the means
    # the new refusals: time_periodic, frames under it, the two new constants
    for tp in (2, -1, 7):
        assert chk(G | N, 3, SPAN, 1.0, tp, **HWC) == bad_arg, tp
    assert chk(G | N, 2, SPAN, 1.0, 1, **HWC) == bad_arg
    assert chk(G | N, 1, SPAN, 1.0, 1, **HWC) == bad_arg
    for v in (float("nan"), float("inf"), float("-inf")):
        assert chk(G | N, 3, SPAN, precond_smooth=v, **HWC) == bad_arg
        assert chk(G | N, 3, SPAN, precond_tau=v, **HWC) == bad_arg
    # everything sc_hip_volume_check refuses, under either kind of time
    for tp, frames in ((0, 2), (1, 3)):
        for f in (1, 0, -3):
            assert chk(G | N, f, SPAN, 1.0, tp, **HWC) == bad_arg
        assert chk(G | N, 64, SPAN, 1.0, tp, **HWC) == capi.SC_OK and chk(G | N, 65, SPAN, 1.0, tp, **HWC) == bad_size
        assert chk(G | N, frames, SPAN - 1, 1.0, tp, **HWC) == bad_arg and chk(G | N, frames, 0, 1.0, tp, **HWC) == bad_arg
        for tau in (0.0, -1.0, float("nan"), float("inf")):
            assert chk(G | N, frames, SPAN, tau, tp, **HWC) == bad_arg, tau
        for bad in (dict(tol=float("nan")), dict(tol=float("inf")), dict(precond_lambda=float("nan"))):
            assert chk(L | N, frames, SPAN, 1.0, tp, **bad, **HWC) == bad_arg, bad
        assert chk(0, frames, SPAN, 1.0, tp, **HWC) == bad_arg
        assert chk(L | N | capi.SC_POISSON_PERIODIC_X, frames, SPAN, 1.0, tp, **HWC) == bad_arg
        assert chk(L | capi.SC_ROBUST_ISOTROPIC, frames, SPAN, 1.0, tp, **HWC) == bad_arg
        assert chk(L | N, frames, SPAN, 1.0, tp, **dict(HWC, row_stride=98)) == bad_arg
        assert chk(L, frames, 14, 1.0, tp, cols=2, rows=7, channels=1, col_stride=1, row_stride=2, channel_stride=14) == bad_size
    assert capi.load().sc_hip_volume_wls_check(None, None) == bad_arg
    # the volume call's verdicts, whatever they are
    for kind in (G, L, L | N, G | capi.SC_POISSON_FREE_LEFT, L | capi.SC_POISSON_PERIODIC_Y):
        for cols, rows in ((2, 2), (3, 3), (2, 9), (8193, 2), (300, 9)):
            lay = dict(cols=cols, rows=rows, channels=1, col_stride=1, row_stride=cols, channel_stride=cols * rows)
            for frames, stride in ((2, cols * rows), (1, cols * rows), (5, cols * rows - 1), (193, cols * rows)):
                assert chk(kind, frames, stride, **lay) == capi.volume_check(kind, frames, stride, **lay), (kind, cols, rows, frames)


def test_volume_wls_arrays_argument_handling():
    T, H, W = 4, 6, 7
    data = np.arange(T * H * W * 3, dtype=np.float32).reshape(T, H, W, 3)
    mask = np.zeros((T, H, W), bool)
    mask[1, 2, 3] = True
    g = np.ones_like(data)
    s3 = np.ones((T, H, W), np.float32)
    kind, d, st, w, sx, sy, smt, gx, gy, gt, lap, b = capi.volume_wls_arrays(data, mask, neumann=True)
    assert sx is None and sy is None and smt is None and gt is None and lap is not None and kind == L | N and st.shape == data.shape
    out = capi.volume_wls_arrays(data, mask, None, s3, g, s3[1:], gx=g, gy=g, gt=g[1:], neumann=True)
    assert out[0] == G | N and out[4].shape == data.shape and out[5].shape == data.shape and out[6].shape == (T - 1, H, W, 3) and out[9].shape == (T - 1, H, W, 3)
    out = capi.volume_wls_arrays(data, mask, None, None, None, s3, gx=g, gy=g, gt=g, loop=True, neumann=True)
    assert out[6].shape == data.shape and out[9].shape == data.shape and out[6].flags.c_contiguous
    for bad in (dict(smooth_x=g), dict(smooth_y=g), dict(smooth_x=g, smooth_y=g[:, :, :-1]), dict(smooth_x=g[:2], smooth_y=g[:2]), dict(smooth_t=g),
                dict(smooth_t=g[1:], loop=True), dict(gx=g, gy=g, gt=g), dict(gx=g, gy=g, gt=g[1:], loop=True), dict(gt=g, loop=True),
                dict(data=data[:2], state=mask[:2], loop=True), dict(tau=0.0), dict(tau=float("nan")), dict(state=np.full((T, H, W), 3, np.uint8)),
                dict(data=data[0], state=mask[0]), dict(data=data[0, 0], state=mask[0, 0])):
        with pytest.raises(ValueError):
            capi.volume_wls_arrays(**dict(dict(data=data, state=mask, neumann=True), **bad))
    with pytest.raises(ValueError):
        capi.volume_wls_arrays(data, mask)                      # a frame needs boundary
    for bad in (dict(smooth_x=g.astype(np.float64), smooth_y=g), dict(smooth_t=g[1:].astype(np.float64)), dict(data=data.astype(np.float64)),
                dict(data=None), dict(smooth_t=[[1.0]])):
        with pytest.raises(TypeError):
            capi.volume_wls_arrays(**dict(dict(data=data, state=mask, neumann=True), **bad))


def test_wrappers_check_their_arguments():
    v = np.ones((4, 6, 7, 3), np.float32)
    m = np.zeros((4, 6, 7), bool)
    m[1, 2:4, 2:5] = True
    guide = np.arange(4 * 6 * 7, dtype=np.float64).reshape(4, 6, 7)
    sc = seamless_clone
    for fn, args, kw in ((sc.wls_filter_video, (v,), dict(lam=0.0)), (sc.wls_filter_video, (v,), dict(eps=0.0)), (sc.wls_filter_video, (v,), dict(alpha=-1.0)),
                         (sc.wls_filter_video, (v,), dict(guide=guide[:3])), (sc.wls_filter_video, (v[0, 0],), {}), (sc.wls_filter_video, (v,), dict(tau=0.0)),
                         (sc.wls_filter_video, (v[:2],), dict(loop=True)),
                         (sc.interpolate_constraints_video, (v, m, None), {}), (sc.interpolate_constraints_video, (v, m[:2], guide), {}),
                         (sc.interpolate_constraints_video, (v, m, guide[:, :, :-1]), {}), (sc.interpolate_constraints_video, (v, m, guide), dict(edge_sigma=0.0)),
                         (sc.interpolate_constraints_video, (v, m, np.zeros((4, 6, 7))), {}), (sc.interpolate_constraints_video, (v, np.zeros_like(m), guide), {}),
                         (sc.interpolate_constraints_video, (v, m, guide), dict(hard=False, strength=0.0)),
                         (sc.interpolate_constraints_video, (v, m, guide), dict(tau=float("nan"))),
                         (sc.make_loop, (v,), dict(lam=0.0)), (sc.make_loop, (v,), dict(lam=-1.0)), (sc.make_loop, (v,), dict(lam=float("nan"))),
                         (sc.make_loop, (v[:2],), {}), (sc.make_loop, (v,), dict(tau=0.0)), (sc.make_loop, (v[0, 0],), {}),
                         (sc.volume_wls_solve, (v, m), dict(smooth_x=v)), (sc.volume_wls_solve, (v, m), dict(smooth_t=v)),
                         (sc.volume_wls_solve, (v[:2], m[:2]), dict(loop=True)), (sc.volume_wls_solve, (v, m), dict(tau=-1.0))):
        with pytest.raises(ValueError):
            fn(*args, **kw)
    for fn, args in ((sc.wls_filter_video, (v.astype(np.float64),)), (sc.interpolate_constraints_video, (v.astype(np.float64), m, guide)),
                     (sc.make_loop, (v.astype(np.float64),)), (sc.volume_wls_solve, (v.astype(np.float64), m))):
        with pytest.raises(TypeError):
            fn(*args)


# ---- the restatement against volume_np and against itself -------------------------------------------------------------------------------
@pytest.mark.parametrize("ones", [False, True])
@pytest.mark.parametrize("i", [0, 9, 14, 22, 31])
def test_unit_links_under_free_time_are_the_volume_restatement(i, ones):
    """no link arrays (or arrays of 1) and free time: folded_rhs in float32 bit for bit and pcg_f32's output equal volume_np's"""
    border, H, W, C, T, tau, pattern, wk, form = vb.matrix()[i]
    p = vb.make_input(border, H, W, C, T, tau, pattern, wk)
    args = vb.np_args(p, form)
    b = p["boundary"] if vw.has_dirichlet(p["sides"], p["periodic"]) else None
    one = np.ones(p["data"].shape, np.float32) if ones else None
    q = dict(p, tper=False, sx=one, sy=one, smt=None if one is None else one[1:])
    wargs = wb.np_args(q, form)
    assert wargs[-1].tobytes() == args[-1].tobytes()                                            # the divergence
    want = volume_np.folded_rhs(*args, b, np.float32)
    got = vw.folded_rhs(*wargs, b, np.float32)
    assert got.dtype == np.float32 and got.tobytes() == want.tobytes()
    u, it, rel = volume_np.pcg_f32(*args, b)
    u2, it2, rel2 = vw.pcg_f32(wargs, b)
    assert it2 == it and u2.tobytes() == u.tobytes()
    assert np.allclose(vw.solve_exact(wargs, b), volume_np.solve_exact(*args, b), rtol=0, atol=1e-11)


@pytest.mark.parametrize("T", [3, 4, 5, 8, 17])
def test_the_hartley_table_is_orthonormal_and_diagonalises_the_periodic_second_difference(T):
    D = vw.time_table(T, True)
    assert np.allclose(D, D.T, atol=1e-14) and np.allclose(D @ D, np.eye(T), atol=1e-13)
    A = vw.weighted_np.axis_matrix(vw.direct_np.PP, T)          # the circulant second difference (negative semidefinite)
    assert np.allclose(D @ A @ D.T, np.diag(-vw.time_modes(T, True)), atol=1e-13)
    # ... and every symmetric circulant, which is what a constant temporal link of any weight gives
    c = np.random.default_rng(T).standard_normal(T)
    c = c + np.roll(c[::-1], 1)
    Cm = np.stack([np.roll(c, k) for k in range(T)])
    M = D @ Cm @ D.T
    assert np.allclose(M, np.diag(np.diag(M)), atol=1e-12)
    # free time: the table and the modes volume_np has
    F = vw.time_table(T, False)
    assert np.array_equal(F, volume_np.dct_table(T))
    assert np.allclose(F @ vw.weighted_np.axis_matrix(vw.direct_np.NN, T) @ F.T, np.diag(-vw.time_modes(T, False)), atol=1e-13)


@pytest.mark.parametrize("time", wb.TIMES)
@pytest.mark.parametrize("border", ["neumann", "free_lt", "periodic_xy"])
def test_constant_links_and_weight_with_every_state_unknown_need_no_iteration(border, time):
    p = wb.make_input(border, 9, 12, 2, 5, 10.0, "all", "constant", "none", time)
    p["state"] = np.zeros_like(p["state"])
    p["sx"] = p["sy"] = np.full(p["data"].shape, 2.5, np.float32)
    p["smt"] = np.full(p["gt"].shape, 0.4, np.float32)
    for form in wb.FORMS:
        y = wb.Yardstick(p, form)
        assert y.iters32 == 0 and y.rel32 <= 1e-5, (form, y.iters32, y.rel32)
        assert y.err32 < 1e-5
    sbar, tbar, wbar, _ = vw.precond_means(p["sides"], p["periodic"], p["tper"], p["state"], p["weight"], p["sx"], p["sy"], p["smt"], p["tau"])
    assert sbar == 2.5 and abs(tbar - 4.0) < 1e-6 and abs(wbar - float(p["weight"].flat[0])) < 1e-7


@pytest.mark.parametrize("r", [1, 3])
def test_rolling_a_periodic_input_along_time_rolls_the_exact_solve(r):
    p = wb.make_input("free_lt", 7, 9, 2, 4, 1.0, "scatter", "sparse", "xyt", "periodic", seed=3)
    b = p["boundary"]
    want = vw.solve_exact(wb.np_args(p, "gt"), b)
    q = {n: (np.roll(a, r, 0) if isinstance(a, np.ndarray) else a) for n, a in p.items()}
    got = vw.solve_exact(wb.np_args(q, "gt"), q["boundary"])
    assert np.allclose(got, np.roll(want, r, 0), rtol=0, atol=1e-11 * np.abs(want).max())
    # ... and the dense solve agrees with the conjugate gradients in float64
    assert np.allclose(vw.solve_exact(wb.np_args(p, "gt"), b, dense=False), want, rtol=0, atol=1e-9 * np.abs(want).max())


def test_nan_at_every_unread_element_changes_nothing():
    for time in wb.TIMES:
        p = wb.make_input("free_lt", 7, 9, 2, 4, 1.0, "scatter", "sparse", "xyt", time, seed=3)
        q = wb.nan_unread(p)
        assert any(np.isnan(q[n]).any() for n in ("sx", "sy", "smt", "gt"))
        for form in wb.FORMS:
            a, b = wb.np_args(p, form), wb.np_args(q, form)
            assert vw.folded_rhs(*a, p["boundary"], np.float32).tobytes() == vw.folded_rhs(*b, q["boundary"], np.float32).tobytes()


# ---- the fairness of the GPU tests' inputs --------------------------------------------------------------------------------------------------
def test_the_matrix_covers_every_value_of_every_axis_at_every_border_and_size():
    m = wb.matrix()
    assert 36 <= len(m) <= 40
    axes = (wb.CHANNELS, wb.FRAMES, wb.TAUS, wb.PATTERNS, wb.WEIGHTS, wb.FORMS, wb.LINKS, wb.TIMES)
    for ax, values in enumerate(axes, start=3):
        assert {c[ax] for c in m} == set(values), ax
        for border, _, _ in wb.BORDERS:
            assert {c[ax] for c in m if c[0] == border} == set(values), (border, ax)
        for H, W in wb.SIZES:
            assert {c[ax] for c in m if c[1:3] == (H, W)} == set(values), (H, W, ax)
    assert {c[0] for c in m} == {b[0] for b in wb.BORDERS} and {c[1:3] for c in m} == set(wb.SIZES)
    assert not any(c[10] == "periodic" and c[4] < 3 for c in m)


@pytest.mark.parametrize("i", range(len(wb.matrix())))
def test_inputs_are_fair(i):
    """a condition on the inputs, not a measurement: the reference iteration reaches the stop rule in fewer than 400 iterations, nothing
    is left unpinned, the links span two decades and the arrays have the header's lengths"""
    border, H, W, C, T, tau, pattern, wk, form, links, time = wb.matrix()[i]
    p, form, y = wb.matrix_case(i)
    assert y.rel32 <= 1e-5 and y.iters32 < wb.MAX_ITERS, (y.rel32, y.iters32)
    assert not vw.unpinned_components(p["sides"], p["periodic"], p["tper"], p["state"], p["weight"]).any()
    assert p["gt"].shape[0] == (T if time == "periodic" else T - 1)
    assert (p["sx"] is not None) == ("xy" in links) == (p["sy"] is not None) and (p["smt"] is not None) == links.endswith("t")
    for a in (p["sx"], p["sy"], p["smt"]):
        if a is not None:
            assert 0.1 <= a.min() and a.max() <= 10.0 and a.max() / a.min() > 30
    assert y.err32 < 1e-3


@pytest.mark.parametrize("at", [0, 2])
def test_the_batch_trio_is_fair_whichever_volume_leaves(at):
    """tests/test_gpu_volume_wls.py refuses volume `at` of this trio: the two that stay, under the means of a chunk of those two, converge
    in the reference iteration to a finite exact solve"""
    probs = [wb.make_input("free_lt", 23, 17, 3, 4, 1.0, pat, "constant", "xyt", "periodic", seed=20 + k) for k, pat in enumerate(("hole", "scatter", "keyframes"))]
    stay = [probs[k] for k in range(3) if k != at]
    means = wb.chunk_means(stay)
    for p in stay:
        y = wb.Yardstick(p, "gt", means=means)
        assert np.isfinite(y.want).all() and np.isfinite([y.err32, y.res32]).all()
        assert y.rel32 <= 1e-5 and y.iters32 < wb.MAX_ITERS, (y.rel32, y.iters32)
        assert not vw.unpinned_components(p["sides"], p["periodic"], p["tper"], p["state"], p["weight"]).any()
