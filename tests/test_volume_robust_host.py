"""CPU tests of the robust volume solve's host side (sc_hip_volume_robust*): the declarations, the ctypes structs, every code of
sc_hip_volume_robust_check, the numpy restatement (tests/volume_robust_np.py) against volume_wls_np and against itself, the fairness of
the GPU tests' inputs (tests/volume_robust_bounds.py) and the outlier problem of the GPU test in float64."""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

from seamlesscloneoptimization_amd import capi

import volume_robust_bounds as rb
import volume_robust_np as vr
import volume_wls_np as vw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G, L, N = capi.SC_POISSON_GUIDANCE, capi.SC_POISSON_LAPLACIAN, capi.SC_POISSON_NEUMANN
HWC = dict(cols=33, rows=47, channels=3, col_stride=3, row_stride=99, channel_stride=1)
SPAN = 33 * 47 * 3          # of one HWC frame


def test_entry_points_are_declared_and_exported():
    lib = capi.load()
    for name in ("sc_hip_volume_robust_check", "sc_hip_volume_robust_device", "sc_hip_volume_robust"):
        assert name in capi.declared_symbols(capi.HEADER_PATH)
        assert hasattr(lib, name), name
    import seamlesscloneoptimization_amd as pkg
    for name in ("volume_robust_solve", "tv_denoise_video", "integrate_gradients_video"):
        assert name in pkg.__all__ and callable(getattr(pkg, name))
    for name in ("volume_robust", "make_volume_robust_jobs", "volume_robust_device"):
        assert callable(getattr(capi.Instance, name))


@pytest.mark.parametrize("cname,pyname", [("sc_volume_robust_params", "VolumeRobustParams"), ("sc_volume_robust_job", "VolumeRobustJob")])
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
    chk = capi.volume_robust_check
    nan, inf = float("nan"), float("inf")
    assert chk(G | N, 2, SPAN, **HWC) == capi.SC_OK
    assert chk(G, 8, SPAN + 1000, 0.1, 1, 0.5, 1e-2, 1.5, 1e-4, 1.0, 1e-3, 3, -1.0, 1e-6, 50, **HWC) == capi.SC_OK
    assert chk(G | N, 3, SPAN, p_grad=2.0, eps_grad=0.0, p_time=2.0, eps_time=nan, p_data=2.0, eps_data=-1.0, **HWC) == capi.SC_OK      # exponent 2: eps unused
    # everything sc_hip_robust_check refuses for exponents, eps, tol, round_tol and a Laplacian base
    for name in ("p_grad", "p_time", "p_data"):
        for v in (0.0, -1.0, 2.5, nan):
            assert chk(G | N, 3, SPAN, **{name: v}, **HWC) == bad_arg, (name, v)
    for p_name, e_name in (("p_grad", "eps_grad"), ("p_time", "eps_time"), ("p_data", "eps_data")):
        for v in (0.0, -1.0, nan, inf):
            assert chk(G | N, 3, SPAN, **{p_name: 1.0, e_name: v}, **HWC) == bad_arg, (e_name, v)
    for bad in (dict(tol=nan), dict(tol=inf), dict(round_tol=nan), dict(round_tol=inf)):
        assert chk(G | N, 3, SPAN, **bad, **HWC) == bad_arg, bad
    assert chk(L | N, 3, SPAN, **HWC) == bad_arg and chk(L, 3, SPAN, **HWC) == bad_arg
    # the coupled forms are not offered on volumes
    for bits in (capi.SC_ROBUST_ISOTROPIC, capi.SC_ROBUST_JOINT_CHANNELS, capi.SC_ROBUST_ISOTROPIC | capi.SC_ROBUST_JOINT_CHANNELS):
        assert chk(G | N | bits, 3, SPAN, **HWC) == bad_arg
    # everything sc_hip_volume_wls_check refuses, under either kind of time
    for tp in (2, -1, 7):
        assert chk(G | N, 3, SPAN, 1.0, tp, **HWC) == bad_arg, tp
    assert chk(G | N, 2, SPAN, 1.0, 1, **HWC) == bad_arg
    for tp, frames in ((0, 2), (1, 3)):
        for f in (1, 0, -3):
            assert chk(G | N, f, SPAN, 1.0, tp, **HWC) == bad_arg
        assert chk(G | N, 64, SPAN, 1.0, tp, **HWC) == capi.SC_OK and chk(G | N, 65, SPAN, 1.0, tp, **HWC) == bad_size
        assert chk(G | N, frames, SPAN - 1, 1.0, tp, **HWC) == bad_arg and chk(G | N, frames, 0, 1.0, tp, **HWC) == bad_arg
        for tau in (0.0, -1.0, nan, inf):
            assert chk(G | N, frames, SPAN, tau, tp, **HWC) == bad_arg, tau
        assert chk(0, frames, SPAN, 1.0, tp, **HWC) == bad_arg
        assert chk(G | N | capi.SC_POISSON_PERIODIC_X, frames, SPAN, 1.0, tp, **HWC) == bad_arg
        assert chk(G | N, frames, SPAN, 1.0, tp, **dict(HWC, row_stride=98)) == bad_arg
        assert chk(G, frames, 14, 1.0, tp, cols=2, rows=7, channels=1, col_stride=1, row_stride=2, channel_stride=14) == bad_size
    assert capi.load().sc_hip_volume_robust_check(None, None) == bad_arg
    # on a guidance base with valid penalties: the WLS volume call's verdicts, whatever they are
    for kind in (G, G | N, G | capi.SC_POISSON_FREE_LEFT, G | capi.SC_POISSON_PERIODIC_Y):
        for cols, rows in ((2, 2), (3, 3), (2, 9), (8193, 2), (300, 9)):
            lay = dict(cols=cols, rows=rows, channels=1, col_stride=1, row_stride=cols, channel_stride=cols * rows)
            for frames, stride, tp in ((2, cols * rows, 0), (1, cols * rows, 0), (5, cols * rows - 1, 1), (193, cols * rows, 0), (3, cols * rows, 1)):
                assert chk(kind, frames, stride, 1.0, tp, **lay) == capi.volume_wls_check(kind, frames, stride, 1.0, tp, **lay), (kind, cols, rows, frames)


def test_volume_robust_arrays_argument_handling():
    T, H, W = 4, 6, 7
    data = np.arange(T * H * W * 3, dtype=np.float32).reshape(T, H, W, 3)
    mask = np.zeros((T, H, W), bool)
    g = np.ones_like(data)
    out = capi.volume_robust_arrays(g, g, data, mask, gt=g[1:], neumann=True)
    assert out[0] == G | N and len(out) == 11 and out[9].shape == (T - 1, H, W, 3) and out[2].shape == data.shape
    out = capi.volume_robust_arrays(g, g, data, mask, smooth_t=g, gt=g, loop=True, neumann=True)
    assert out[6].shape == data.shape and out[9].shape == data.shape
    for bad in (dict(gx=None), dict(gy=None), dict(p_grad=0.0), dict(p_time=2.5), dict(p_data=float("nan")), dict(p_grad=1.0, eps_grad=0.0),
                dict(p_time=1.0, eps_time=float("inf")), dict(p_data=1.0, eps_data=-1.0), dict(smooth_x=g), dict(gt=g), dict(tau=0.0)):
        a = dict(gx=g, gy=g, data=data, state=mask, neumann=True)
        a.update(bad)
        with pytest.raises(ValueError):
            capi.volume_robust_arrays(**a)


def test_matrix_covers_every_value_under_every_border_and_size():
    m = rb.matrix()
    assert len(m) == 2 * (len(rb.BORDERS) * len(rb.SIZES) - 1)
    axes = {3: rb.CHANNELS, 4: rb.FRAMES, 5: rb.TAUS, 6: rb.PATTERNS, 7: rb.WEIGHTS, 8: rb.LINKS, 9: rb.TIMES, 10: rb.GT, 11: rb.EXPONENTS, 12: rb.EPS}
    for col, values in axes.items():
        for border, _, _ in rb.BORDERS:
            assert {c[col] for c in m if c[0] == border} == set(values), (col, border)
        for H, W in rb.SIZES:
            assert {c[col] for c in m if (c[1], c[2]) == (H, W)} == set(values), (col, H, W)
    assert all(c[9] == "free" for c in m if c[4] == 2)
    assert not any(c[0] == "frame" and min(c[1], c[2]) < 3 for c in m)


def test_quadratic_exponents_are_the_wls_volume_solve():
    p = rb.make_input("free_lt", 5, 16, 3, 3, 1.0, "scatter", "sparse", "xyt", "periodic")
    pen = (2.0, 2.0, 2.0, 0.0, 0.0, 0.0)
    exact = vr.irls_exact(p, pen, 3)
    lap = vw.divergence(p["sides"], p["periodic"], p["tper"], p["state"], p["sx"], p["sy"], p["smt"], p["tau"], p["gx"], p["gy"], p["gt"])
    args = (p["sides"], p["periodic"], p["tper"], p["state"], p["weight"], p["sx"], p["sy"], p["smt"], p["tau"], p["data"], lap)
    assert len(exact) == 1 and np.array_equal(exact[0], vw._thwc(vw.solve_exact(args, None if not vw.has_dirichlet(p["sides"], p["periodic"]) else p["boundary"])))
    us, its = vr.irls_f32(p, pen, 3)
    assert len(us) == 1 and len(its) == 1
    # phi_2 is the square: the energy is the quadratic form the WLS volume solve minimises, so no nearby field has less
    e0 = vr.energy(p, pen, exact[0]).sum()
    rng = np.random.default_rng(1)
    unk = vw.kinds(p["sides"], p["periodic"], p["state"]) == vw.UNKNOWN
    for _ in range(3):
        assert vr.energy(p, pen, exact[0] + 1e-3 * rng.standard_normal(unk.shape) * unk).sum() > e0


@pytest.mark.parametrize("i", range(len(rb.matrix())))
def test_energy_does_not_rise_and_the_rounds_keep_the_zero_condition(i):
    p, pen, y = rb.matrix_case(i)
    energies = [y.energy(u) for u in y.exact]
    for a, b in zip(energies, energies[1:]):
        assert (b <= a * (1 + 1e-12)).all(), (rb.matrix()[i], energies)
    # the folded right-hand side and the coefficient planes of a round's system are 0 at every pixel that is not UNKNOWN
    args = vr.round_args(p, pen, y.u32[-1])
    k = vw.kinds(p["sides"], p["periodic"], p["state"])
    blk = (slice(None),) + vw.unknowns(p["sides"], p["periodic"], *k.shape[1:3])
    other = (k != vw.UNKNOWN)[blk]
    links, dg = vw._planes(*args[:9], np.float32)
    b = vw.folded_rhs(*args, vr._boundary(p), np.float32)
    assert not b[other].any() and not dg[other].any() and not any(l[other].any() for l in links)
    # the NaN copy spoils nothing the restatement reads
    q = rb.nan_unread(p)
    assert np.array_equal(vr.energy(q, pen, y.exact[-1]), energies[-1])


@pytest.mark.parametrize("T,H,W,loop", [(4, 12, 19, False), (5, 10, 17, True), (3, 7, 9, False)])
def test_float64_rounds_beat_the_quadratic_solve_on_the_outlier_problem(T, H, W, loop):
    p, truth = rb.outlier_problem(T, H, W, loop)
    eps = 1e-3 * p["range"]
    pen = (1.0, 1.0, 2.0, eps, eps, eps)
    us = vr.irls_exact(p, pen, 8)
    unk = vw.kinds(p["sides"], p["periodic"], p["state"]) == vw.UNKNOWN
    err = lambda u: float(np.abs(u - truth)[unk].max()) / p["range"]
    assert err(us[-1]) * 20 <= err(us[0]), (err(us[0]), err(us[-1]))
