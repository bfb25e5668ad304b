"""CPU tests of the bounded solve's host side and of its float64 restatement (tests/bounded_np.py, tests/bounded_bounds.py): no GPU.

1. bounded_np.solve_exact's answers satisfy the KKT conditions to 1e-10 on the whole matrix of the GPU tests, within
   MAX_REFERENCE_ROUNDS rounds.
2. on three tiny inputs (at most 60 unknowns) it agrees with projected Gauss-Seidel run to convergence.
3. sc_hip_bounded_check's codes, capi.bounded_arrays' refusals, the ctypes structs against the header."""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

from seamlesscloneoptimization_amd import capi

import bounded_bounds as bb
import bounded_np
import region_bounds as rb
import region_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G, L, N = capi.SC_POISSON_GUIDANCE, capi.SC_POISSON_LAPLACIAN, capi.SC_POISSON_NEUMANN
_CASES = bb.matrix()


def test_entry_points_are_declared_and_exported():
    lib = capi.load()
    for name in ("sc_hip_bounded_check", "sc_hip_bounded_device", "sc_hip_bounded", "sc_hip_bounded_trace"):
        assert name in capi.declared_symbols(capi.HEADER_PATH)
        assert hasattr(lib, name), name
    import seamlesscloneoptimization_amd as pkg
    for name in ("bounded_solve", "bounded_solve_batch", "poisson_clone_in_range", "interpolate_in_range"):
        assert name in pkg.__all__ and callable(getattr(pkg, name))
    for name in ("bounded", "make_bounded_jobs", "bounded_device", "bounded_trace"):
        assert callable(getattr(capi.Instance, name))


@pytest.mark.parametrize("cname, cls", [("sc_bounded_params", capi.BoundedParams), ("sc_bounded_job", capi.BoundedJob)])
def test_structs_match_the_header_layout(tmp_path, cname, cls):
    import ctypes
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


def test_the_structs_extend_the_region_calls():
    assert capi.BoundedParams._fields_[:5] == capi.RegionParams._fields_
    assert [f for f, _ in capi.BoundedJob._fields_ if f not in ("lower", "upper")] == [f for f, _ in capi.RegionJob._fields_]


def test_check_codes():
    bad_arg, nan, inf = capi.SC_ERR_BAD_ARG, float("nan"), float("inf")
    lay = dict(cols=33, rows=47, channels=3, col_stride=3, row_stride=99, channel_stride=1)
    chk = capi.bounded_check
    assert chk(G | N, **lay) == chk(L, lower=0.0, upper=1.0, **lay) == chk(G, lower=-inf, upper=0.5, max_rounds=3, **lay) == capi.SC_OK
    assert chk(G, lower=0.25, upper=0.25, **lay) == capi.SC_OK
    assert chk(G, lower=1.0, upper=0.5, **lay) == bad_arg
    assert chk(G, lower=nan, **lay) == chk(G, upper=nan, **lay) == bad_arg
    assert chk(G, lower=inf, upper=-inf, **lay) == bad_arg
    # everything the region call's check refuses
    assert chk(G, tol=nan, **lay) == chk(G, precond_lambda=inf, **lay) == chk(G, precond_smooth=nan, **lay) == bad_arg
    for kw in (dict(tol=nan), dict(precond_lambda=inf), dict(kind=77)):
        assert chk(**{"kind": G, **kw}, **lay) == capi.region_check(**{"kind": G, **kw}, **lay) != capi.SC_OK
    assert chk(G, cols=2, rows=7, channels=1, col_stride=1, row_stride=2, channel_stride=14) == \
        capi.region_check(G, cols=2, rows=7, channels=1, col_stride=1, row_stride=2, channel_stride=14) == capi.SC_ERR_BAD_SIZE
    assert capi.load().sc_hip_bounded_check(None, None) == bad_arg


def test_bounded_arrays_argument_handling():
    H, W = 6, 7
    data = np.arange(H * W * 3, dtype=np.float32).reshape(H, W, 3)
    state = np.zeros((H, W), np.uint8)
    state[0, 0] = 1
    ok = capi.bounded_arrays(data, state, 0.0, 1.0, neumann=True)
    assert ok[11:] == (0.0, 1.0, None, None) and ok[2].shape == data.shape and ok[2].dtype == np.float32
    assert capi.bounded_arrays(data, state, None, None, neumann=True)[11:13] == (-np.inf, np.inf)
    lo2 = np.zeros((H, W), np.float32)
    out = capi.bounded_arrays(data, state, lo2, 3.0, neumann=True)
    assert out[11] == -np.inf and out[12] == 3.0 and out[13].shape == data.shape and out[14] is None
    with pytest.raises(ValueError):
        capi.bounded_arrays(data, state, float("nan"), 1.0, neumann=True)
    with pytest.raises(ValueError):
        capi.bounded_arrays(data, state, 2.0, 1.0, neumann=True)
    with pytest.raises(TypeError):
        capi.bounded_arrays(data, state, np.zeros((H, W), np.float64), 1.0, neumann=True)
    with pytest.raises(ValueError):
        capi.bounded_arrays(data, state, np.zeros((H, W + 1), np.float32), 1.0, neumann=True)
    # a defect at an UNKNOWN pixel is refused, the same at a KNOWN one is not read
    hi = np.ones((H, W), np.float32)
    for bad in (np.float32("nan"), np.float32(-1.0)):
        b = hi.copy()
        b[0, 0] = bad
        capi.bounded_arrays(data, state, lo2, b, neumann=True)
        b[2, 3] = bad
        with pytest.raises(ValueError):
            capi.bounded_arrays(data, state, lo2, b, neumann=True)
    # the region call's refusals come first
    with pytest.raises(ValueError):
        capi.bounded_arrays(data, np.full((H, W), 3, np.uint8), 0.0, 1.0, neumann=True)
    with pytest.raises(ValueError):
        capi.bounded_arrays(data, state, 0.0, 1.0)          # a Dirichlet line needs boundary


def test_wrappers_refuse_bad_arguments_before_any_device():
    import seamlesscloneoptimization_amd as pkg
    img = np.zeros((6, 7), np.float32)
    mask = np.zeros((6, 7), bool)
    mask[2:4, 2:4] = True
    with pytest.raises(ValueError):
        pkg.poisson_clone_in_range(img, img, mask, lo=1.0, hi=0.0)
    with pytest.raises(TypeError):
        pkg.poisson_clone_in_range(img.astype(np.float64), img, mask)
    with pytest.raises(ValueError):
        pkg.poisson_clone_in_range(img, img, np.ones((6, 7), bool))
    with pytest.raises(ValueError):
        pkg.interpolate_in_range(img, mask, 0.0, 1.0, edge_sigma=0.1)
    with pytest.raises(ValueError):
        pkg.interpolate_in_range(img, mask, float("nan"), 1.0)
    with pytest.raises(ValueError):
        pkg.bounded_solve(img, mask, lower=2.0, upper=1.0)


def test_matrix_shape():
    assert 80 <= len(_CASES) <= 120 and len(set(_CASES)) == len(_CASES)
    assert {c[0] for c in _CASES} == {b[0] for b in rb.BORDERS} and {(c[1], c[2]) for c in _CASES} == set(bb.SIZES)
    for border, _, _ in rb.BORDERS:
        mine = [c for c in _CASES if c[0] == border]
        assert {c[8] for c in mine if c[3] == 1} == set(bb.BOUNDS) == {c[8] for c in mine if c[3] == 3}
        assert {c[4] for c in mine} == set(rb.PATTERNS)


@pytest.mark.parametrize("case", _CASES, ids=[bb.case_id(c) for c in _CASES])
def test_reference_meets_the_kkt_conditions_within_ten_rounds(case):
    p, y = bb.case_input(case, True, False)
    assert y.rounds <= bb.MAX_REFERENCE_ROUNDS, y.rounds
    rng, res, sign = bounded_np.kkt(y.args, y.boundary, y.want, y.lower, y.upper)
    assert rng == 0.0 and res <= 1e-10 and sign <= 1e-10, (rng, res, sign)
    active = int((y.set != 0).sum())
    assert 0 < active < int(y.unk.sum()), "the bounds must bind somewhere and leave something free"
    # the set is the answer's: active pixels on their bound, the others strictly inside or on it with r = 0
    lo, hi = bounded_np._bounds(y.want.shape, y.lower, y.upper)
    assert (y.want[y.set > 0] == hi[y.set > 0]).all() and (y.want[y.set < 0] == lo[y.set < 0]).all()
    # ... and it is not the clamped unconstrained answer
    free = region_np._hwc(region_np.solve_exact(*y.args, y.boundary, dense=False))
    assert np.abs(np.clip(free, lo, hi) - y.want)[y.unk].max() > 1e-6 * np.abs(y.want[y.unk]).max()


@pytest.mark.parametrize("border, bkind, wk, sk", [("neumann", "both", None, "loguniform"), ("frame", "arrays", "sparse", None),
                                                   ("periodic_x", "upper", "constant", "constant")])
def test_agrees_with_projected_gauss_seidel_on_tiny_inputs(border, bkind, wk, sk):
    p = rb.make_input(border, 5, 6, 2, "scatter", wk, sk)
    y = bb.Yardstick(p, "guidance", bkind, f32=False)
    assert 0 < int(y.unk.sum()) <= 60
    u = bounded_np.projected_gauss_seidel(y.args, y.boundary, y.lower, y.upper)
    assert np.abs(u - y.want)[y.unk].max() <= 1e-9 * max(1.0, np.abs(y.want[y.unk]).max())
    assert (y.set != 0).any()
