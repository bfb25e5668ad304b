"""Every solver on fields of many planes against the exact solve (the GPU side of tests/test_plane_counts_host.py).

The solver kernels were written for one clone, a field of 3 planes; Poisson device batches solve same-size jobs as one field of up to
SC_POISSON_MAX_PLANES = 192 planes and edit batches one of 3n.  Here, along the plane-count axis:

1. the field hooks at C in {1, 2, 4, 5, 7, 16}: sweeps and residuals bit for bit against the C oracle, fixed-count multigrid cycles
   against oracle/mg_np.py, and plane independence (a plane of a C-plane field has the bits it has alone) under every sweep form, the
   cycles and the direct solvers;
2. sc_hip_poisson_device under every method at plane totals 1 ... 390 (one and two chunk boundaries): every job against the float64
   solve, against its solo call, under permutations of the job order, inside guard bands;
3. the shapes of test_plane_counts_host.DECISION_CASES, which reach both sides of every plane-count-dependent launch decision, checked
   by reconstruction from forward differences (the exact answer is the image);
4. edit batches pinned to the direct solvers: every member equals its solo call byte for byte."""
from __future__ import annotations

import numpy as np
import pytest

from seamlesscloneoptimization_amd import capi
from seamlesscloneoptimization_amd.seamless_clone import poisson_tol

import poisson_np
from test_gpu_poisson import TOL, Dev, _batch, _problems, bound, configure, frame_equal
from test_plane_counts_host import DECISION_CASES, bottom_kind, chunks

pytestmark = pytest.mark.gpu

PLANE_COUNTS = (1, 2, 4, 5, 7, 16)
METHODS = {
    "mg": (capi.SC_METHOD_MULTIGRID, 0),
    "fft32": (capi.SC_METHOD_FFT, 0),
    "fft64": (capi.SC_METHOD_FFT, capi.SC_FLAG_FFT_FP64),
    "dst": (capi.SC_METHOD_DST, 0),
}
SOR_SWEEPS = 600                 # the fixed-count sweep method of the batches: SOR to a fixed count, at sizes where that converges


@pytest.fixture(scope="module")
def inst():
    i = capi.Instance(0)
    yield i
    i.destroy()


@pytest.fixture(scope="module")
def oc():
    from oracle import oracle_c
    oracle_c.build()
    return oracle_c


def _field(C, H, W, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(100, 50, (C, H, W)).astype(np.float32), rng.normal(0, 30, (C, H, W)).astype(np.float32)


def _alone(inst, U, F, c, run):
    """plane c loaded as a field of its own, `run` applied, the result"""
    inst.field_load(U[c:c + 1], F[c:c + 1])
    run()
    return inst.field_store()[0]


# ---------------------------------------------------------------------------------------------------------------- 1. the field hooks

SWEEP_SIZES = [(600, 200), (253, 130), (1030, 70), (249, 61), (9, 5), (3, 3)]
SWEEP_FORMS = (0, -1, 1, 2, 3, 4, 6, 8)
SWEEP_RUNS = [(capi.SC_METHOD_JACOBI, n, 1.0) for n in (1, 7, 17)] + [(capi.SC_METHOD_RBGS, n, 1.0) for n in (2, 5)] + \
             [(capi.SC_METHOD_SOR, 5, 1.7)]


@pytest.mark.parametrize("C", PLANE_COUNTS)
def test_sweeps_bit_exact_at_every_plane_count(inst, oc, C):
    """Jacobi, RBGS and SOR(1.7) at every sweeps_per_launch form, sweep counts that leave remainders, tile seams and ragged edges:
    bit for bit against the C oracle, the residual within 1e-9; the last plane also bit for bit alone (plane independence)"""
    configure(inst, capi.SC_METHOD_MULTIGRID)
    for W, H in SWEEP_SIZES:
        U, F = _field(C, H, W, seed=W * 1000 + H + C)
        want = {}
        for method, n, om in SWEEP_RUNS:
            want[method, n] = oc.jacobi(U, F, n) if method == capi.SC_METHOD_JACOBI else oc.rbgs(U, F, n, om)
        for spl in SWEEP_FORMS:
            for method, n, om in SWEEP_RUNS:
                inst.field_load(U, F)
                inst.field_sweep(method, n, om, spl)
                got = inst.field_store()
                assert np.array_equal(got, want[method, n]), (C, W, H, method, n, spl)
                alone = _alone(inst, U, F, C - 1, lambda: inst.field_sweep(method, n, om, spl))
                assert np.array_equal(alone, got[C - 1]), (C, W, H, method, n, spl)
        for method, n, om in SWEEP_RUNS:
            inst.field_load(U, F)
            inst.field_sweep(method, n, om, 1)
            r, rc = inst.field_residual(), oc.residual(want[method, n], F)
            assert r[0] == pytest.approx(rc[0], rel=1e-9, abs=1e-12) and r[1] == pytest.approx(rc[1], rel=1e-9, abs=1e-12), (C, W, H)


@pytest.mark.parametrize("rows", [16, 32, 64])
def test_lds_tiled_jacobi_at_every_plane_count(oc, rows):
    i = capi.Instance(0)
    try:
        i.set_solver(jacobi_tile_rows=rows)
        for C in PLANE_COUNTS:
            for W, H in [(33, 17), (513, 129), (257, 65), (1030, 70), (3, 3)]:
                U, F = _field(C, H, W, seed=W * 31 + H + 7 * C)
                for n in (1, 6):
                    i.field_load(U, F)
                    i.field_sweep(capi.SC_METHOD_JACOBI, n, 1.0, 1)
                    got = i.field_store()
                    assert np.array_equal(got, oc.jacobi(U, F, n)), (rows, C, W, H, n)
                    alone = _alone(i, U, F, C // 2, lambda: i.field_sweep(capi.SC_METHOD_JACOBI, n, 1.0, 1))
                    assert np.array_equal(alone, got[C // 2]), (rows, C, W, H, n)
    finally:
        i.destroy()


MG_SIZES = [(300, 260), (77, 53), (300, 9)]        # a k_mg_tail level, a level-1 direct bottom, no level for the direct solver


def test_mg_sizes_end_the_way_the_tests_say():
    assert [bottom_kind(W, H) for W, H in MG_SIZES] == ["tail", "level1", "none"]


def _mg_field(C, H, W, seed):
    rng = np.random.default_rng(seed)
    U = rng.uniform(0, 255, (C, H, W)).astype(np.float32)
    F = np.zeros((C, H, W), np.float32)
    F[:, 1:-1, 1:-1] = rng.normal(0, 30, (C, H - 2, W - 2)).astype(np.float32)
    return U, F


@pytest.mark.parametrize("W,H", MG_SIZES)
@pytest.mark.parametrize("C", PLANE_COUNTS)
def test_multigrid_cycles_at_every_plane_count(inst, C, W, H):
    """one and three fixed cycles, fused and unfused, against mg_np under the bounds of test_multigrid_cycles_follow_the_spec (first and
    last plane); every plane bit for bit equal to the same cycles on that plane alone"""
    from oracle import mg_np
    U, F = _mg_field(C, H, W, seed=W * 13 + H + C)
    for cycles in (1, 3):
        for fused in (True, False):
            configure(inst, capi.SC_METHOD_MULTIGRID, max_sweeps=cycles, update_tol=1e-30, tol=0.0, sweeps_per_launch=0 if fused else 1)
            inst.field_load(U, F)
            inst.field_solve(allow_not_converged=True)
            got = inst.field_store()
            for c in sorted({0, C - 1}):
                want = mg_np.solve(U[c], F[c], cycles=cycles, fused=fused)
                assert np.abs(got[c] - want).max() < 2e-3 * (10.0 if cycles == 1 else 1.0), (C, W, H, cycles, fused, c)
            for c in range(C):
                alone = _alone(inst, U, F, c, lambda: inst.field_solve(allow_not_converged=True))
                assert np.array_equal(alone, got[c]), (C, W, H, cycles, fused, c)


@pytest.mark.parametrize("name", ["fft32", "fft64", "dst"])
def test_direct_field_solves_are_plane_independent(inst, name):
    """field_solve under the direct solvers: every plane of a C-plane field has the bits it has alone (workspaces sized by plane * C,
    grids of C or 2C in one dimension; both FFT launch counts at 1030 x 1100)"""
    method, flags = METHODS[name]
    for C in PLANE_COUNTS:
        for W, H in [(61, 37), (300, 260), (1030, 70)] + ([(1030, 1100)] if C <= 2 else []):
            U, F = _mg_field(C, H, W, seed=W + 17 * H + C)
            configure(inst, method, flags)
            inst.field_load(U, F)
            inst.field_solve()
            assert inst.info().method == method
            got = inst.field_store()
            for c in range(C):
                alone = _alone(inst, U, F, c, lambda: inst.field_solve())
                assert np.array_equal(alone, got[c]), (name, C, W, H, c)


# ------------------------------------------------------------------------------------------- 2. Poisson device batches under every method

BATCH_W, BATCH_H = 29, 23
BATCHES = [(1, 1), (5, 1), (12, 4), (191, 1), (64, 3), (96, 2), (193, 1), (97, 2), (130, 3), (200, 1)]     # (jobs, C)


def _configure_named(i, name):
    if name == "sor":
        configure(i, capi.SC_METHOD_SOR, max_sweeps=SOR_SWEEPS, tol=0.0)
    elif name == "mg3":
        configure(i, capi.SC_METHOD_MULTIGRID, max_sweeps=3)
    else:
        configure(i, *METHODS[name])


def _call_tol(name):
    return 1e-30 if name == "mg3" else 0.0        # mg3: three cycles, never judged converged; 0: the call's default stop (1e-3)


def _outputs_only_written(dev, full, ids, span):
    written = np.zeros(full.size, bool)
    for (_, _, _, ko) in ids:
        off = dev.parts[ko][0] // 4
        written[off:off + span] = True
    return np.array_equal(full[~written], dev.host[~written])


def _run(i, name, ps):
    rc, outs, jobs, info, dev, full, ids = _batch(i, ps, tol=_call_tol(name))
    try:
        H, W, C = ps[0][0].shape
        assert _outputs_only_written(dev, full, ids, H * W * C), (name, len(ps), C)
    finally:
        dev.free()
    return rc, outs, [j.rc for j in jobs], info


@pytest.mark.parametrize("n,C", BATCHES)
def test_batches_under_every_method_against_the_exact_solve_and_their_solo_calls(n, C):
    ps = _problems(n, BATCH_H, BATCH_W, C, seed=1000 + 7 * n + C)
    want = [poisson_np.solve_guidance(b, gx, gy) for b, gx, gy in ps]
    per = capi.SC_POISSON_MAX_PLANES // C
    i = capi.Instance(0)
    try:
        for name in ("mg", "fft32", "fft64", "dst", "sor", "mg3"):
            _configure_named(i, name)
            rc, outs, rcs, info = _run(i, name, ps)
            ok = capi.SC_ERR_NOT_CONVERGED if name == "mg3" else capi.SC_OK
            assert rc == ok and all(r == ok for r in rcs), (name, n, C, rc)
            assert info.group_members == (chunks(n, C)[-1] if chunks(n, C)[-1] > 1 else 0), (name, info.group_members)
            batch_sweeps = info.sweeps
            for k, (b, gx, gy) in enumerate(ps):
                assert frame_equal(outs[k], b), (name, n, C, k)
                if name != "mg3":
                    R = float(np.abs(want[k]).max())
                    err = float(np.abs(outs[k] - want[k]).max())
                    lim = 1e-4 * R if name == "sor" else bound(info.method, name, R)
                    assert err <= lim, (name, n, C, k, err)
                solo = i.poisson(b, gx=gx, gy=gy, tol=_call_tol(name), allow_not_converged=name == "mg3")
                if name == "mg" and (i.info().sweeps != batch_sweeps or n > per):
                    assert np.abs(outs[k] - solo).max() <= TOL, (name, n, C, k)       # the stop rule saw the group's largest correction
                else:
                    assert np.array_equal(outs[k], solo), (name, n, C, k)
    finally:
        i.destroy()


@pytest.mark.parametrize("n,C", [(5, 1), (12, 4), (64, 3), (130, 3)])
def test_job_order_permutes_the_outputs(n, C):
    """reversed and rotated job orders give the same outputs, permuted, bit for bit -- under the multigrid stop rule as well, and the
    largest correction over all planes is the same (within one chunk: the stop rule sees the chunk's planes)"""
    ps = _problems(n, BATCH_H, BATCH_W, C, seed=2000 + n + C)
    single_chunk = len(chunks(n, C)) == 1
    i = capi.Instance(0)
    try:
        for name in ("mg", "fft32", "fft64", "dst", "sor", "mg3"):
            if name == "mg" and not single_chunk:
                continue
            _configure_named(i, name)
            _, base, _, info0 = _run(i, name, ps)
            for order in (list(range(n))[::-1], list(range(1, n)) + [0]):
                _, outs, _, info = _run(i, name, [ps[k] for k in order])
                for pos, k in enumerate(order):
                    assert np.array_equal(outs[pos], base[k]), (name, n, C, k)
                if single_chunk:
                    assert info.sweeps == info0.sweeps and info.last_update == info0.last_update, (name, n, C)
    finally:
        i.destroy()


def _lap_call(i, ps, tol):
    """the LAPLACIAN form of _batch (dense H x W x C layout)"""
    H, W, C = ps[0][0].shape
    span = H * W * C
    dev = Dev(i)
    ids = [(dev.add(poisson_np.divergence(gx, gy).ravel()), dev.add(b.ravel()), dev.add(np.full(span, -3.5, np.float32))) for b, gx, gy in ps]
    dev.upload()
    try:
        jobs = capi.Instance.make_poisson_jobs(len(ps))
        for j, (kl, kb, ko) in zip(jobs, ids):
            j.lap, j.boundary, j.out = dev.ptr(kl), dev.ptr(kb), dev.ptr(ko)
        rc = i.poisson_device(capi.PoissonParams(capi.SC_POISSON_LAPLACIAN, float(tol)), capi.PoissonLayout(W, H, C, C, C * W, 1), jobs,
                              allow_job_errors=True)
        full = dev.download()
        written = np.zeros(full.size, bool)
        for (_, _, ko) in ids:
            written[dev.parts[ko][0] // 4:dev.parts[ko][0] // 4 + span] = True
        assert np.array_equal(full[~written], dev.host[~written])
        return rc, [full[dev.parts[ko][0] // 4:][:span].reshape(H, W, C).copy() for (_, _, ko) in ids]
    finally:
        dev.free()


def test_laplacian_batch_across_two_chunk_boundaries():
    """the LAPLACIAN form with the documented divergence gives the GUIDANCE form's bits, 130 jobs of 3 channels (chunks 64 + 64 + 2)"""
    ps = _problems(130, BATCH_H, BATCH_W, 3, seed=31)
    i = capi.Instance(0)
    try:
        for name in ("mg", "fft64", "dst"):
            _configure_named(i, name)
            rc, outs, _, _ = _run(i, name, ps)
            rc_l, outs_l = _lap_call(i, ps, _call_tol(name))
            assert rc == rc_l == capi.SC_OK
            for k in range(len(ps)):
                assert np.array_equal(outs_l[k], outs[k]), (name, k)
    finally:
        i.destroy()


# -------------------------------------------------------------------------- 3. both sides of every plane-count-dependent launch decision

DISTINCT = 7            # distinct inputs of a decision case; job k reads input k % 7, so neighbouring jobs always differ


def _image(H, W, C, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    smooth = 120 + 80 * np.sin(xx / 37.0 + seed) * np.cos(yy / 23.0 - seed)
    return (smooth[:, :, None] + rng.uniform(-40, 40, (H, W, C))).astype(np.float32)


def _shared_inputs_call(i, imgs, n, tol):
    """n GUIDANCE jobs reconstructing imgs[k % len(imgs)] from forward differences, each into an output of its own; returns (rc, job
    codes, info, outputs); asserts that nothing outside the outputs was written"""
    H, W, C = imgs[0].shape
    span = H * W * C
    dev = Dev(i)
    ins = []
    for img in imgs:
        gx, gy = poisson_np.forward_differences(img)
        ins.append((dev.add(np.ascontiguousarray(gx).ravel()), dev.add(np.ascontiguousarray(gy).ravel()), dev.add(img.ravel())))
    outs_id = [dev.add(np.full(span, -3.5, np.float32)) for _ in range(n)]
    dev.upload()
    try:
        jobs = capi.Instance.make_poisson_jobs(n)
        for k, j in enumerate(jobs):
            kx, ky, kb = ins[k % len(imgs)]
            j.gx, j.gy, j.boundary, j.out = dev.ptr(kx), dev.ptr(ky), dev.ptr(kb), dev.ptr(outs_id[k])
        rc = i.poisson_device(capi.PoissonParams(capi.SC_POISSON_GUIDANCE, float(tol)), capi.PoissonLayout(W, H, C, C, C * W, 1), jobs,
                              allow_job_errors=True)
        info = i.info()
        full = dev.download()
        written = np.zeros(full.size, bool)
        for ko in outs_id:
            written[dev.parts[ko][0] // 4:dev.parts[ko][0] // 4 + span] = True
        assert np.array_equal(full[~written], dev.host[~written])
        del written
        outs = [full[dev.parts[ko][0] // 4:][:span].reshape(H, W, C) for ko in outs_id]
        return rc, [j.rc for j in jobs], info, outs
    finally:
        dev.free()


@pytest.mark.parametrize("W,H,C,n,methods", DECISION_CASES)
def test_decision_sides(W, H, C, n, methods):
    imgs = [_image(H, W, C, seed=W + H + 5 * k) for k in range(min(n, DISTINCT))]
    R = max(float(np.abs(a).max()) for a in imgs)
    i = capi.Instance(0)
    try:
        for name in methods:
            configure(i, *METHODS[name])
            tol = poisson_tol(imgs[0], R) if name == "mg" else 0.0
            rc, rcs, info, outs = _shared_inputs_call(i, imgs, n, tol)
            assert rc == capi.SC_OK and all(r == capi.SC_OK for r in rcs), (name, W, H, C, n, rc)
            assert info.method == METHODS[name][0], (name, info.method)
            for k, out in enumerate(outs):
                img = imgs[k % len(imgs)]
                err = float(np.abs(out.astype(np.float64) - img).max())
                assert err <= bound(info.method, name, R, tol), (name, W, H, C, n, k, err, info.sweeps)
                assert frame_equal(out, img), (name, k)
                if k >= len(imgs):          # the same input in the same chunk: the same bits (one stop rule, one set of launches)
                    assert np.array_equal(out, outs[k - len(imgs)]), (name, k)
            del outs
    finally:
        i.destroy()


# ------------------------------------------------------------------------------------------------- 4. edit batches under the direct solvers

@pytest.mark.parametrize("method", [capi.SC_METHOD_FFT, capi.SC_METHOD_DST])
@pytest.mark.parametrize("n", [2, 5, 17])
def test_edit_batches_under_the_direct_solvers_match_their_solo_calls(method, n):
    import test_gpu_edit_batch as eb
    W, H = 131, 97
    ops = ["color", "texture"] if n == 5 else ["color"]
    imgs = [eb._rand(W, H, 300 + 11 * k + n) for k in range(n)]
    masks = [eb._mask(W, H, "ellipse", k) for k in range(n)]
    i = capi.Instance(0)
    try:
        i.set_solver(method=method)
        for op in ops:
            code, kw = eb.OPS[op]
            with eb.Dev(i) as d:
                outs = [d.put(np.full_like(img, 0x5A)) for img in imgs]
                jobs = eb._jobs(i, d, [(d.put(img), img.shape, d.put(m), o) for img, m, o in zip(imgs, masks, outs)])
                assert i.edit_device_batch(i.edit_params(code, **kw), jobs) == capi.SC_OK
                info = i.info()
                got = [i.from_device(o, img.shape) for o, img in zip(outs, imgs)]
            assert info.method == method and info.group_members == n, (op, info.method, info.group_members)
            for k, (img, m) in enumerate(zip(imgs, masks)):
                with eb.Dev(i) as d:
                    s, dm, o = d.put(img), d.put(m), d.put(np.zeros_like(img))
                    i.edit_device(i.edit_params(code, **kw), s, (H, W), dm, o, sync=True)
                    solo = i.from_device(o, img.shape)
                assert i.info().method == method
                assert np.array_equal(got[k], solo), (op, method, n, k)
    finally:
        i.destroy()
