"""Decided output bytes against the float-table solve, exactly (tests/decided_np.py), and the float-table correction at every launch
geometry against its float64 restatement (oracle/lowmode_np.py).  The shapes and the proof that they reach both sides of every launch
decision of the correction are in tests/test_decided_host.py.

The end-to-end tests before this file held most clone paths to "max <= 1 and a small share of channels off" against the C oracle: an
error of a few tenths of a grey level in one node column, one cell row or one size-class member's tables passes that.  Here every
channel whose float-table value lies farther than the path's documented error delta from a byte boundary must equal the oracle's byte;
each test prints the undecided share, the mismatches and the largest lower bound on |u_gpu - u_ref| they imply."""
from __future__ import annotations

import numpy as np
import pytest

from seamlesscloneoptimization_amd import capi

import clone_modes_np as cm
import decided_np as dn
import photo_edits_np as pe
from test_decided_host import (BANDS_CASES, BIG_SHAPES, CLASSES, FIELD_CASES, MG_RESIDUE_SHAPES, SATURATING_CLASS, VARIANT_SHAPES,
                               lm_geometry)

pytestmark = pytest.mark.gpu

KEEP, FF, NOSPEC, LEGACY = capi.SC_FLAG_KEEP_FIELD, capi.SC_FLAG_FLOAT_FIELD, capi.SC_FLAG_NO_SPECULATE, capi.SC_FLAG_LEGACY_PATHS
MG = capi.SC_METHOD_MULTIGRID
# (name, solver options): the multigrid default and its flag variants; update_tol 0.02 makes the stop rule reject judged cycles that
# already wrote output bytes, so the same cycle is launched again in the field-keeping form
MG_VARIANTS = [("mg", dict(method=MG)), ("keep_field", dict(method=MG, flags=KEEP)), ("float_field", dict(method=MG, flags=FF)),
               ("no_speculate", dict(method=MG, flags=NOSPEC)),
               ("separate_restrict", dict(method=MG, flags=LEGACY, legacy_paths=capi.SC_LEGACY_SEPARATE_RESTRICT)),
               ("tight_update_tol", dict(method=MG, update_tol=0.02))]
DIRECT = [("dst", dict(method=capi.SC_METHOD_DST)), ("fft64", dict(method=capi.SC_METHOD_FFT, flags=capi.SC_FLAG_FFT_FP64)),
          ("fft32", dict(method=capi.SC_METHOD_FFT))]
# correction against lowmode_np: the bound of test_gpu_round2.py::test_float_table_correction_alone
CORR_REL, CORR_ABS = 3e-4, 1e-4


@pytest.fixture(scope="module")
def oc():
    from oracle import oracle_c
    oracle_c.build()
    return oracle_c


def _nt(oc):
    return min(16, oc.max_threads())


def _inputs(W, H, seed=0):
    from oracle import oracle_np
    return oracle_np.synth_inputs(W, H, seed_dst=5000 + seed, seed_patch=6000 + seed, margin=2 if min(W, H) < 64 else 24)


def _report(label, res, delta):
    und, mism, bound = res
    print("%-34s delta %.2e: %7.4f %% undecided, %6d mismatches, worst |u_gpu - u_ref| >= %.4f" % (label, delta, 100.0 * und, mism, bound))
    return res


def _opts(inst, **kw):
    """solver options from the defaults: nothing of an earlier configuration carries over"""
    o = inst.default_opts()
    for k, v in kw.items():
        setattr(o, k, v)
    inst.set_solver(**{k: getattr(o, k) for k, _ in capi.SolverOpts._fields_})


def _run(inst, inputs):
    dst, patch, mask, cx, cy = inputs
    body = dst.copy()
    assert inst.run(patch, body, mask, cx, cy) == 0
    return body


def _delta(oc, case, solver):
    if solver.get("method") == capi.SC_METHOD_FFT and not solver.get("flags", 0) & capi.SC_FLAG_FFT_FP64:
        return case.delta_fft32(oc, _nt(oc))
    return dn.DELTA_MG if solver.get("method", capi.SC_METHOD_AUTO) == MG else dn.DELTA_DIRECT


# ---------------------------------------------------------------------------------------------------------------- 2. end to end

@pytest.mark.parametrize("W,H", [(700, 500), (1030, 1000), (2048, 2048)])
def test_every_solver_and_flag(oc, W, H):
    """SC_METHOD_AUTO (the direct solve at 700 x 500, multigrid above), SC_METHOD_DST, SC_METHOD_FFT in double and in float, and the
    multigrid default under every flag that changes its launches"""
    inputs = _inputs(W, H, seed=W)
    case = dn.clone_case(oc, *inputs, nthreads=_nt(oc))
    inst = capi.Instance(0)
    try:
        _opts(inst)
        body = _run(inst, inputs)
        auto_direct = capi.auto_takes_direct(W - 2, H - 2)
        assert inst.info().method == (capi.SC_METHOD_FFT if auto_direct else MG)
        d = dn.DELTA_DIRECT if auto_direct else dn.DELTA_MG
        _report("%dx%d auto" % (W, H), dn.check(case, body, d, "auto"), d)
        for name, solver in DIRECT + MG_VARIANTS:
            _opts(inst, **solver)
            body = _run(inst, inputs)
            assert inst.info().method == solver["method"], name
            d = _delta(oc, case, solver)
            _report("%dx%d %s" % (W, H, name), dn.check(case, body, d, name), d)
    finally:
        inst.destroy()


@pytest.mark.parametrize("W,H", MG_RESIDUE_SHAPES + VARIANT_SHAPES + BIG_SHAPES)
def test_multigrid_shapes(hip, oc, W, H):
    """the multigrid default at every residue of W - 2 and H - 2 mod 8, the shapes of test_output_and_restriction_variants_agree, a
    wide ROI whose projection has 32 parts (k_lm_parts_sum), 4096^2 (36 parts) and 3120^2, where the early correction is taken only
    if the judged cycle's measured update allows it (lowmode_early_kind 3)"""
    if (W, H) == (3120, 3120):
        assert capi.plan_size(W, H)["conditional"] == 1
    if (W, H) in [(3700, 600), (4096, 4096)]:
        assert lm_geometry(W, H)["parts_sum"]
    inputs = _inputs(W, H, seed=W + 7 * H)
    case = dn.clone_case(oc, *inputs, nthreads=_nt(oc))
    body = _run(hip, inputs)
    assert hip.info().method == MG
    _report("%dx%d multigrid" % (W, H), dn.check(case, body, dn.DELTA_MG, "%dx%d" % (W, H)), dn.DELTA_MG)


@pytest.mark.parametrize("W,H", [(1033, 1030), (2048, 2048), (3700, 600), (4096, 4096)])
def test_post_process_of_a_kept_field(oc, W, H):
    """SC_FLAG_KEEP_FIELD: the post-process adds the node correction of the kept field U (k_postprocess, lm_add4).  Its bytes against
    U + lowmode_np.correction(U) at the correction's own float32 tolerance -- a delta a hundred times tighter than the solve's, so an
    error in the last node column, where the correction is small, shows too"""
    from oracle import lowmode_np as lm
    inputs = _inputs(W, H, seed=11 * W + H)
    inst = capi.Instance(0)
    try:
        _opts(inst, method=MG, flags=KEEP)
        body = _run(inst, inputs)
        i = inst.info()
        U = inst.field_store()
    finally:
        inst.destroy()
    u = np.empty((3, H - 2, W - 2), np.float64)
    delta = 0.0
    for c in range(3):
        corr = lm.correction(U[c, 1:-1, 1:-1])
        u[c] = U[c, 1:-1, 1:-1] + corr
        delta = max(delta, CORR_REL * max(1.0, float(np.abs(corr).max())) + CORR_ABS)
    case = dn.Case(inputs[0], W, H, i.ltx, i.lty, u.astype(np.float32))
    _report("%dx%d kept field" % (W, H), dn.check(case, body, delta, "%dx%d kept" % (W, H)), delta)


def _device_jobs(inst, items):
    jobs = capi.Pool.make_jobs(len(items))
    keep = []
    for j, (dst, patch, mask, cx, cy) in zip(jobs, items):
        f, b0, b, m = inst.to_device(patch), inst.to_device(dst), inst.to_device(np.zeros_like(dst)), inst.to_device(mask)
        keep.append((f, b0, b, m, dst.shape))
        j.face, j.face_cols, j.face_rows, j.face_step = f, patch.shape[1], patch.shape[0], 3 * patch.shape[1]
        j.body, j.body_cols, j.body_rows, j.body_step = b, dst.shape[1], dst.shape[0], 3 * dst.shape[1]
        j.mask, j.mask_cols, j.mask_rows, j.mask_step = m, mask.shape[1], mask.shape[0], mask.shape[1]
        j.centerX, j.centerY, j.body_restore = cx, cy, b0
    return jobs, keep


def _free_jobs(inst, keep):
    for k in keep:
        for p in k[:4]:
            inst.free(p)


def _batch(inst, items):
    """one sc_hip_run_device_batch call; the members' output images"""
    jobs, keep = _device_jobs(inst, items)
    try:
        assert inst.run_device_batch(jobs) == 0
        assert all(j.rc == 0 for j in jobs)
        return [inst.from_device(b, shape) for _, _, b, _, shape in keep]
    finally:
        _free_jobs(inst, keep)


def test_device_resident_single_clone(hip, oc):
    inputs = _inputs(1030, 1000, seed=3)
    case = dn.clone_case(oc, *inputs, nthreads=_nt(oc))
    dst, patch, mask, cx, cy = inputs
    d_f, d_b, d_m = hip.to_device(patch), hip.to_device(dst), hip.to_device(mask)
    try:
        assert hip.run_device(d_f, patch.shape[:2], d_b, dst.shape[:2], d_m, mask.shape[:2], cx, cy) == 0
        body = hip.from_device(d_b, dst.shape)
    finally:
        for p in (d_f, d_b, d_m):
            hip.free(p)
    _report("1030x1000 device", dn.check(case, body, dn.DELTA_MG, "device"), dn.DELTA_MG)


def _worst(rows):
    return max(r[0] for r in rows), sum(r[1] for r in rows), max(r[2] for r in rows)


def test_group_of_16(hip, oc):
    """16 clones of one size: one field of 48 planes"""
    items = [_inputs(300, 260, seed=100 + k) for k in range(16)]
    assert capi.plan_groups([(300, 260)] * 16)[1] == [1] * 16
    outs = _batch(hip, items)
    assert hip.info().group_members == 16
    rows = [dn.check(dn.clone_case(oc, *it, nthreads=_nt(oc)), got, dn.DELTA_MG, "member %d" % k) for k, (it, got) in enumerate(zip(items, outs))]
    _report("group of 16 (300x260)", _worst(rows), dn.DELTA_MG)


def test_pool(oc):
    """the native pool, groups formed by its planner (host images)"""
    sizes = [(400, 300), (400, 300), (410, 305), (1030, 1000), (64, 71), (520, 330)]
    items = [_inputs(W, H, seed=200 + k) for k, (W, H) in enumerate(sizes)]
    pool = capi.Pool(0, streams=2, group=capi.SC_POOL_GROUP_AUTO, method=MG)
    try:
        bodies = [it[0].copy() for it in items]
        pool.run_host([(it[1], b, it[2], it[3], it[4]) for it, b in zip(items, bodies)])
    finally:
        pool.close()
    rows = [dn.check(dn.clone_case(oc, *it, nthreads=_nt(oc)), got, dn.DELTA_MG, "pool job %d" % k) for k, (it, got) in enumerate(zip(items, bodies))]
    _report("pool", _worst(rows), dn.DELTA_MG)


@pytest.mark.parametrize("sizes", CLASSES, ids=["n512_513", "n1024_1025"])
def test_size_class_across_a_k_step(hip, oc, sizes):
    """members with different mode counts in one size class: per-member tables (k_lm_table_rag), k_lm_cproject<true>,
    k_lm_cexpand<true>, k_lm_bands_to_cells with the members' own maps"""
    items = [_inputs(W, H, seed=300 + k) for k, (W, H) in enumerate(sizes)]
    outs = _batch(hip, items)
    i = hip.info()
    assert i.group_ragged == 1 and i.group_members == len(sizes)
    for (W, H), it, got in zip(sizes, items, outs):
        _report("class member %dx%d" % (W, H), dn.check(dn.clone_case(oc, *it, nthreads=_nt(oc)), got, dn.DELTA_MG, "%dx%d" % (W, H)),
                dn.DELTA_MG)


def test_size_class_with_a_saturating_member(hip, oc):
    """one member's 16-bit field saturates: the class is solved again on float fields (field_retry)"""
    from test_gpu_round4 import ring_ramp_inputs
    from oracle import oracle_np
    items = [oracle_np.synth_inputs(640, 560, margin=32, seed_dst=11, seed_patch=12), ring_ramp_inputs(652, 571),
             oracle_np.synth_inputs(625, 583, margin=32, seed_dst=13, seed_patch=14)]
    jobs, keep = _device_jobs(hip, items)
    try:
        assert hip.run_device_batch(jobs) == 0
        i = hip.info()
        assert i.field_retry == 1 and i.group_ragged == 1 and i.group_members == 3
        outs = [hip.from_device(b, shape) for _, _, b, _, shape in keep]
    finally:
        _free_jobs(hip, keep)
    for (W, H), it, got in zip(SATURATING_CLASS, items, outs):
        _report("saturating class %dx%d" % (W, H), dn.check(dn.clone_case(oc, *it, nthreads=_nt(oc)), got, dn.DELTA_MG, "%dx%d" % (W, H)),
                dn.DELTA_MG)


@pytest.mark.parametrize("mode", [cm.MIXED, cm.MONOCHROME], ids=["mixed", "monochrome"])
def test_clone_modes(oc, mode):
    """MIXED_CLONE and MONOCHROME_TRANSFER through the default (multigrid at this size); the right-hand side is the restatement's,
    bit-exact with the library's (test_gpu_clone_modes.py::test_rhs_is_bit_exact)"""
    from oracle import oracle_np
    dst, patch, mask, cx, cy = oracle_np.synth_inputs(1100, 1030, seed_dst=3100, seed_patch=4100, margin=40, ellipse=True)
    geo = oracle_np.mask_stage(mask, cx, cy)
    B, lap, _ = cm.build_rhs(dst, patch, geo, mode)
    case = dn.rhs_case(oc, dst, geo["W"], geo["H"], geo["ltx"], geo["lty"], np.moveaxis(B, 2, 0), np.moveaxis(lap, 2, 0), _nt(oc))
    inst = capi.Instance(0)
    try:
        inst.set_clone_mode(mode)
        body = _run(inst, (dst, patch, mask, cx, cy))
        assert inst.info().method == MG
    finally:
        inst.destroy()
    _report("clone mode %d" % mode, dn.check(case, body, dn.DELTA_MG, "mode %d" % mode), dn.DELTA_MG)


EDITS = [("color", capi.SC_EDIT_COLOR_CHANGE, dict(red_mul=1.6, green_mul=0.8, blue_mul=1.2)),
         ("texture", capi.SC_EDIT_TEXTURE_FLATTENING, dict(low_threshold=25.0, high_threshold=60.0, kernel_size=3)),
         ("illumination", capi.SC_EDIT_ILLUMINATION_CHANGE, dict(alpha=0.3, beta=0.5))]


@pytest.mark.parametrize("name,op,kw", EDITS, ids=[e[0] for e in EDITS])
def test_edits(oc, name, op, kw):
    """colorChange and textureFlattening against the restatement's right-hand side (bit-exact with the library's); illuminationChange
    against the oracle's solve of the library's own right-hand side (its powf differs from the host's in the last bits), so that only
    the solver is judged"""
    from test_gpu_photo_edits import _ellipse, _rand
    W, H = 1100, 800
    img, mask = _rand(W, H, 41 + op), _ellipse(W, H)
    inst = capi.Instance(0)
    try:
        p = inst.edit_params(op, **kw)
        if op == capi.SC_EDIT_ILLUMINATION_CHANGE:
            _, lap = inst.edit_rhs(p, img, mask)
        else:
            _, lap, _ = pe.build_rhs(img, mask, {capi.SC_EDIT_COLOR_CHANGE: pe.COLOR, capi.SC_EDIT_TEXTURE_FLATTENING: pe.TEXTURE}[op], **kw)
        out = inst.edit(p, img, mask)
        assert inst.info().method == MG
    finally:
        inst.destroy()
    case = dn.rhs_case(oc, img, W, H, 0, 0, np.moveaxis(img, 2, 0).astype(np.float32), lap, _nt(oc))
    _report("edit %s" % name, dn.check(case, out, dn.DELTA_MG, name), dn.DELTA_MG)


# ------------------------------------------------------------------------------------------- 3. the correction at every launch geometry

def _smooth_field(C, H, W, seed):
    """strong low modes (what the correction acts on) plus noise, a different mix per plane"""
    rng = np.random.default_rng(seed)
    y = np.linspace(0.0, 1.0, H)[:, None]
    x = np.linspace(0.0, 1.0, W)[None, :]
    U = np.empty((C, H, W), np.float32)
    for c in range(C):
        a, b, p = rng.uniform(40, 120), rng.uniform(-60, 60), rng.uniform(0, np.pi)
        U[c] = 128 + a * np.sin(np.pi * x + p) * np.sin(np.pi * y) + b * np.cos(3 * np.pi * x * y + p) + rng.normal(0, 10, (H, W))
    return U


def _check_correction(U, got, label):
    from oracle import lowmode_np as lm
    assert np.array_equal(got[:, 0, :], U[:, 0, :]) and np.array_equal(got[:, -1, :], U[:, -1, :]), label      # ring untouched
    assert np.array_equal(got[:, :, 0], U[:, :, 0]) and np.array_equal(got[:, :, -1], U[:, :, -1]), label
    worst = 0.0
    for c in range(U.shape[0]):
        d = got[c, 1:-1, 1:-1].astype(np.float64) - U[c, 1:-1, 1:-1]
        want = lm.correction(U[c, 1:-1, 1:-1])
        scale = max(1.0, float(np.abs(want).max()))
        err = float(np.abs(d - want).max())
        assert err < CORR_REL * scale + CORR_ABS, (label, c, err, scale)
        worst = max(worst, err / scale)
    print("%-34s correction within %.2e x max|correction| of lowmode_np" % (label, worst))


@pytest.mark.parametrize("W,H,C", FIELD_CASES)
def test_correction_at_every_launch_geometry(W, H, C):
    """sc_hip_field_lowmode (cells from a pass over the field: k_lm_restrict) on a loaded field against lowmode_np.correction.  (A field
    of the hooks holds at most 16 planes; the 48 planes of a group of 16 are covered end to end, test_group_of_16.)"""
    U = _smooth_field(C, H, W, seed=W * 7 + H + C)
    inst = capi.Instance(0)
    try:
        inst.field_load(U, np.zeros_like(U))
        inst.field_lowmode()
        got = inst.field_store()
    finally:
        inst.destroy()
    _check_correction(U, got, "%dx%d C=%d" % (W, H, C))


@pytest.mark.parametrize("W,H,C,post", BANDS_CASES)
def test_correction_from_the_cell_shares_of_a_solve(W, H, C, post):
    """after sc_hip_field_solve (multigrid with `post` post-smoothing sweeps: the tiling of the judged level-0 launch) that launch has
    left the correction's cell shares in parts; sc_hip_field_lowmode builds the cells from them (k_lm_bands_to_cells and the part map
    of that tiling) -- against lowmode_np.correction of the stored field"""
    rng = np.random.default_rng(W + H + C + post)
    U0 = _smooth_field(C, H, W, seed=W + H * 3 + C)
    lap = np.zeros_like(U0)
    lap[:, 1:-1, 1:-1] = rng.normal(0, 4, (C, H - 2, W - 2)).astype(np.float32)
    inst = capi.Instance(0)
    try:
        _opts(inst, method=MG, mg_post=post)
        inst.field_load(U0, lap)
        inst.field_solve()
        U = inst.field_store()
        inst.field_lowmode()
        got = inst.field_store()
    finally:
        inst.destroy()
    _check_correction(U, got, "%dx%d C=%d post %d (bands)" % (W, H, C, post))
