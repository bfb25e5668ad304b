"""MIXED_CLONE and MONOCHROME_TRANSFER on the MI355X (sc_hip_set_clone_mode; k_preprocess / k_preprocess_group MODE).

PARITY UNPINNED: OpenCV is not available to compare against and the reference holds no fixture for these modes; the modes are
checked against the restatement in tests/clone_modes_np.py (OpenCV 3.4.5 Cloning::normalClone) and tied to the pinned NORMAL
path by identities.  Every test uses instances of its own: the shared `hip` fixture keeps mode NORMAL."""
import numpy as np
import pytest

from oracle import oracle_np
import clone_modes_np as cm

pytestmark = pytest.mark.gpu

MODES = {"mixed": cm.MIXED, "monochrome": cm.MONOCHROME}


def _dmax(a, b):
    return int(np.abs(a.astype(np.int16) - b.astype(np.int16)).max())


def _new(mode=cm.NORMAL, **solver):
    from seamlesscloneoptimization_amd import capi
    inst = capi.Instance(0)
    if solver:
        inst.set_solver(**solver)
    if mode != cm.NORMAL:
        inst.set_clone_mode(mode)
    return inst


def _inputs(W, H, seed=0, ellipse=False, margin=40):
    return oracle_np.synth_inputs(W, H, seed_dst=3000 + seed, seed_patch=4000 + seed, margin=margin, ellipse=ellipse)


def _clone(inst, dst, patch, mask, cx, cy):
    body = dst.copy()
    assert inst.run(patch, body, mask, cx, cy) == 0
    return body


# ---- the right-hand side, bit for bit --------------------------------------------------------------------------------------------
RHS_CASES = [(37, 29, False), (40, 33, True), (131, 45, False), (301, 70, True), (258, 19, True), (9, 8, False)]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("W,H,ellipse", RHS_CASES)
def test_rhs_is_bit_exact(mode, W, H, ellipse):
    """sc_hip_build_rhs under the mode against the restatement: widths that are and are not multiples of 4, ROIs of one, two and
    three 128-pixel tiles, rectangle and ellipse masks."""
    dst, patch, mask, cx, cy = _inputs(W, H, seed=W + H, ellipse=ellipse)
    inst = _new(MODES[mode])
    try:
        geo, B, lap = inst.build_rhs(patch, dst, mask, cx, cy)
    finally:
        inst.destroy()
    g = oracle_np.mask_stage(mask, cx, cy)
    Bw, lapw, _ = cm.build_rhs(dst, patch, g, MODES[mode])
    assert (int(geo[2]), int(geo[3])) == (g["W"], g["H"])
    assert np.array_equal(B, np.moveaxis(Bw, 2, 0))
    assert np.array_equal(lap, np.moveaxis(lapw, 2, 0)), int((lap != np.moveaxis(lapw, 2, 0)).sum())
    # the mode really changed something
    assert not np.array_equal(lapw, oracle_np.build_rhs(dst, patch, g)[1])


# ---- end to end --------------------------------------------------------------------------------------------------------------------
E2E = [("auto_direct", None, 300, 200), ("auto_multigrid", None, 1100, 1030), ("multigrid", "SC_METHOD_MULTIGRID", 640, 480),
       ("fft", "SC_METHOD_FFT", 640, 480), ("dst", "SC_METHOD_DST", 400, 300)]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name,method,W,H", E2E)
def test_end_to_end_against_the_restatement(mode, name, method, W, H):
    """The host-image call under each solver against the restatement plus the float-table direct solve: within one grey level,
    the tolerance the NORMAL tests hold every method to."""
    from seamlesscloneoptimization_amd import capi
    dst, patch, mask, cx, cy = _inputs(W, H, seed=W, ellipse=(name == "multigrid"))
    want = cm.seamless_clone(dst, patch, mask, cx, cy, MODES[mode])
    inst = _new(MODES[mode], **({"method": getattr(capi, method)} if method else {}))
    try:
        body = _clone(inst, dst, patch, mask, cx, cy)
        i = inst.info()
    finally:
        inst.destroy()
    if name == "auto_direct":
        assert i.method == capi.SC_METHOD_FFT
    if name == "auto_multigrid":
        assert i.method == capi.SC_METHOD_MULTIGRID
    assert _dmax(body, want) <= 1, (mode, name)
    assert not np.array_equal(body, oracle_np.seamless_clone(dst, patch, mask, cx, cy, float_tables=True))


def _embed(a, rows, cols, oy, ox):
    out = np.zeros((rows, cols) + a.shape[2:], np.uint8)
    out[oy:oy + a.shape[0], ox:ox + a.shape[1]] = a
    return out


@pytest.mark.parametrize("mode", list(MODES))
def test_device_call_at_every_alignment(mode):
    """sc_hip_run_device with the patch and the destination at every byte alignment the staged windows handle: each one gives the
    bytes of the first, which is within one grey level of the restatement."""
    W, H = 261, 97
    dst, patch, mask, cx, cy = _inputs(W, H, seed=9, ellipse=True)
    want = cm.seamless_clone(dst, patch, mask, cx, cy, MODES[mode])
    inst = _new(MODES[mode])
    outs = []
    try:
        for fo, bo in ((0, 0), (1, 2), (2, 3), (3, 1), (5, 0)):
            face = _embed(patch, patch.shape[0] + 3, patch.shape[1] + 6, 1, fo)
            fmask = _embed(mask, patch.shape[0] + 3, patch.shape[1] + 6, 1, fo)
            body = _embed(dst, dst.shape[0], dst.shape[1] + 5, 0, bo)
            d = [inst.to_device(a) for a in (face, body, fmask)]
            try:
                inst.run_device(d[0], face.shape[:2], d[1], body.shape[:2], d[2], fmask.shape[:2], cx + bo, cy, sync=True)
                outs.append(inst.from_device(d[1], body.shape)[:, bo:bo + dst.shape[1]])
            finally:
                for p in d:
                    inst.free(p)
    finally:
        inst.destroy()
    assert _dmax(outs[0], want) <= 1
    for k, o in enumerate(outs[1:]):
        assert np.array_equal(o, outs[0]), (mode, k)


def test_c1_airplane_on_sky_mixed(c1_inputs):
    c = c1_inputs
    want = cm.seamless_clone(c["dst"], c["patch"], c["mask"], c["cx"], c["cy"], cm.MIXED)
    inst = _new(cm.MIXED)
    try:
        body = _clone(inst, c["dst"], c["patch"], c["mask"], c["cx"], c["cy"])
    finally:
        inst.destroy()
    assert _dmax(body, want) <= 1
    normal = oracle_np.seamless_clone(c["dst"], c["patch"], c["mask"], c["cx"], c["cy"], float_tables=True)
    assert _dmax(body, normal) > 1


# ---- identities with the pinned NORMAL path ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,W,H", [(None, 300, 200), ("SC_METHOD_MULTIGRID", 1030, 1030)])
def test_monochrome_on_a_grey_patch_is_normal(method, W, H):
    from seamlesscloneoptimization_amd import capi
    dst, patch, mask, cx, cy = _inputs(W, H, seed=5, ellipse=True)
    patch = np.ascontiguousarray(np.repeat(patch[:, :, 1:2], 3, axis=2))
    solver = {"method": getattr(capi, method)} if method else {}
    a, b = _new(cm.NORMAL, **solver), _new(cm.MONOCHROME, **solver)
    try:
        assert np.array_equal(_clone(b, dst, patch, mask, cx, cy), _clone(a, dst, patch, mask, cx, cy))
    finally:
        a.destroy(); b.destroy()


def test_mixed_with_a_constant_patch_returns_the_destination():
    from seamlesscloneoptimization_amd import capi
    dst, patch, mask, cx, cy = _inputs(500, 380, seed=6, ellipse=True)
    patch[:] = 90
    inst = _new(cm.MIXED, method=capi.SC_METHOD_MULTIGRID, flags=capi.SC_FLAG_EXACT_TABLES)
    try:
        body = _clone(inst, dst, patch, mask, cx, cy)
    finally:
        inst.destroy()
    assert _dmax(body, dst) <= 1


# ---- groups and the pool -----------------------------------------------------------------------------------------------------------
def _device_jobs(inst, items):
    from seamlesscloneoptimization_amd import capi
    jobs = capi.Pool.make_jobs(len(items)); keep = []
    for j, (dst, patch, mask, cx, cy) in zip(jobs, items):
        f, b0, b, m = inst.to_device(patch), inst.to_device(dst), inst.to_device(np.zeros_like(dst)), inst.to_device(mask)
        keep.append((f, b0, b, m, dst.shape))
        j.face, j.face_cols, j.face_rows, j.face_step = f, patch.shape[1], patch.shape[0], 3 * patch.shape[1]
        j.body, j.body_cols, j.body_rows, j.body_step = b, dst.shape[1], dst.shape[0], 3 * dst.shape[1]
        j.mask, j.mask_cols, j.mask_rows, j.mask_step = m, mask.shape[1], mask.shape[0], mask.shape[1]
        j.centerX, j.centerY, j.body_restore = cx, cy, b0
    return jobs, keep


def _free_jobs(inst, keep):
    for f, b0, b, m, _ in keep:
        for p in (f, b0, b, m):
            inst.free(p)


def _solo(items, mode):
    from seamlesscloneoptimization_amd import capi
    inst = _new(mode, method=capi.SC_METHOD_MULTIGRID)
    out, cycles = [], []
    try:
        for it in items:
            out.append(_clone(inst, *it)); cycles.append(inst.info().sweeps)
    finally:
        inst.destroy()
    return out, cycles


GROUPS = {"same_size": [(320, 300)] * 4, "size_class": [(300, 310), (318, 333), (336, 305), (325, 337)]}


@pytest.mark.parametrize("kind", list(GROUPS))
def test_group_members_get_their_solo_bytes_under_mixed(kind):
    from seamlesscloneoptimization_amd import capi
    sizes = GROUPS[kind]
    assert set(capi.plan_groups(sizes)[1]) == {1 if kind == "same_size" else 2}
    items = []
    for k, (W, H) in enumerate(sizes):
        dst, patch, mask, cx, cy = _inputs(W, H, seed=70 + 13 * k, ellipse=(k % 2 == 1))
        items.append((dst, patch, mask, cx + k, cy - k))
    alone, cycles = _solo(items, cm.MIXED)
    inst = _new(cm.MIXED, method=capi.SC_METHOD_MULTIGRID)
    try:
        jobs, keep = _device_jobs(inst, items)
        assert inst.run_device_batch(jobs) == 0 and all(j.rc == 0 for j in jobs)
        i = inst.info()
        assert i.group_members == len(items) and i.group_ragged == (kind == "size_class"), (i.group_members, i.group_ragged)
        for k, ((f, b0, b, m, shape), it) in enumerate(zip(keep, items)):
            got = inst.from_device(b, shape)
            assert _dmax(got, cm.seamless_clone(*it, mode=cm.MIXED)) <= 1, k
            assert _dmax(got, alone[k]) <= 1, k
            if cycles[k] == i.sweeps:
                assert np.array_equal(got, alone[k]), (k, int((got != alone[k]).sum()))
        assert i.sweeps >= max(cycles) - 1
        _free_jobs(inst, keep)
    finally:
        inst.destroy()


def test_pool_with_a_clone_mode_gives_the_solo_bytes():
    from seamlesscloneoptimization_amd import capi
    items = [_inputs(W, H, seed=90 + W) for W, H in ((200, 150), (233, 170), (181, 199))]
    alone, _ = _solo(items, cm.MIXED)
    for how in ("setter", "keyword"):
        if how == "setter":
            pool = capi.Pool(0, streams=2, method=capi.SC_METHOD_MULTIGRID)
            pool.set_clone_mode(capi.SC_MIXED_CLONE)
        else:
            pool = capi.Pool(0, streams=2, clone_mode=capi.SC_MIXED_CLONE, method=capi.SC_METHOD_MULTIGRID)
        try:
            assert all(i.clone_mode == capi.SC_MIXED_CLONE for i in pool.instances)
            inst = pool.instances[0]
            jobs, keep = _device_jobs(inst, items)
            pool.run(jobs, device_resident=True)
            for k, (f, b0, b, m, shape) in enumerate(keep):
                assert np.array_equal(inst.from_device(b, shape), alone[k]), (how, k)
            _free_jobs(inst, keep)
            bodies = [it[0].copy() for it in items]
            pool.run_host([(it[1], bd, it[2], it[3], it[4]) for it, bd in zip(items, bodies)])
            for k, bd in enumerate(bodies):
                assert np.array_equal(bd, alone[k]), (how, "host", k)
        finally:
            pool.close()


# ---- default, reset, errors --------------------------------------------------------------------------------------------------------
def test_default_and_reset():
    from seamlesscloneoptimization_amd import capi
    dst, patch, mask, cx, cy = _inputs(150, 120, seed=31)
    fresh = _new()
    inst = _new()
    try:
        assert fresh.clone_mode == capi.SC_NORMAL_CLONE and inst.clone_mode == capi.SC_NORMAL_CLONE
        want = _clone(fresh, dst, patch, mask, cx, cy)
        inst.set_clone_mode(capi.SC_MIXED_CLONE)
        assert inst.clone_mode == capi.SC_MIXED_CLONE
        mixed = _clone(inst, dst, patch, mask, cx, cy)
        assert not np.array_equal(mixed, want)
        inst.set_solver(method=capi.SC_METHOD_AUTO, flags=0)          # set_solver leaves the mode alone
        assert inst.clone_mode == capi.SC_MIXED_CLONE
        assert np.array_equal(_clone(inst, dst, patch, mask, cx, cy), mixed)
        inst.set_clone_mode(capi.SC_NORMAL_CLONE)
        assert np.array_equal(_clone(inst, dst, patch, mask, cx, cy), want)
    finally:
        fresh.destroy(); inst.destroy()


def test_bad_modes_and_grey_mask_combination_are_refused():
    from seamlesscloneoptimization_amd import capi
    dst, patch, mask, cx, cy = _inputs(120, 90, seed=41)
    inst = _new()
    try:
        for bad in (0, 4):
            with pytest.raises(capi.SeamlessCloneError) as e:
                inst.set_clone_mode(bad)
            assert e.value.code == capi.SC_ERR_BAD_ARG
            assert inst.L.sc_hip_set_clone_mode(inst.h, bad) == capi.SC_ERR_BAD_ARG
            assert inst.clone_mode == capi.SC_NORMAL_CLONE
        inst.set_clone_mode(capi.SC_MIXED_CLONE)
        inst.set_solver(flags=capi.SC_FLAG_OPENCV_GREY_MASK)
        body = dst.copy()
        with pytest.raises(capi.SeamlessCloneError):
            inst.run(patch, body, mask, cx, cy)
        assert b"GREY_MASK" in inst.L.sc_hip_last_error(inst.h)
        assert np.array_equal(body, dst)
        jobs, keep = _device_jobs(inst, [(dst, patch, mask, cx, cy)] * 2)
        assert inst.L.sc_hip_run_device_batch(inst.h, jobs, len(jobs)) == capi.SC_ERR_BAD_ARG
        inst.sync()
        assert all(j.rc == capi.SC_ERR_BAD_ARG for j in jobs)
        _free_jobs(inst, keep)
        inst.set_clone_mode(capi.SC_NORMAL_CLONE)            # NORMAL with the grey-mask flag still runs
        assert inst.run(patch, body, mask, cx, cy) == 0
    finally:
        inst.destroy()
    assert capi.load().sc_hip_pool_set_clone_mode(None, 2) == capi.SC_ERR_BAD_ARG


def test_seamless_clone_function_takes_the_cv_flags():
    from seamlesscloneoptimization_amd import capi, seamless_clone
    dst, patch, mask, cx, cy = _inputs(180, 140, seed=51)
    for flags in (cm.MIXED, cm.MONOCHROME):
        got = seamless_clone.seamlessClone(patch, dst, mask, (cx, cy), flags=flags)
        inst = _new(flags)
        try:
            assert np.array_equal(got, _clone(inst, dst, patch, mask, cx, cy))
        finally:
            inst.destroy()
    with pytest.raises(ValueError):
        seamless_clone.seamlessClone(patch, dst, mask, (cx, cy), flags=4)
    sc = seamless_clone.SeamlessClone()
    try:
        sc.setCloneMode(capi.SC_MONOCHROME_TRANSFER)
        body = dst.copy()
        sc.loadMatsInSeamlessClone(patch, body, mask, cx, cy, 0)
        out = sc.seamlessClone()
        assert sc.instance_ptr.clone_mode == capi.SC_MONOCHROME_TRANSFER
        inst = _new(cm.MONOCHROME)
        try:
            assert np.array_equal(out[:, :, :], _clone(inst, dst, patch, mask, cx, cy))
        finally:
            inst.destroy()
    finally:
        sc.destroy()
