"""GPU parity tests added in round 5 (through the C ABI, against the CPU oracle): the scan's completion fence without stage
marks, the host-image call's ROI-only return under concurrent writers, groups of clones with different ROI sizes."""
import os
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def oracles():
    from oracle import oracle_np, oracle_c
    oracle_c.build()
    return oracle_np, oracle_c


@pytest.fixture()
def inst():
    """A fresh instance with the library's DEFAULT options (the session fixture `hip` is pinned to multigrid)."""
    from seamlesscloneoptimization_amd import capi
    i = capi.Instance(0)
    yield i
    i.destroy()


def _dmax(a, b):
    return int(np.abs(a.astype(np.int16) - b.astype(np.int16)).max())


@pytest.mark.parametrize("flags_name", ["NO_STAGE_MARKS", "NO_STAGE_MARKS|ROWS_RETURN", "default"])
def test_changed_mask_without_stage_marks_is_noticed(inst, oracles, flags_name):
    """with SC_FLAG_NO_STAGE_MARKS the host-image call used stage mark 5 -- which that flag never records --
    as the completion fence of the bounding-box scan that rides in the pre-process launch; the wait returned at once, the
    comparison read the PREVIOUS call's rectangle, which equals the remembered guess, and a call whose mask had changed at the
    same size returned SC_OK with nothing cloned (the direct solve has no other host wait before that point).  The fence is an
    event of its own now.  AUTO on a 300 x 200 mask = the direct FFT solve; every call must match the oracle on ITS mask and
    report ITS geometry."""
    from seamlesscloneoptimization_amd import capi
    o, _ = oracles
    flags = {"NO_STAGE_MARKS": capi.SC_FLAG_NO_STAGE_MARKS, "NO_STAGE_MARKS|ROWS_RETURN": capi.SC_FLAG_NO_STAGE_MARKS | capi.SC_FLAG_ROWS_RETURN,
             "default": 0}[flags_name]
    inst.set_solver(flags=flags)
    rng = np.random.default_rng(11)
    H, W = 200, 300
    dst = rng.integers(0, 256, (H + 60, W + 60, 3), dtype=np.uint8)
    patch = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    full = np.full((H, W), 255, np.uint8)
    blob = np.zeros((H, W), np.uint8); blob[30:170, 40:220] = 255
    other = np.zeros((H, W), np.uint8); other[60:190, 100:290] = 255
    cx, cy = (W + 60) // 2, (H + 60) // 2
    for k, m in enumerate([full, full, blob, blob, other, full, other, other, blob]):
        want = o.seamless_clone(dst, patch, m, cx, cy, float_tables=True)
        body = dst.copy()
        assert inst.run(patch, body, m, cx, cy) == 0
        i = inst.info()
        assert i.method == capi.SC_METHOD_FFT
        ys, xs = np.nonzero(m[1:-1, 1:-1])
        assert (i.x0, i.y0, i.W, i.H) == (xs.min() + 1, ys.min() + 1, xs.max() - xs.min() + 1, ys.max() - ys.min() + 1), k
        assert _dmax(want, body) <= 1, k
        assert not np.array_equal(body, dst), k


def test_two_host_calls_into_disjoint_rois_of_one_destination(oracles):
    """the default return of the host-image call writes ROI bytes only (as the reference's splice does,
    seamlessClone_imp.cpp:470-483), so two calls that clone into disjoint column ranges of ONE destination at the same time --
    two threads with an instance each, and two host jobs of one pool -- both keep their result.  (Late round 4's default wrote
    whole rows back: the later call erased the earlier one's ROI.)"""
    from seamlesscloneoptimization_amd import capi
    o, oc = oracles
    rng = np.random.default_rng(3)
    Hd, Wd = 700, 1500                        # the two ROIs cover most of a row together, so each would qualify for the row return alone
    dst = rng.integers(0, 256, (Hd, Wd, 3), dtype=np.uint8)
    pa = rng.integers(0, 256, (640, 700, 3), dtype=np.uint8)
    pb = rng.integers(0, 256, (640, 700, 3), dtype=np.uint8)
    mask = np.full((640, 700), 255, np.uint8)
    ca, cb = (370, 350), (1120, 350)
    want = oc.seamless_clone(dst, pa, mask, ca[0], ca[1], min(16, oc.max_threads()))
    want = oc.seamless_clone(want, pb, mask, cb[0], cb[1], min(16, oc.max_threads()))      # disjoint ROIs: the order does not matter
    # (a) two threads, one instance each
    for rep in range(3):
        body = dst.copy()
        insts = [capi.Instance(0), capi.Instance(0)]
        try:
            bar = threading.Barrier(2)
            rcs = [None, None]

            def work(k, patch, c):
                bar.wait()
                rcs[k] = insts[k].run(patch, body, mask, c[0], c[1])
            th = [threading.Thread(target=work, args=(0, pa, ca)), threading.Thread(target=work, args=(1, pb, cb))]
            for t in th: t.start()
            for t in th: t.join()
        finally:
            for i in insts: i.destroy()
        assert rcs == [0, 0]
        assert _dmax(want, body) <= 1, rep
    # (b) two host jobs of one pool sharing the destination
    pool = capi.Pool(0, streams=2)
    try:
        body = dst.copy()
        pool.run_host([(pa, body, mask, ca[0], ca[1]), (pb, body, mask, cb[0], cb[1])])
        assert _dmax(want, body) <= 1
    finally:
        pool.close()


def _device_jobs(inst, items):
    """(dst, patch, mask, cx, cy) -> device-resident sc_batch_jobs on `inst` (bodies refreshed from a pristine copy by every call)."""
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


def _solo_results(items):
    """Every item alone through the multigrid path (what a group member must reproduce): bodies and cycle counts."""
    from seamlesscloneoptimization_amd import capi
    seq = capi.Instance(0)
    seq.set_solver(method=capi.SC_METHOD_MULTIGRID)
    alone, cycles = [], []
    try:
        for dst, patch, mask, cx, cy in items:
            b = dst.copy(); seq.run(patch, b, mask, cx, cy); alone.append(b); cycles.append(seq.info().sweeps)
    finally:
        seq.destroy()
    return alone, cycles


SIZE_CLASSES = {
    # five sizes whose hierarchies end alike (level 2 in k_mg_tail, a 37..42-wide level solved directly at padding 64)
    "300s": [(300, 310), (318, 333), (336, 305), (325, 337), (307, 322), (318, 333)],
    # 1000..1027: level 3 (<= 127 unknowns) in k_mg_tail, a 61..63-wide level solved directly
    "1000s": [(1003, 1010), (1020, 1001), (1012, 1024), (1025, 1025)],
    # above 1027 per side the hierarchy is one level deeper (33 x 33 solved directly at padding 64)
    "1100s": [(1078, 1090), (1099, 1080), (1085, 1075), (1092, 1099)],
    # one side below, one above that boundary (31 x 32 solved directly at padding 32)
    "mixed_depth": [(1010, 1060), (1022, 1065), (1001, 1033)],
    # BASELINE config 3's size and two neighbours
    "2048s": [(2048, 2048), (2000, 2040), (1990, 2050)],
    # the reference's own small patches (154 x 100; its size sets 109 x 164, 181 x 153): level 2 in k_mg_tail, alone and in a class
    "150s": [(154, 160), (150, 171), (165, 158), (158, 164), (161, 152)],
    # ROIs of at most ~130 pixels: a solo clone solves their level 1 directly (64 x 64 on the matrix cores), a class runs the general
    # hierarchy -- within one grey level of the solo run, not its bytes (plan_size: solo_differs)
    "110s": [(104, 118), (110, 99), (126, 112), (98, 121), (115, 107)],
    # across 2050 unknowns per side the float-table correction keeps 40 instead of 32 modes (mode-block padding 64 / 32) and the
    # directly solved level flips between 32 and 33 unknowns at ~2110 (operand padding 32 / 64): all four combinations in one class
    "2100s": [(2040, 2100), (2140, 2120), (2085, 2170), (2200, 2060), (2190, 2195)],
    # sizes whose float tables are off by more than 4 % in their lowest modes (plan_size: conditional): the output's form is decided by
    # the judged cycle's measured update, for the whole group (smooth inputs: the same way as in each solo run)
    "2100c": [(2107, 2053), (2137, 2072), (2132, 2077), (2120, 2064)],
    # the first member's hierarchy is one level shallower than the others' (both sides below 1027): the leftover of its class, it is
    # moved onto theirs (plan_groups kind 3: within one grey level of its solo run, the others keep their solo bytes)
    "straddle": [(1010, 1015), (1050, 1060), (1070, 1040), (1090, 1080)],
}
EXPECTED_KINDS = {"110s": [3] * 5, "straddle": [3, 2, 2, 2]}


def test_size_classes_are_what_the_tests_think_they_are():
    """(host arithmetic only, but it guards the GPU tests below: each list must be ONE size class)"""
    from seamlesscloneoptimization_amd import capi
    for name, sizes in SIZE_CLASSES.items():
        g, k = capi.plan_groups(sizes)
        assert set(g) == {0} and k == EXPECTED_KINDS.get(name, [2] * len(sizes)), (name, g, k)
        assert all(capi.plan_size(*sz)["conditional"] == (name == "2100c") for sz in sizes), name
    # a conditional size never shares a class with one whose bound holds a priori
    g, k = capi.plan_groups([(2107, 2053), (2090, 2050), (2137, 2072), (2090, 2055)])
    assert g[0] == g[2] and g[1] == g[3] and g[0] != g[1] and set(k) == {2}, (g, k)


@pytest.mark.parametrize("name", list(SIZE_CLASSES))
def test_size_class_members_match_their_solo_runs(oracles, name):
    """Round 5, size classes (csrc/sc_ragged.cpp): clones of DIFFERENT ROI sizes whose solves are the same program share one set of
    launches through a per-member geometry table.  Every member must come out with the bytes of its solo run whenever the group
    took the cycle count the solo run took (the stop rule sees the group's largest correction), within one grey level of the
    float-table port always, and the call must really have shared its launches (sc_run_info.group_members / group_ragged)."""
    from seamlesscloneoptimization_amd import capi
    o, oc = oracles
    sizes = SIZE_CLASSES[name]
    kinds = capi.plan_groups(sizes)[1]
    items = []
    for k, (W, H) in enumerate(sizes):
        dst, patch, mask, cx, cy = o.synth_inputs(W, H, seed_dst=500 + 7 * k, seed_patch=600 + 11 * k, margin=40)
        if k == 1:                                           # holes in one member's mask (its bounding box stays the interior)
            mask = mask.copy(); mask[H // 3:H // 3 + 25, W // 4:W // 4 + 90] = 0
        items.append((dst, patch, mask, cx + 2 * k - 3, cy - k))
    alone, cycles = _solo_results(items)
    inst = capi.Instance(0)                                  # library defaults: a group takes the cycles at every size
    try:
        jobs, keep = _device_jobs(inst, items)
        for rep in range(2):                                 # twice: the second call re-uses every buffer of the first
            assert inst.run_device_batch(jobs) == 0 and all(j.rc == 0 for j in jobs)
            inst.sync()
            i = inst.info()
            assert i.group_members == len(items) and i.group_ragged == 1, (i.group_members, i.group_ragged)
            assert i.W == max(w for w, _ in sizes) and i.H == max(h for _, h in sizes)
            group_cycles = i.sweeps
            assert group_cycles >= max(cycles) - 1
            for k, ((f, b0, b, m, shape), it) in enumerate(zip(keep, items)):
                got = inst.from_device(b, shape)
                want = oc.seamless_clone(it[0], it[1], it[2], it[3], it[4], nthreads=min(16, oc.max_threads()), exact_den=False)
                assert _dmax(got, want) <= 1, (name, k, rep)
                assert not np.array_equal(got, it[0])
                assert _dmax(got, alone[k]) <= 1, (name, k, rep)
                if cycles[k] == group_cycles and kinds[k] == 2:
                    assert np.array_equal(got, alone[k]), (name, k, rep, int((got != alone[k]).sum()))
        # the same members in another order, one of them twice: the table is per slot, not per size
        order = [2, 0, 1, 0] if len(items) >= 3 else [1, 0]
        jobs2, keep2 = _device_jobs(inst, [items[q] for q in order])
        assert inst.run_device_batch(jobs2) == 0
        inst.sync()
        assert inst.info().group_members == len(order)
        if inst.info().sweeps == group_cycles:
            for (f, b0, b, m, shape), q in zip(keep2, order):
                if cycles[q] == group_cycles and kinds[q] == 2 and name != "straddle":
                    assert np.array_equal(inst.from_device(b, shape), alone[q]), (name, q)
        _free_jobs(inst, keep); _free_jobs(inst, keep2)
    finally:
        inst.destroy()


def test_mixed_batch_is_partitioned_into_classes_groups_and_singles(oracles):
    """One call with members of two size classes, a same-size pair, a size that fits nothing and a member whose ROI leaves its
    destination: every usable member gets the bytes of its solo run (same cycle counts) or is within one of it, the failing member
    reports its own error and nobody else is affected."""
    from seamlesscloneoptimization_amd import capi
    o, oc = oracles
    sizes = [(300, 310), (1003, 1010), (318, 333), (640, 480), (1020, 1001), (640, 480), (90, 70), (340, 305), (1012, 1024)]
    items = [o.synth_inputs(W, H, seed_dst=40 + k, seed_patch=90 + k, margin=36) for k, (W, H) in enumerate(sizes)]
    alone, cycles = _solo_results(items)
    inst = capi.Instance(0)
    try:
        jobs, keep = _device_jobs(inst, items)
        assert inst.run_device_batch(jobs) == 0 and all(j.rc == 0 for j in jobs)
        inst.sync()
        for k, ((f, b0, b, m, shape), it) in enumerate(zip(keep, items)):
            got = inst.from_device(b, shape)
            if _dmax(got, alone[k]) > 1:                     # say WHICH of the two is off, and where (seen once in a full-suite run, never alone)
                want = oc.seamless_clone(it[0], it[1], it[2], it[3], it[4], nthreads=min(16, oc.max_threads()), exact_den=False)
                d = np.abs(got.astype(np.int16) - alone[k].astype(np.int16)).max(axis=2)
                ys, xs = np.nonzero(d > 1)
                raise AssertionError("member %d %s: batch vs alone differ in %d pixels (box x %d..%d y %d..%d of %s); batch vs port max %d, alone vs port max %d, "
                                     "batch == untouched destination there: %s" % (k, sizes[k], len(ys), xs.min(), xs.max(), ys.min(), ys.max(), got.shape,
                                     _dmax(got, want), _dmax(alone[k], want), bool(np.array_equal(got[ys, xs], it[0][ys, xs]))))
            assert not np.array_equal(got, it[0]), k
        jobs[4].centerX = 2                                  # its ROI leaves the destination
        rc = inst.L.sc_hip_run_device_batch(inst.h, jobs, len(jobs))
        inst.sync()
        assert rc == capi.SC_ERR_ROI_OOB and jobs[4].rc == capi.SC_ERR_ROI_OOB
        assert all(j.rc == 0 for q, j in enumerate(jobs) if q != 4)
        for k, ((f, b0, b, m, shape), it) in enumerate(zip(keep, items)):
            if k != 4:
                assert _dmax(inst.from_device(b, shape), alone[k]) <= 1, k
        _free_jobs(inst, keep)
    finally:
        inst.destroy()


def test_pool_buckets_48_random_sizes(oracles):
    """The review's test of round 5's first item: 48 random ROI sizes in [1000, 1100]^2 and 48 in [300, 340]^2 through the pool
    (groups of 16): every member within one grey level of the float-table port AND of its solo run, byte-identical to the latter
    wherever the member's group took the solo run's cycle count -- which the pool cannot report per member, so: identical on at
    least 90 % of the members that kept their own hierarchy (plan_groups kind 2; the few leftovers moved onto a deeper one are kind 3) (tests/tools/fuzz_classes.py makes the exact comparison: 192 of 192)."""
    from seamlesscloneoptimization_amd import capi
    o, oc = oracles
    rng = np.random.default_rng(2025)
    for lo, hi in ((300, 340), (1000, 1100)):
        sizes = [(int(rng.integers(lo, hi + 1)), int(rng.integers(lo, hi + 1))) for _ in range(48)]
        base = {}
        items = []
        for k, (W, H) in enumerate(sizes):                   # two image pairs per range, cropped: synthesising 48 is the slow part
            key = k & 1
            if key not in base:
                base[key] = o.synth_inputs(hi, hi, seed_dst=7 + key, seed_patch=17 + key, margin=40)
            dst, patch, mask, cx, cy = base[key]
            items.append((dst, np.ascontiguousarray(patch[:H + 2, :W + 2]), np.full((H + 2, W + 2), 255, np.uint8), cx, cy))
        alone, cycles = _solo_results(items)
        kinds = capi.plan_groups(sizes, 16)[1]                # what the pool does with these sizes (the same planner)
        assert all(kk in (2, 3) for kk in kinds) and sum(kk == 3 for kk in kinds) <= 8, kinds
        pool = capi.Pool(0, streams=2, group=16)
        try:
            inst = pool.instances[0]
            jobs, keep = _device_jobs(inst, items)
            pool.run(jobs, device_resident=True)
            same = 0
            for k, ((f, b0, b, m, shape), it) in enumerate(zip(keep, items)):
                got = inst.from_device(b, shape)
                assert _dmax(got, alone[k]) <= 1, (lo, k, sizes[k])
                want = oc.seamless_clone(it[0], it[1], it[2], it[3], it[4], nthreads=min(16, oc.max_threads()), exact_den=False)
                assert _dmax(got, want) <= 1, (lo, k, sizes[k])
                assert not np.array_equal(got, it[0])
                same += int(kinds[k] == 2 and np.array_equal(got, alone[k]))
            assert same >= 0.9 * sum(kk == 2 for kk in kinds), (lo, same)
            _free_jobs(inst, keep)
        finally:
            pool.close()


def test_fft_lengths_with_odd_factors_every_7th_size(inst, oracles):
    """Round 5: SC_METHOD_FFT's circular convolution takes the shortest length M = r 2^k >= 2n - 1 with r in {1, 3, 5} (one 3- or
    5-point register pass in front of the power-of-two passes; powers of two only until then: up to 2x the work).  Field-level check
    against the C port's direct solve (double transforms) for every n = 5, 12, 19, ... 2098 unknowns along x (7 along y) and every
    third of those along y.  Each precision meets both its earlier bound (float32 transforms: 1e-2 scaled by the field's magnitude,
    double transforms (SC_FLAG_FFT_FP64) 1e-4) and tests/test_gpu_direct_lengths.py's: float32 within 4x the port's own float32
    transforms on the same input (scaled, floor F32_FLOOR), double within F64_ULPS float32 ulps of max|want|."""
    from seamlesscloneoptimization_amd import capi
    from test_gpu_direct_lengths import F32_FACTOR, F32_FLOOR, F64_ULPS
    _, oc = oracles
    rng = np.random.default_rng(77)
    lens = set()
    worst = {0: 0.0, capi.SC_FLAG_FFT_FP64: 0.0}
    fails = []
    for idx, n in enumerate(range(5, 2101, 7)):
        shapes = [(n + 2, 9)] + ([(9, n + 2)] if idx % 3 == 0 else [])
        for W, H in shapes:
            B = rng.integers(0, 256, (3, H, W)).astype(np.float32)
            lap = np.zeros((3, H, W), np.float32)
            lap[:, 1:-1, 1:-1] = rng.integers(-600, 601, (3, H - 2, W - 2)).astype(np.float32)
            g = oc.fold(B, lap)
            want = oc.solve_dst(g, 1, exact_den=False)
            top = float(np.abs(want).max())
            scale = max(1.0, top / 500.0)
            e32 = float(np.abs(oc.solve_dst(g, 1, exact_den=False, internals="f32") - want).max()) / scale
            for flags in (0, capi.SC_FLAG_FFT_FP64):
                inst.set_solver(method=capi.SC_METHOD_FFT, flags=flags)
                inst.field_load(B, lap)
                inst.field_solve()
                got = inst.field_store()
                d = float(np.abs(got[:, 1:-1, 1:-1] - want).max())
                err = d / scale
                if flags:
                    ok = err < 1e-4 and d <= F64_ULPS * float(np.spacing(np.float32(top)))
                else:
                    ok = err < 1e-2 and err <= max(F32_FACTOR * e32, F32_FLOOR)
                worst[flags] = max(worst[flags], d / float(np.spacing(np.float32(top))) if flags else err)
                if not ok:
                    fails.append((W, H, flags, d, e32))
        need = 2 * n - 1
        M = 2
        while M < need:
            M *= 2
        for r in (3, 5):
            k = 4
            while (r << k) < M:
                if (r << k) >= need:
                    M = r << k
                    break
                k += 1
        lens.add(M)
    assert any(m % 3 == 0 for m in lens) and any(m % 5 == 0 for m in lens) and any(m & (m - 1) == 0 for m in lens)
    print("worst error: float32 %.2e (scaled), double %.2f float32 ulps over %d lengths" % (worst[0], worst[capi.SC_FLAG_FFT_FP64], len(lens)))
    assert not fails, fails


def test_saturating_member_of_a_size_class_repeats_the_class_on_float_fields(oracles):
    """The 16-bit field's range check (round 4) inside a size class: one member (rings of inward ramps: a non-conservative guidance
    field) saturates -> nobody is written by the first solve, the class runs again on float fields -- the table-reading forms of the
    float-field launches -- and every member is within one of the port; the ordinary members get the bytes SC_FLAG_FLOAT_FIELD
    gives them alone (same cycle counts)."""
    from seamlesscloneoptimization_amd import capi
    from test_gpu_round4 import ring_ramp_inputs
    o, oc = oracles
    items = [o.synth_inputs(640, 560, margin=32, seed_dst=11, seed_patch=12), ring_ramp_inputs(652, 571), o.synth_inputs(625, 583, margin=32, seed_dst=13, seed_patch=14)]
    g, k = capi.plan_groups([(640, 560), (652, 571), (625, 583)])
    assert set(g) == {0} and set(k) == {2}
    inst = capi.Instance(0)
    solo = capi.Instance(0)
    try:
        solo.set_solver(method=capi.SC_METHOD_MULTIGRID, flags=capi.SC_FLAG_FLOAT_FIELD)
        jobs, keep = _device_jobs(inst, items)
        assert inst.run_device_batch(jobs, ) in (0, capi.SC_ERR_NOT_CONVERGED)
        i = inst.info()
        assert i.field_retry == 1 and i.group_ragged == 1 and i.group_members == 3
        for k_, ((f, b0, b, m, shape), it) in enumerate(zip(keep, items)):
            got = inst.from_device(b, shape)
            want = oc.seamless_clone(it[0], it[1], it[2], it[3], it[4], min(16, oc.max_threads()))
            assert _dmax(got, want) <= 1, k_
            if k_ != 1:
                body = it[0].copy()
                solo.run(it[1], body, it[2], it[3], it[4], allow_not_converged=True)
                if solo.info().sweeps == i.sweeps:
                    assert np.array_equal(body, got), k_
        _free_jobs(inst, keep)
    finally:
        inst.destroy(); solo.destroy()


def test_both_clis_dump_the_reference_intermediates(tmp_path, golden_dir, c1_inputs, oracles):
    """VERDICT round 4, missing 3: the second half of the reference's compare/vs.py workflow (vs.py:12-34, 81-86) from the command
    line.  The reference's SCDEBUG build dumps ucMask0.yml and g{0,1,2}.yml (seamlessClone_imp.cpp:2110-2117); `cli.py --dump-rhs DIR`
    and the native CLI's 9th argument write the same files.  Checked on the reference's own inputs: the mask and the three planes
    bit-exact against the C oracle (planes in the reference's R, G, B order), the two CLIs identical to each other, and
    compare.rhs_diff_bgr_vs_rgb_planes -- vs.py's sum of absolute differences against OpenCV's mod_diff{2,1,0} -- zero."""
    import gzip, shutil, subprocess
    from seamlesscloneoptimization_amd import capi, cli, compare, ymlio
    _, oc = oracles
    for n in ("src.yml", "src_mask.yml"):
        with gzip.open(os.path.join(golden_dir, n + ".gz"), "rb") as f, open(tmp_path / n, "wb") as g:
            shutil.copyfileobj(f, g)
    ymlio.write_yml(tmp_path / "dst.yml", c1_inputs["dst"], name="dst")
    py_dir, cc_dir = tmp_path / "py", tmp_path / "cc"
    cc_dir.mkdir()
    args = [str(tmp_path / "src.yml"), str(tmp_path / "dst.yml"), str(tmp_path / "src_mask.yml"), "800", "150", "0"]
    assert cli.main(args + ["--dump-rhs", str(py_dir)]) == 0
    exe = os.path.join(os.path.dirname(capi.LIB_PATH), "seamlessClone_main")
    r = subprocess.run([exe] + args + [str(tmp_path / "o.bmp"), "auto", str(cc_dir)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "g2.yml" in r.stdout, (r.stdout[-500:], r.stderr[-500:])
    geo, M = oc.mask_stage(c1_inputs["mask"], 800, 150)
    B, lap = oc.build_rhs(c1_inputs["dst"], c1_inputs["patch"], geo, M)
    g_bgr = oc.fold(B, lap)                                      # [3][190][296], planes B, G, R
    for d in (py_dir, cc_dir):
        assert np.array_equal(ymlio.read_yml(str(d / "ucMask0.yml")), M), d
        planes = [ymlio.read_yml(str(d / ("g%d.yml" % ch))) for ch in range(3)]
        assert all(p.dtype == np.float32 and p.shape == (190, 296) for p in planes)
        for ch in range(3):
            assert np.array_equal(planes[ch], g_bgr[2 - ch]), (d, ch)
        assert compare.rhs_diff_bgr_vs_rgb_planes([g_bgr[0], g_bgr[1], g_bgr[2]], planes) == [0.0, 0.0, 0.0]
    bad = subprocess.run([exe] + args + [str(tmp_path / "o.bmp"), "auto", str(tmp_path / "no_such_dir")], capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0 and "cannot write the intermediates" in bad.stderr


def test_one_call_with_more_members_than_a_job_table_holds(oracles):
    """The kernels that take their per-member jobs by value hold 16 (MaskJobs / ImageJobs / CopyJobs) and are launched in slices; the
    size class's own table has no such limit.  27 members of one class (sizes in [250, 500]^2: up to 2x apart) in ONE
    sc_hip_run_device_batch call: all share the launches, every member within one grey level of the port and with the bytes of its
    solo run where the cycle counts agree."""
    from seamlesscloneoptimization_amd import capi
    o, oc = oracles
    rng = np.random.default_rng(31)
    sizes = [(int(rng.integers(250, 501)), int(rng.integers(250, 501))) for _ in range(27)]
    g, kinds = capi.plan_groups(sizes)
    assert set(g) == {0} and set(kinds) == {2}, (g, kinds)
    items = []
    for k, (W, H) in enumerate(sizes):
        dst, patch, mask, cx, cy = o.synth_inputs(W, H, seed_dst=900 + k, seed_patch=950 + k, margin=30)
        items.append((dst, patch, mask, cx + (k % 5) - 2, cy - (k % 3)))
    alone, cycles = _solo_results(items)
    inst = capi.Instance(0)
    try:
        jobs, keep = _device_jobs(inst, items)
        assert inst.run_device_batch(jobs) == 0 and all(j.rc == 0 for j in jobs)
        inst.sync()
        i = inst.info()
        assert i.group_members == 27 and i.group_ragged == 1
        same = 0
        for k, ((f, b0, b, m, shape), it) in enumerate(zip(keep, items)):
            got = inst.from_device(b, shape)
            want = oc.seamless_clone(it[0], it[1], it[2], it[3], it[4], nthreads=min(16, oc.max_threads()), exact_den=False)
            assert _dmax(got, want) <= 1, k
            assert not np.array_equal(got, it[0])
            if cycles[k] == i.sweeps:
                assert np.array_equal(got, alone[k]), (k, sizes[k], int((got != alone[k]).sum()))
                same += 1
        assert same >= 20, same
        _free_jobs(inst, keep)
    finally:
        inst.destroy()


def test_size_class_without_speculation_and_with_a_member_guessed_wrong(oracles):
    """A size class the two other ways a group can be launched: (a) SC_FLAG_NO_SPECULATE -- the call waits for the device's bounding
    boxes before it plans -- gives every member the bytes of the default (speculative) call; (b) a member whose mask does not fill
    its image (bounding box smaller than the mask's interior: the predicted box is wrong) is left untouched by the class's splice
    and repeated alone on its true box, the other members keep their bytes."""
    from seamlesscloneoptimization_amd import capi
    o, oc = oracles
    sizes = SIZE_CLASSES["300s"][:5]
    items = [o.synth_inputs(W, H, seed_dst=700 + k, seed_patch=720 + k, margin=40) for k, (W, H) in enumerate(sizes)]
    inst = capi.Instance(0)
    try:
        jobs, keep = _device_jobs(inst, items)
        assert inst.run_device_batch(jobs) == 0
        inst.sync()
        assert inst.info().group_members == 5 and inst.info().group_ragged == 1
        base = [inst.from_device(b, shape) for (f, b0, b, m, shape) in keep]
        inst.set_solver(flags=capi.SC_FLAG_NO_SPECULATE)
        assert inst.run_device_batch(jobs) == 0
        inst.sync()
        assert inst.info().group_members == 5 and inst.info().group_ragged == 1
        for k, (f, b0, b, m, shape) in enumerate(keep):
            assert np.array_equal(inst.from_device(b, shape), base[k]), k
        inst.set_solver(flags=0)
        # (b) member 2's mask loses rows at the top and columns at the right
        odd = list(items[2]); m_odd = odd[2].copy(); m_odd[:9, :] = 0; m_odd[:, -13:] = 0; odd[2] = m_odd
        items_b = items[:2] + [tuple(odd)] + items[3:]
        jobs_b, keep_b = _device_jobs(inst, items_b)
        assert inst.run_device_batch(jobs_b) == 0 and all(j.rc == 0 for j in jobs_b)
        inst.sync()
        for k, ((f, b0, b, m, shape), it) in enumerate(zip(keep_b, items_b)):
            got = inst.from_device(b, shape)
            want = oc.seamless_clone(it[0], it[1], it[2], it[3], it[4], nthreads=min(16, oc.max_threads()), exact_den=False)
            assert _dmax(got, want) <= 1, k
            assert not np.array_equal(got, it[0]), k
            if k != 2:
                assert _dmax(got, base[k]) <= 1, k
        _free_jobs(inst, keep); _free_jobs(inst, keep_b)
    finally:
        inst.destroy()


@pytest.mark.parametrize("W,H", [(154, 100), (300, 194), (420, 300), (592, 592), (900, 700)])
def test_small_host_call_paths_give_the_ordinary_bytes(oracles, W, H):
    """Round 5, late: a host-image call whose inputs total at most 1 MB packs mask, patch ROI and destination ROI into one pinned block
    that a kernel reads across PCIe (one upload), and an output of at most 2 MB is written by the output launch straight into pinned
    memory (no device-to-host copy command).  Both need nothing but a predicted box; SC_FLAG_NO_SPECULATE takes the ordinary path
    (three uploads) -- the bytes must be the same, for a patch inside a much larger destination, a strided view of one, and a mask
    whose box is not its interior (the first call's guess is wrong: the ROI uploads are repeated the ordinary way)."""
    from seamlesscloneoptimization_amd import capi
    o, oc = oracles
    dst, patch, mask, cx, cy = o.synth_inputs(W, H, seed_dst=41, seed_patch=42, margin=180)
    big = np.zeros((dst.shape[0] + 7, dst.shape[1] + 13, 3), np.uint8)
    big[3:3 + dst.shape[0], 5:5 + dst.shape[1]] = dst
    m_odd = mask.copy(); m_odd[:7, :] = 0; m_odd[:, -11:] = 0
    want = oc.seamless_clone(dst, patch, mask, cx, cy, nthreads=min(16, oc.max_threads()), exact_den=False)
    want_odd = oc.seamless_clone(dst, patch, m_odd, cx, cy, nthreads=min(16, oc.max_threads()), exact_den=False)
    results = {}
    for name, flags in (("default", 0), ("ordinary", capi.SC_FLAG_NO_SPECULATE)):
        inst = capi.Instance(0)
        try:
            inst.set_solver(flags=flags)
            outs = []
            for rep in range(2):                              # (the second call predicts the first call's box)
                body = dst.copy(); inst.run(patch, body, mask, cx, cy); outs.append(body)
            view = big.copy()
            inst.run(patch, view[3:3 + dst.shape[0], 5:5 + dst.shape[1]], mask, cx, cy)
            outs.append(view)
            body = dst.copy(); inst.run(patch, body, m_odd, cx, cy); outs.append(body)     # predicted: the full mask's box -- wrong
            body = dst.copy(); inst.run(patch, body, m_odd, cx, cy); outs.append(body)     # predicted right
            results[name] = outs
        finally:
            inst.destroy()
    for a, b in zip(results["default"], results["ordinary"]):
        assert np.array_equal(a, b)
    d = results["default"]
    assert np.array_equal(d[0], d[1]) and _dmax(d[0], want) <= 1 and not np.array_equal(d[0], dst)
    assert np.array_equal(d[2][3:3 + dst.shape[0], 5:5 + dst.shape[1]], d[0])
    frame = d[2].copy(); frame[3:3 + dst.shape[0], 5:5 + dst.shape[1]] = 0
    assert not frame.any()                                    # nothing outside the view was touched
    assert np.array_equal(d[3], d[4]) and _dmax(d[3], want_odd) <= 1


def test_pool_with_automatic_group_sizes(oracles):
    """SC_POOL_GROUP_AUTO: 48 clones of 48 different small sizes on two streams go out as two groups of 24 (sc_hip_plan_groups_pool
    says so in advance), every member within one grey level of the port and with the bytes the pool gives it in groups of 16 wherever
    both runs took the same cycle count (same class, same hierarchy: the group's size does not enter the arithmetic)."""
    from seamlesscloneoptimization_amd import capi
    from collections import Counter
    o, oc = oracles
    rng = np.random.default_rng(77)
    sizes = [(int(rng.integers(140, 200)), int(rng.integers(140, 200))) for _ in range(48)]
    g, k = capi.plan_groups_pool(sizes, capi.SC_POOL_GROUP_AUTO, 2)
    assert sorted(Counter(g).values()) == [24, 24] and set(k) == {2}
    base = o.synth_inputs(200, 200, seed_dst=5, seed_patch=6, margin=30)
    items = [(base[0], np.ascontiguousarray(base[1][:H + 2, :W + 2]), np.full((H + 2, W + 2), 255, np.uint8), base[3], base[4]) for W, H in sizes]
    outs = {}
    for group in (16, capi.SC_POOL_GROUP_AUTO):
        pool = capi.Pool(0, streams=2, group=group)
        try:
            inst = pool.instances[0]
            jobs, keep = _device_jobs(inst, items)
            pool.run(jobs, device_resident=True)
            outs[group] = [inst.from_device(b, shape) for (f, b0, b, m, shape) in keep]
            if group == capi.SC_POOL_GROUP_AUTO:
                assert max(i.info().group_members for i in pool.instances) == 24
            _free_jobs(inst, keep)
        finally:
            pool.close()
    same = 0
    for k_, it in enumerate(items):
        got = outs[capi.SC_POOL_GROUP_AUTO][k_]
        want = oc.seamless_clone(it[0], it[1], it[2], it[3], it[4], nthreads=min(16, oc.max_threads()), exact_den=False)
        assert _dmax(got, want) <= 1 and _dmax(got, outs[16][k_]) <= 1, k_
        same += int(np.array_equal(got, outs[16][k_]))
    assert same >= 40, same


@pytest.mark.parametrize("W,H,method", [(200, 120, "fft"), (900, 520, "mg"), (900, 520, "mg_keep_field")])
def test_output_rows_at_every_alignment(oracles, W, H, method):
    """The output launches write words where a row's bytes are word aligned and single bytes around them (store_run, late round 5:
    three of four ROI positions leave 3 x column odd).  Every alignment: eight consecutive ROI columns in a destination whose row
    step is NOT a multiple of four (1601 pixels: the alignment also changes from row to row) and in one whose step is -- through the
    post-process launch (direct solve; multigrid keeping its field) and the planar splice (multigrid default): within one of the
    port, the ring and everything outside the ROI untouched."""
    from seamlesscloneoptimization_amd import capi
    o, oc = oracles
    flags = capi.SC_FLAG_KEEP_FIELD if method == "mg_keep_field" else 0
    meth = capi.SC_METHOD_FFT if method == "fft" else capi.SC_METHOD_MULTIGRID
    rng = np.random.default_rng(W + H)
    inst = capi.Instance(0)
    try:
        inst.set_solver(method=meth, flags=flags)
        for Wd in (1601, 1600):
            Hd = H + 60
            dst = np.clip(128.0 + rng.normal(0.0, 20.0, (Hd, Wd, 3)), 0, 255).astype(np.uint8)
            patch = np.clip(100.0 + rng.normal(0.0, 25.0, (H + 2, W + 2, 3)), 0, 255).astype(np.uint8)
            mask = np.full((H + 2, W + 2), 255, np.uint8)
            f, m = inst.to_device(patch), inst.to_device(mask)
            for shift in range(8):
                cx, cy = Wd // 2 - 300 + shift, Hd // 2
                want = oc.seamless_clone(dst, patch, mask, cx, cy, nthreads=min(16, oc.max_threads()), exact_den=False)
                b = inst.to_device(dst)
                inst.run_device(f, patch.shape, b, dst.shape, m, mask.shape, cx, cy)
                got = inst.from_device(b, dst.shape)
                inst.free(b)
                assert _dmax(got, want) <= 1, (Wd, shift, int(np.count_nonzero(np.abs(got.astype(np.int16) - want.astype(np.int16)) > 1)))
                changed = np.nonzero((got != dst).any(axis=2))
                assert len(changed[0]) > 0.9 * W * H
                x0 = cx - (W + 2) // 2
                assert changed[1].min() >= x0 + 1 and changed[1].max() <= x0 + W, (Wd, shift, int(changed[1].min()), int(changed[1].max()), x0)
            inst.free(f); inst.free(m)
    finally:
        inst.destroy()


def test_poisoned_arena_gives_the_same_bytes(oracles):
    """"Zero only what is read before it is written" (round 5's arena) put to the test: with SC_FLAG_POISON_ARENA every device block
    the arena hands out unzeroed is filled with 0xFF bytes (NaN as float32 / float16) and fresh pinned staging with 0x5A -- what
    RECYCLED memory may hold, where fresh memory reads as zero and hides a read of something nobody wrote.  The mixed batch (two size
    classes, a same-size pair, a single), a class on float fields, solo clones through every back-end on host images (the small-input
    and direct-output paths among them): the same bytes as without the flag."""
    from seamlesscloneoptimization_amd import capi
    o, oc = oracles
    P = capi.SC_FLAG_POISON_ARENA

    def batch(sizes, flags):
        items = [o.synth_inputs(W, H, seed_dst=40 + k, seed_patch=90 + k, margin=36) for k, (W, H) in enumerate(sizes)]
        inst = capi.Instance(0)
        try:
            inst.set_solver(flags=flags)
            jobs, keep = _device_jobs(inst, items)
            outs = []
            for rep in range(2):
                inst.run_device_batch(jobs)
                outs += [inst.from_device(b, shape) for (f, b0, b, m, shape) in keep]
            _free_jobs(inst, keep)
            return outs
        finally:
            inst.destroy()

    def solo(W, H, flags, method):
        dst, patch, mask, cx, cy = o.synth_inputs(W, H, seed_dst=7, seed_patch=8, margin=36)
        inst = capi.Instance(0)
        try:
            inst.set_solver(flags=flags, method=method)
            outs = []
            for rep in range(2):
                body = dst.copy(); inst.run(patch, body, mask, cx, cy); outs.append(body)
            return outs
        finally:
            inst.destroy()

    cases = [lambda f: batch([(300, 310), (1003, 1010), (318, 333), (640, 480), (1020, 1001), (640, 480), (90, 70), (340, 305), (1012, 1024)], f),
             lambda f: batch([(1003, 1010), (1020, 1001), (300, 310), (318, 333), (157, 160), (150, 171)], f),
             lambda f: batch([(300, 310), (318, 333), (340, 305)], f | capi.SC_FLAG_FLOAT_FIELD | capi.SC_FLAG_FLOAT_RHS),
             lambda f: solo(1500, 900, f, capi.SC_METHOD_MULTIGRID), lambda f: solo(700, 333, f, capi.SC_METHOD_MULTIGRID),
             lambda f: solo(592, 592, f, capi.SC_METHOD_FFT), lambda f: solo(300, 194, f, capi.SC_METHOD_DST), lambda f: solo(154, 100, f, capi.SC_METHOD_AUTO)]
    for ci, fn in enumerate(cases):
        for k, (a, b) in enumerate(zip(fn(0), fn(P))):
            assert np.array_equal(a, b), (ci, k, int((a != b).any(axis=2).sum()))
