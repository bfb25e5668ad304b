"""Batches of whole-image edits on the MI355X (sc_hip_edit_device_batch, sc_hip_pool_edit, edit_batch).

Same-size images are solved as one field of 3n channels.  Every member is checked against the restatement in tests/photo_edits_np.py
(within one grey level; PARITY UNPINNED, as for the single edits) and against its own solo SC_METHOD_MULTIGRID run on the device: the
same bytes when the cycle counts agree, within one grey level otherwise (the group's stop rule sees its largest correction)."""
import numpy as np
import pytest

import photo_edits_np as pe

pytestmark = pytest.mark.gpu

OPS = {"color": (1, dict(red_mul=1.6, green_mul=0.8, blue_mul=1.2)),
       "illumination": (2, dict(alpha=0.3, beta=0.5)),
       "texture": (3, dict(low_threshold=25.0, high_threshold=60.0, kernel_size=3))}


def _rand(W, H, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = 128 + 60 * np.sin(xx / 7.0 + seed)[:, :, None] * np.cos(yy / 5.0)[:, :, None] * np.array([1.0, 0.6, -0.8])
    img = base + rng.normal(0, 18, (H, W, 3))
    img[(xx // 9 + yy // 7 + seed) % 5 == 0] += 70
    return np.clip(img, 0, 255).astype(np.uint8)


def _ellipse(W, H, cx=None, cy=None, a=None, b=None):
    yy, xx = np.mgrid[0:H, 0:W]
    cx = W / 2 if cx is None else cx
    cy = H / 2 if cy is None else cy
    a = W / 3 if a is None else a
    b = H / 3 if b is None else b
    m = np.zeros((H, W), np.uint8)
    m[((xx - cx) / a) ** 2 + ((yy - cy) / b) ** 2 <= 1] = 255
    return m


def _mask(W, H, kind, k):
    """ellipse / grey / rectangle masks, moved a little with k so that the members differ"""
    if kind == "ellipse":
        return _ellipse(W, H, cx=W / 2 + (k % 5) - 2, cy=H / 2 + (k % 3) - 1, a=W / 3 - k % 4, b=H / 3)
    if kind == "grey":
        g = _ellipse(W, H, a=W / 3 + k % 3)
        g[g > 0] = ((np.arange(int((g > 0).sum())) + 11 * k) * 37 % 256).astype(np.uint8)
        return g
    m = np.zeros((H, W), np.uint8)
    m[: H // 2 + k % 4, : W // 3 + k] = 255          # touches the top and left edges
    return m


def _serpentine(W=700, H=420, pitch=24, band=8):
    """The long hysteresis chain of test_gpu_photo_edits.py: a snake of grey 40 on black, one white end."""
    img = np.zeros((H, W, 3), np.uint8)
    rows = list(range(10, H - band - 10, pitch))
    for i, y in enumerate(rows):
        img[y:y + band, 10:W - 10] = 40
        if i + 1 < len(rows):
            x = W - 10 - band if i % 2 == 0 else 10
            img[y:rows[i + 1] + band, x:x + band] = 40
    img[rows[0]:rows[0] + band, 10:40] = 255
    return img


def _dmax(a, b):
    return int(np.abs(a.astype(np.int16) - b.astype(np.int16)).max())


def _new(**solver):
    from seamlesscloneoptimization_amd import capi
    i = capi.Instance(0)
    if solver:
        i.set_solver(**solver)
    return i


@pytest.fixture(scope="module")
def solo():
    """the reference runs: one image at a time, SC_METHOD_MULTIGRID"""
    from seamlesscloneoptimization_amd import capi
    i = _new(method=capi.SC_METHOD_MULTIGRID)
    yield i
    i.destroy()


class Dev:
    """device copies of images, freed on exit"""

    def __init__(self, inst):
        self.inst, self.ptrs = inst, []

    def put(self, a):
        p = self.inst.to_device(a)
        self.ptrs.append(p)
        return p

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.ptrs:
            self.inst.free(p)


def _solo_run(solo, op, img, mask):
    """(result, cycles) of one image alone, device-resident, SC_METHOD_MULTIGRID; op: a key of OPS or (code, params)"""
    code, kw = OPS[op] if isinstance(op, str) else op
    H, W = img.shape[:2]
    with Dev(solo) as d:
        s, m, o = d.put(img), d.put(mask), d.put(np.zeros_like(img))
        solo.edit_device(solo.edit_params(code, **kw), s, (H, W), m, o, sync=True)
        return solo.from_device(o, img.shape), solo.info().sweeps


def _jobs(inst, d, items):
    """items: (src pointer, shape, mask pointer, dst pointer) -> an EditJob array of dense rows"""
    jobs = inst.make_edit_jobs(len(items))
    for j, (s, shape, m, o) in zip(jobs, items):
        H, W = shape[:2]
        j.src, j.cols, j.rows, j.src_step = s, W, H, 3 * W
        j.mask, j.mask_step = m, W
        j.dst, j.dst_step = o, 3 * W
    return jobs


def _check_member(solo, op, img, mask, out, group_cycles, oracle=True):
    want_solo, cycles = _solo_run(solo, op, img, mask)
    d = _dmax(out, want_solo)
    if cycles == group_cycles:
        assert d == 0, (op, img.shape, cycles)
    else:
        assert d <= 1, (op, img.shape, cycles, group_cycles)
    if oracle:
        code, kw = OPS[op] if isinstance(op, str) else op
        assert _dmax(out, pe.edit(img, mask, code, **kw)) <= 1
    # the frame is src's
    assert np.array_equal(out[0], img[0]) and np.array_equal(out[-1], img[-1])
    assert np.array_equal(out[:, 0], img[:, 0]) and np.array_equal(out[:, -1], img[:, -1])
    return cycles == group_cycles


def _group_run(op, imgs, masks):
    """(results, cycles) of same-size images as a batch call of their own on a fresh instance (SC_METHOD_AUTO): what a group of exactly
    these members computes, and its cycle count"""
    code, kw = OPS[op] if isinstance(op, str) else op
    inst = _new()
    try:
        with Dev(inst) as d:
            outs = [d.put(np.zeros_like(img)) for img in imgs]
            jobs = _jobs(inst, d, [(d.put(img), img.shape, d.put(m), o) for img, m, o in zip(imgs, masks, outs)])
            inst.edit_device_batch(inst.edit_params(code, **kw), jobs)
            info = inst.info()
            assert info.group_members == len(imgs)
            return [inst.from_device(o, img.shape) for o, img in zip(outs, imgs)], info.sweeps
    finally:
        inst.destroy()


def _check_groups(solo, op, imgs, masks, got, groups):
    """groups: lists of indices that went through one set of launches.  Every member has the bytes of the same group run as a call of
    its own, and (through that run's cycle count) its solo run's bytes when the counts agree, within one grey level otherwise."""
    for g in groups:
        ref, cycles = _group_run(op, [imgs[i] for i in g], [masks[i] for i in g])
        for i, r in zip(g, ref):
            assert np.array_equal(got[i], r), (i, imgs[i].shape)
            _check_member(solo, op, imgs[i], masks[i], got[i], cycles)


@pytest.mark.parametrize("op", list(OPS))
@pytest.mark.parametrize("W,H,mask_kind", [(301, 203, "ellipse"), (258, 131, "grey"), (640, 360, "rect")])
def test_group_of_sixteen_matches_solo_runs_and_the_oracle(solo, op, W, H, mask_kind):
    n = 16
    imgs = [_rand(W, H, 100 * k + W) for k in range(n)]
    masks = [_mask(W, H, mask_kind, k) for k in range(n)]
    inst = _new()              # SC_METHOD_AUTO: a group takes the cycles
    try:
        with Dev(inst) as d:
            outs = [d.put(np.full_like(img, 0x5A)) for img in imgs]
            jobs = _jobs(inst, d, [(d.put(img), img.shape, d.put(m), o) for img, m, o in zip(imgs, masks, outs)])
            code, kw = OPS[op]
            assert inst.edit_device_batch(inst.edit_params(code, **kw), jobs) == 0
            info = inst.info()
            got = [inst.from_device(o, img.shape) for o, img in zip(outs, imgs)]
            counts = inst.edit_counts()
    finally:
        inst.destroy()
    from seamlesscloneoptimization_amd import capi
    assert all(j.rc == capi.SC_OK for j in jobs)
    assert info.group_members == n and info.method == capi.SC_METHOD_MULTIGRID
    assert (info.W, info.H, info.x0, info.y0, info.ltx, info.lty) == (W, H, 0, 0, 0, 0)
    if op == "texture":
        assert counts[0] >= 4 and counts[1] >= 1
    same = sum(_check_member(solo, op, img, m, out, info.sweeps) for img, m, out in zip(imgs, masks, got))
    print("%s %dx%d %s: %d cycles, %d of %d members with the solo cycle count" % (op, W, H, mask_kind, info.sweeps, same, n))


def test_one_call_with_two_groups_and_a_single(solo):
    from seamlesscloneoptimization_amd import capi
    sizes = [(301, 203)] * 5 + [(258, 131)] * 4 + [(97, 60)]
    order = [0, 5, 1, 9, 6, 2, 7, 3, 8, 4]                        # the sizes interleaved in the call
    items = [(sizes[i], _rand(*sizes[i], 7 + i), _mask(*sizes[i], "ellipse", i)) for i in order]
    inst = _new()
    try:
        with Dev(inst) as d:
            outs = [d.put(np.zeros_like(img)) for _, img, _ in items]
            jobs = _jobs(inst, d, [(d.put(img), img.shape, d.put(m), o) for (_, img, m), o in zip(items, outs)])
            code, kw = OPS["color"]
            inst.edit_device_batch(inst.edit_params(code, **kw), jobs)
            info = inst.info()
            got = [inst.from_device(o, img.shape) for o, (_, img, _) in zip(outs, items)]
    finally:
        inst.destroy()
    assert all(j.rc == capi.SC_OK for j in jobs)
    assert info.group_members in (4, 5)
    # the two groups, members in call order: each as a call of its own, then against the solo runs through that call's cycle count
    groups = [[k for k, it in enumerate(items) if it[0] == size] for size in ((301, 203), (258, 131))]
    _check_groups(solo, "color", [it[1] for it in items], [it[2] for it in items], got, groups)
    for (size, img, m), out in zip(items, got):
        assert _dmax(out, pe.edit(img, m, OPS["color"][0], **OPS["color"][1])) <= 1, size
        if size == (97, 60):                # the single runs through the single-image path: the solo bytes exactly
            inst2 = _new()
            try:
                with Dev(inst2) as d:
                    o = d.put(np.zeros_like(img))
                    inst2.edit_device(inst2.edit_params(OPS["color"][0], **OPS["color"][1]), d.put(img), img.shape, d.put(m), o)
                    assert np.array_equal(out, inst2.from_device(o, img.shape))
            finally:
                inst2.destroy()


@pytest.mark.parametrize("op", list(OPS))
def test_shared_mask_shared_src_and_in_place(solo, op):
    W, H = 258, 131
    code, kw = OPS[op]
    imgs = [_rand(W, H, 50 + k) for k in range(6)]
    shared_mask = _mask(W, H, "grey", 3)
    masks = [_mask(W, H, "ellipse", k) for k in range(4)]
    inst = _new()
    try:
        with Dev(inst) as d:
            # one mask for every job
            dm = d.put(shared_mask)
            outs = [d.put(np.zeros_like(img)) for img in imgs]
            jobs = _jobs(inst, d, [(d.put(img), img.shape, dm, o) for img, o in zip(imgs, outs)])
            inst.edit_device_batch(inst.edit_params(code, **kw), jobs)
            assert inst.info().group_members == 6
            a = [inst.from_device(o, img.shape) for o, img in zip(outs, imgs)]
            # one src for jobs with different masks
            ds = d.put(imgs[0])
            outs2 = [d.put(np.zeros_like(imgs[0])) for _ in masks]
            jobs2 = _jobs(inst, d, [(ds, imgs[0].shape, d.put(m), o) for m, o in zip(masks, outs2)])
            inst.edit_device_batch(inst.edit_params(code, **kw), jobs2)
            b = [inst.from_device(o, imgs[0].shape) for o in outs2]
            assert np.array_equal(inst.from_device(ds, imgs[0].shape), imgs[0])
            # the first call again in place: dst = src
            srcs = [d.put(img) for img in imgs]
            jobs3 = _jobs(inst, d, [(s, img.shape, dm, s) for s, img in zip(srcs, imgs)])
            inst.edit_device_batch(inst.edit_params(code, **kw), jobs3)
            c = [inst.from_device(s, img.shape) for s, img in zip(srcs, imgs)]
            assert np.array_equal(inst.from_device(dm, shared_mask.shape), shared_mask)
    finally:
        inst.destroy()
    for img, out, inplace in zip(imgs, a, c):
        assert np.array_equal(out, inplace)
        want, _ = _solo_run(solo, op, img, shared_mask)
        assert _dmax(out, want) <= 1
    for m, out in zip(masks, b):
        want, _ = _solo_run(solo, op, imgs[0], m)
        assert _dmax(out, want) <= 1


def test_texture_group_with_one_long_hysteresis_chain(solo):
    """One member is the serpentine (many hysteresis batches), the others settle at once: the group's loop runs until the chain is
    done, the settled members' maps are untouched by the extra launches, and every member matches its solo run."""
    from seamlesscloneoptimization_amd import capi
    W, H = 700, 420
    imgs = [_rand(W, H, 900 + k) for k in range(5)]
    imgs.insert(2, _serpentine(W, H))
    masks = [_ellipse(W, H, a=W / 2.2, b=H / 2.2) for _ in imgs]
    kw = dict(low_threshold=100.0, high_threshold=600.0, kernel_size=3)
    inst = _new()
    try:
        with Dev(inst) as d:
            outs = [d.put(np.zeros_like(img)) for img in imgs]
            jobs = _jobs(inst, d, [(d.put(img), img.shape, d.put(m), o) for img, m, o in zip(imgs, masks, outs)])
            inst.edit_device_batch(inst.edit_params(capi.SC_EDIT_TEXTURE_FLATTENING, **kw), jobs)
            info = inst.info()
            counts = inst.edit_counts()
            got = [inst.from_device(o, img.shape) for o, img in zip(outs, imgs)]
        solo_counts = solo.canny(imgs[2], 100, 600, 3)[2]
    finally:
        inst.destroy()
    assert info.group_members == 6
    assert counts[1] >= 2 and counts[0] >= solo_counts[0], (counts, solo_counts)
    for img, m, out in zip(imgs, masks, got):
        _check_member(solo, (capi.SC_EDIT_TEXTURE_FLATTENING, kw), img, m, out, info.sweeps)


def test_a_bad_job_gets_its_own_code_and_the_others_run(solo):
    from seamlesscloneoptimization_amd import capi
    W, H = 301, 203
    imgs = [_rand(W, H, 70 + k) for k in range(6)]
    masks = [_mask(W, H, "ellipse", k) for k in range(6)]
    inst = _new()
    try:
        with Dev(inst) as d:
            outs = [d.put(np.full_like(img, 0x11)) for img in imgs]
            jobs = _jobs(inst, d, [(d.put(img), img.shape, d.put(m), o) for img, m, o in zip(imgs, masks, outs)])
            jobs[1].cols, jobs[1].rows = 2, 2                      # too small
            jobs[3].src_step = 3 * W - 1                            # short step
            jobs[4].mask = None                                     # null mask
            code, kw = OPS["color"]
            rc = inst.edit_device_batch(inst.edit_params(code, **kw), jobs, allow_job_errors=True)
            info = inst.info()
            got = [inst.from_device(o, img.shape) for o, img in zip(outs, imgs)]
    finally:
        inst.destroy()
    assert [j.rc for j in jobs] == [capi.SC_OK, capi.SC_ERR_BAD_SIZE, capi.SC_OK, capi.SC_ERR_BAD_SIZE, capi.SC_ERR_BAD_ARG, capi.SC_OK]
    assert rc in (capi.SC_ERR_BAD_SIZE, capi.SC_ERR_BAD_ARG)
    assert info.group_members == 3
    for k in (1, 3, 4):
        assert (got[k] == 0x11).all(), k                            # skipped: not written
    for k in (0, 2, 5):
        _check_member(solo, "color", imgs[k], masks[k], got[k], info.sweeps, oracle=False)


@pytest.mark.parametrize("group", [16, 0])
def test_pool_device_resident_and_host(solo, group):
    from seamlesscloneoptimization_amd import capi
    sizes = [(301, 203) if k % 3 else (258, 131) for k in range(40)]
    imgs = [_rand(W, H, 300 + k) for k, (W, H) in enumerate(sizes)]
    masks = [_mask(W, H, "ellipse" if k % 2 else "grey", k) for k, (W, H) in enumerate(sizes)]
    code, kw = OPS["illumination"]
    pool = capi.Pool(0, streams=2, group=group)
    try:
        inst = pool.instances[0]
        p = inst.edit_params(code, **kw)
        with Dev(inst) as d:
            outs = [d.put(np.zeros_like(img)) for img in imgs]
            jobs = _jobs(inst, d, [(d.put(img), img.shape, d.put(m), o) for img, m, o in zip(imgs, masks, outs)])
            pool.edit(p, jobs, device_resident=True)
            dev = [inst.from_device(o, img.shape) for o, img in zip(outs, imgs)]
        assert all(j.rc == capi.SC_OK for j in jobs)
        assert max(pool.instances[k].info().group_members for k in range(2)) >= 2
        host = [np.zeros_like(img) for img in imgs]
        hjobs = pool.edit_host(p, list(zip(imgs, masks, host)))
        assert all(j.rc == capi.SC_OK for j in hjobs)
    finally:
        pool.close()
    # device-resident: the pool's chunks (as the planner forms them) each as a call of its own, and the solo runs through its cycles
    g = capi.plan_edit_groups_pool(sizes, group, 2)
    chunks = [[i for i in range(len(sizes)) if g[i] == c] for c in range(max(g) + 1)]
    assert all(len(c) >= 2 for c in chunks)
    _check_groups(solo, "illumination", imgs, masks, dev, chunks)
    for img, m, a in zip(imgs, masks, dev):
        assert _dmax(a, pe.edit(img, m, code, **kw)) <= 1
    # host images: one sc_hip_edit per job under SC_METHOD_AUTO -- the bytes of the same call on an instance of its own
    ref = _new()
    try:
        for img, m, b in zip(imgs, masks, host):
            assert np.array_equal(b, ref.edit(ref.edit_params(code, **kw), img, m))
            assert _dmax(b, pe.edit(img, m, code, **kw)) <= 1
    finally:
        ref.destroy()


def test_a_clone_after_a_batch_edit_is_unchanged():
    from oracle import oracle_np
    from seamlesscloneoptimization_amd import capi
    dst, patch, mask, cx, cy = oracle_np.synth_inputs(300, 200, margin=32)
    fresh = _new(method=capi.SC_METHOD_MULTIGRID)
    try:
        want = dst.copy()
        fresh.run(patch, want, mask, cx, cy)
    finally:
        fresh.destroy()
    i = _new(method=capi.SC_METHOD_MULTIGRID)
    try:
        W, H = 320, 240
        imgs = [_rand(W, H, k) for k in range(4)]
        with Dev(i) as d:
            dm = d.put(_ellipse(W, H))
            for code, kw in OPS.values():
                outs = [d.put(np.zeros_like(img)) for img in imgs]
                jobs = _jobs(i, d, [(d.put(img), img.shape, dm, o) for img, o in zip(imgs, outs)])
                i.edit_device_batch(i.edit_params(code, **kw), jobs)
        got = dst.copy()
        i.run(patch, got, mask, cx, cy)
    finally:
        i.destroy()
    assert np.array_equal(got, want)


def test_edit_batch_equals_the_cv2_shaped_functions():
    import seamlesscloneoptimization_amd as pkg
    from seamlesscloneoptimization_amd import capi
    W, H = 258, 131
    imgs = [_rand(W, H, 40 + k) for k in range(5)] + [_rand(97, 60, 1)]
    masks = [_mask(W, H, "ellipse", k) for k in range(5)] + [_mask(97, 60, "rect", 0)]
    masks3 = [np.repeat(m[:, :, None], 3, axis=2) if k % 2 else m for k, m in enumerate(masks)]
    keep = [img.copy() for img in imgs]
    mg = dict(method=capi.SC_METHOD_MULTIGRID)
    for fn, code, kw in ((pkg.colorChange, capi.SC_EDIT_COLOR_CHANGE, dict(red_mul=1.5, green_mul=0.7, blue_mul=1.1)),
                         (pkg.illuminationChange, capi.SC_EDIT_ILLUMINATION_CHANGE, dict(alpha=0.2, beta=0.4)),
                         (pkg.textureFlattening, capi.SC_EDIT_TEXTURE_FLATTENING, dict(low_threshold=30, high_threshold=45, kernel_size=3))):
        got = pkg.edit_batch(code, imgs, masks3, streams=2, **kw, **mg)
        assert len(got) == len(imgs)
        for img, m, out in zip(imgs, masks3, got):
            want = fn(img, m, **kw, **mg)
            assert out.shape == img.shape and _dmax(out, want) <= 1, fn.__name__
    # one mask for all
    one = pkg.edit_batch(capi.SC_EDIT_COLOR_CHANGE, imgs[:5], masks[0], red_mul=2.0)
    for img, out in zip(imgs[:5], one):
        assert _dmax(out, pkg.colorChange(img, masks[0], red_mul=2.0, **mg)) <= 1
    assert all(np.array_equal(a, b) for a, b in zip(imgs, keep))
