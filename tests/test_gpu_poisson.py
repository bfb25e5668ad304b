"""GPU checks of the Poisson solver on float32 images with caller guidance fields (sc_hip_poisson, sc_hip_poisson_device) against the
test side's restatement (tests/poisson_np.py): reconstruction of an image from its forward differences and random problems against
the exact solve under every solver, the LAPLACIAN and GUIDANCE forms, layouts and guard bands, batches, warm starts, the stop rule and
the instance's state afterwards.  R = max |u_exact|."""
from __future__ import annotations


import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from seamlesscloneoptimization_amd import capi  # noqa: E402
from seamlesscloneoptimization_amd.seamless_clone import poisson_tol  # noqa: E402

import poisson_np  # noqa: E402

TOL = 1e-3          # the call's default multigrid stop (sc_poisson_params.tol <= 0): reached at the small sizes of the batch tests
METHODS = {
    "dst": (capi.SC_METHOD_DST, 0),
    "fft64": (capi.SC_METHOD_FFT, capi.SC_FLAG_FFT_FP64),
    "auto": (capi.SC_METHOD_AUTO, 0),
    "fft32": (capi.SC_METHOD_FFT, 0),
    "mg": (capi.SC_METHOD_MULTIGRID, 0),
}


@pytest.fixture(scope="module")
def inst():
    i = capi.Instance(0)
    yield i
    i.destroy()


def configure(inst, method, flags=0, **kw):
    d = inst.default_opts()
    inst.set_solver(**{k: getattr(d, k) for k, _ in capi.SolverOpts._fields_})
    inst.set_solver(method=method, flags=flags, **kw)


def bound(method_ran, name, R, tol=TOL):
    if method_ran == capi.SC_METHOD_MULTIGRID:
        return tol + 1e-4 * R
    if name == "fft32":
        return 4e-3 * R
    return 1e-4 * R


def image(H, W, C, seed):
    return np.random.default_rng(seed).uniform(-50, 300, (H, W, C)).astype(np.float32)


def frame_equal(a, b):
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[-1], b[-1]) and np.array_equal(a[:, 0], b[:, 0]) and
            np.array_equal(a[:, -1], b[:, -1]))


SIZES = [(3, 3), (3, 41), (41, 3), (37, 29), (722, 722), (723, 723), (4000, 142), (4000, 143), (2050, 1030)]      # (W, H)


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("name", list(METHODS))
def test_reconstruction_from_forward_differences(inst, name, W, H):
    method, flags = METHODS[name]
    for C in (1, 2, 3, 4):
        img = image(H, W, C, seed=W * 7 + H * 13 + C)
        gx, gy = poisson_np.forward_differences(img)
        configure(inst, method, flags)
        tol = poisson_tol(img)          # a stop float32 can reach (the default 1e-3 is below its floor at these magnitudes)
        out = inst.poisson(img, gx=gx, gy=gy, tol=tol)
        i = inst.info()
        want_method = method
        if method == capi.SC_METHOD_AUTO:     # one problem: AUTO decides as for a single clone, whatever C
            want_method = capi.SC_METHOD_FFT if capi.auto_takes_direct(W - 2, H - 2) else capi.SC_METHOD_MULTIGRID
        assert i.method == want_method and (i.W, i.H) == (W, H), (name, W, H, C, i.method)
        assert out.dtype == np.float32 and out.shape == img.shape
        R = float(np.abs(img).max())
        err = float(np.abs(out.astype(np.float64) - img).max())
        assert err <= bound(i.method, name, R, tol), (name, W, H, C, err, i.sweeps)
        assert frame_equal(out, img), (name, W, H, C)


@pytest.mark.parametrize("W,H", [(3, 3), (17, 5), (37, 29), (300, 200), (723, 723)])
@pytest.mark.parametrize("name", list(METHODS))
def test_random_guidance_and_boundary_against_the_exact_solve(inst, name, W, H):
    method, flags = METHODS[name]
    for C in (1, 3):
        rng = np.random.default_rng(W * 101 + H + C)
        b = rng.uniform(-100, 400, (H, W, C)).astype(np.float32)
        gx = rng.normal(0, 20, (H, W, C)).astype(np.float32)
        gy = rng.normal(0, 20, (H, W, C)).astype(np.float32)
        want = poisson_np.solve_guidance(b, gx, gy)
        R = float(np.abs(want).max())
        tol = poisson_tol(b, R)
        configure(inst, method, flags)
        out = inst.poisson(b, gx=gx, gy=gy, tol=tol)
        i = inst.info()
        err = float(np.abs(out - want).max())
        assert err <= bound(i.method, name, R, tol), (name, W, H, C, err)
        assert frame_equal(out, b)
        # ... and the LAPLACIAN form with the divergence numpy computes in the documented order: the same bits
        lap = poisson_np.divergence(gx, gy)
        out_l = inst.poisson(b, lap=lap, tol=tol)
        assert np.array_equal(out_l, out), (name, W, H, C)


def test_sor_at_a_tiny_size(inst):
    img = image(7, 9, 2, seed=3)
    gx, gy = poisson_np.forward_differences(img)
    configure(inst, capi.SC_METHOD_SOR, max_sweeps=400, tol=0.0)
    out = inst.poisson(img, gx=gx, gy=gy)
    assert inst.info().method == capi.SC_METHOD_SOR
    assert np.abs(out - img).max() <= 1e-4 * np.abs(img).max()


def _layout_views(H, W, C, kind, fill):
    """Arrays of one layout holding the given H x W x C content: (make(content) -> view, the underlying buffer of a view)."""
    def make(content=None):
        if kind == "hwc":
            buf = np.full((H, W, C), fill, np.float32); v = buf
        elif kind == "chw":
            buf = np.full((C, H, W), fill, np.float32); v = buf.transpose(1, 2, 0)
        elif kind == "padded":
            buf = np.full((H, W + 5, C), fill, np.float32); v = buf[:, :W]
        else:                     # rgba-strided C = 3
            buf = np.full((H, W, 4), fill, np.float32); v = buf[:, :, :C]
        if content is not None:
            v[...] = content
        return v, buf
    return make


@pytest.mark.parametrize("method", [capi.SC_METHOD_MULTIGRID, capi.SC_METHOD_FFT])
def test_layouts_give_the_same_bits_and_write_only_what_they_name(inst, method):
    H, W, C = 203, 301, 3
    rng = np.random.default_rng(9)
    b = rng.uniform(-50, 300, (H, W, C)).astype(np.float32)
    gx = rng.normal(0, 10, (H, W, C)).astype(np.float32)
    gy = rng.normal(0, 10, (H, W, C)).astype(np.float32)
    configure(inst, method)
    tol = poisson_tol(b)
    ref = None
    for kind in ("hwc", "chw", "padded", "rgba"):
        make = _layout_views(H, W, C, kind, 0.0)
        vb, _ = make(b)
        vx, _ = make(gx)
        vy, _ = make(gy)
        vo, obuf = _layout_views(H, W, C, kind, -7.25)()
        before = obuf.copy()
        l = capi.poisson_layout_of(vo)
        for a in (vb, vx, vy):
            la = capi.poisson_layout_of(a)
            assert (la.col_stride, la.row_stride, la.channel_stride) == (l.col_stride, l.row_stride, l.channel_stride), kind
        got = inst.poisson(vb, gx=vx, gy=vy, out=vo, tol=tol)
        assert got is vo
        named = np.zeros(obuf.shape, bool)
        if kind == "chw":
            named[...] = True
        elif kind == "padded":
            named[:, :W] = True
        elif kind == "rgba":
            named[:, :, :C] = True
        else:
            named[...] = True
        assert np.array_equal(obuf[~named], before[~named]), kind           # padding / the unused channel slot untouched
        out = np.array(vo)
        assert frame_equal(out, b), kind
        if ref is None:
            ref = out
        assert np.array_equal(out, ref), kind
    # in place: out is boundary
    vb = b.copy()
    got = inst.poisson(vb, gx=gx, gy=gy, out=vb, tol=tol)
    assert got is vb and np.array_equal(vb, ref)


class Dev:
    """Device arrays of one call: each array at a 256-byte boundary of one block, with `guard` floats of sentinel on both sides."""

    def __init__(self, inst, guard=64):
        self.inst, self.guard, self.parts, self.at = inst, guard, [], 0

    def add(self, host_flat):
        off = self.at + 4 * self.guard
        self.parts.append((off, host_flat))
        self.at = (off + 4 * host_flat.size + 4 * self.guard + 255) // 256 * 256
        return len(self.parts) - 1

    def upload(self, sentinel=-3.5):
        self.nfloat = self.at // 4 + 64
        host = np.full(self.nfloat, sentinel, np.float32)
        for off, a in self.parts:
            host[off // 4:off // 4 + a.size] = a
        self.host = host
        self.d = self.inst.malloc(4 * self.nfloat)
        self.inst._check(self.inst.L.sc_hip_memcpy_h2d(self.inst.h, self.d, host.ctypes.data, 4 * self.nfloat))

    def ptr(self, k):
        return self.d + self.parts[k][0]

    def download(self):
        return self.inst.from_device(self.d, (self.nfloat,), np.float32)

    def free(self):
        self.inst.free(self.d)


def _batch(inst, problems, layout_kind="hwc", tol=0.0, sync=True, tamper=None):
    """problems: [(boundary, gx, gy)] H x W x C.  Runs one sc_hip_poisson_device call; returns (rc, outputs, jobs, info, dev, out ids)."""
    H, W, C = problems[0][0].shape
    if layout_kind == "rgba":
        cs, rs, chs, span = 4, 4 * W, 1, 4 * W * H
    else:
        cs, rs, chs, span = C, C * W, 1, C * W * H

    def flat(a):
        f = np.zeros(span, np.float32)
        v = np.lib.stride_tricks.as_strided(f, shape=(H, W, C), strides=(4 * rs, 4 * cs, 4 * chs))
        v[...] = a
        return f

    dev = Dev(inst)
    ids = []
    for b, gx, gy in problems:
        ids.append((dev.add(flat(gx)), dev.add(flat(gy)), dev.add(flat(b)), dev.add(np.full(span, -3.5, np.float32))))
    dev.upload()
    jobs = capi.Instance.make_poisson_jobs(len(problems))
    for j, (kx, ky, kb, ko) in zip(jobs, ids):
        j.gx, j.gy, j.boundary, j.out = dev.ptr(kx), dev.ptr(ky), dev.ptr(kb), dev.ptr(ko)
    if tamper:
        tamper(jobs)
    layout = capi.PoissonLayout(W, H, C, cs, rs, chs)
    rc = inst.poisson_device(capi.PoissonParams(capi.SC_POISSON_GUIDANCE, float(tol)), layout, jobs, sync=sync, allow_job_errors=True)
    info = inst.info()
    full = dev.download()
    outs = []
    for (_, _, _, ko) in ids:
        off = dev.parts[ko][0] // 4
        f = full[off:off + span]
        outs.append(np.array(np.lib.stride_tricks.as_strided(f, shape=(H, W, C), strides=(4 * rs, 4 * cs, 4 * chs))))
    return rc, outs, jobs, info, dev, full, ids


def _problems(n, H, W, C, seed):
    rng = np.random.default_rng(seed)
    ps = []
    for _ in range(n):
        b = rng.uniform(-50, 300, (H, W, C)).astype(np.float32)
        ps.append((b, rng.normal(0, 15, (H, W, C)).astype(np.float32), rng.normal(0, 15, (H, W, C)).astype(np.float32)))
    return ps


@pytest.mark.parametrize("n,H,W,C", [(2, 48, 64, 1), (16, 61, 97, 2), (70, 30, 40, 3)])
def test_batches_match_their_solo_runs(inst, n, H, W, C):
    ps = _problems(n, H, W, C, seed=n)
    configure(inst, capi.SC_METHOD_AUTO)          # a batch: AUTO takes the cycles
    rc, outs, jobs, info, dev, full, ids = _batch(inst, ps)
    try:
        assert rc == capi.SC_OK and all(j.rc == capi.SC_OK for j in jobs)
        per = capi.SC_POISSON_MAX_PLANES // C
        assert info.method == capi.SC_METHOD_MULTIGRID and info.group_members == n - per * ((n - 1) // per)     # the last chunk's
        batch_sweeps = info.sweeps
        # nothing outside the outputs' spans was written (guard bands, inputs)
        written = np.zeros(full.size, bool)
        for (_, _, _, ko) in ids:
            off = dev.parts[ko][0] // 4
            written[off:off + H * W * C] = True
        assert np.array_equal(full[~written], dev.host[~written])
    finally:
        dev.free()
    configure(inst, capi.SC_METHOD_MULTIGRID)
    same = 0
    for k, (b, gx, gy) in enumerate(ps):
        solo = inst.poisson(b, gx=gx, gy=gy)
        if inst.info().sweeps == batch_sweeps and n <= capi.SC_POISSON_MAX_PLANES // C:
            assert np.array_equal(outs[k], solo), k
            same += 1
        else:
            assert np.abs(outs[k] - solo).max() <= TOL, k
        assert frame_equal(outs[k], b)
    assert n > capi.SC_POISSON_MAX_PLANES // C or same > 0


def test_batch_with_bad_jobs(inst):
    ps = _problems(5, 40, 50, 3, seed=77)

    def tamper(jobs):
        jobs[1].gx = None
        jobs[3].boundary = jobs[3].boundary + 2          # not 4-byte aligned
    configure(inst, capi.SC_METHOD_MULTIGRID)
    rc, outs, jobs, info, dev, full, ids = _batch(inst, ps, tamper=tamper)
    dev.free()
    assert rc == capi.SC_ERR_BAD_ARG
    assert [j.rc for j in jobs] == [capi.SC_OK, capi.SC_ERR_BAD_ARG, capi.SC_OK, capi.SC_ERR_BAD_ARG, capi.SC_OK]
    for k in (1, 3):
        assert np.all(outs[k] == -3.5), k                # skipped: never written
    for k in (0, 2, 4):
        b, gx, gy = ps[k]
        want = poisson_np.solve_guidance(b, gx, gy)
        assert np.abs(outs[k] - want).max() <= TOL + 1e-4 * np.abs(want).max(), k


def test_batch_rgba_layout_leaves_the_fourth_float(inst):
    ps = _problems(3, 33, 45, 3, seed=5)
    configure(inst, capi.SC_METHOD_MULTIGRID)
    rc, outs, jobs, info, dev, full, ids = _batch(inst, ps, layout_kind="rgba")
    dev.free()
    assert rc == capi.SC_OK
    for (_, _, _, ko) in ids:
        off = dev.parts[ko][0] // 4
        span = full[off:off + 4 * 45 * 33].reshape(33, 45, 4)
        assert np.all(span[:, :, 3] == -3.5)
    rc2, outs2, _, _, dev2, _, _ = _batch(inst, ps, layout_kind="hwc")
    dev2.free()
    assert rc2 == capi.SC_OK
    for a, b in zip(outs, outs2):
        assert np.array_equal(a, b)


def test_warm_start(inst):
    H, W, C = 260, 330, 3
    rng = np.random.default_rng(31)
    b = rng.uniform(-50, 300, (H, W, C)).astype(np.float32)
    gx = rng.normal(0, 10, (H, W, C)).astype(np.float32)
    gy = rng.normal(0, 10, (H, W, C)).astype(np.float32)
    want = poisson_np.solve_guidance(b, gx, gy)
    configure(inst, capi.SC_METHOD_MULTIGRID)
    tol = poisson_tol(b, np.abs(want).max())
    cold = b.copy()
    cold[1:-1, 1:-1] = 0.0
    inst.poisson(cold, gx=gx, gy=gy, tol=tol)
    cold_sweeps = inst.info().sweeps
    warm = want.astype(np.float32)
    warm[0], warm[-1], warm[:, 0], warm[:, -1] = b[0], b[-1], b[:, 0], b[:, -1]
    out = inst.poisson(warm, gx=gx, gy=gy, tol=tol)
    assert inst.info().sweeps <= cold_sweeps
    assert np.abs(out - want).max() <= tol + 1e-4 * np.abs(want).max()


def test_not_converged_still_writes_a_result(inst):
    img = image(200, 300, 3, seed=8)
    gx, gy = poisson_np.forward_differences(img)
    configure(inst, capi.SC_METHOD_MULTIGRID, max_sweeps=1)
    out = np.full_like(img, np.nan)
    with pytest.raises(capi.SeamlessCloneError) as e:
        inst.poisson(img, gx=gx, gy=gy, out=out, tol=1e-9)
    assert e.value.code == capi.SC_ERR_NOT_CONVERGED
    out = inst.poisson(img, gx=gx, gy=gy, out=out, tol=1e-9, allow_not_converged=True)
    i = inst.info()
    assert i.converged == 0 and i.sweeps == 1 and np.isfinite(out).all()


def test_host_call_reports_stage_times(inst):
    img = image(500, 600, 3, seed=2)
    gx, gy = poisson_np.forward_differences(img)
    configure(inst, capi.SC_METHOD_MULTIGRID)
    inst.poisson(img, gx=gx, gy=gy, tol=poisson_tol(img))
    i = inst.info()
    assert i.ms_pre > 0 and i.ms_solve > 0 and i.ms_post > 0 and i.ms_call >= i.ms_device_total > 0
    assert i.converged == 1 and i.sweeps >= 1


def test_the_instance_after_a_poisson_call(inst):
    """A clone and an edit on an instance that solved a Poisson problem give the bytes of a fresh instance; its options are unchanged."""
    from oracle import oracle_np
    dst, patch, mask, cx, cy = oracle_np.synth_inputs(300, 200, margin=32)
    emask = np.zeros(dst.shape[:2], np.uint8)
    emask[40:160, 60:260] = 255

    def clone_and_edit(i):
        body = dst.copy()
        i.run(patch, body, mask, cx, cy)
        ed = i.edit(i.edit_params(capi.SC_EDIT_COLOR_CHANGE, red_mul=1.5), dst, emask)
        return body, ed

    for method in (capi.SC_METHOD_AUTO, capi.SC_METHOD_MULTIGRID):
        fresh = capi.Instance(0)
        used = capi.Instance(0)
        try:
            fresh.set_solver(method=method)
            used.set_solver(method=method)
            before = used.get_solver()
            img = image(200, 300, 3, seed=1)
            gx, gy = poisson_np.forward_differences(img)
            used.poisson(img, gx=gx, gy=gy, tol=poisson_tol(img))
            after = used.get_solver()
            assert bytes(before) == bytes(after)
            a = clone_and_edit(fresh)
            b = clone_and_edit(used)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), method
        finally:
            fresh.destroy()
            used.destroy()


def test_poisson_solve_functions(inst):
    import seamlesscloneoptimization_amd as pkg
    img = image(90, 120, 3, seed=4)
    gx, gy = poisson_np.forward_differences(img)
    out = pkg.poisson_solve(img, gx, gy, method=capi.SC_METHOD_DST)
    assert np.abs(out - img).max() <= 1e-4 * np.abs(img).max()
    two = pkg.poisson_solve_batch([img, img[::-1].copy()], [gx, poisson_np.forward_differences(img[::-1].copy())[0]],
                                  [gy, poisson_np.forward_differences(img[::-1].copy())[1]])
    tol = poisson_tol(img)
    assert np.abs(two[0] - img).max() <= tol + 1e-4 * np.abs(img).max()
    assert np.abs(two[1] - img[::-1]).max() <= tol + 1e-4 * np.abs(img).max()
    lap = poisson_np.divergence(gx, gy)
    one = pkg.poisson_solve_batch([img], laplacians=[lap], method=capi.SC_METHOD_MULTIGRID)[0]
    ref = pkg.poisson_solve(img, laplacian=lap, method=capi.SC_METHOD_MULTIGRID)
    assert np.array_equal(one, ref)
    # 2-D arrays are one channel
    g2x, g2y = poisson_np.forward_differences(img[:, :, 0])
    out2 = pkg.poisson_solve(img[:, :, 0], g2x, g2y)
    assert out2.shape == img.shape[:2] and np.abs(out2 - img[:, :, 0]).max() <= 1e-4 * np.abs(img).max()
