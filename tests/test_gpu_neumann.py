"""GPU checks of the Neumann option of the Poisson solver (SC_POISSON_NEUMANN through sc_hip_poisson and sc_hip_poisson_device) against
the test side's restatement (tests/direct_np.py) on the same float32 inputs: reconstruction from forward differences and random
guidance fields under every method that serves the option, the LAPLACIAN and GUIDANCE forms, the mean anchor, layouts and guard bands,
batches, the refused methods and sizes, and the instance's state afterwards.  R = max |u_exact|.

Bounds.  Double transforms (SC_FLAG_FFT_FP64): 1e-6 R -- the restatement sees the same float32 right-hand side, so what is left is the
float32 rounding of the stored result (<= 6e-8 R), of the mean's addition, and the double transforms' error times the worst
amplification 1 / lambda_min ~ (n / pi)^2 ~ 1.7e6 at n = 4096, ~1e-9 R.  Float32 transforms: 3e-2 R = 4 x the worst value
tools/neumann_probe.py measured over SIZES and C = 1 .. 4 on this file's images (6.3e-3 R, reconstruction at 8192 x 64, C = 3;
profiles/neumann_probe.json), rounded up to one digit: the error is a sum of ~n log n roundings amplified by 1 / lambda_min in the
lowest modes along the long side, not a worst case, and it varies fourfold from seed to seed at that size (1.6e-3 .. 6.3e-3 R over
four images; every other size stays below 1.7e-3 R) -- the margin is for other seeds and runtime versions.  DESIGN.md section 4 says
which step loses the digits.  The mean: 1e-6 R per channel under both.  Beside these, the reconstruction test holds the residual
ratio and the error to the float32 restatement on the same input (tests/direct_bounds.py): the 3e-2 R above lets a wrong
coefficient through."""
from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from seamlesscloneoptimization_amd import capi  # noqa: E402

import direct_np as dn  # noqa: E402
import poisson_np  # noqa: E402
from direct_bounds import NEUMANN  # noqa: E402

NEU = capi.SC_POISSON_NEUMANN
Yardstick = NEUMANN.yardstick
METHODS = {
    "auto": (capi.SC_METHOD_AUTO, 0),
    "fft32": (capi.SC_METHOD_FFT, 0),
    "fft64": (capi.SC_METHOD_FFT, capi.SC_FLAG_FFT_FP64),
}
BOUND = {"auto": 3e-2, "fft32": 3e-2, "fft64": 1e-6}       # x R (module docstring)
MEAN_BOUND = 1e-6                                          # x R
SIZES = [(2, 2), (2, 41), (41, 2), (37, 29), (300, 200), (723, 722), (1280, 721), (4000, 143), (2050, 1030), (8192, 64)]      # (W, H)


@pytest.fixture(scope="module")
def inst():
    i = capi.Instance(0)
    yield i
    i.destroy()


def configure(inst, method, flags=0, **kw):
    d = inst.default_opts()
    inst.set_solver(**{k: getattr(d, k) for k, _ in capi.SolverOpts._fields_})
    inst.set_solver(method=method, flags=flags, **kw)


def methods_for(W, H):
    return [m for m in METHODS if not (m == "fft64" and max(W, H) > 4096)]          # (8192, 64): float32 only


def check_info(inst, W, H):
    i = inst.info()
    assert i.method == capi.SC_METHOD_FFT and i.sweeps == 1 and i.converged == 1 and (i.W, i.H) == (W, H)


@pytest.mark.parametrize("W,H", SIZES)
def test_reconstruction_and_random_guidance_against_the_restatement(inst, W, H):
    for C in (1, 2, 3, 4):
        rng = np.random.default_rng(W * 7 + H * 13 + C)
        img = rng.uniform(-50, 300, (H, W, C)).astype(np.float32)
        fx, fy = dn.forward_differences(img)
        b = rng.uniform(-100, 400, (H, W, C)).astype(np.float32)
        gx = rng.normal(0, 20, (H, W, C)).astype(np.float32)
        gy = rng.normal(0, 20, (H, W, C)).astype(np.float32)
        for what, ax, ay, bb in (("reconstruction", fx, fy, img), ("random", gx, gy, b), ("random, no boundary", gx, gy, None)):
            want = dn.solve_free(dn.divergence(ax, ay), bb)
            R = float(np.abs(want).max())
            mean = dn.mean_of(bb) if bb is not None else np.zeros(C)
            lap = dn.divergence(ax, ay)
            yard = Yardstick("lrtb", "", 0.0, None, lap, bb)          # RES and ERR against the float32 restatement (direct_bounds.py)
            for name in methods_for(W, H):
                configure(inst, *METHODS[name])
                out = inst.poisson(bb, gx=ax, gy=ay, neumann=True)
                check_info(inst, W, H)
                assert out.dtype == np.float32 and out.shape == (H, W, C)
                err = float(np.abs(out.astype(np.float64) - want).max())
                merr = float(np.abs(out.astype(np.float64).mean(axis=(0, 1)) - mean).max())
                print(f"{W}x{H}x{C} {what} {name}: err {err / R:.3g} R, mean {merr / R:.3g} R")
                assert err <= BOUND[name] * R, (what, name, W, H, C, err / R)
                assert merr <= MEAN_BOUND * R, (what, name, W, H, C, merr / R)
                bad, e, r = yard.check(out, name == "fft64", name != "fft64" or what == "reconstruction")
                print(f"    RES {r:.3g} ERR {e:.3g} / solve_f32 RES {yard.res32:.3g} ERR {yard.err32:.3g}")
                assert not bad, (what, name, W, H, C, bad)
                # the LAPLACIAN form fed the divergence numpy computes in the documented order: the same bits
                out_l = inst.poisson(bb, lap=lap, neumann=True)
                assert np.array_equal(out_l, out), (what, name, W, H, C)


@pytest.mark.parametrize("name", list(METHODS))
def test_a_constant_added_to_lap_is_projected_out(inst, name):
    """Within the bound, not the same bits: adding the constant rounds every element of lap again in float32 (so "want" is the
    restatement on the shifted float32 array, which projects its mean out as well), and the transforms see the DC term -- its
    roundings reach the other coefficients -- before the (0, 0) coefficient is dropped."""
    H, W, C = 200, 300, 3
    rng = np.random.default_rng(12)
    lap = dn.divergence(rng.normal(0, 20, (H, W, C)).astype(np.float32), rng.normal(0, 20, (H, W, C)).astype(np.float32))
    shifted = (lap + np.float32(3.0)).astype(np.float32)
    b = rng.uniform(-100, 400, (H, W, C)).astype(np.float32)
    configure(inst, *METHODS[name])
    for rhs in (lap, shifted):
        want = dn.solve_free(rhs, b)
        R = float(np.abs(want).max())
        out = inst.poisson(b, lap=rhs, neumann=True)
        assert np.abs(out.astype(np.float64) - want).max() <= BOUND[name] * R
        assert np.abs(out.astype(np.float64).mean(axis=(0, 1)) - dn.mean_of(b)).max() <= MEAN_BOUND * R
    # the two right-hand sides differ by the constant and by float32 rounding only: so do the exact answers
    assert np.abs(dn.solve_free(shifted, b) - dn.solve_free(lap, b)).max() <= 1e-5 * R


@pytest.mark.parametrize("name", list(METHODS))
def test_the_last_column_of_gx_and_the_last_row_of_gy_are_never_read(inst, name):
    H, W, C = 61, 97, 3
    rng = np.random.default_rng(4)
    gx = rng.normal(0, 20, (H, W, C)).astype(np.float32)
    gy = rng.normal(0, 20, (H, W, C)).astype(np.float32)
    b = rng.uniform(-100, 400, (H, W, C)).astype(np.float32)
    configure(inst, *METHODS[name])
    ref = inst.poisson(b, gx=gx, gy=gy, neumann=True)
    gx[:, -1] = np.nan
    gy[-1] = np.nan
    out = inst.poisson(b, gx=gx, gy=gy, neumann=True)
    assert np.isfinite(out).all() and np.array_equal(out, ref)


def _layout_views(H, W, C, kind, fill):
    """Arrays of one layout holding the given H x W x C content: make(content) -> (view, the underlying buffer)."""
    def make(content=None):
        if kind == "hwc":
            buf = np.full((H, W, C), fill, np.float32); v = buf
        elif kind == "chw":
            buf = np.full((C, H, W), fill, np.float32); v = buf.transpose(1, 2, 0)
        elif kind == "padded":
            buf = np.full((H, W + 5, C), fill, np.float32); v = buf[:, :W]
        elif kind == "transposed":
            buf = np.full((W, H, C), fill, np.float32); v = buf.transpose(1, 0, 2)
        else:                     # rgba-strided C = 3
            buf = np.full((H, W, 4), fill, np.float32); v = buf[:, :, :C]
        if content is not None:
            v[...] = content
        return v, buf
    return make


@pytest.mark.parametrize("name", list(METHODS))
def test_layouts_give_the_same_bits_and_write_only_what_they_name(inst, name):
    H, W, C = 203, 301, 3
    rng = np.random.default_rng(9)
    b = rng.uniform(-50, 300, (H, W, C)).astype(np.float32)
    gx = rng.normal(0, 10, (H, W, C)).astype(np.float32)
    gy = rng.normal(0, 10, (H, W, C)).astype(np.float32)
    configure(inst, *METHODS[name])
    ref = None
    for kind in ("hwc", "chw", "padded", "rgba", "transposed"):
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
        got = inst.poisson(vb, gx=vx, gy=vy, out=vo, neumann=True)
        assert got is vo
        named = np.ones(obuf.shape, bool)
        if kind == "padded":
            named[:, W:] = False
        elif kind == "rgba":
            named[:, :, C:] = False
        assert np.array_equal(obuf[~named], before[~named]), kind           # padding / the unused channel slot untouched
        out = np.array(vo)
        if ref is None:
            ref = out
        assert np.array_equal(out, ref), kind
    # in place: out is boundary
    vb = b.copy()
    got = inst.poisson(vb, gx=gx, gy=gy, out=vb, neumann=True)
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


def _batch(inst, problems, layout_kind="hwc", tamper=None, kind=capi.SC_POISSON_GUIDANCE | NEU):
    """problems: [(boundary or None, gx, gy)] H x W x C.  One sc_hip_poisson_device call; (rc, outputs, jobs, info, dev, memory, ids)."""
    H, W, C = problems[0][1].shape
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
        ids.append((dev.add(flat(gx)), dev.add(flat(gy)), None if b is None else dev.add(flat(b)), dev.add(np.full(span, -3.5, np.float32))))
    dev.upload()
    jobs = capi.Instance.make_poisson_jobs(len(problems))
    for j, (kx, ky, kb, ko) in zip(jobs, ids):
        j.gx, j.gy, j.boundary, j.out = dev.ptr(kx), dev.ptr(ky), None if kb is None else dev.ptr(kb), dev.ptr(ko)
    if tamper:
        tamper(jobs)
    layout = capi.PoissonLayout(W, H, C, cs, rs, chs)
    rc = inst.poisson_device(capi.PoissonParams(kind, 0.0), layout, jobs, sync=True, allow_job_errors=True)
    info = inst.info()
    full = dev.download()
    outs = []
    for (_, _, _, ko) in ids:
        off = dev.parts[ko][0] // 4
        f = full[off:off + span]
        outs.append(np.array(np.lib.stride_tricks.as_strided(f, shape=(H, W, C), strides=(4 * rs, 4 * cs, 4 * chs))))
    return rc, outs, jobs, info, dev, full, ids


def _problems(n, H, W, C, seed, none_every=0):
    rng = np.random.default_rng(seed)
    ps = []
    for k in range(n):
        b = rng.uniform(-50, 300, (H, W, C)).astype(np.float32)
        ps.append((None if none_every and k % none_every == 1 else b, rng.normal(0, 15, (H, W, C)).astype(np.float32),
                   rng.normal(0, 15, (H, W, C)).astype(np.float32)))
    return ps


@pytest.mark.parametrize("name", list(METHODS))
@pytest.mark.parametrize("n,H,W,C", [(2, 48, 64, 1), (16, 61, 97, 2), (70, 30, 40, 3)])
def test_batches_equal_their_solo_runs_bit_for_bit(inst, name, n, H, W, C):
    ps = _problems(n, H, W, C, seed=n, none_every=5)
    configure(inst, *METHODS[name])          # AUTO stays direct for n > 1
    rc, outs, jobs, info, dev, full, ids = _batch(inst, ps)
    try:
        assert rc == capi.SC_OK and all(j.rc == capi.SC_OK for j in jobs)
        per = capi.SC_POISSON_MAX_PLANES // C
        last = n - per * ((n - 1) // per)
        assert info.method == capi.SC_METHOD_FFT and info.sweeps == 1 and info.converged == 1
        assert info.group_members == (last if last > 1 else 0)
        assert info.ms_solve > 0 and info.ms_device_total > 0
        # nothing outside the outputs' spans was written (guard bands, inputs)
        written = np.zeros(full.size, bool)
        for (_, _, _, ko) in ids:
            off = dev.parts[ko][0] // 4
            written[off:off + H * W * C] = True
        assert np.array_equal(full[~written], dev.host[~written])
    finally:
        dev.free()
    for k, (b, gx, gy) in enumerate(ps):
        solo = inst.poisson(b, gx=gx, gy=gy, neumann=True)
        assert np.array_equal(outs[k], solo), k
    want = dn.solve_free(dn.divergence(ps[1][1], ps[1][2]), ps[1][0])          # (a member without boundary)
    assert ps[1][0] is None and np.abs(outs[1] - want).max() <= BOUND[name] * np.abs(want).max()


def test_batch_with_bad_jobs(inst):
    ps = _problems(5, 40, 50, 3, seed=77)

    def tamper(jobs):
        jobs[1].out = None
        jobs[3].gx = jobs[3].gx + 2          # not 4-byte aligned
    configure(inst, capi.SC_METHOD_AUTO)
    rc, outs, jobs, info, dev, full, ids = _batch(inst, ps, tamper=tamper)
    dev.free()
    assert rc == capi.SC_ERR_BAD_ARG
    assert [j.rc for j in jobs] == [capi.SC_OK, capi.SC_ERR_BAD_ARG, capi.SC_OK, capi.SC_ERR_BAD_ARG, capi.SC_OK]
    for k in (1, 3):
        assert np.all(outs[k] == -3.5), k                # skipped: never written
    for k in (0, 2, 4):
        b, gx, gy = ps[k]
        want = dn.solve_free(dn.divergence(gx, gy), b)
        assert np.abs(outs[k] - want).max() <= BOUND["auto"] * np.abs(want).max(), k


def test_batch_rgba_layout_leaves_the_fourth_float(inst):
    ps = _problems(3, 33, 45, 3, seed=5)
    configure(inst, capi.SC_METHOD_FFT)
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


@pytest.mark.parametrize("method", [capi.SC_METHOD_MULTIGRID, capi.SC_METHOD_JACOBI, capi.SC_METHOD_RBGS, capi.SC_METHOD_SOR,
                                    capi.SC_METHOD_DST])
def test_other_methods_are_refused_and_write_nothing(inst, method):
    H, W, C = 40, 50, 3
    rng = np.random.default_rng(1)
    g = rng.normal(0, 10, (H, W, C)).astype(np.float32)
    configure(inst, method)
    out = np.full((H, W, C), -7.25, np.float32)
    with pytest.raises(capi.SeamlessCloneError) as e:
        inst.poisson(None, gx=g, gy=g, out=out, neumann=True)
    assert e.value.code == capi.SC_ERR_BAD_ARG
    assert "SC_METHOD_AUTO" in str(e.value) and "SC_METHOD_FFT" in str(e.value)
    assert np.all(out == -7.25)
    rc, outs, jobs, info, dev, full, ids = _batch(inst, _problems(2, H, W, C, seed=2))
    dev.free()
    assert rc == capi.SC_ERR_BAD_ARG and np.array_equal(full, dev.host)


def test_double_transforms_stop_at_4096_per_side(inst):
    g = np.zeros((8, 4097, 1), np.float32)
    configure(inst, capi.SC_METHOD_FFT, capi.SC_FLAG_FFT_FP64)
    out = np.full_like(g, -7.25)
    with pytest.raises(capi.SeamlessCloneError) as e:
        inst.poisson(None, lap=g, out=out, neumann=True)
    assert e.value.code == capi.SC_ERR_BAD_SIZE and np.all(out == -7.25)
    configure(inst, capi.SC_METHOD_FFT)
    assert not inst.poisson(None, lap=g, out=out, neumann=True).any()            # float32 transforms take it: lap = 0 -> u = 0


def test_host_call_reports_stage_times(inst):
    rng = np.random.default_rng(2)
    b = rng.uniform(-50, 300, (500, 600, 3)).astype(np.float32)
    gx, gy = dn.forward_differences(b)
    configure(inst, capi.SC_METHOD_AUTO)
    inst.poisson(b, gx=gx, gy=gy, neumann=True)
    i = inst.info()
    assert i.ms_pre > 0 and i.ms_solve > 0 and i.ms_post >= 0 and i.ms_call >= i.ms_device_total > 0
    assert i.ms_h2d > 0 and i.ms_d2h > 0


def test_the_instance_after_a_neumann_call():
    """A Dirichlet Poisson call, a clone and an edit on an instance that solved Neumann problems give the bytes of a fresh instance (the
    DCT tables share the DST tables' cache, at lengths both kinds use here); its options are unchanged."""
    from oracle import oracle_np
    dst, patch, mask, cx, cy = oracle_np.synth_inputs(300, 200, margin=32)
    emask = np.zeros(dst.shape[:2], np.uint8)
    emask[40:160, 60:260] = 255
    rng = np.random.default_rng(1)
    img = rng.uniform(-50, 300, (200, 300, 3)).astype(np.float32)
    gx, gy = poisson_np.forward_differences(img)

    def dirichlet_clone_and_edit(i):
        body = dst.copy()
        i.run(patch, body, mask, cx, cy)
        ed = i.edit(i.edit_params(capi.SC_EDIT_COLOR_CHANGE, red_mul=1.5), dst, emask)
        return i.poisson(img, gx=gx, gy=gy, tol=0.05), body, ed

    for method, flags in ((capi.SC_METHOD_AUTO, 0), (capi.SC_METHOD_FFT, 0), (capi.SC_METHOD_FFT, capi.SC_FLAG_FFT_FP64)):
        fresh = capi.Instance(0)
        used = capi.Instance(0)
        try:
            fresh.set_solver(method=method, flags=fresh.default_opts().flags | flags)
            used.set_solver(method=method, flags=used.default_opts().flags | flags)
            before = used.get_solver()
            for shape in ((200, 300, 3), (198, 298, 3), (64, 300, 1)):          # the image's lengths, the Dirichlet interior's, a clone ROI's
                g = rng.normal(0, 10, shape).astype(np.float32)
                used.poisson(None, gx=g, gy=g, neumann=True)
            assert bytes(before) == bytes(used.get_solver())
            a = dirichlet_clone_and_edit(fresh)
            b = dirichlet_clone_and_edit(used)
            for x, y in zip(a, b):
                assert np.array_equal(x, y), (method, flags)
            # ... and a Neumann call after those: the same bits as before them
            g = rng.normal(0, 10, (198, 298, 3)).astype(np.float32)
            assert np.array_equal(used.poisson(None, gx=g, gy=g, neumann=True), fresh.poisson(None, gx=g, gy=g, neumann=True))
        finally:
            fresh.destroy()
            used.destroy()


def test_poisson_solve_functions():
    import seamlesscloneoptimization_amd as pkg
    rng = np.random.default_rng(4)
    img = rng.uniform(-50, 300, (90, 120, 3)).astype(np.float32)
    gx, gy = dn.forward_differences(img)
    R = float(np.abs(img).max())
    out = pkg.poisson_solve(img, gx, gy, neumann=True)
    assert np.abs(out - img).max() <= BOUND["auto"] * R
    zero = pkg.poisson_solve(None, gx, gy, neumann=True, method=capi.SC_METHOD_FFT, flags=capi.SC_FLAG_FFT_FP64)
    assert np.abs(zero.astype(np.float64) - (img - dn.mean_of(img))).max() <= 1e-5 * R      # (img's own float32 differences)
    two = pkg.poisson_solve_batch([img, None], [gx, gx], [gy, gy], neumann=True)
    assert np.array_equal(two[0], out)
    assert np.array_equal(two[1], pkg.poisson_solve(None, gx, gy, neumann=True))
    lap = dn.divergence(gx, gy)
    one = pkg.poisson_solve_batch([img], laplacians=[lap], neumann=True)[0]
    assert np.array_equal(one, out)
    out2 = pkg.poisson_solve(img[:, :, 0], gx[:, :, 0].copy(), gy[:, :, 0].copy(), neumann=True)      # 2-D arrays are one channel
    assert out2.shape == img.shape[:2] and np.abs(out2 - img[:, :, 0]).max() <= BOUND["auto"] * R
