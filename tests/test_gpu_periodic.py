"""The float32 Poisson and screened solves with periodic axes (SC_POISSON_PERIODIC_X / _Y) on the GPU: the nine combinations against the
float64 restatement (tests/direct_np.py), the identity and what is never read, the singular combinations, cyclic shifts, lengths 2
and 3, layouts, batches, refusals, the instance afterwards and make_tileable.  Bounds: tests/direct_bounds.py."""
import numpy as np
import pytest

import direct_np as pn
from direct_bounds import PERIODIC

Yardstick = PERIODIC.yardstick

pytestmark = pytest.mark.gpu

from seamlesscloneoptimization_amd import capi, seamless_clone  # noqa: E402

from test_gpu_neumann import Dev, _batch, _layout_views  # noqa: E402

G, L = capi.SC_POISSON_GUIDANCE, capi.SC_POISSON_LAPLACIAN
PREC = {"f32": 0, "f64": capi.SC_FLAG_FFT_FP64}
COMBOS = pn.COMBOS
SINGULAR = [c for c in COMBOS if pn.singular(*c)]
H0, W0, C0 = 29, 37, 3


def kind_of(sides, periodic, base=G):
    return base | capi.free_side_bits(sides) | capi.periodic_bits(periodic)


@pytest.fixture()
def inst():
    i = capi.Instance(0)
    yield i
    i.destroy()


def configure(inst, method=capi.SC_METHOD_FFT, prec="f32"):
    inst.set_solver(method=method, flags=(inst.default_opts().flags & ~capi.SC_FLAG_FFT_FP64) | PREC[prec])


_INPUTS = {}


def inputs(H=H0, W=W0, C=C0, seed=5):
    """(img, gx, gy of a random guidance field, boundary, data), computed once per shape and never changed"""
    key = (H, W, C, seed)
    if key not in _INPUTS:
        rng = np.random.default_rng(seed)
        img = rng.uniform(-50, 300, (H, W, C)).astype(np.float32)
        gx = rng.normal(0, 20, (H, W, C)).astype(np.float32)
        gy = rng.normal(0, 20, (H, W, C)).astype(np.float32)
        b = rng.uniform(-100, 400, (H, W, C)).astype(np.float32)
        d = rng.uniform(-50, 300, (H, W, C)).astype(np.float32)
        for a in (img, gx, gy, b, d):
            a.flags.writeable = False
        _INPUTS[key] = (img, gx, gy, b, d)
    return _INPUTS[key]


# ---- 1
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("sides,periodic", COMBOS)
def test_every_combination_against_the_restatement(inst, sides, periodic, prec):
    """37 x 29, C = 3: guidance, laplacian (the same bits), screened with lam 1e-3 and 10; SC_METHOD_AUTO is SC_METHOD_FFT."""
    img, gx, gy, b, d = inputs()
    lap = pn.divergence(gx, gy, periodic)
    known = pn.dirichlet_mask(sides, periodic, H0, W0)
    kw = dict(free_sides=sides, periodic=periodic)
    fails = []
    for method in (capi.SC_METHOD_FFT, capi.SC_METHOD_AUTO):
        configure(inst, method, prec)
        out = inst.poisson(b, gx=gx, gy=gy, **kw)
        i = inst.info()
        assert i.method == capi.SC_METHOD_FFT and i.sweeps == 1 and i.converged == 1 and (i.W, i.H) == (W0, H0)
        assert np.array_equal(inst.poisson(b, lap=lap, **kw), out)
        assert np.array_equal(out[known], b[known])
        bad, err, res = Yardstick(sides, periodic, 0.0, None, lap, b).check(out, prec == "f64")
        print("PER [%s] %s %s poisson ERR %.2e RES %.2e" % (sides, periodic, prec, err, res))
        fails.extend((sides, periodic, "poisson") + t for t in bad)
    for lam in (1e-3, 10.0):
        out = inst.screened(d, gx=gx, gy=gy, lam=lam, boundary=b, **kw)
        assert inst.info().method == capi.SC_METHOD_FFT
        assert np.array_equal(inst.screened(d, lap=lap, lam=lam, boundary=b, **kw), out)
        assert np.array_equal(out[known], b[known])
        bad, err, res = Yardstick(sides, periodic, lam, d, lap, b).check(out, prec == "f64")
        print("PER [%s] %s %s screened %g ERR %.2e RES %.2e" % (sides, periodic, prec, lam, err, res))
        fails.extend((sides, periodic, lam) + t for t in bad)
    assert not fails, fails


# ---- 2
@pytest.mark.parametrize("sides,periodic", COMBOS)
def test_wrapped_forward_differences_give_back_the_image(inst, sides, periodic):
    """g = the wrapped differences of I with boundary = I returns I (a singular combination: up to the mean, which boundary = I fixes),
    and so does the screened solve with d = I.  NaN where nothing is read: gx's last column / gy's last row along a non-periodic axis,
    boundary everywhere but on its Dirichlet lines."""
    img = inputs()[0]
    gx, gy = pn.forward_differences(img, periodic)
    lap = pn.divergence(gx, gy, periodic)
    if "x" not in periodic:
        gx[:, -1] = np.nan
    if "y" not in periodic:
        gy[-1] = np.nan
    known = pn.dirichlet_mask(sides, periodic, H0, W0)
    R = float(np.abs(img).max())
    kw = dict(free_sides=sides, periodic=periodic)
    configure(inst)
    y = Yardstick(sides, periodic, 0.0, None, lap, img)
    out = inst.poisson(img, gx=gx, gy=gy, **kw)
    assert np.isfinite(out).all() and np.abs(out - img).max() <= (y.bounds()[0] + 1e-5) * R      # 1e-5: the float32 differences of float32 pixels (solve_exact's own distance from I)
    assert np.array_equal(out[known], img[known])
    ys = Yardstick(sides, periodic, 0.5, img, lap, img)
    outs = inst.screened(img, gx=gx, gy=gy, lam=0.5, boundary=img, **kw)
    assert np.isfinite(outs).all() and np.abs(outs - img).max() <= (ys.bounds()[0] + 1e-5) * R
    if not pn.singular(sides, periodic):          # (a singular call reads all of boundary, for its mean)
        nb = img.copy()
        nb[~known] = np.nan
        assert np.array_equal(inst.poisson(nb, gx=gx, gy=gy, **kw), out)
        assert np.array_equal(inst.screened(img, gx=gx, gy=gy, lam=0.5, boundary=nb, **kw), outs)
    else:
        assert np.array_equal(inst.screened(img, gx=gx, gy=gy, lam=0.5, boundary=np.full_like(img, np.nan), **kw), outs)
    configure(inst, prec="f64")
    out = inst.poisson(img, gx=gx, gy=gy, **kw)
    assert np.abs(out - img).max() <= 1e-5 * R


# ---- 3
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("sides,periodic", SINGULAR)
def test_the_singular_combinations(inst, sides, periodic, prec):
    img, gx, gy, b, d = inputs()
    lap = pn.divergence(gx, gy, periodic)
    kw = dict(free_sides=sides, periodic=periodic)
    configure(inst, prec=prec)
    y = Yardstick(sides, periodic, 0.0, None, lap, b)
    eb = y.bounds()[0] if prec == "f32" else 1e-6
    out = inst.poisson(b, lap=lap, **kw)
    mean = lambda a: np.asarray(a, np.float64).mean(axis=(0, 1))          # noqa: E731
    assert np.abs(mean(out) - mean(b)).max() <= eb * y.R
    zero = inst.poisson(None, lap=lap, **kw)
    y0 = Yardstick(sides, periodic, 0.0, None, lap, None)
    assert np.abs(mean(zero)).max() <= eb * y0.R
    assert np.abs(zero.astype(np.float64) - y0.want).max() <= eb * y0.R
    shifted = inst.poisson(b, lap=lap + np.float32(3.0), **kw)              # lap's DC coefficient is ignored
    assert np.abs(shifted.astype(np.float64) - out).max() <= eb * y.R
    ys = Yardstick(sides, periodic, 0.25, d, lap + np.float32(3.0), None)  # screened: the DC is divided by -lam, no boundary
    souts = inst.screened(d, lap=lap + np.float32(3.0), lam=0.25, **kw)
    bad, err, res = ys.check(souts, prec == "f64")
    assert not bad, bad
    assert np.abs(mean(souts) - mean(ys.want)).max() <= (ys.bounds()[0] if prec == "f32" else 1e-6) * ys.R


# ---- 4
@pytest.mark.parametrize("periodic", pn.PERIODIC)
def test_cyclic_shift(inst, periodic):
    """Every input rolled by 5 along a periodic axis: the rolled output, within twice the ERR bound (each run is within the bound of the
    exact answer of its own problem, and those are rolls of each other).  A wrap term taken from the wrong end breaks it."""
    img, gx, gy, b, d = inputs()
    sides = ""
    configure(inst)
    for lam in (0.0, 1e-3):
        solve = (lambda d_, gx_, gy_, b_: inst.screened(d_, gx=gx_, gy=gy_, lam=lam, boundary=b_, free_sides=sides, periodic=periodic)) if lam else \
                (lambda d_, gx_, gy_, b_: inst.poisson(b_, gx=gx_, gy=gy_, free_sides=sides, periodic=periodic))
        out = solve(d, gx, gy, b)
        y = Yardstick(sides, periodic, lam, d, pn.divergence(gx, gy, periodic), b)
        assert np.abs(out.astype(np.float64) - y.want).max() <= y.bounds()[0] * y.R
        for axis, name in ((1, "x"), (0, "y")):
            if name not in periodic:
                continue
            r = lambda a: np.ascontiguousarray(np.roll(a, 5, axis))          # noqa: E731
            other = solve(r(d), r(gx), r(gy), r(b))
            assert np.abs(other.astype(np.float64) - r(out)).max() <= 2 * y.bounds()[0] * y.R, (periodic, name, lam)


# ---- 5
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("axis", ["x", "y"])
def test_lengths_2_and_3_along_a_periodic_axis(inst, axis, n):
    """1 x 1 .. 3 x 3 unknowns the other way (pixels less the other axis's Dirichlet lines), every kind of the other axis"""
    fails = []
    for sides, periodic in COMBOS:
        if axis not in periodic:
            continue
        for other_unknowns in (1, 2, 3):
            ax, ay = pn.axis_kinds(sides, periodic)
            ok = ay if axis == "x" else ax
            if ok == pn.PP and other_unknowns == 1:
                continue                                   # (a periodic axis has at least 2 pixels)
            other = other_unknowns + {pn.DD: 2, pn.DN: 1, pn.ND: 1, pn.NN: 0, pn.PP: 0}[ok]
            if other < 2:
                continue                                   # (an image is at least 2 x 2)
            W, H = (n, other) if axis == "x" else (other, n)
            img, gx, gy, b, d = inputs(H, W, 3, seed=10 * n + other)
            lap = pn.divergence(gx, gy, periodic)
            for prec in ("f32", "f64"):
                configure(inst, prec=prec)
                for lam in (0.0, 0.5):
                    if lam:
                        out = inst.screened(d, gx=gx, gy=gy, lam=lam, boundary=b, free_sides=sides, periodic=periodic)
                    else:
                        out = inst.poisson(b, gx=gx, gy=gy, free_sides=sides, periodic=periodic)
                    bad, err, res = Yardstick(sides, periodic, lam, d, lap, b).check(out, prec == "f64")
                    print("PER n=%d %s [%s] %s %dx%d %s lam %g ERR %.2e RES %.2e" % (n, axis, sides, periodic, W, H, prec, lam, err, res))
                    fails.extend((sides, periodic, W, H, prec, lam) + t for t in bad)
    assert not fails, fails


# ---- 6
@pytest.mark.parametrize("sides,periodic", [("", "x"), ("", "y"), ("", "xy"), ("t", "x")])
def test_layouts_give_the_same_bits_and_write_only_what_they_name(inst, sides, periodic):
    H, W, C = 43, 61, 3
    img, gx, gy, b, d = inputs(H, W, C, seed=9)
    kw = dict(free_sides=sides, periodic=periodic)
    configure(inst)
    for screened in (False, True):
        ref = None
        for kind in ("hwc", "chw", "padded", "rgba", "transposed"):
            make = _layout_views(H, W, C, kind, 0.0)
            vb, vx, vy, vd = make(b)[0], make(gx)[0], make(gy)[0], make(d)[0]
            vo, obuf = _layout_views(H, W, C, kind, -7.25)()
            before = obuf.copy()
            if screened:
                got = inst.screened(vd, gx=vx, gy=vy, lam=0.25, boundary=vb, out=vo, **kw)
            else:
                got = inst.poisson(vb, gx=vx, gy=vy, out=vo, **kw)
            assert got is vo
            named = np.ones(obuf.shape, bool)
            if kind == "padded":
                named[:, W:] = False
            elif kind == "rgba":
                named[:, :, C:] = False
            assert np.array_equal(obuf[~named], before[~named]), kind           # padding / the fourth float untouched
            out = np.array(vo)
            if ref is None:
                ref = out
            assert np.array_equal(out, ref), (kind, screened)
        vb = b.copy()                                                            # in place: out is boundary
        if screened:
            got = inst.screened(d, gx=gx, gy=gy, lam=0.25, boundary=vb, out=vb, **kw)
        else:
            got = inst.poisson(vb, gx=gx, gy=gy, out=vb, **kw)
        assert got is vb and np.array_equal(vb, ref)
        if screened:                                                             # ... out is data
            vd = d.copy()
            got = inst.screened(vd, gx=gx, gy=gy, lam=0.25, boundary=b, out=vd, **kw)
            assert got is vd and np.array_equal(vd, ref)


# ---- 7
def _problems(n, H, W, C, seed):
    rng = np.random.default_rng(seed)
    return [(rng.uniform(-50, 300, (H, W, C)).astype(np.float32), rng.normal(0, 15, (H, W, C)).astype(np.float32),
             rng.normal(0, 15, (H, W, C)).astype(np.float32)) for _ in range(n)]


@pytest.mark.parametrize("sides,periodic", [("", "x"), ("", "xy"), ("lr", "y")])
def test_batches_equal_their_solo_runs_bit_for_bit(inst, sides, periodic):
    n, H, W, C = 70, 10, 12, 3                               # 64 jobs per chunk: two chunks
    ps = _problems(n, H, W, C, seed=n)
    if pn.singular(sides, periodic):
        ps = [((None if k % 3 == 1 else b), gx, gy) for k, (b, gx, gy) in enumerate(ps)]          # some without boundary: mean zero
    configure(inst, capi.SC_METHOD_AUTO)                     # AUTO stays direct for n > 1
    rc, outs, jobs, info, dev, full, ids = _batch(inst, ps, kind=kind_of(sides, periodic))
    try:
        assert rc == capi.SC_OK and all(j.rc == capi.SC_OK for j in jobs)
        per = capi.SC_POISSON_MAX_PLANES // C
        last = n - per * ((n - 1) // per)
        assert info.method == capi.SC_METHOD_FFT and info.sweeps == 1 and info.converged == 1
        assert info.group_members == (last if last > 1 else 0)
        written = np.zeros(full.size, bool)                  # nothing outside the outputs' spans was written (guard bands, inputs)
        for (_, _, _, ko) in ids:
            off = dev.parts[ko][0] // 4
            written[off:off + H * W * C] = True
        assert np.array_equal(full[~written], dev.host[~written])
    finally:
        dev.free()
    for k, (b, gx, gy) in enumerate(ps):
        assert np.array_equal(outs[k], inst.poisson(b, gx=gx, gy=gy, free_sides=sides, periodic=periodic)), k
    b, gx, gy = ps[n - 1]
    bad, err, res = Yardstick(sides, periodic, 0.0, None, pn.divergence(gx, gy, periodic), b).check(outs[n - 1], False)
    assert not bad, bad


def test_batch_with_a_job_that_lacks_a_pointer(inst):
    ps = _problems(5, 10, 12, 3, seed=77)

    def tamper(jobs):
        jobs[1].boundary = None              # a Dirichlet line is left (top and bottom): boundary is required
        jobs[3].gy = None
    configure(inst, capi.SC_METHOD_AUTO)
    rc, outs, jobs, info, dev, full, ids = _batch(inst, ps, tamper=tamper, kind=kind_of("", "x"))
    dev.free()
    assert rc == capi.SC_ERR_BAD_ARG
    assert [j.rc for j in jobs] == [capi.SC_OK, capi.SC_ERR_BAD_ARG, capi.SC_OK, capi.SC_ERR_BAD_ARG, capi.SC_OK]
    for k in (1, 3):
        assert np.all(outs[k] == -3.5), k                # skipped: never written
    for k in (0, 2, 4):
        b, gx, gy = ps[k]
        assert np.array_equal(outs[k], inst.poisson(b, gx=gx, gy=gy, periodic="x")), k
    rc, outs, jobs, info, dev, full, ids = _batch(inst, ps, tamper=tamper, kind=kind_of("", "xy"))      # singular: boundary may be NULL
    dev.free()
    assert [j.rc for j in jobs] == [capi.SC_OK, capi.SC_OK, capi.SC_OK, capi.SC_ERR_BAD_ARG, capi.SC_OK]
    assert np.array_equal(outs[1], inst.poisson(None, gx=ps[1][1], gy=ps[1][2], periodic="xy"))


# ---- 8
@pytest.mark.parametrize("method", [capi.SC_METHOD_MULTIGRID, capi.SC_METHOD_JACOBI, capi.SC_METHOD_RBGS, capi.SC_METHOD_SOR,
                                    capi.SC_METHOD_DST])
def test_other_methods_are_refused_and_write_nothing(inst, method):
    H, W, C = 20, 24, 3
    g = np.random.default_rng(1).normal(0, 10, (H, W, C)).astype(np.float32)
    inst.set_solver(method=method)
    before = inst.get_solver()
    out = np.full((H, W, C), -7.25, np.float32)
    with pytest.raises(capi.SeamlessCloneError) as e:
        inst.poisson(g, gx=g, gy=g, out=out, periodic="x")
    assert e.value.code == capi.SC_ERR_BAD_ARG
    assert "SC_METHOD_AUTO" in str(e.value) and "SC_METHOD_FFT" in str(e.value)
    with pytest.raises(capi.SeamlessCloneError) as e:
        inst.screened(g, gx=g, gy=g, lam=1.0, out=out, periodic="xy")
    assert e.value.code == capi.SC_ERR_BAD_ARG and "SC_METHOD_FFT" in str(e.value)
    assert np.all(out == -7.25)
    rc, outs, jobs, info, dev, full, ids = _batch(inst, _problems(2, H, W, C, seed=2), kind=kind_of("", "y"))
    dev.free()
    assert rc == capi.SC_ERR_BAD_ARG and np.array_equal(full, dev.host)
    assert bytes(before) == bytes(inst.get_solver())


def test_fp64_length_limit_on_an_instance(inst):
    configure(inst, prec="f64")
    before = inst.get_solver()
    for shape, periodic in (((3, 4097, 1), "x"), ((4097, 3, 1), "y"), ((4097, 2, 1), "xy")):
        g = np.zeros(shape, np.float32)
        out = np.full(shape, -7.25, np.float32)
        with pytest.raises(capi.SeamlessCloneError) as e:
            inst.poisson(g, gx=g, gy=g, out=out, periodic=periodic)
        assert e.value.code == capi.SC_ERR_BAD_SIZE and np.all(out == -7.25)
        with pytest.raises(capi.SeamlessCloneError) as e:
            inst.screened(g, gx=g, gy=g, lam=1.0, boundary=g, out=out, periodic=periodic)
        assert e.value.code == capi.SC_ERR_BAD_SIZE and np.all(out == -7.25)
    assert bytes(before) == bytes(inst.get_solver())
    g = np.random.default_rng(3).normal(0, 10, (3, 4096, 1)).astype(np.float32)
    assert np.isfinite(inst.poisson(g, gx=g, gy=g, periodic="x")).all()          # 4096 is served


def test_the_instance_after_a_periodic_call():
    """A Dirichlet, a Neumann and a free-side call on an instance that solved periodic problems (at the same lengths: the tables share
    the cache, under their own kind) give the bits of a fresh instance; its options are unchanged."""
    rng = np.random.default_rng(1)
    img = rng.uniform(-50, 300, (60, 90, 3)).astype(np.float32)
    gx, gy = pn.forward_differences(img, "")

    def others(i):
        return (i.poisson(img, gx=gx, gy=gy, tol=0.05), i.poisson(img, gx=gx, gy=gy, neumann=True), i.poisson(img, gx=gx, gy=gy, free_sides="lt"),
                i.screened(img, gx=gx, gy=gy, lam=0.5, boundary=img, free_sides="r"))

    for method, flags in ((capi.SC_METHOD_AUTO, 0), (capi.SC_METHOD_FFT, 0), (capi.SC_METHOD_FFT, capi.SC_FLAG_FFT_FP64)):
        fresh, used = capi.Instance(0), capi.Instance(0)
        try:
            fresh.set_solver(method=method, flags=fresh.default_opts().flags | flags)
            used.set_solver(method=method, flags=used.default_opts().flags | flags)
            before = used.get_solver()
            first = others(used)
            for shape, sides, periodic in (((60, 90, 3), "", "xy"), ((60, 90, 3), "t", "x"), ((59, 89, 1), "lr", "y"), ((58, 88, 2), "", "y")):
                g = rng.normal(0, 10, shape).astype(np.float32)
                used.poisson(g, gx=g, gy=g, free_sides=sides, periodic=periodic)
                used.screened(g, gx=g, gy=g, lam=0.5, boundary=g, free_sides=sides, periodic=periodic)
            assert bytes(before) == bytes(used.get_solver())
            for x, y, z in zip(others(fresh), others(used), first):
                assert np.array_equal(x, y) and np.array_equal(x, z), (method, flags)
        finally:
            fresh.destroy()
            used.destroy()


# ---- 9
def test_make_tileable():
    H, W = 40, 48
    rng = np.random.default_rng(11)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    img = (2.0 * xx + 1.5 * yy)[:, :, None] + rng.normal(0, 1, (H, W, 3)).astype(np.float32)
    img = np.ascontiguousarray(img, np.float32)
    gx, gy = seamless_clone.wrapped_forward_differences(img, "")
    jump = lambda a: float(np.abs(a[:, 0] - a[:, -1]).mean())          # noqa: E731
    for axes, free in (("x", "tb"), ("xy", ""), ("y", "lr")):
        out = seamless_clone.make_tileable(img, axes=axes)
        assert np.array_equal(out, seamless_clone.poisson_solve(img, gx, gy, periodic=axes, free_sides=free))
        outs = seamless_clone.make_tileable(img, lam=0.01, axes=axes)
        assert np.array_equal(outs, seamless_clone.screened_solve(img, gx, gy, lam=0.01, periodic=axes))
        assert np.abs(out.astype(np.float64).mean(axis=(0, 1)) - img.astype(np.float64).mean(axis=(0, 1))).max() <= 1e-3
        if "x" in axes:
            assert jump(out) < 0.1 * jump(img) and jump(outs) < jump(img)
        if "y" in axes:
            assert float(np.abs(out[0] - out[-1]).mean()) < 0.1 * float(np.abs(img[0] - img[-1]).mean())
    two = seamless_clone.poisson_solve_batch([img, img], [gx, gx], [gy, gy], periodic="xy")
    assert np.array_equal(two[0], seamless_clone.make_tileable(img)) and np.array_equal(two[1], two[0])
    s = seamless_clone.screened_solve_batch([img], [gx], [gy], lam=0.01, periodic="x")
    assert np.array_equal(s[0], seamless_clone.make_tileable(img, lam=0.01, axes="x"))
    gf = seamless_clone.gradient_filter(img, 1.0, 0.5, periodic="xy")
    assert np.abs(gf - img).max() <= 1e-3 * np.abs(img).max()
