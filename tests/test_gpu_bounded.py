"""GPU tests of the bounded solve (sc_hip_bounded, sc_hip_bounded_device, sc_hip_bounded_trace) through capi: the region problem under
lower <= u <= upper at every UNKNOWN pixel, by the primal-dual active set method.

1. against the float64 active-set reference (tests/bounded_np.py) on tests/bounded_bounds.py's matrix: 33 x 47, 16 x 5 and 300 x 9
   pixels, five border kinds, four state patterns, links and weights rotating, both forms of the right-hand side, bounds at the
   quartiles of the unconstrained answer -- both, upper only, lower only, per-pixel arrays --, 3 channels and 1: RANGE == 0, converged,
   the rounds within twice the reference's + 2, ERR, RES_FREE and SIGN within their measured bounds, the copied bits.  Every element
   the header says is not read holds NaN.
2. the exact ties: no finite bound, bounds the unconstrained answer satisfies (a trace of one entry each, the bytes of sc_hip_region),
   lower == upper (the bound's bits), two runs of one call.
3. the trace: changed ends in 0, the final set agrees with the reference's but for degenerate pixels; on one instance the robust
   calls' trace and this one stay apart, whichever call ran last.
4. layouts: HWC, CHW with padded rows, RGBA-strided C = 3 inside guard bands: nothing but the named elements is written; out may be data.
5. refusals: a NaN bound or lower > upper at an UNKNOWN pixel (not at a KNOWN one), a bound array's NULL-ness unlike the first job's.
6. batches: three jobs with different states and bounds, twenty 4-channel jobs, each against its solo run.
7. bounded_solve, poisson_clone_in_range and interpolate_in_range against the reference."""
from __future__ import annotations

import numpy as np
import pytest

from seamlesscloneoptimization_amd import capi, seamless_clone

import bounded_bounds as bb
import bounded_np
import direct_np
import region_bounds as rb
import region_np

pytestmark = pytest.mark.gpu

L, G = capi.SC_POISSON_LAPLACIAN, capi.SC_POISSON_GUIDANCE
SENTINEL = -7.25
BORDERS = {b[0]: b[1:] for b in rb.BORDERS}
INF = float("inf")


@pytest.fixture(scope="module")
def inst():
    i = capi.Instance(0)
    yield i
    i.destroy()


def configure(inst, flags=0):
    d = inst.default_opts()
    inst.set_solver(**{k: getattr(d, k) for k, _ in capi.SolverOpts._fields_})
    inst.set_solver(flags=flags)


def boundary_of(p):
    return p["boundary"] if region_np.has_dirichlet(p["sides"], p["periodic"]) else None


def borders_of(p):
    return dict(boundary=boundary_of(p), free_sides=p["sides"], periodic=p["periodic"])


def guidance_of(p, form):
    return dict(gx=p["gx"], gy=p["gy"]) if form == "guidance" else dict(lap=p["lap"])


def solve(inst, p, form="lap", **kw):
    return inst.bounded(p["data"], p["state"], p["lower"], p["upper"], p["weight"], p["sx"], p["sy"], **borders_of(p), **guidance_of(p, form), **kw)


def region(inst, p, form="lap", **kw):
    return inst.region(p["data"], p["state"], p["weight"], p["sx"], p["sy"], **borders_of(p), **guidance_of(p, form), **kw)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_copied_bits(p, out):
    """region's assertion: out at KNOWN and OUTSIDE pixels is data, on the Dirichlet lines boundary, bit for bit"""
    k = region_np.kinds(p["sides"], p["periodic"], p["state"])
    out = out.reshape(k.shape)
    held = (k == region_np.KNOWN) | (k == region_np.OUTSIDE)
    assert np.array_equal(bits(out)[held], bits(p["data"].reshape(k.shape))[held]), "KNOWN and OUTSIDE pixels must be data's bits"
    line = k == region_np.DIRICHLET
    assert np.array_equal(bits(out)[line], bits(p["boundary"].reshape(k.shape))[line]), "Dirichlet lines must be boundary's bits"
    assert np.isfinite(out[k == region_np.UNKNOWN]).all(), "an unread element's NaN reached the answer"


# ---- 1. against the active-set reference ----------------------------------------------------------------------------------------
_CASES = bb.matrix()
_IDS = [bb.case_id(c) for c in _CASES]


@pytest.mark.parametrize("case", _CASES, ids=_IDS)
def test_against_the_reference(inst, case):
    configure(inst)
    p, y = bb.case_input(case)
    assert y.rounds <= bb.MAX_REFERENCE_ROUNDS
    out = solve(inst, p, case[7])
    info = inst.info()
    changed, active, iters = inst.bounded_trace()
    bad, (rng, err, res, sign) = y.check(out)
    print(f"BOUNDED {bb.case_id(case)}: rounds {len(iters)} (reference {y.rounds}, pdas_f32 {y.rounds32}) sweeps {info.sweeps} "
          f"(pdas_f32 {sum(y.iters32)}) RANGE {rng:.3g} ERR {err:.3g} ({y.err32:.3g}) RES_FREE {res:.3g} ({y.res32:.3g}) "
          f"SIGN {sign:.3g} ({y.sign32:.3g})")
    assert (info.method, info.converged, info.W, info.H) == (capi.SC_METHOD_FFT, 1, case[2], case[1])
    assert rng == 0.0
    assert len(iters) <= y.max_rounds() and info.sweeps == int(iters.sum()), (len(iters), y.rounds)
    assert changed[-1] == 0 and (changed[:-1] > 0).all()
    assert not bad, bad
    assert_copied_bits(p, out)


# ---- 2. the exact ties --------------------------------------------------------------------------------------------------------------
_TIE = [(border, size) for border in ("neumann", "free_lt", "periodic_x") for size in ((47, 33), (9, 300))]
_TIE_IDS = [f"{b}-{s[1]}x{s[0]}" for b, s in _TIE]


def _tie_input(border, size):
    return rb.nan_unread(rb.make_input(border, size[0], size[1], 3, "scatter", "sparse", "loguniform", seed=5))


@pytest.mark.parametrize("border, size", _TIE, ids=_TIE_IDS)
def test_no_finite_bound_gives_the_region_bytes(inst, border, size):
    configure(inst)
    p = dict(_tie_input(border, size), lower=None, upper=None)
    for params in (dict(), dict(tol=3e-6, max_iters=77, precond_lambda=0.2, precond_smooth=0.4, allow_not_converged=True)):
        a = solve(inst, p, "guidance", **params)
        sweeps = inst.info().sweeps
        changed, active, iters = inst.bounded_trace()
        b = region(inst, p, "guidance", **params)
        assert a.tobytes() == b.tobytes() and sweeps == inst.info().sweeps
        assert (list(changed), list(active), list(iters)) == ([0], [0], [sweeps])


@pytest.mark.parametrize("border, size", _TIE, ids=_TIE_IDS)
def test_bounds_already_satisfied_give_the_region_bytes_after_one_mark(inst, border, size):
    configure(inst)
    p = _tie_input(border, size)
    b = region(inst, p, "guidance")
    sweeps = inst.info().sweeps
    unk = region_np.kinds(p["sides"], p["periodic"], p["state"]) == region_np.UNKNOWN
    lo, hi = np.float32(b[unk].min()), np.float32(b[unk].max())          # touched, not crossed
    ramp = np.where(unk, b + np.float32(0.5), np.float32(np.nan)).astype(np.float32)
    for lower, upper in ((lo, hi), (-INF, hi), (lo, None), (lo, ramp)):
        a = solve(inst, dict(p, lower=lower, upper=upper), "guidance")
        changed, active, iters = inst.bounded_trace()
        assert a.tobytes() == b.tobytes()
        assert (list(changed), list(active), list(iters)) == ([0], [0], [sweeps]) and inst.info().converged == 1


@pytest.mark.parametrize("border, size", _TIE, ids=_TIE_IDS)
def test_equal_bounds_give_the_bounds_bits(inst, border, size):
    configure(inst)
    p = _tie_input(border, size)
    k = region_np.kinds(p["sides"], p["periodic"], p["state"])
    unk = k == region_np.UNKNOWN
    rng = np.random.default_rng(1)
    level = np.where(unk, rng.standard_normal(k.shape), np.nan).astype(np.float32)
    level[tuple(np.argwhere(unk)[0])] = np.float32(-0.0)
    for lower, upper in ((np.float32(0.375), np.float32(0.375)), (level, level)):
        out = solve(inst, dict(p, lower=lower, upper=upper), "guidance")
        want = np.broadcast_to(np.float32(lower), k.shape)
        assert np.array_equal(bits(out)[unk], bits(want)[unk]) and inst.info().converged == 1
        assert_copied_bits(p, out)


def test_two_runs_give_the_same_bytes(inst):
    configure(inst)
    case = next(c for c in _CASES if c[0] == "periodic_x" and c[2] == 300 and c[8] == "both")
    p, _ = bb.case_input(case)
    a, ta = solve(inst, p, case[7]), inst.bounded_trace()
    b, tb = solve(inst, p, case[7]), inst.bounded_trace()
    assert a.tobytes() == b.tobytes() and all(np.array_equal(x, y) for x, y in zip(ta, tb)) and len(ta[0]) > 1


# ---- 3. the trace ---------------------------------------------------------------------------------------------------------------------
def test_the_trace_ends_on_the_references_set(inst):
    configure(inst)
    case = next(c for c in _CASES if c[0] == "free_lt" and c[2] == 300 and c[4] == "scatter")
    p, y = bb.case_input(case)
    out = region_np._hwc(solve(inst, p, case[7]))
    changed, active, iters = inst.bounded_trace()
    assert changed[-1] == 0 and len(changed) == len(active) == len(iters) > 2 and (iters[1:] > 0).all()
    lo, hi = bounded_np._bounds(out.shape, y.lower, y.upper)
    got = np.where(y.unk, np.where(out == hi, 1, np.where(out == lo, -1, 0)), 0)
    differ = (got != y.set) & y.unk
    n = int(y.unk.sum())
    # (a free pixel may sit on its bound: the count of the trace is that of the library's own set)
    assert int(active[-1]) <= int((got != 0).sum()) and abs(int(active[-1]) - int((y.set != 0).sum())) <= 0.01 * n
    assert int(differ.sum()) <= 0.01 * n, int(differ.sum())
    # A pixel the two disagree on is degenerate, at the inner tolerance's scale.  Its distance to the bound: one of the two answers sits
    # on the bound there, so the distance is at most |out - want|, within item 1's ERR bound.  Its residual, where the library left it
    # free: |r_i| <= ||r||_2 <= tol ||b||_2 <= tol sqrt(n) max |b| by the stop rule (tol 1e-5, n the plane's unknowns at the most).
    r = bounded_np.residual(y.args, y.boundary, out)
    b = region_np.folded_rhs(*y.args[:6], *y.args[6:], y.boundary)
    scale_b, scale_u = float(np.abs(b).max()), float(np.abs(y.want[y.unk]).max())
    dist = np.minimum(np.abs(out - lo), np.abs(out - hi))
    assert (dist[differ] <= y.bounds()[0] * scale_u).all()
    assert (np.abs(r[differ & (got == 0)]) <= 1e-5 * np.sqrt(y.unk.sum(axis=(0, 1)).max()) * scale_b).all()


def _robust_rounds(inst, p, rounds):
    inst.region_robust(p["gx"], p["gy"], p["data"], p["state"], p["weight"], p["sx"], p["sy"], **borders_of(p), p_grad=1.0, eps_grad=1e-2,
                       max_rounds=rounds, round_tol=-1.0)
    return inst.robust_trace()


@pytest.mark.parametrize("rounds", [2, 12], ids=["fewer_robust_rounds", "more_robust_rounds"])
def test_the_robust_and_the_bounded_trace_do_not_mix(inst, rounds):
    """one instance, a robust call and a bounded call in either order: each trace is its own family's last call, whole and unchanged
    by the other's (the robust call runs fewer rounds than the bounded one, then more)"""
    configure(inst)
    case = next(c for c in _CASES if c[0] == "periodic_x" and c[2] == 300 and c[8] == "both")
    p, _ = bb.case_input(case)
    energy, r_iters = _robust_rounds(inst, p, rounds)
    solve(inst, p, case[7])
    changed, active, b_iters = inst.bounded_trace()
    assert len(energy) == len(r_iters) == rounds + 1 and len(changed) == len(active) == len(b_iters) > 2 and len(b_iters) != len(r_iters)

    def same(got, want):
        return len(got) == len(want) and all(np.array_equal(x, y) for x, y in zip(got, want))
    # robust, then bounded: the robust trace is still the robust call's
    assert same(inst.robust_trace(), (energy, r_iters)) and same(inst.bounded_trace(), (changed, active, b_iters))
    # bounded, then robust
    _robust_rounds(inst, p, rounds)
    assert same(inst.bounded_trace(), (changed, active, b_iters)) and same(inst.robust_trace(), (energy, r_iters))
    solve(inst, p, case[7])
    assert same(inst.robust_trace(), (energy, r_iters)) and same(inst.bounded_trace(), (changed, active, b_iters))


# ---- 4. layouts -----------------------------------------------------------------------------------------------------------------------
def _layout_views(name, H, W, fill):
    if name == "hwc":
        back = np.full((H, W, 3), fill, np.float32)
        return back, back
    if name == "chw_padded":
        back = np.full((3, H, W + 5), fill, np.float32)
        return back, back[:, :, :W].transpose(1, 2, 0)
    back = np.full((H + 4, W, 4), fill, np.float32)          # RGBA-strided C = 3 inside guard bands of two rows
    return back, back[2:-2, :, :3]


_FIELDS = (("data", "data"), ("state", "state"), ("weight", "weight"), ("sx", "smooth_x"), ("sy", "smooth_y"), ("gx", "gx"), ("gy", "gy"),
           ("boundary", "boundary"), ("lower", "lower"), ("upper", "upper"))


@pytest.mark.parametrize("alias", ["none", "data"])
@pytest.mark.parametrize("layout", ["hwc", "chw_padded", "rgba_guarded"])
def test_layouts_write_only_named_elements(inst, layout, alias):
    configure(inst)
    H, W = 23, 17
    p = rb.nan_unread(rb.make_input("free_lt", H, W, 3, "scatter", "sparse", "loguniform", seed=3))
    y = bb.Yardstick(p, "guidance", "arrays", f32=False)
    p["lower"], p["upper"] = bb.nan_unread_bounds(p, y.lower, y.upper)
    arrays = {}
    for name, _ in _FIELDS + (("out", "out"),):
        back, view = _layout_views(layout, H, W, np.nan if name in ("sx", "sy", "gx", "gy", "lower", "upper") else SENTINEL)
        if name != "out":
            view[...] = p[name]
        arrays[name] = (back, view)
    lay = capi.poisson_layout_of(arrays["data"][1])
    off = lambda name: arrays[name][1].__array_interface__["data"][0] - arrays[name][0].__array_interface__["data"][0]
    dev = {name: inst.to_device(back) for name, (back, _) in arrays.items()}
    try:
        jobs = capi.Instance.make_bounded_jobs(1)
        j = jobs[0]
        for name, field in _FIELDS:
            setattr(j, field, dev[name] + off(name))
        target = "out" if alias == "none" else alias
        j.out = dev[target] + off(target)
        kind = G | capi.border_bits(p["sides"], False, p["periodic"])
        rc = inst.bounded_device(capi.BoundedParams(kind, 0.0, 0, 0.0, 0.0, -INF, INF, 0), lay, jobs)
        assert rc == capi.SC_OK and j.rc == capi.SC_OK and inst.info().converged == 1
        got_back = inst.from_device(dev[target], arrays[target][0].shape, np.float32)
        others = {n: inst.from_device(dev[n], arrays[n][0].shape, np.float32) for n in arrays if n != target}
    finally:
        for q in dev.values():
            inst.free(q)
    for n, a in others.items():
        assert np.array_equal(a, arrays[n][0], equal_nan=True), f"{n} was written"
    probe = arrays[target][0].copy()
    view_of = lambda back: back if layout == "hwc" else back[:, :, :W].transpose(1, 2, 0) if layout == "chw_padded" else back[2:-2, :, :3]
    got = view_of(got_back).copy()
    view_of(probe)[...] = got
    assert np.array_equal(probe, got_back, equal_nan=True), "padding, the 4th slot or a guard band was written"
    assert_copied_bits(p, got)
    rng, err, _, _ = y.measure(got)
    assert rng == 0.0 and err <= 1e-3, (rng, err)          # (the sharp bounds are item 1's; here: the answer is in place)


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------
def _device_jobs(inst, probs, skip=()):
    """BoundedJob array of the inputs on device arrays (lap form; a bound that is an array goes along), each with an out full of SENTINEL"""
    jobs = capi.Instance.make_bounded_jobs(len(probs))
    dev = []
    for k, p in enumerate(probs):
        for name, field in (("lap", "lap"), ("data", "data"), ("state", "state"), ("weight", "weight"), ("sx", "smooth_x"), ("sy", "smooth_y"),
                            ("boundary", "boundary"), ("lower", "lower"), ("upper", "upper")):
            if isinstance(p.get(name), np.ndarray) and p[name].ndim and (k, field) not in skip:
                dev.append(inst.to_device(np.ascontiguousarray(p[name], np.float32)))
                setattr(jobs[k], field, dev[-1])
        dev.append(inst.to_device(np.full(p["data"].shape, SENTINEL, np.float32)))
        jobs[k].out = dev[-1]
    return jobs, dev


def _run_jobs(inst, probs, lower, upper, skip=(), want_codes=None):
    """the device call with the scalars lower, upper; a refused job's out must be untouched, the others must hold their answers"""
    shape = probs[0]["data"].shape
    jobs, dev = _device_jobs(inst, probs, skip)
    try:
        kind = L | capi.border_bits(probs[0]["sides"], False, probs[0]["periodic"])
        rc = inst.bounded_device(capi.BoundedParams(kind, 0.0, 0, 0.0, 0.0, lower, upper, 0), capi.poisson_layout_of(probs[0]["data"]), jobs,
                                 allow_job_errors=True)
        codes = [j.rc for j in jobs]
        outs = [inst.from_device(j.out, shape, np.float32) for j in jobs]
    finally:
        for q in dev:
            inst.free(q)
    assert codes == want_codes and rc == (capi.SC_ERR_BAD_ARG if any(codes) else capi.SC_OK), (rc, codes)
    for k, code in enumerate(codes):
        if code != capi.SC_OK:
            assert (outs[k] == SENTINEL).all(), "a refused job must not be written"
        else:
            p = probs[k]
            lo, hi = (p[n] if isinstance(p.get(n), np.ndarray) and (k, n) not in skip else s for n, s in (("lower", lower), ("upper", upper)))
            y = bb.Yardstick(p, "lap", bounds=(lo, hi), f32=False)
            rng, err, _, _ = y.measure(outs[k])
            assert rng == 0.0 and err <= 1e-3, (k, rng, err)
            assert_copied_bits(p, outs[k])
    return outs


def _three(seed, arrays=True):
    probs = [rb.make_input("free_lt", 23, 17, 3, pat, "constant", "loguniform", seed=seed + k) for k, pat in enumerate(("ellipse", "scatter", "split"))]
    for p in probs:
        y = bb.Yardstick(p, "lap", "arrays", f32=False)
        p["lower"], p["upper"] = (y.lower.copy(), y.upper.copy()) if arrays else (None, None)
    return probs


def _unknown_pixel(p, nth=5):
    k = region_np.kinds(p["sides"], p["periodic"], p["state"])
    return tuple(np.argwhere(k == region_np.UNKNOWN)[nth]), tuple(np.argwhere(k == region_np.KNOWN)[nth])


@pytest.mark.parametrize("defect", ["nan_lower", "nan_upper", "crossed"])
def test_a_bad_bound_at_an_unknown_pixel_fails_its_job_only(inst, defect):
    configure(inst)
    ok = [capi.SC_OK] * 3

    def spoil(p, at):
        if defect == "crossed":
            p["lower"][at] = p["upper"][at] + np.float32(1.0)
        else:
            p["lower" if defect == "nan_lower" else "upper"][at] = np.nan
    probs = _three(20)
    spoil(probs[1], _unknown_pixel(probs[1])[1])          # at a KNOWN pixel the bounds are not read
    _run_jobs(inst, probs, -INF, INF, want_codes=ok)
    spoil(probs[1], _unknown_pixel(probs[1])[0])
    _run_jobs(inst, probs, -INF, INF, want_codes=[capi.SC_OK, capi.SC_ERR_BAD_ARG, capi.SC_OK])


def test_bound_arrays_must_agree_with_the_first_job(inst):
    configure(inst)
    bad = capi.SC_ERR_BAD_ARG
    # the first job has both arrays: one without an upper array is refused
    _run_jobs(inst, _three(30), -INF, INF, skip={(1, "upper")}, want_codes=[capi.SC_OK, bad, capi.SC_OK])
    # the first job has no lower array: one with it is refused; the scalar serves the others
    probs = _three(30)
    q25 = float(min(p["lower"].min() for p in probs))
    _run_jobs(inst, probs, q25, INF, skip={(0, "lower"), (2, "lower")}, want_codes=[capi.SC_OK, bad, capi.SC_OK])
    # no arrays at all, scalars only
    _run_jobs(inst, _three(30, arrays=False), -0.25, 0.5, want_codes=[capi.SC_OK] * 3)


def test_a_bound_array_must_not_overlap_out(inst):
    configure(inst)
    probs = _three(40)[:1]
    jobs, dev = _device_jobs(inst, probs)
    try:
        jobs[0].out = jobs[0].upper + 4 * 10
        kind = L | capi.border_bits(probs[0]["sides"], False, probs[0]["periodic"])
        rc = inst.bounded_device(capi.BoundedParams(kind, 0.0, 0, 0.0, 0.0, -INF, INF, 0), capi.poisson_layout_of(probs[0]["data"]), jobs,
                                 allow_job_errors=True)
        hi = inst.from_device(jobs[0].upper, probs[0]["upper"].shape, np.float32)
    finally:
        for q in dev:
            inst.free(q)
    assert rc == capi.SC_ERR_BAD_ARG and jobs[0].rc == capi.SC_ERR_BAD_ARG and np.array_equal(hi, probs[0]["upper"])


def test_scalar_bounds_are_refused_before_anything_runs(inst):
    configure(inst)
    p = rb.make_input("neumann", 23, 17, 3, "ellipse", None, None)
    lay = capi.poisson_layout_of(p["data"])
    for lo, hi in ((1.0, 0.5), (float("nan"), 1.0), (0.0, float("nan"))):
        jobs, dev = _device_jobs(inst, [p])
        try:
            with pytest.raises(capi.SeamlessCloneError) as e:
                inst.bounded_device(capi.BoundedParams(L | capi.SC_POISSON_NEUMANN, 0.0, 0, 0.0, 0.0, lo, hi, 0), lay, jobs)
            out = inst.from_device(jobs[0].out, p["data"].shape, np.float32)
        finally:
            for q in dev:
                inst.free(q)
        assert e.value.code == capi.SC_ERR_BAD_ARG and (out == SENTINEL).all()


# ---- 6. batches ---------------------------------------------------------------------------------------------------------------------------
def _batch(probs, lower, upper, **kw):
    return seamless_clone.bounded_solve_batch([p["data"] for p in probs], [p["state"] for p in probs], lower, upper,
                                              laplacians=[p["lap"] for p in probs],
                                              weights=None if probs[0]["weight"] is None else [p["weight"] for p in probs],
                                              smooth_xs=None if probs[0]["sx"] is None else [p["sx"] for p in probs],
                                              smooth_ys=None if probs[0]["sy"] is None else [p["sy"] for p in probs], **kw)


def _check_members(inst, probs, outs, bounds_of, solo_of):
    """every member within item 1's bounds of its own reference (the yardstick: its solo pdas_f32; a member and its solo run are two
    stopped iterations around one exact answer: within the sum of their ERR bounds of each other)"""
    for k, p in enumerate(probs):
        lo, hi = bounds_of(k)
        y = bb.Yardstick(p, "lap", bounds=(lo, hi), f32=k in solo_of)
        rng, err, res, sign = y.measure(outs[k])
        assert rng == 0.0, (k, rng)
        assert_copied_bits(p, outs[k])
        if k not in solo_of:
            assert err <= 1e-3, (k, err)
            continue
        bad, _ = y.check(outs[k])
        assert not bad, (k, bad)
        solo = solve(inst, dict(p, lower=lo, upper=hi))
        bad, m = y.check(solo)
        assert not bad and inst.info().converged == 1, (k, bad)
        diff = float(np.abs(outs[k].astype(np.float64) - solo)[y.unk].max()) / float(np.abs(y.want[y.unk]).max())
        print(f"BOUNDED batch member {k}: ERR {err:.3g}, solo ERR {m[1]:.3g}, max |member - solo| / R {diff:.3g} (bound {2 * y.bounds()[0]:.3g})")
        assert diff <= 2 * y.bounds()[0], (k, diff)


def test_batch_of_three_different_states_and_bounds(inst):
    """The third job's bounds lie outside its unconstrained answer: it rides along, in range from round 0 on.  The stop rule is joint
    across the chunk and the trace is the chunk's, so a member has no iteration count of its own to hold at 0; what riding along must
    mean for its answer is checked in its place: no later round moves it away from the unconstrained solve -- its bytes are those of
    sc_hip_region on the same input to the stop rule's error (two stopped iterations around one exact answer: the sum of their ERR
    bounds, tests/region_bounds.py)."""
    configure(inst)
    probs = [rb.nan_unread(rb.make_input("neumann", 23, 17, 3, pat, "sparse", "loguniform", seed=50 + k))
             for k, pat in enumerate(("ellipse", "scatter", "split"))]
    bounds = []
    for k, p in enumerate(probs):
        y = bb.Yardstick(p, "lap", "arrays", f32=False)
        wide = np.float32(10.0) * np.float32(np.abs(y.want[y.unk]).max())
        bounds.append(bb.nan_unread_bounds(p, y.lower - wide, y.upper + wide) if k == 2 else bb.nan_unread_bounds(p, y.lower, y.upper))
    lower, upper = [b[0] for b in bounds], [b[1] for b in bounds]
    runs = [_batch(probs, lower, upper, neumann=True) for _ in range(2)]
    for a, b in zip(*runs):
        assert a.tobytes() == b.tobytes(), "two identical calls must give identical bytes"
    _check_members(inst, probs, runs[0], lambda k: bounds[k], solo_of={0, 1, 2})
    # the member that was in range all along: its solo run is the region call's after one mark ...
    solo = solve(inst, dict(probs[2], lower=lower[2], upper=upper[2]))
    assert len(inst.bounded_trace()[0]) == 1
    free = region(inst, probs[2])
    assert solo.tobytes() == free.tobytes()
    # ... and in the batch, through every later round of the others, it stays the region call's answer to the stop rule's error
    y = rb.Yardstick(probs[2])
    unk = region_np.kinds(probs[2]["sides"], probs[2]["periodic"], probs[2]["state"]) == region_np.UNKNOWN
    diff = float(np.abs(runs[0][2].astype(np.float64) - free)[unk].max()) / float(np.abs(y.want[unk]).max())
    print(f"BOUNDED batch rider: max |member - region| / R {diff:.3g} (bound {2 * y.bounds()[0]:.3g})")
    assert diff <= 2 * y.bounds()[0], diff
    assert np.array_equal(bits(runs[0][2])[~unk], bits(free)[~unk])


def test_batch_of_twenty_four_channel_jobs(inst):
    configure(inst)
    n = 20
    probs = [rb.nan_unread(rb.make_input("periodic_x", 5, 16, 4, rb.PATTERNS[k % 4], None, "constant", seed=60 + k)) for k in range(n)]
    outs = _batch(probs, -0.3, 0.4, boundaries=[p["boundary"] for p in probs], neumann=False, free_sides="", periodic="x")
    _check_members(inst, probs, outs, lambda k: (np.float32(-0.3), np.float32(0.4)), solo_of={0, n - 1})


# ---- 7. the Python surface ------------------------------------------------------------------------------------------------------------------
def _image(H, W, C, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    return (0.5 + 0.3 * np.sin(xx / 6.0 + seed)[:, :, None] + 0.2 * np.cos(yy / 9.0)[:, :, None] * np.linspace(1.0, 0.4, C) +
            0.03 * rng.standard_normal((H, W, C))).astype(np.float32)


def _mask(H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    return ((yy - 20) / 13.0) ** 2 + ((xx - 15) / 9.0) ** 2 <= 1.0


def _surface_check(out, state, data, lap, lo, hi, sx=None, sy=None):
    st = np.broadcast_to(state[:, :, None], data.shape).astype(np.float32)
    p = dict(sides="lrtb", periodic="", state=st, data=data, weight=None, sx=sx, sy=sy, lap=lap, gx=None, gy=None, boundary=None)
    y = bb.Yardstick(p, "lap", bounds=(np.float32(lo), np.float32(hi)))
    bad, m = y.check(out)
    assert not bad, bad
    assert np.array_equal(bits(out)[st != 0], bits(data)[st != 0])
    return y


def test_bounded_solve_broadcasts_a_mask_and_validates():
    H, W = 47, 33
    img = _image(H, W, 3, 5)
    known = ~_mask(H, W)
    img[~known] = 0.0
    lap = np.full_like(img, -0.02)          # a load that lifts the membrane over its rim
    a = seamless_clone.bounded_solve(img, known, upper=0.6, laplacian=lap, validate=True)
    b = seamless_clone.bounded_solve(img, np.repeat(known[:, :, None], 3, 2).astype(np.uint8), None, np.full((H, W), 0.6, np.float32), laplacian=lap)
    assert a.tobytes() == b.tobytes()
    y = _surface_check(a, np.where(known, 1, 0), img, lap, -INF, 0.6)
    assert (y.set != 0).any() and a[~known].max() == np.float32(0.6)


@pytest.mark.parametrize("mixed", [False, True])
def test_poisson_clone_in_range(mixed):
    H, W = 47, 33
    mask = _mask(H, W)
    yy, xx = np.mgrid[0:H, 0:W]
    bump = np.exp(-(((yy - 20) / 6.0) ** 2 + ((xx - 15) / 5.0) ** 2))[:, :, None]
    src = (0.3 * _image(H, W, 3, 2) + 1.0 * bump).astype(np.float32)
    dst = np.clip(_image(H, W, 3, 3) + 0.2, 0, 1).astype(np.float32)
    free = seamless_clone.poisson_clone(src, dst, mask, mixed=mixed)
    assert free[mask].max() > 1.05, "the input must overshoot"
    out = seamless_clone.poisson_clone_in_range(src, dst, mask, mixed=mixed)
    gx, gy = direct_np.forward_differences(src)
    if mixed:
        dx, dy = direct_np.forward_differences(dst)
        gx, gy = np.where(np.abs(dx) > np.abs(gx), dx, gx), np.where(np.abs(dy) > np.abs(gy), dy, gy)
    st = np.broadcast_to(np.where(mask, 0, 1)[:, :, None], dst.shape).astype(np.float32)
    lap = region_np.divergence("lrtb", "", st, None, None, gx, gy)
    y = _surface_check(out, np.where(mask, 0, 1), dst, lap, 0.0, 1.0)
    assert out[mask].max() == np.float32(1.0) and out[mask].min() >= 0.0
    # not the clamped clone: the excess is spread over the free pixels
    assert np.abs(np.clip(free, 0, 1) - out)[mask].max() > 1e-3
    # bounds far outside the data: the bytes of poisson_clone
    assert seamless_clone.poisson_clone_in_range(src, dst, mask, lo=-100.0, hi=100.0, mixed=mixed).tobytes() == free.tobytes()


def test_interpolate_in_range_holds_the_samples_and_the_range():
    H, W = 47, 33
    rng = np.random.default_rng(9)
    vals = _image(H, W, 3, 4)
    known = rng.random((H, W)) < 0.05
    gx, gy = direct_np.forward_differences((2.0 * vals).astype(np.float32))          # gradients twice too steep: their integral leaves the range
    lo, hi = float(vals[known].min()), float(vals[known].max())
    out = seamless_clone.interpolate_in_range(vals, known, lo, hi, image_gradients=(gx, gy))
    st = np.broadcast_to(np.where(known, 1, 0)[:, :, None], vals.shape).astype(np.float32)
    lap = region_np.divergence("lrtb", "", st, None, None, gx, gy)
    y = _surface_check(out, np.where(known, 1, 0), vals, lap, lo, hi)
    assert (y.set > 0).any() and (y.set < 0).any() and np.array_equal(out[known], vals[known])
    assert out[~known].min() >= np.float32(lo) and out[~known].max() <= np.float32(hi)
    # with a guide: the bounded solve under the guide's link weights
    guide = (np.where(np.arange(W)[None, :] < W // 2, 0.0, 1.0) * np.ones((H, 1))).astype(np.float32)
    out = seamless_clone.interpolate_in_range(vals, known, lo, hi, guide=guide, edge_sigma=0.1, image_gradients=(gx, gy))
    sx, sy = ((np.exp(-d * d / (2.0 * 0.1 * 0.1)) + 1e-3).astype(np.float32) for d in seamless_clone._forward_abs_differences(guide))
    b3 = lambda a: np.ascontiguousarray(np.broadcast_to(a[:, :, None], vals.shape))
    lap = region_np.divergence("lrtb", "", st, b3(sx), b3(sy), gx, gy)
    _surface_check(out, np.where(known, 1, 0), vals, lap, lo, hi, b3(sx), b3(sy))
