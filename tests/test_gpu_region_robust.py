"""GPU tests of the robust region solve (sc_hip_region_robust, sc_hip_region_robust_device) through capi: Lp penalties, isotropic and
joint-channel coupling included, on a domain of any shape, by reweighting on the device.

1. against the rounds of tests/region_robust_np.py on tests/region_robust_bounds.py's matrix through the host call, NaN in every element
   the header says is not read: ERR, RES and ENERGY within the bounds, a trace that does not rise, sweeps = the sum of the trace's
   iterations, the same bytes as the clean input, out's bits at KNOWN and OUTSIDE pixels data's and on the Dirichlet lines boundary's.
2. round by round at 12 x 19 and 5 x 260: max_rounds = 1, 2, 3 each within the bound of the restatement's iterate of that round, the
   trace's iteration counts within region_bounds' rule (twice the restatement's + SC_WEIGHTED_POLL).
3. the five ties of the header, byte for byte on out with equal sweeps.
4. what is written and what reaches the answer: guard bands around out untouched, KNOWN / OUTSIDE / Dirichlet bits kept, values at
   OUTSIDE pixels and at KNOWN pixels without an UNKNOWN neighbour change no byte of the answer (they would through any coefficient or
   right-hand side that is not 0 off the UNKNOWN pixels: the work plane holds M^-1's values there), out == data.
5. a device batch of 17 jobs -- two job tables, 16 + 1; a chunk holds 64 jobs of three channels, so 17 jobs cannot span two chunks --
   with one bad state and one job with links where the first has none: the codes, the others against the restatement's chunk.
6. the refusals, "nothing pins the channel" included.
7. behaviour against irls_exact: tv_inpaint keeps a step edge through a hole where inpaint's membrane does not;
   integrate_gradients_masked returns a smooth field on an annulus with 5 % gross outliers, where p = 2 does not.

The constants of region_robust_bounds were measured on one MI355X (profiles/region_robust_lengths.txt)."""
from __future__ import annotations

import numpy as np
import pytest

import seamlesscloneoptimization_amd as pkg
from seamlesscloneoptimization_amd import capi

import region_bounds as gb
import region_np
import region_robust_bounds as rb
import region_robust_np as rr

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
FIXED = dict(round_tol=-1.0, allow_not_converged=True)          # every round runs; an inner solve may run out of max_iters as the restatement's does
G = capi.SC_POISSON_GUIDANCE


@pytest.fixture(scope="module")
def inst():
    i = capi.Instance(0)
    yield i
    i.destroy()


def configure(inst, flags=0):
    d = inst.default_opts()
    inst.set_solver(**{k: getattr(d, k) for k, _ in capi.SolverOpts._fields_})
    inst.set_solver(flags=flags)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def solve(inst, p, pen, rounds, coupling=0, **kw):
    return inst.region_robust(**rb.call_args(p, pen, coupling, max_rounds=rounds, **{**FIXED, **kw}))


def quadratic(inst, p):
    """Instance.region on the robust call's input, guidance base, default precond_*: the quadratic round"""
    return inst.region(p["data"], p["state"], p["weight"], p["sx"], p["sy"], gx=p["gx"], gy=p["gy"], boundary=rr._boundary(p), free_sides=p["sides"],
                       periodic=p["periodic"], allow_not_converged=True)


def assert_copied_bits(p, out):
    k = region_np.kinds(p["sides"], p["periodic"], p["state"])
    out = out.reshape(k.shape)
    held = (k == region_np.KNOWN) | (k == region_np.OUTSIDE)
    assert np.array_equal(bits(out)[held], bits(p["data"].reshape(k.shape))[held]), "KNOWN and OUTSIDE pixels must be data's bits"
    line = k == region_np.DIRICHLET
    assert np.array_equal(bits(out)[line], bits(p["boundary"].reshape(k.shape))[line]), "Dirichlet lines must be boundary's bits"
    assert np.isfinite(out[k == region_np.UNKNOWN]).all(), "an unread element's NaN reached the answer"


def assert_round(tag, y, prev, out, k=None):
    bad, err, res = y.check(prev, out, k)
    eb, rb_ = y.bounds(k)
    print(f"{tag}: ERR {err:.3e} (bound {eb:.3e}) RES {res:.3e} (bound {rb_:.3e})")
    assert not bad, (tag, bad)


def assert_energy(tag, inst, y, out, rounds):
    energy, iters = inst.robust_trace()
    assert len(energy) == rounds + 1 and len(iters) == rounds + 1
    assert inst.info().sweeps == int(iters.sum())
    want = float(y.energy(out).sum())
    rel = abs(float(energy[-1]) - want) / want
    rise = max((float(b) - float(a)) / float(a) for a, b in zip(energy, energy[1:]))
    print(f"{tag}: ENERGY {rel:.3e} (bound {rb.ENERGY_REL:.1e}) largest step of the trace {rise:.3e}")
    assert rel <= rb.ENERGY_REL, (tag, rel)
    assert rise <= rb.ENERGY_REL, (tag, "the trace rose", list(energy))


# ---- 1. the matrix ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(rb.matrix())))
def test_against_the_reference_rounds(inst, i):
    configure(inst)
    clean, pen, coupling, y = rb.matrix_case(i)
    p = rb.nan_unread(clean)
    tag = " ".join(map(str, rb.matrix()[i]))
    prev = solve(inst, p, pen, rb.ROUNDS - 1, coupling)
    out = solve(inst, p, pen, rb.ROUNDS, coupling)
    assert_energy(tag, inst, y, out, rb.ROUNDS)
    assert_round(tag, y, prev, out)
    assert_copied_bits(clean, out)
    assert np.array_equal(bits(solve(inst, clean, pen, rb.ROUNDS, coupling)), bits(out)), "an element the header says is not read changed the answer"


# ---- 2. round by round -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [("frame", 12, 19, 3, "scatter", "sparse", "loguniform", 0, (1.0, 2.0), 1e-2),
                                  ("frame", 12, 19, 3, "split", None, None, 3, (1.0, 2.0), 1e-2),
                                  ("neumann", 5, 260, 1, "seam", None, None, 1, (0.8, 2.0), 1e-3),
                                  ("periodic_x", 5, 260, 3, "ellipse", "constant", "loguniform", 2, (1.0, 1.0), 1e-3)])
def test_round_by_round(inst, case):
    configure(inst)
    clean = rb.make_input(*case[:7])
    pen, coupling = rb.penalties(clean, case[8], case[9]), case[7]
    y = rb.Yardstick(clean, pen, coupling, rounds=3)
    p = rb.nan_unread(clean)
    prev = quadratic(inst, p)
    for k in (1, 2, 3):
        out = solve(inst, p, pen, k, coupling)
        _, iters = inst.robust_trace()
        assert len(iters) == k + 1 and inst.info().sweeps == int(iters.sum())
        assert all(int(a) <= 2 * b + gb.POLL for a, b in zip(iters, y.iters32)), (list(iters), y.iters32)
        assert_round(f"{case[0]} {case[1]} x {case[2]} coupling {coupling} round {k}", y, prev, out, k)
        prev = out


# ---- 3. ties ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp64", [False, True])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("links", [None, "loguniform"])
@pytest.mark.parametrize("coupling", rr.COUPLINGS)
def test_tie_a_every_state_zero_gives_the_robust_calls_bytes(inst, coupling, links, C, fp64):
    configure(inst, capi.SC_FLAG_FFT_FP64 if fp64 else 0)
    try:
        for border, exps in (("free_lt", (1.0, 2.0)), ("periodic_x", (0.8, 1.0))):
            p = rb.make_input(border, 12, 19, C, "zero", "sparse", links)
            assert not p["state"].any()
            pen = rb.penalties(p, exps, 1e-2)
            for kw in (dict(max_rounds=3, round_tol=-1.0), dict(max_rounds=0, round_tol=0.0)):          # fixed rounds, and the round rule's own stop
                got = inst.region_robust(**rb.call_args(p, pen, coupling, allow_not_converged=True, **kw))
                sweeps, conv, trace = inst.info().sweeps, inst.info().converged, inst.robust_trace()
                want = inst.robust(p["gx"], p["gy"], p["data"], p["weight"], p["sx"], p["sy"], boundary=rr._boundary(p), free_sides=p["sides"],
                                   periodic=p["periodic"], p_grad=pen[0], eps_grad=pen[2], p_data=pen[1], eps_data=pen[3], allow_not_converged=True,
                                   isotropic=bool(coupling & rr.ISO), joint_channels=bool(coupling & rr.JOINT), **kw)
                assert np.array_equal(bits(got), bits(want)), (border, kw)
                assert (sweeps, conv) == (inst.info().sweeps, inst.info().converged)
                assert np.array_equal(trace[1], inst.robust_trace()[1]) and np.array_equal(trace[0], inst.robust_trace()[0])
    finally:
        configure(inst)


@pytest.mark.parametrize("links", [None, "loguniform"])
@pytest.mark.parametrize("wkind", [None, "sparse"])
def test_tie_b_exponents_of_two_give_the_region_calls_bytes(inst, links, wkind):
    configure(inst)
    p = rb.nan_unread(rb.make_input("free_lt", 12, 19, 3, "scatter", wkind, links))
    for coupling in rr.COUPLINGS:
        out = solve(inst, p, (2.0, 2.0, 0.0, 0.0), 5, coupling)
        _, iters = inst.robust_trace()
        sweeps = inst.info().sweeps
        assert len(iters) == 1 and inst.info().converged == 1, "no reweighting round runs"
        assert np.array_equal(bits(out), bits(quadratic(inst, p))) and sweeps == inst.info().sweeps


@pytest.mark.parametrize("coupling", rr.COUPLINGS)
def test_ties_c_d_e_unit_links_zero_weights_and_two_runs(inst, coupling):
    configure(inst)
    # (c) link arrays of 1.0f give the bytes of NULL arrays; (e) two runs give the same bytes
    p = rb.make_input("periodic_x", 12, 19, 3, "split", "constant", None)
    pen = rb.penalties(p, (1.0, 1.0), 1e-2)
    want = solve(inst, p, pen, 3, coupling)
    sweeps = inst.info().sweeps
    ones = np.ones_like(p["data"])
    assert np.array_equal(bits(solve(inst, dict(p, sx=ones, sy=ones), pen, 3, coupling)), bits(want)) and inst.info().sweeps == sweeps
    assert np.array_equal(bits(solve(inst, p, pen, 3, coupling)), bits(want)) and inst.info().sweeps == sweeps
    # (d) every state 0 with weight NULL gives the bytes of a weight array of 0.0f (a frame: its Dirichlet lines pin the channels)
    p = rb.make_input("frame", 12, 19, 3, "zero", None, "loguniform")
    assert not p["state"].any()
    pen = rb.penalties(p, (0.8, 1.0), 1e-3)
    want = solve(inst, p, pen, 3, coupling)
    sweeps = inst.info().sweeps
    assert np.array_equal(bits(solve(inst, dict(p, weight=np.zeros_like(p["data"])), pen, 3, coupling)), bits(want)) and inst.info().sweeps == sweeps


# ---- 4. what is written, what reaches the answer -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("coupling", [0, 3])
def test_guard_bands_and_copied_bits(inst, coupling):
    configure(inst)
    clean = rb.make_input("free_lt", 12, 19, 3, "scatter", "sparse", "loguniform")
    pen = rb.penalties(clean, (1.0, 2.0), 1e-2)
    want = solve(inst, clean, pen, 2, coupling)
    H, W, C = clean["data"].shape

    def padded(a, fill):          # the array as a view inside a larger one: two guard rows above and below, three guard columns each side
        big = np.full((H + 4, W + 6, C), fill, np.float32)
        big[2:H + 2, 3:W + 3] = a
        return big, big[2:H + 2, 3:W + 3]
    p = rb.nan_unread(clean)
    views = {n: padded(p[n], np.nan)[1] for n in ("gx", "gy", "data", "state", "weight", "sx", "sy")}
    big, out = padded(np.full((H, W, C), SENTINEL, np.float32), SENTINEL)
    # through the C entry, so that every array is read and written in place under the padded layout (free left + top: boundary's right
    # and bottom lines are read)
    import ctypes
    views["boundary"] = padded(p["boundary"], np.nan)[1]
    lay = capi.poisson_layout_of(out)
    assert lay.row_stride == (W + 6) * C
    kind = G | capi.border_bits(clean["sides"], False, clean["periodic"]) | capi.robust_coupling_bits(bool(coupling & 1), bool(coupling & 2))
    prm = capi.RobustParams(kind, pen[0], pen[2], pen[1], pen[3], 2, -1.0, 0.0, 0)
    rc = inst.L.sc_hip_region_robust(inst.h, ctypes.byref(prm), ctypes.byref(lay), *(views[n].ctypes.data for n in
                                     ("gx", "gy", "data", "state", "weight", "sx", "sy", "boundary")), out.ctypes.data)
    assert rc in (capi.SC_OK, capi.SC_ERR_NOT_CONVERGED)
    assert np.array_equal(bits(out), bits(want))
    guard = np.ones(big.shape, bool)
    guard[2:H + 2, 3:W + 3] = False
    assert (big[guard] == np.float32(SENTINEL)).all(), "a guard band around out was written"
    assert_copied_bits(clean, out)


@pytest.mark.parametrize("coupling", [0, 1, 2, 3])
def test_nothing_off_the_unknown_pixels_reaches_the_answer(inst, coupling):
    """the zero condition, seen from outside: values at OUTSIDE pixels and at KNOWN pixels without an UNKNOWN neighbour are copied and
    nothing else -- through a right-hand side or a coefficient that is not 0 there they would change the iteration's dot products"""
    configure(inst)
    p = rb.make_input("neumann", 12, 19, 3, "ellipse", None, "loguniform")
    p["state"][2:5, 14:17, :] = 2
    pen = rb.penalties(p, (1.0, 2.0), 1e-2)
    k = region_np.kinds(p["sides"], p["periodic"], p["state"])
    near = np.zeros(k.shape, bool)
    for shift, axis in ((1, 0), (-1, 0), (1, 1), (-1, 1)):
        near |= region_np._neighbour(k, shift, axis, p["periodic"], region_np.OUTSIDE) == region_np.UNKNOWN
    far = (k == region_np.OUTSIDE) | ((k == region_np.KNOWN) & ~near)
    assert (k == region_np.OUTSIDE).any() and ((k == region_np.KNOWN) & ~near).any()
    want = solve(inst, p, pen, 3, coupling)
    sweeps = inst.info().sweeps
    rng = np.random.default_rng(9)
    q = dict(p, data=np.where(far, (1e30 * rng.standard_normal(k.shape)).astype(np.float32), p["data"]))
    got = solve(inst, q, pen, 3, coupling)
    unk = k == region_np.UNKNOWN
    assert np.array_equal(bits(got)[unk], bits(want)[unk]) and inst.info().sweeps == sweeps
    assert_copied_bits(q, got)


def test_out_may_be_data(inst):
    configure(inst)
    p = rb.make_input("frame", 12, 19, 3, "split", "constant", None)
    pen = rb.penalties(p, (1.0, 2.0), 1e-2)
    want = solve(inst, p, pen, 2, 1)
    data = p["data"].copy()
    got = inst.region_robust(**rb.call_args(dict(p, data=data), pen, 1, max_rounds=2, out=data, **FIXED))
    assert got is data and np.array_equal(bits(data), bits(want))


# ---- 5. a device batch -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coupling", [0, rr.ISO | rr.JOINT, rr.ISO])      # (coupled: the second job table's rho planes)
def test_a_batch_of_seventeen_jobs(inst, coupling):
    configure(inst)
    n, bad_state, stray = 17, 5, 16
    case = ("free_lt", 9, 11, 3, "scatter", "sparse", None)
    probs = [rb.make_input(*case, seed=20 + k) for k in range(n)]
    pen = rb.penalties(probs[0], (1.0, 2.0), 1e-2)
    members = [dict(p) for p in probs]
    members[bad_state]["state"] = probs[bad_state]["state"].copy()
    members[bad_state]["state"][3, 4, 1] = 3.0
    ones = np.ones_like(probs[0]["data"])
    members[stray].update(sx=ones, sy=ones)          # links where the first job has none
    H, W, C = probs[0]["data"].shape
    jobs = capi.Instance.make_region_robust_jobs(n)
    dev = []
    for k, p in enumerate(members):
        fields = dict(gx=p["gx"], gy=p["gy"], data=p["data"], state=p["state"], weight=p["weight"], smooth_x=p["sx"], smooth_y=p["sy"],
                      boundary=rr._boundary(p))
        for name, a in fields.items():
            if a is not None:
                dev.append(inst.to_device(np.ascontiguousarray(a, np.float32)))
                setattr(jobs[k], name, dev[-1])
        dev.append(inst.to_device(np.full((H, W, C), SENTINEL, np.float32)))
        jobs[k].out = dev[-1]
    try:
        kind = G | capi.border_bits(probs[0]["sides"], False, probs[0]["periodic"]) | capi.robust_coupling_bits(bool(coupling & rr.ISO), bool(coupling & rr.JOINT))
        params = capi.RobustParams(kind, pen[0], pen[2], pen[1], pen[3], rb.ROUNDS, -1.0, 0.0, 0)
        rc = inst.region_robust_device(params, capi.poisson_layout_of(probs[0]["data"]), jobs, allow_job_errors=True)
        codes = [j.rc for j in jobs]
        outs = [inst.from_device(j.out, (H, W, C), np.float32) for j in jobs]
    finally:
        for q in dev:
            inst.free(q)
    refused = (bad_state, stray)
    assert rc == capi.SC_ERR_BAD_ARG and codes == [capi.SC_ERR_BAD_ARG if k in refused else capi.SC_OK for k in range(n)]
    for k in refused:
        assert (outs[k] == np.float32(SENTINEL)).all(), "a refused job's out was written"
    stay = [k for k in range(n) if k not in refused]
    chunk = rr.irls_f32([probs[k] for k in stay], pen, rb.ROUNDS, coupling)
    for k, (u32, its) in zip(stay, chunk):
        y = rb.Yardstick(probs[k], pen, coupling, u32=u32, iters32=its)
        err, res = y.measure(u32[-2], outs[k])          # (the iterate before the last: the restatement's, the library's own stays on the device)
        eb, _ = y.bounds()
        assert err <= eb, (k, err, eb)
        assert_copied_bits(probs[k], outs[k])
    # one member against its solo run: they differ by no more than both bounds
    k = stay[-1]
    y = rb.Yardstick(probs[k], pen, coupling)
    solo = solve(inst, probs[k], pen, rb.ROUNDS, coupling)
    assert float(np.abs(outs[k] - solo).max()) / probs[k]["range"] <= 2 * max(rb.ERR_FACTOR * y.err32, rb.ERR_FLOOR)


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals(inst):
    configure(inst)
    p = rb.make_input("neumann", 12, 19, 3, "ellipse", "sparse", "loguniform")
    pen = rb.penalties(p, (1.0, 2.0), 1e-2)
    unk = np.argwhere(region_np.kinds(p["sides"], p["periodic"], p["state"]) == region_np.UNKNOWN)

    def refused(q, why, coupling=0):
        with pytest.raises(capi.SeamlessCloneError) as e:
            solve(inst, q, pen, 2, coupling)
        assert e.value.code == capi.SC_ERR_BAD_ARG and why in str(e.value), str(e.value)
    # nothing pins the channel: no Dirichlet line, every pixel UNKNOWN, no weight -- in one channel only
    loose = dict(p, weight=None, state=p["state"].copy())
    loose["state"][:, :, 1] = 0
    refused(loose, "nothing pins the channel")
    refused(loose, "nothing pins the channel", 3)
    w = p["weight"].copy()
    w[tuple(unk[3])] = -1.0
    refused(dict(p, weight=w), "weight")
    sx = p["sx"].copy()
    lx, _ = region_np.live_links(p["sides"], p["periodic"], p["state"])
    sx[tuple(np.argwhere(lx)[7])] = 0.0
    refused(dict(p, sx=sx), "link")
    # through the C entry: a state that is not 0, 1 or 2 (the Python layer refuses it first), exactly one link array
    L, lay = inst.L, capi.poisson_layout_of(p["data"])
    prm = capi.RobustParams(G | capi.SC_POISSON_NEUMANN, 1.0, pen[2], 2.0, pen[3], 2, -1.0, 0.0, 0)
    out = np.full_like(p["data"], SENTINEL)
    st = p["state"].copy()
    st[tuple(unk[0])] = 0.5
    ptr = lambda a: None if a is None else a.ctypes.data
    import ctypes
    call = lambda **kw: L.sc_hip_region_robust(inst.h, ctypes.byref(prm), ctypes.byref(lay), *(ptr({**p, **kw}[n]) for n in
                                               ("gx", "gy", "data", "state", "weight", "sx", "sy")), None, out.ctypes.data)
    assert call(state=st) == capi.SC_ERR_BAD_ARG and (out == np.float32(SENTINEL)).all()
    assert call(sy=None) == capi.SC_ERR_BAD_ARG and call(gx=None) == capi.SC_ERR_BAD_ARG
    prm.p_grad = 2.5
    assert call() == capi.SC_ERR_BAD_ARG
    prm.p_grad, prm.kind = 1.0, capi.SC_POISSON_LAPLACIAN | capi.SC_POISSON_NEUMANN
    assert call() == capi.SC_ERR_BAD_ARG and (out == np.float32(SENTINEL)).all()


# ---- 7. behaviour ----------------------------------------------------------------------------------------------------------------------
def test_tv_inpaint_keeps_a_step_edge_where_the_membrane_does_not(inst):
    configure(inst)
    img, hole = rb.step_hole(24, 31)
    assert int(hole.sum()) == 9
    rounds = 15
    got = pkg.tv_inpaint(img, hole, p=1.0, eps=1e-2, isotropic=True, max_rounds=rounds, round_tol=-1.0)
    zero = np.zeros_like(img)
    state = np.where(hole, 0, 1).astype(np.float32)
    want = inst.region_robust(zero, zero, img, state, neumann=True, p_grad=1.0, eps_grad=1e-2, max_rounds=rounds, round_tol=-1.0, isotropic=True)
    assert np.array_equal(bits(got), bits(want)), "tv_inpaint is the call it documents"
    assert np.array_equal(bits(got)[~hole], bits(img)[~hole])
    p = dict(sides="lrtb", periodic="", state=state, weight=None, sx=None, sy=None, gx=zero, gy=zero, data=img, boundary=img, range=1.0)
    y = rb.Yardstick(p, (1.0, 2.0, 1e-2, 1e-2), rr.ISO, rounds=rounds)
    err = float(np.abs(got - y.exact[-1][:, :, 0])[hole].max())
    eb, _ = y.bounds()
    print(f"tv_inpaint: {err:.3e} from the float64 rounds (bound {eb:.3e}, irls_f32 {y.err32:.3e})")
    assert err <= eb
    membrane = pkg.inpaint(img, hole)
    tv_off, membrane_off = float(np.abs(got - img)[hole].max()), float(np.abs(membrane - img)[hole].max())
    print(f"tv_inpaint: {tv_off:.3f} of the step off its side, the membrane {membrane_off:.3f}")
    assert tv_off < 0.1 and membrane_off > 0.2


def test_masked_integration_ignores_gross_outliers(inst):
    configure(inst)
    gx, gy, valid, known, values, truth = rb.annulus_problem(33, 47)
    rounds = 8
    got = pkg.integrate_gradients_masked(gx, gy, valid, known, values, p=1.0, eps=1e-3, max_rounds=rounds, round_tol=-1.0)
    state = np.where(valid, np.where(known, 1, 0), 2).astype(np.float32)
    data = np.where(valid, values, 0).astype(np.float32)
    want = inst.region_robust(gx, gy, data, state, neumann=True, p_grad=1.0, eps_grad=1e-3, max_rounds=rounds, round_tol=-1.0)
    assert np.array_equal(bits(got), bits(want)), "integrate_gradients_masked is the call it documents"
    assert not got[~valid].any()
    scale = float(truth[valid].max() - truth[valid].min())
    p = dict(sides="lrtb", periodic="", state=state, weight=None, sx=None, sy=None, gx=gx, gy=gy, data=data, boundary=data, range=scale)
    y = rb.Yardstick(p, (1.0, 2.0, 1e-3, 1e-3), 0, rounds=rounds)
    unk = valid & ~known
    err = float(np.abs(got - y.exact[-1][:, :, 0])[unk].max()) / scale
    eb, _ = y.bounds()
    print(f"masked integration: {err:.3e} from the float64 rounds (bound {eb:.3e}, irls_f32 {y.err32:.3e})")
    assert err <= eb
    plain = pkg.integrate_gradients_masked(gx, gy, valid, known, values, p=2.0)
    robust_off, plain_off = (rb.error_up_to_a_constant(u, truth, unk, scale) for u in (got, plain))
    print(f"masked integration: L1 {robust_off:.3e} of the range from the field, least squares {plain_off:.3e}")
    assert robust_off * 20 <= plain_off
    # without anchors: the data term of weight `anchor` holds the constant
    free = pkg.integrate_gradients_masked(gx, gy, valid, p=1.0, eps=1e-3, anchor=1e-3, max_rounds=rounds, round_tol=-1.0)
    assert rb.error_up_to_a_constant(free, truth, valid, scale) * 20 <= plain_off
