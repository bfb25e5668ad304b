"""GPU tests of the coupled flow volume solve (sc_hip_volume_flow_coupled, sc_hip_volume_flow_coupled_device) through capi: the coupled
volume call's magnitudes and rounds with every temporal link along a caller's whole-numbered flow, a temporal link owned by its source.

1. against the rounds of tests/volume_flow_coupled_np.py on tests/volume_flow_coupled_bounds.py's matrix through the host call, NaN in
   every element the header says is not read: ERR, RES and ENERGY within the bounds, a trace of ROUNDS + 1 entries whose iteration
   counts sum to info().sweeps, out's bits at KNOWN and OUTSIDE pixels data's and on the Dirichlet lines boundary's, the bytes of the
   clean input.
2. round by round on two inputs -- SPACE | TIME under split with periodic time, SPACE | CHANNELS with per-channel states under random
   --: max_rounds = 1, 2, 3 each within the bound of the restatement's iterate of that round.
3. ties, to the byte and with the trace's counts: a flow of zeros (-0.0 among them) and no flow arrays give sc_hip_volume_coupled for
   each of the five couplings, free and periodic time; coupling 0, CHANNELS on one channel and SPACE with p_grad = 2 give
   sc_hip_volume_flow_robust; every exponent 2 gives sc_hip_volume_flow; link arrays of ones give the bytes of none; two runs of a
   collapse and of a random input give the same bytes.
4. equivariance: the constant pan on rolled frames under periodic x and y against the straight coupled call on the unrolled frames,
   both held to the flow input's yardstick, under SPACE | TIME | CHANNELS.
5. tiling under SPACE | TIME, where the back link's rho is read where another workgroup wrote it: a frame seam inside a band, a link
   whose ends lie in different bands, in different 256-column groups, a link that wraps from frame T - 1 to frame 0; collapse under
   CHANNELS, where most pixels hold no link and one pixel has an arriving link from far away.
6. the device call: HWC and CHW with padded rows, a frame stride with a gap, guard frames, a sentinel around every output, nothing
   but the named elements written, out may be data.
7. batches: a fractional flow fails its volume only, in the first and in a later position (the matching and the rho planes follow the
   volumes that stay); a NaN weight fails its volume only; nine volumes run in two chunks.
8. what it is for: on a disc that pans by (2, 1) per frame, tv_denoise_video_along_flow(isotropic=True) against the straight isotropic
   call and against the anisotropic flow call -- the inequalities the float64 restatement shows with a clear margin.
9. volume_flow_coupled_solve and tv_denoise_video_along_flow give the bytes of the Instance.volume_flow_coupled call they document."""
from __future__ import annotations

import numpy as np
import pytest

import seamlesscloneoptimization_amd as pkg
from seamlesscloneoptimization_amd import capi

import volume_coupled_bounds as cb
import volume_flow_bounds as fb
import volume_flow_coupled_bounds as fcb
import volume_flow_coupled_np as vfc
import volume_flow_robust_bounds as frb
import volume_robust_np as vr
import volume_wls_np as vw

pytestmark = pytest.mark.gpu

G = capi.SC_POISSON_GUIDANCE
S, T_, J = vfc.SPACE, vfc.TIME, vfc.CHANNELS
SENTINEL = -7.25
FIXED = dict(round_tol=-1.0, allow_not_converged=True)          # every round runs; an inner solve may run out of max_iters as the restatement's does


@pytest.fixture(scope="module")
def inst():
    i = capi.Instance(0)
    yield i
    i.destroy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def solve(inst, p, pen, coupling, rounds, **kw):
    return inst.volume_flow_coupled(**fcb.call_args(p, pen, coupling, max_rounds=rounds, **FIXED, **kw))


def solve_straight(inst, p, pen, coupling, rounds, **kw):
    return inst.volume_coupled(**cb.call_args(p, pen, coupling, max_rounds=rounds, **FIXED, **kw))


def solve_uncoupled(inst, p, pen, rounds, **kw):
    return inst.volume_flow_robust(**frb.call_args(p, pen, max_rounds=rounds, **FIXED, **kw))


def quadratic(inst, p):
    """Instance.volume_flow on the call's input: the quadratic round"""
    return inst.volume_flow(p["data"], p["state"], p["flow"], p["weight"], p["sx"], p["sy"], p["smt"], p["gx"], p["gy"], p["gt"], boundary=vr._boundary(p),
                            tau=p["tau"], loop=p["tper"], free_sides=p["sides"], periodic=p["periodic"], allow_not_converged=True)


def trace(inst):
    energy, iters = inst.robust_trace()
    return energy.tobytes(), list(map(int, iters)), inst.info().sweeps


def assert_copied_bits(p, out):
    k = vw.kinds(p["sides"], p["periodic"], p["state"])
    out = out.reshape(k.shape)
    held = (k == vw.KNOWN) | (k == vw.OUTSIDE)
    assert np.array_equal(bits(out)[held], bits(p["data"].reshape(k.shape))[held]), "KNOWN and OUTSIDE pixels must be data's bits"
    line = k == vw.DIRICHLET
    assert np.array_equal(bits(out)[line], bits(p["boundary"].reshape(k.shape))[line]), "Dirichlet lines must be boundary's bits"
    assert np.isfinite(out[k == vw.UNKNOWN]).all(), "an unread element's NaN reached the answer"


def assert_round(tag, y, prev, out, k=None):
    bad, err, res = y.check(prev, out, k)
    eb, rb_ = y.bounds(k)
    e32, r32 = y.fig32[-1 if k is None else k]
    print(f"VOLUME_FLOW_COUPLED {tag}: ERR {err:.3e} (irls_f32 {e32:.3e}, bound {eb:.3e}) RES {res:.3e} (irls_f32 {r32:.3e}, bound {rb_:.3e})")
    assert not bad, (tag, bad)


def assert_energy(tag, inst, y, out, rounds):
    energy, iters = inst.robust_trace()
    assert len(energy) == rounds + 1 and len(iters) == rounds + 1
    assert inst.info().sweeps == int(iters.sum())
    want = float(y.energy(out).sum())
    rel = abs(float(energy[-1]) - want) / want
    print(f"VOLUME_FLOW_COUPLED {tag}: ENERGY {rel:.3e} (bound {fcb.ENERGY_REL:.1e}) iterations {list(map(int, iters))} (irls_f32 {y.iters32})")
    assert rel <= fcb.ENERGY_REL, (tag, rel)


# ---- 1. the matrix ---------------------------------------------------------------------------------------------------------------------
_CASES = fcb.matrix()
_IDS = [f"{b}-{W}x{H}x{C}x{T}-tau{tau:g}-{p}-{wk}-{ln}-{tm}-gt{int(gt)}-{'_'.join(f'{e:g}' for e in ex)}-eps{ef:g}-{fl}-{vfc.NAMES[cpl]}"
        for b, H, W, C, T, tau, p, wk, ln, tm, gt, ex, ef, fl, cpl in _CASES]


@pytest.mark.parametrize("i", range(len(_CASES)), ids=_IDS)
def test_against_the_reference_rounds(inst, i):
    clean, pen, coupling, y = fcb.matrix_case(i)
    assert max(y.rels32) <= 1e-5 and max(y.iters32) <= fcb.MAX_ITERS, "every round of the reference stops by its rule on every input"
    p = fcb.nan_unread(clean)
    prev = solve(inst, p, pen, coupling, fcb.ROUNDS - 1)
    out = solve(inst, p, pen, coupling, fcb.ROUNDS)
    assert_energy(_IDS[i], inst, y, out, fcb.ROUNDS)
    assert_round(_IDS[i], y, prev, out)
    assert_copied_bits(clean, out)
    assert np.array_equal(bits(solve(inst, clean, pen, coupling, fcb.ROUNDS)), bits(out)), "an element the header says is not read changed the answer"


# ---- 2. round by round -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [("frame", 12, 19, 3, 5, 1.0, "hole", "sparse", "xyt", "periodic", True, (1.0, 1.0, 2.0), 1e-2, "split", S | T_),
                                  ("neumann", 5, 260, 3, 3, 0.1, "scatter", None, "t", "free", True, (1.0, 2.0, 1.0), 1e-3, "random", S | J)],
                         ids=["frame-19x12x3x5-split-spacetime", "neumann-260x5x3x3-random-space+channels"])
def test_round_by_round(inst, case):
    clean = fcb.make_input(*case[:11], case[13])
    coupling = case[14]
    if coupling & J:
        assert (clean["state"] != clean["state"][..., :1]).any(), "states that differ between the channels"
    pen = fcb.penalties(clean, case[11], case[12])
    y = fcb.Yardstick(clean, pen, coupling, rounds=3)
    assert max(y.rels32) <= 1e-5
    p = fcb.nan_unread(clean)
    prev = quadratic(inst, p)
    for k in (1, 2, 3):
        out = solve(inst, p, pen, coupling, k)
        assert_round(f"{case[0]} {case[1]} x {case[2]} x {case[4]} {case[13]} {vfc.NAMES[coupling]} round {k}", y, prev, out, k)
        prev = out


# ---- 3. ties ---------------------------------------------------------------------------------------------------------------------------
def _zeros_with_minus_zero(p):
    f = np.zeros_like(p["flow"])
    f[:, ::2, 1::3] = -0.0
    return f


@pytest.mark.parametrize("coupling", vfc.LEGAL, ids=[vfc.NAMES[c] for c in vfc.LEGAL])
@pytest.mark.parametrize("time", fcb.TIMES)
def test_a_flow_of_zeros_and_no_flow_give_the_coupled_volume_call(inst, time, coupling):
    p = fcb.nan_unread(fcb.make_input("free_lt", 23, 17, 3, 4, 1.7, "scatter", "sparse", "xyt", time, True, "zero", seed=4))
    pen = fcb.penalties(p, (1.0, 1.0, 1.5) if coupling & T_ else (1.0, 0.8, 1.5), 1e-2)
    want = solve_straight(inst, p, pen, coupling, 3)
    want_trace = trace(inst)
    assert len(want_trace[1]) == 4
    got = solve(inst, dict(p, flow=_zeros_with_minus_zero(p)), pen, coupling, 3)
    assert got.tobytes() == want.tobytes() and trace(inst) == want_trace, "a flow of zeros: the bytes, the rounds' energies and their inner iterations"
    got = solve(inst, dict(p, flow=None), pen, coupling, 3)
    assert got.tobytes() == want.tobytes() and trace(inst) == want_trace, "no flow arrays: sc_hip_volume_coupled itself"


@pytest.mark.parametrize("what", ["coupling 0", "channels on one channel", "space with p_grad 2"])
def test_no_effective_coupling_gives_the_robust_flow_call(inst, what):
    C, coupling, exps = {"coupling 0": (3, 0, (1.0, 0.8, 1.5)), "channels on one channel": (1, J, (1.0, 0.8, 1.5)),
                         "space with p_grad 2": (3, S, (2.0, 1.0, 1.5))}[what]
    p = fcb.nan_unread(fcb.make_input("free_lt", 23, 17, C, 4, 1.7, "scatter", "sparse", "xyt", "periodic", True, "random", seed=4))
    pen = fcb.penalties(p, exps, 1e-2)
    assert vfc.effective(coupling, pen, C) == 0
    want = solve_uncoupled(inst, p, pen, 3)
    want_trace = trace(inst)
    got = solve(inst, p, pen, coupling, 3)
    assert got.tobytes() == want.tobytes() and trace(inst) == want_trace


@pytest.mark.parametrize("time", fcb.TIMES)
def test_exponents_of_two_give_the_bytes_of_the_flow_volume_call(inst, time):
    p = fcb.nan_unread(fcb.make_input("free_lt", 12, 19, 3, 5, 0.3, "scatter", "sparse", "xyt", time, True, "random", seed=6))
    for coupling in (S | T_ | J, S | J):
        out = solve(inst, p, (2.0, 2.0, 2.0, 0.0, 0.0, 0.0), coupling, 5)
        energy, iters = inst.robust_trace()
        assert len(iters) == 1 and inst.info().converged == 1, "no reweighting round runs"
        sweeps = inst.info().sweeps
        assert np.array_equal(bits(out), bits(quadratic(inst, p))) and inst.info().sweeps == sweeps


@pytest.mark.parametrize("coupling", [S | T_, S | J], ids=["spacetime", "space+channels"])
@pytest.mark.parametrize("time", fcb.TIMES)
def test_link_arrays_of_ones_give_the_bytes_of_none(inst, time, coupling):
    p = fcb.make_input("periodic_x", 12, 19, 3, 3, 10.0, "hole", "constant", "none", time, True, "split")
    pen = fcb.penalties(p, (1.0, 1.0, 1.0), 1e-2)
    want = solve(inst, p, pen, coupling, 3)
    want_trace = trace(inst)
    ones = np.ones_like(p["data"])
    q = dict(p, sx=ones, sy=ones, smt=np.ones_like(p["gt"]))
    assert np.array_equal(bits(solve(inst, q, pen, coupling, 3)), bits(want)) and trace(inst) == want_trace
    assert np.array_equal(bits(solve(inst, dict(p, smt=np.ones_like(p["gt"])), pen, coupling, 3)), bits(want)) and trace(inst) == want_trace


@pytest.mark.parametrize("coupling", [S | T_, S | T_ | J], ids=["spacetime", "spacetime+channels"])
@pytest.mark.parametrize("flow", ["collapse", "random"])
def test_two_runs_give_the_same_bytes(inst, flow, coupling):
    p = fcb.nan_unread(fcb.make_input("periodic_x", 47, 33, 3, 5, 1.0, "scatter", "sparse", "xyt", "periodic", True, flow))
    pen = fcb.penalties(p, (1.0, 1.0, 2.0), 1e-2)
    a = solve(inst, p, pen, coupling, 3)
    ta = trace(inst)
    b = solve(inst, p, pen, coupling, 3)
    assert a.tobytes() == b.tobytes() and trace(inst) == ta


# ---- 4. equivariance -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("time", fcb.TIMES)
def test_a_constant_pan_is_the_straight_coupled_call_on_rolled_frames(inst, time):
    """periodic x and y, every state 0, a sparse weight, flow = a constant pan (dx, dy): frame t rolled back by t pans turns every link
    into a straight one (under periodic time the wrapping link too when T pans are a whole number of periods: 6 frames x (3, 2) on
    18 x 12), and every pixel's own link stays its own, so the magnitudes are the straight call's.  The rolled straight answer is held
    to the flow input's yardstick, ERR and RES, as the flow call's own answer is: within the bounds, not to the byte, because the sums
    run in another order."""
    T, H, W, C, pan = 6, 12, 18, 3, (3, 2)
    coupling = S | T_ | J
    p = fcb.make_input("periodic_xy", H, W, C, T, 1.0, "all", "sparse", "xyt", time, True, "zero", seed=8)
    p["flow"] = np.broadcast_to(np.float32(pan), p["flow"].shape).copy()
    p["links"] = fb.links_of(p)
    pen = fcb.penalties(p, (1.0, 1.0, 2.0), 1e-2)
    y = fcb.Yardstick(p, pen, coupling, rounds=3)
    assert max(y.rels32) <= 1e-5
    prev, out = solve(inst, p, pen, coupling, 2), solve(inst, p, pen, coupling, 3)
    assert_round(f"pan {time}", y, prev, out)
    back = lambda a: a if a is None else np.stack([np.roll(a[t], (-t * pan[1], -t * pan[0]), (0, 1)) for t in range(a.shape[0])])
    q = {n: (back(a) if isinstance(a, np.ndarray) and n != "flow" else a) for n, a in p.items() if n != "links"}
    forward = lambda a: np.stack([np.roll(a[t], (t * pan[1], t * pan[0]), (0, 1)) for t in range(T)])
    sprev, sout = forward(solve_straight(inst, q, pen, coupling, 2)), forward(solve_straight(inst, q, pen, coupling, 3))
    assert_round(f"pan {time}, the rolled straight answer", y, sprev, sout)
    assert_copied_bits(p, sout)


# ---- 5. tiling -------------------------------------------------------------------------------------------------------------------------
# (border, H, W, T, time, flow, coupling, what the shape is there for)
_TILINGS = [("neumann", 47, 33, 5, "free", "split", S | T_, "seam_in_band"), ("neumann", 47, 33, 5, "free", "split", S | T_, "ends_in_other_bands"),
            ("neumann", 9, 300, 3, "free", "split", S | T_, "ends_in_other_groups"), ("neumann", 47, 33, 3, "periodic", "split", S | T_, "wrap_to_frame_0"),
            ("neumann", 47, 33, 5, "free", "collapse", J, "arrives_from_far"), ("neumann", 9, 300, 3, "free", "collapse", S | T_ | J, "arrives_from_far")]


@pytest.mark.parametrize("case", _TILINGS, ids=[f"{c[7]}-{c[2]}x{c[1]}x{c[3]}-{c[5]}-{vfc.NAMES[c[6]]}" for c in _TILINGS])
def test_links_across_the_tiling(inst, case):
    border, H, W, T, time, flow, coupling, what = case
    args = (dict(column=256, amount=5) if flow == "split" else dict(column=280)) if W > 256 else {}          # (collapse: onto column 280)
    clean = fcb.make_input(border, H, W, 3, T, 1.0, "scatter", "sparse", "t", time, True, flow, seed=11, **args)
    plan = capi.pcg_plan(W, H, G | capi.border_bits(clean["sides"], False, clean["periodic"]), T)
    ny, nx, rows = plan["ny"] // T, plan["nx"], plan["rows"]
    fwd, _ = clean["links"]
    src = np.flatnonzero(fwd.reshape(-1) >= 0)
    dst = fwd.reshape(-1)[src]
    if what == "seam_in_band":
        assert any(0 < (t * ny) % rows for t in range(1, T)), ("a frame boundary strictly inside a band", plan)
    elif what == "ends_in_other_bands":
        assert plan["bands"] > 1 and ((src // nx) // rows != (dst // nx) // rows).any(), ("a link whose ends lie in different bands", plan)
    elif what == "ends_in_other_groups":
        assert plan["cg"] > 1 and ((src % nx) // 256 != (dst % nx) // 256).any(), ("a link whose ends lie in different column groups", plan)
    elif what == "wrap_to_frame_0":
        wraps = (src // (nx * ny) == T - 1) & (dst // (nx * ny) == 0)
        assert wraps.any() and (src[wraps] % (nx * ny) != dst[wraps] % (nx * ny)).any(), "a link from frame T - 1 to another pixel of frame 0"
    else:
        held = fwd >= 0
        far = np.abs(src % nx - dst % nx) + np.abs((src // nx) % ny - (dst // nx) % ny)
        assert held[:-1].mean() < 0.5 and far.max() >= min(nx, ny) // 2, "most pixels hold no link, one arrives from far away"
    pen = fcb.penalties(clean, (1.0, 1.0, 2.0), 1e-2)
    y = fcb.Yardstick(clean, pen, coupling, rounds=2)
    assert max(y.rels32) <= 1e-5
    p = fcb.nan_unread(clean)
    prev, out = solve(inst, p, pen, coupling, 1), solve(inst, p, pen, coupling, 2)
    assert_energy(f"tiling {what} {flow}", inst, y, out, 2)
    assert_round(f"tiling {what} {flow}", y, prev, out)
    assert_copied_bits(clean, out)


# ---- 6. the device call ----------------------------------------------------------------------------------------------------------------
def _layout_views(name, T, H, W, fill):
    """(backing array filled with `fill`, its T x H x W x 3 view): a guard frame before and after, a gap between the frames"""
    if name == "hwc":
        back = np.full((T + 2, H + 2, W, 3), fill, np.float32)          # two rows between the frames
        return back, back[1:-1, :H]
    back = np.full((T + 2, 3, H + 1, W + 5), fill, np.float32)          # CHW, padded rows, a row between the planes
    return back, back[1:-1, :, :H, :W].transpose(0, 2, 3, 1)


_FIELDS = ("data", "state", "weight", "gx", "gy", "gt", "boundary", "smooth_x", "smooth_y", "smooth_t")
_NAMES = dict(smooth_x="sx", smooth_y="sy", smooth_t="smt")


def _params(p0, pen, rounds, stride=None):
    T, H, W, C = p0["data"].shape
    kind = G | capi.border_bits(p0["sides"], False, p0["periodic"])
    return capi.volume_robust_params(kind, T, H * W * C if stride is None else stride, p0["tau"], p0["tper"], pen[0], pen[3], pen[1], pen[4], pen[2],
                                     pen[5], rounds, -1.0)


@pytest.mark.parametrize("alias", ["none", "data"])
@pytest.mark.parametrize("layout,coupling", [("hwc", S | T_ | J), ("chw_padded", S | T_)], ids=["hwc-spacetime+channels", "chw_padded-spacetime"])
def test_device_layouts_write_only_named_elements(inst, layout, coupling, alias):
    T, H, W = 4, 23, 17
    clean = fcb.make_input("free_lt", H, W, 3, T, 1.3, "scatter", "sparse", "xyt", "periodic", True, "random", seed=3)          # Dirichlet lines right and bottom
    pen = fcb.penalties(clean, (1.0, 1.0, 2.0), 1e-2)
    p = fcb.nan_unread(clean)          # gt and smooth_t NaN where no live matched link has its source, the flow NaN off the work rectangle
    arrays = {}
    for name in _FIELDS + ("out",):
        back, view = _layout_views(layout, T, H, W, np.nan if name in ("gx", "gy", "gt", "smooth_x", "smooth_y", "smooth_t") else SENTINEL)
        if name != "out":
            view[...] = p[_NAMES.get(name, name)]          # (gt and smooth_t: T frames under periodic time)
        arrays[name] = (back, view)
    for name, plane in zip(("flow_x", "flow_y"), (p["flow"][..., 0], p["flow"][..., 1])):          # dense whatever the layout, a guard frame on either side
        back = np.full((T + 2, H, W), np.nan, np.float32)
        back[1:-1] = plane
        arrays[name] = (back, back[1:-1])
    lay = capi.poisson_layout_of(arrays["data"][1][0])
    stride = arrays["data"][1].strides[0] // 4
    assert stride > (H - 1) * lay.row_stride + (W - 1) * lay.col_stride + 2 * lay.channel_stride + 1, "the frames leave a gap"
    off = lambda name: arrays[name][1].__array_interface__["data"][0] - arrays[name][0].__array_interface__["data"][0]
    dev = {name: inst.to_device(back) for name, (back, _) in arrays.items()}
    try:
        jobs = capi.Instance.make_volume_flow_robust_jobs(1)
        j = jobs[0]
        for name in _FIELDS + ("flow_x", "flow_y"):
            setattr(j, name, dev[name] + off(name))
        target = "out" if alias == "none" else alias
        j.out = dev[target] + off(target)
        rc = inst.volume_flow_coupled_device(_params(clean, pen, 2, stride), coupling, lay, jobs)
        assert rc == capi.SC_OK and j.rc == capi.SC_OK
        got_back = inst.from_device(dev[target], arrays[target][0].shape, np.float32)
        others = {n: inst.from_device(dev[n], arrays[n][0].shape, np.float32) for n in arrays if n != target}
    finally:
        for q in dev.values():
            inst.free(q)
    for n, a in others.items():
        assert np.array_equal(a, arrays[n][0], equal_nan=True), f"{n} was written"
    view_of = lambda back: back[1:-1, :H] if layout == "hwc" else back[1:-1, :, :H, :W].transpose(0, 2, 3, 1)
    probe = arrays[target][0].copy()
    got = view_of(got_back).copy()
    view_of(probe)[...] = got
    assert np.array_equal(probe, got_back, equal_nan=True), "a guard frame, the padding or a gap between frames was written"
    assert_copied_bits(clean, got)
    assert got.tobytes() == solve(inst, clean, pen, coupling, 2).tobytes(), "the device call on any layout writes the host call's bytes"
    y = fcb.Yardstick(clean, pen, coupling, rounds=2)
    assert_round(f"device {layout} out={alias}", y, solve(inst, clean, pen, coupling, 1), got)


# ---- 7. batches ------------------------------------------------------------------------------------------------------------------------
def _device_jobs(inst, probs):
    """VolumeFlowRobustJob array of the inputs on dense device arrays, each with an out full of SENTINEL; (jobs, pointers to free)"""
    jobs = capi.Instance.make_volume_flow_robust_jobs(len(probs))
    dev = []
    for k, p in enumerate(probs):
        T, H, W = p["state"].shape[:3]
        fx, fy = (None, None) if p["flow"] is None else (p["fx"], p["fy"]) if "fx" in p else capi.volume_flow_planes(p["flow"], T, H, W, p["tper"])
        fields = dict(gx=p["gx"], gy=p["gy"], gt=p["gt"], data=p["data"], state=p["state"], weight=p["weight"], boundary=vr._boundary(p), smooth_x=p["sx"],
                      smooth_y=p["sy"], smooth_t=p["smt"], flow_x=fx, flow_y=fy)
        for name, a in fields.items():
            if a is not None:
                dev.append(inst.to_device(np.ascontiguousarray(a, np.float32)))
                setattr(jobs[k], name, dev[-1])
        dev.append(inst.to_device(np.full(p["data"].shape, SENTINEL, np.float32)))
        jobs[k].out = dev[-1]
    return jobs, dev


def _run_batch(inst, probs, pen, coupling, rounds=fcb.ROUNDS):
    p0 = probs[0]
    jobs, dev = _device_jobs(inst, probs)
    try:
        rc = inst.volume_flow_coupled_device(_params(p0, pen, rounds), coupling, capi.poisson_layout_of(p0["data"][0]), jobs, allow_job_errors=True)
        codes = [j.rc for j in jobs]
        outs = [inst.from_device(j.out, p0["data"].shape, np.float32) for j in jobs]
    finally:
        for q in dev:
            inst.free(q)
    return rc, codes, outs


def _check_members(probs, outs, chunks, pen, coupling, rounds=fcb.ROUNDS):
    """every member of every chunk against the restatement's rounds under the chunk's means (the iterate before the last: the
    restatement's, the library's own stays on the device)"""
    for members in chunks:
        rels = []
        chunk = vfc.irls_f32([probs[k] for k in members], pen, rounds, coupling, rels=rels)
        assert max(rels) <= 1e-5, "every round of the reference stops by its rule"
        for k, (u32, its) in zip(members, chunk):
            y = fcb.Yardstick(probs[k], pen, coupling, rounds, u32=u32, iters32=its)
            err, res = y.measure(u32[-2], outs[k])
            eb, _ = y.bounds()
            print(f"VOLUME_FLOW_COUPLED batch member {k}: ERR {err:.3e} (irls_f32 {y.err32:.3e}, bound {eb:.3e})")
            assert err <= eb, (k, err, eb)
            assert_copied_bits(probs[k], outs[k])


@pytest.mark.parametrize("at", [1, 0])
def test_a_fractional_flow_fails_its_volume_only(inst, at):
    """the two that stay run as a chunk of two: their bytes are those of the call with those two alone (the chunk's means), and the
    link planes and the rho planes follow the volumes when the refused one leaves from the front"""
    trio, pen, coupling = fcb.batch_trio()
    probs = list(trio)
    T, H, W = probs[at]["state"].shape[:3]
    fx, fy = capi.volume_flow_planes(probs[at]["flow"], T, H, W, True)
    fx = fx.copy()
    fx[1, H // 2, W // 2] = 0.5
    probs[at] = dict(probs[at], fx=fx, fy=fy)
    stay = [k for k in range(3) if k != at]
    rc, codes, outs = _run_batch(inst, probs, pen, coupling)
    assert rc == capi.SC_ERR_BAD_ARG and codes == [capi.SC_ERR_BAD_ARG if k == at else capi.SC_OK for k in range(3)], (rc, codes)
    assert (outs[at] == SENTINEL).all(), "a refused volume must not be written"
    rc2, codes2, outs2 = _run_batch(inst, [probs[k] for k in stay], pen, coupling)
    assert rc2 == capi.SC_OK
    for k, alone in zip(stay, outs2):
        assert outs[k].tobytes() == alone.tobytes(), "a member's bytes are those of the call without the refused volume"
    _check_members(probs, outs, [stay], pen, coupling)


def test_a_bad_weight_fails_its_volume_only(inst):
    trio, pen, coupling = fcb.batch_trio()
    bad = dict(trio[1], weight=trio[1]["weight"].copy())
    at = tuple(np.argwhere(vw.kinds(bad["sides"], bad["periodic"], bad["state"]) == vw.UNKNOWN)[5])
    bad["weight"][at] = np.nan
    probs = [trio[0], bad, trio[2]]
    rc, codes, outs = _run_batch(inst, probs, pen, coupling)
    assert rc == capi.SC_ERR_BAD_ARG and codes == [capi.SC_OK, capi.SC_ERR_BAD_ARG, capi.SC_OK], (rc, codes)
    assert (outs[1] == np.float32(SENTINEL)).all(), "the refused volume's out was written"
    _check_members(probs, outs, [[0, 2]], pen, coupling)


def test_nine_volumes_run_in_two_chunks(inst):
    """8 frames x 3 channels are 24 planes: a chunk holds 8 volumes, the ninth runs in a second one"""
    pats = ("hole", "scatter", "keyframes", "split", "all")
    flows = ("split", "random", "pan", "collapse", "far", "pan1", "zero")
    probs = [fcb.make_input("neumann", 7, 5, 3, 8, 1.0, pats[k % 5], "sparse", "xyt", "periodic", True, flows[k % 7], seed=50 + k,
                            **(dict(amount=2) if flows[k % 7] in ("split", "random") else {})) for k in range(9)]
    pen = fcb.penalties(probs[0], (1.0, 1.0, 2.0), 1e-2)
    coupling = S | T_ | J
    rc, codes, outs = _run_batch(inst, probs, pen, coupling, 2)
    assert rc == capi.SC_OK and codes == [capi.SC_OK] * 9, (rc, codes)
    _check_members(probs, outs, [list(range(8)), [8]], pen, coupling, 2)


# ---- 8. what it is for -----------------------------------------------------------------------------------------------------------------
def test_isotropic_tv_along_the_flow_on_a_panning_disc():
    """a disc that pans by (2, 1) per frame, noise of sigma 0.1, lam 4, tau 1, 8 rounds.  Decided with the float64 restatement's exact
    rounds before it was fixed here: the rms error against the clean video is 0.0603 along the flow against 0.1156 for the straight
    isotropic call (a factor of 1.9: the straight temporal term ties the disc's rim to the background two pixels on); against the
    anisotropic call along the same flow each answer has the lower energy under its own functional -- 557.39 against 563.60 under the
    isotropic one (1.1 %), 643.00 against 654.87 under the anisotropic one (1.8 %), where the library's answers lie within 1e-3 of the
    restatement's.  Inequalities, not thresholds.  (The rms errors of the two flow calls differ by under 1 % in the restatement, either
    way with the noise: no inequality between them is kept.)"""
    T, H, W = 4, 24, 24
    p, pen, clean = fcb.panning_disc(T, H, W, lam=4.0, noise=0.1)
    frames, flow = p["data"][..., 0], p["flow"]
    args = dict(tau=1.0, p=1.0, p_time=1.0, eps=1e-2, max_rounds=8, round_tol=-1.0)
    rms = lambda u: float(np.sqrt(np.mean((u.astype(np.float64) - clean) ** 2)))
    iso = pkg.tv_denoise_video_along_flow(frames, 4.0, flow, isotropic=True, **args)
    ani = pkg.tv_denoise_video_along_flow(frames, 4.0, flow, isotropic=False, **args)
    straight = pkg.tv_denoise_video(frames, 4.0, isotropic=True, **args)
    print(f"VOLUME_FLOW_COUPLED disc: rms error isotropic along the flow {rms(iso):.4f}, isotropic straight {rms(straight):.4f}, "
          f"anisotropic along the flow {rms(ani):.4f}, of the noisy frames {rms(frames):.4f}")
    assert rms(iso) < rms(straight)
    energy = lambda u, coupling: float(vfc.energy(p, pen, u.reshape(p["data"].shape), coupling).sum())
    e_ii, e_ia, e_aa, e_ai = energy(iso, S), energy(ani, S), energy(ani, 0), energy(iso, 0)
    print(f"VOLUME_FLOW_COUPLED disc: isotropic energy {e_ii:.3f} (of the anisotropic answer {e_ia:.3f}), anisotropic energy {e_aa:.3f} "
          f"(of the isotropic answer {e_ai:.3f})")
    assert e_ii < e_ia and e_aa < e_ai


# ---- 9. the Python wrappers ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loop", [False, True])
def test_the_python_calls_are_the_c_calls_they_document(inst, loop):
    T, H, W = 6, 24, 32
    _, frames = frb.panning_texture(T, H, W)
    flow = frb.pan_flow(T, H, W, loop=loop)
    zero = np.zeros_like(frames)
    state, lam = np.zeros(frames.shape, np.float32), np.full(frames.shape, 4.0, np.float32)
    for kw in (dict(), dict(isotropic=False, joint_channels=True), dict(spacetime=True), dict(isotropic=False)):
        coupling = capi.volume_coupling(kw.get("isotropic", True), kw.get("spacetime", False), kw.get("joint_channels", False))
        got = pkg.tv_denoise_video_along_flow(frames, 4.0, flow, tau=0.5, p=1.0, p_time=1.0, q=2.0, eps=1e-2, loop=loop, max_rounds=3, round_tol=-1.0, **kw)
        want = inst.volume_flow_coupled(coupling, zero, zero, frames, state, flow, lam, tau=0.5, loop=loop, neumann=True, p_grad=1.0, eps_grad=1e-2,
                                        p_time=1.0, eps_time=1e-2, p_data=2.0, eps_data=1e-2, max_rounds=3, round_tol=-1.0)
        assert got.shape == frames.shape and np.array_equal(bits(got), bits(want)), kw
    straight = pkg.tv_denoise_video(frames, 4.0, tau=0.5, p=1.0, p_time=1.0, q=2.0, eps=1e-2, loop=loop, max_rounds=3, round_tol=-1.0, isotropic=True)
    along = pkg.tv_denoise_video_along_flow(frames, 4.0, flow, tau=0.5, p=1.0, p_time=1.0, q=2.0, eps=1e-2, loop=loop, max_rounds=3, round_tol=-1.0)
    assert not np.array_equal(bits(along), bits(straight)), "the flow changes the answer"
    uncoupled = pkg.tv_denoise_video(frames, 4.0, tau=0.5, p=1.0, p_time=1.0, q=2.0, eps=1e-2, loop=loop, max_rounds=3, round_tol=-1.0, flow=flow)
    assert not np.array_equal(bits(along), bits(uncoupled)), "the coupling changes the answer"
    p, _ = frb.panning_outlier_problem(T, H, W)
    gx, gy, gt = p["gx"], p["gy"], p["gt"]
    if loop:
        gt = np.concatenate([gt, np.zeros_like(gt[:1])])
    known, values = p["state"][..., 0] == 1, p["data"]
    got = pkg.volume_flow_coupled_solve(gx, gy, values, known.astype(np.uint8), flow, gt=gt, loop=loop, p=1.0, p_time=1.0, max_rounds=2, round_tol=-1.0,
                                        spacetime=True)
    want = inst.volume_flow_coupled(S | T_, gx, gy, values, known.astype(np.float32), flow, None, gt=gt, tau=1.0, loop=loop, neumann=True, max_rounds=2,
                                    round_tol=-1.0)
    assert np.array_equal(bits(got), bits(want))
    got = pkg.volume_flow_coupled_solve(gx, gy, values, known.astype(np.uint8), None, gt=gt, loop=loop, p=1.0, p_time=1.0, max_rounds=2, round_tol=-1.0,
                                        isotropic=True)
    want = inst.volume_coupled(S, gx, gy, values, known.astype(np.float32), None, gt=gt, tau=1.0, loop=loop, neumann=True, max_rounds=2, round_tol=-1.0)
    assert np.array_equal(bits(got), bits(want)), "flow None: volume_coupled() itself"
