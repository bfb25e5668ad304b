"""GPU tests of the robust sub-pixel flow volume solve (sc_hip_volume_subflow_robust, sc_hip_volume_subflow_robust_device) through capi:
the robust volume call's penalties and rounds with every temporal link a bilinear stencil along a caller's real-valued flow.

1. against the rounds of tests/volume_subflow_robust_np.py on tests/volume_subflow_robust_bounds.py's matrix through the host call, NaN
   in every element the header says is not read: ERR, RES and ENERGY within the bounds, the trace's energy never rising by more than
   ENERGY_REL of itself from one round to the next, out's bits at KNOWN and OUTSIDE pixels data's and on the Dirichlet lines boundary's.
2. round by round on two inputs: max_rounds = 1, 2, 3 each within the bound of the restatement's iterate of that round, the iterate
   before it read from the run of one round less; the second input has p_time = 2, where LT of every round is round 0's bit for bit
   in the restatement (tests/test_volume_subflow_robust_host.py) that the library is held to here.
3. ties, to the byte and with the trace's round and inner-iteration counts: no flow arrays give sc_hip_volume_robust, free and periodic
   time, with and without link arrays; every exponent 2 gives sc_hip_volume_subflow and no round runs; link arrays of ones give the
   bytes of none; two runs of a collapse and of a random input give the same bytes.
4. a constant whole pan on rolled frames under periodic x and y: this call, sc_hip_volume_flow_robust on the same flow (no
   collisions: the same system, no byte tie) and the straight robust call on the rolled frames are all held to this call's yardstick.
5. tiling: a frame seam inside a band, a link's ends in different bands and in different 256-column groups; collapse and edge with
   (1, 1, 2) penalties.
6. the device call: HWC and CHW with padded rows, a frame stride with a gap, guard frames, NaN in every element that is not read, out
   may be data, nothing but the named elements written.
7. batches: a bad weight fails its volume only; a flow where the first volume has none, or the reverse, and exactly one flow array
   are refused; a flow array overlapping out is refused; nine volumes run in two chunks, one of them leaving the first chunk, whose
   transposed links are built again for the volumes that stay.
8. what it is for: tv_denoise_video(flow=, subpixel=True) on a texture panning by (0.5, 0.5) has a smaller error than the rounded call at
   the same tau; integrate_gradients_video(subpixel=True) with gross temporal outliers lands closer to the truth under p_time = 1 than
   under p_time = 2.
9. volume_robust_solve, tv_denoise_video and integrate_gradients_video with subpixel=True give the bytes of the
   Instance.volume_subflow_robust call they document; the default keeps the rounded call's bytes."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import seamlesscloneoptimization_amd as pkg
from seamlesscloneoptimization_amd import capi

import volume_flow_robust_bounds as frb
import volume_robust_bounds as rb
import volume_robust_np as vr
import volume_subflow_bounds as sb
import volume_subflow_robust_bounds as srb
import volume_subflow_robust_np as vsr
import volume_wls_np as vw

pytestmark = pytest.mark.gpu

G = capi.SC_POISSON_GUIDANCE
SENTINEL = -7.25
FIXED = dict(round_tol=-1.0, allow_not_converged=True)          # every round runs; an inner solve may run out of max_iters as the restatement's does


@pytest.fixture(scope="module")
def inst():
    i = capi.Instance(0)
    yield i
    i.destroy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def solve(inst, p, pen, rounds, **kw):
    return inst.volume_subflow_robust(**srb.call_args(p, pen, max_rounds=rounds, **FIXED, **kw))


def solve_straight(inst, p, pen, rounds, **kw):
    return inst.volume_robust(**rb.call_args(p, pen, max_rounds=rounds, **FIXED, **kw))


def quadratic(inst, p):
    """Instance.volume_subflow on the robust sub-pixel call's input: the quadratic round"""
    return inst.volume_subflow(p["data"], p["state"], p["flow"], p["weight"], p["sx"], p["sy"], p["smt"], p["gx"], p["gy"], p["gt"], boundary=vr._boundary(p),
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
    print(f"VOLUME_SUBFLOW_ROBUST {tag}: ERR {err:.3e} (irls_f32 {e32:.3e}, bound {eb:.3e}) RES {res:.3e} (irls_f32 {r32:.3e}, bound {rb_:.3e})")
    assert not bad, (tag, bad)


def assert_energy(tag, inst, y, out, rounds):
    energy, iters = inst.robust_trace()
    assert len(energy) == rounds + 1 and len(iters) == rounds + 1
    assert inst.info().sweeps == int(iters.sum())
    want = float(y.energy(out).sum())
    rel = abs(float(energy[-1]) - want) / want
    rise = max((float(b) - float(a)) / float(a) for a, b in zip(energy, energy[1:]))
    print(f"VOLUME_SUBFLOW_ROBUST {tag}: ENERGY {rel:.3e} (bound {srb.ENERGY_REL:.1e}) worst rise {rise:.3e} iterations {list(map(int, iters))} "
          f"(irls_f32 {y.iters32})")
    assert rel <= srb.ENERGY_REL, (tag, rel)
    assert rise <= srb.ENERGY_REL, (tag, "the energy rose from one round to the next", list(map(float, energy)))


# ---- 1. the matrix ---------------------------------------------------------------------------------------------------------------------
_CASES = srb.matrix()
_IDS = [f"{b}-{W}x{H}x{C}x{T}-tau{tau:g}-{p}-{wk}-{ln}-{tm}-gt{int(gt)}-{'_'.join(f'{e:g}' for e in ex)}-eps{ef:g}-{fl}"
        for b, H, W, C, T, tau, p, wk, ln, tm, gt, ex, ef, fl in _CASES]


@pytest.mark.parametrize("i", range(len(_CASES)), ids=_IDS)
def test_against_the_reference_rounds(inst, i):
    clean, pen, y = srb.matrix_case(i)
    assert max(y.rels32) <= 1e-5 and max(y.iters32) <= srb.MAX_ITERS, "every round of the reference stops by its rule on every input"
    p = srb.nan_unread(clean)
    prev = solve(inst, p, pen, srb.ROUNDS - 1)
    out = solve(inst, p, pen, srb.ROUNDS)
    assert_energy(_IDS[i], inst, y, out, srb.ROUNDS)
    assert_round(_IDS[i], y, prev, out)
    assert_copied_bits(clean, out)
    assert np.array_equal(bits(solve(inst, clean, pen, srb.ROUNDS)), bits(out)), "an element the header says is not read changed the answer"


# ---- 2. round by round -----------------------------------------------------------------------------------------------------------------
_ROUND_CASES = [("frame", 12, 19, 3, 5, 1.0, "hole", "sparse", "xyt", "periodic", True, (1.0, 1.0, 2.0), 1e-2, "random"),
                ("neumann", 5, 260, 1, 3, 0.1, "scatter", None, "t", "free", True, (1.0, 2.0, 1.0), 1e-3, "pan")]


def round_case(case):
    """(the input, its penalties, its Yardstick of three rounds)"""
    clean = srb.make_input(*case[:11], case[13])
    pen = srb.penalties(clean, case[11], case[12])
    return clean, pen, srb.Yardstick(clean, pen, rounds=3)


@pytest.mark.parametrize("case", _ROUND_CASES, ids=["frame-19x12x3x5-random", "neumann-260x5x1x3-pan-p_time2"])
def test_round_by_round(inst, case):
    clean, pen, y = round_case(case)
    assert max(y.rels32) <= 1e-5
    p = srb.nan_unread(clean)
    prev = quadratic(inst, p)
    for k in (1, 2, 3):
        out = solve(inst, p, pen, k)
        assert_round(f"{case[0]} {case[1]} x {case[2]} x {case[4]} {case[13]} round {k}", y, prev, out, k)
        prev = out


# ---- 3. ties ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("links", ["none", "xyt"])
@pytest.mark.parametrize("time", srb.TIMES)
def test_no_flow_arrays_give_the_robust_volume_call(inst, time, links):
    p = srb.nan_unread(srb.make_input("free_lt", 23, 17, 3, 4, 1.7, "scatter", "sparse", links, time, True, "zero", seed=4))
    pen = srb.penalties(p, (1.0, 0.8, 1.5), 1e-2)
    want = solve_straight(inst, p, pen, 3)
    want_trace = trace(inst)
    assert len(want_trace[1]) == 4
    got = solve(inst, dict(p, flow=None), pen, 3)
    assert got.tobytes() == want.tobytes() and trace(inst) == want_trace, "no flow arrays: sc_hip_volume_robust itself"


@pytest.mark.parametrize("flow", ["random", "collapse"])
@pytest.mark.parametrize("time", srb.TIMES)
def test_exponents_of_two_give_the_bytes_of_the_subpixel_volume_call(inst, time, flow):
    p = srb.nan_unread(srb.make_input("free_lt", 12, 19, 3, 5, 0.3, "scatter", "sparse", "xyt", time, True, flow, seed=6))
    out = solve(inst, p, (2.0, 2.0, 2.0, 0.0, 0.0, 0.0), 5)
    energy, iters = inst.robust_trace()
    assert len(iters) == 1 and inst.info().converged == 1, "no reweighting round runs"
    sweeps = inst.info().sweeps
    assert np.array_equal(bits(out), bits(quadratic(inst, p))) and inst.info().sweeps == sweeps


@pytest.mark.parametrize("time", srb.TIMES)
def test_link_arrays_of_ones_give_the_bytes_of_none(inst, time):
    p = srb.make_input("periodic_x", 12, 19, 3, 3, 1.0, "hole", "constant", "none", time, True, "axis")
    pen = srb.penalties(p, (1.0, 1.0, 1.0), 1e-2)
    want = solve(inst, p, pen, 3)
    want_trace = trace(inst)
    ones = np.ones_like(p["data"])
    q = dict(p, sx=ones, sy=ones, smt=np.ones_like(p["gt"]))
    assert np.array_equal(bits(solve(inst, q, pen, 3)), bits(want)) and trace(inst) == want_trace
    assert np.array_equal(bits(solve(inst, dict(p, smt=np.ones_like(p["gt"])), pen, 3)), bits(want)) and trace(inst) == want_trace


_TWICE = dict(collapse=("periodic_x", 47, 33, 3, 5), random=("periodic_x", 47, 33, 3, 5))


@pytest.mark.parametrize("flow", ["collapse", "random"])
def test_two_runs_give_the_same_bytes(inst, flow):
    """collapse: every link of a frame arrives at one of four pixels, rows as long as a frame"""
    border, H, W, C, T = _TWICE[flow]
    p = srb.nan_unread(srb.make_input(border, H, W, C, T, 1.0, "scatter", "sparse", "xyt", "periodic", True, flow))
    pen = srb.penalties(p, (1.0, 1.0, 2.0), 1e-2)
    a = solve(inst, p, pen, 3)
    ta = trace(inst)
    b = solve(inst, p, pen, 3)
    assert a.tobytes() == b.tobytes() and trace(inst) == ta


# ---- 4. a whole pan: three calls, one yardstick --------------------------------------------------------------------------------------
_PAN = dict(T=6, H=12, W=18, C=3, pan=(3, 2))


def pan_case(time):
    """periodic x and y, every state 0, a sparse weight, flow = a constant whole pan: (the input, its penalties, its Yardstick of three
    rounds)"""
    p = srb.make_input("periodic_xy", _PAN["H"], _PAN["W"], _PAN["C"], _PAN["T"], 1.0, "all", "sparse", "xyt", time, True, "zero", seed=8)
    p["flow"] = np.broadcast_to(np.float32(_PAN["pan"]), p["flow"].shape).copy()
    p["links"] = sb.links_of(p)
    pen = srb.penalties(p, (1.0, 1.0, 2.0), 1e-2)
    return p, pen, srb.Yardstick(p, pen, rounds=3)


@pytest.mark.parametrize("time", srb.TIMES)
def test_a_constant_whole_pan_is_the_straight_call_on_rolled_frames(inst, time):
    """frame t rolled back by t pans turns every link into a straight one (under periodic time the wrapping link too when T pans are a
    whole number of periods: 6 frames x (3, 2) on 18 x 12).  A whole pan has no collisions, so sc_hip_volume_flow_robust solves the same
    rounds.  All three answers are held to this call's float64 rounds, ERR and RES within the bounds: not to the byte, because the
    product form and the rolled sums round differently."""
    T, pan = _PAN["T"], _PAN["pan"]
    p, pen, y = pan_case(time)
    assert max(y.rels32) <= 1e-5
    prev, out = solve(inst, p, pen, 2), solve(inst, p, pen, 3)
    assert_round(f"pan {time}", y, prev, out)
    fargs = lambda rounds: frb.call_args(p, pen, max_rounds=rounds, **FIXED)
    fprev, fout = inst.volume_flow_robust(**fargs(2)), inst.volume_flow_robust(**fargs(3))
    assert_round(f"pan {time}, sc_hip_volume_flow_robust on the whole flow", y, fprev, fout)
    back = lambda a: a if a is None else np.stack([np.roll(a[t], (-t * pan[1], -t * pan[0]), (0, 1)) for t in range(a.shape[0])])
    q = {n: (back(a) if isinstance(a, np.ndarray) and n != "flow" else a) for n, a in p.items() if n != "links"}
    forward = lambda a: np.stack([np.roll(a[t], (t * pan[1], t * pan[0]), (0, 1)) for t in range(T)])
    sprev, sout = forward(solve_straight(inst, q, pen, 2)), forward(solve_straight(inst, q, pen, 3))
    assert_round(f"pan {time}, the rolled straight answer", y, sprev, sout)
    assert_copied_bits(p, sout)


# ---- 5. tiling -------------------------------------------------------------------------------------------------------------------------
# (border, H, W, T, what the shape is there for): the shapes of tests/test_gpu_volume_flow_robust.py
_TILINGS = [("neumann", 47, 33, 5, "seam_in_band"), ("neumann", 47, 33, 5, "ends_in_other_bands"), ("neumann", 9, 300, 3, "ends_in_other_groups")]


@functools.lru_cache(maxsize=None)
def tiling_input(border, H, W, T, flow):
    """(the input, its penalties, its Yardstick of two rounds), shared by the tests of one shape; nobody writes into them.  One channel;
    under `collapse`, where a whole frame's links meet in one point, tau 0.1 (volume_subflow_robust_bounds' rule: at tau 1 the
    reference rounds at 47 x 33 x 5 run out of their 400 iterations)"""
    args = dict(column=280) if flow == "collapse" and W > 256 else {}          # (collapse: onto column 280)
    clean = srb.make_input(border, H, W, 1, T, 0.1 if flow == "collapse" else 1.0, "scatter", "sparse", "t", "free", True, flow, seed=11, **args)
    pen = srb.penalties(clean, (1.0, 1.0, 2.0), 1e-2)
    return clean, pen, srb.Yardstick(clean, pen, rounds=2)


def tiling_case(case, flow):
    return tiling_input(*case[:4], flow)


@pytest.mark.parametrize("flow", ["collapse", "edge"])
@pytest.mark.parametrize("case", _TILINGS, ids=[f"{c[4]}-{c[2]}x{c[1]}x{c[3]}" for c in _TILINGS])
def test_links_across_the_tiling(inst, case, flow):
    border, H, W, T, what = case
    clean, pen, y = tiling_case(case, flow)
    plan = capi.pcg_plan(W, H, G | capi.border_bits(clean["sides"], False, clean["periodic"]), T)
    ny, nx, rows = plan["ny"] // T, plan["nx"], plan["rows"]
    idx, _ = clean["links"]
    src = np.repeat(np.arange(idx[..., 0].size), 4)[idx.reshape(-1) >= 0]
    dst = idx.reshape(-1)[idx.reshape(-1) >= 0]
    if what == "seam_in_band":
        assert any(0 < (t * ny) % rows for t in range(1, T)), ("a frame boundary strictly inside a band", plan)
    elif what == "ends_in_other_bands":
        assert plan["bands"] > 1 and ((src // nx) // rows != (dst // nx) // rows).any(), ("a link whose ends lie in different bands", plan)
    else:
        assert plan["cg"] > 1 and ((src % nx) // 256 != (dst % nx) // 256).any(), ("a link whose ends lie in different column groups", plan)
    assert max(y.rels32) <= 1e-5
    p = srb.nan_unread(clean)
    prev, out = solve(inst, p, pen, 1), solve(inst, p, pen, 2)
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


def device_case():
    clean = srb.make_input("free_lt", 23, 17, 3, 4, 1.3, "scatter", "sparse", "xyt", "periodic", True, "random", seed=3)          # Dirichlet lines right and bottom
    pen = srb.penalties(clean, (1.0, 1.0, 2.0), 1e-2)
    return clean, pen, srb.Yardstick(clean, pen, rounds=2)


@pytest.mark.parametrize("alias", ["none", "data"])
@pytest.mark.parametrize("layout", ["hwc", "chw_padded"])
def test_device_layouts_write_only_named_elements(inst, layout, alias):
    T, H, W = 4, 23, 17
    clean, pen, y = device_case()
    p = srb.nan_unread(clean)          # gt and smooth_t NaN where no live link has its source, the flow NaN off the work rectangle
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
        rc = inst.volume_subflow_robust_device(_params(clean, pen, 2, stride), lay, jobs)
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
    assert got.tobytes() == solve(inst, clean, pen, 2).tobytes(), "the device call on any layout writes the host call's bytes"
    assert_round(f"device {layout} out={alias}", y, solve(inst, clean, pen, 1), got)


# ---- 7. batches ------------------------------------------------------------------------------------------------------------------------
def _device_jobs(inst, probs):
    """VolumeFlowRobustJob array of the inputs on dense device arrays, each with an out full of SENTINEL; (jobs, pointers to free)"""
    jobs = capi.Instance.make_volume_flow_robust_jobs(len(probs))
    dev = []
    for k, p in enumerate(probs):
        T, H, W = p["state"].shape[:3]
        fx, fy = (None, None) if p["flow"] is None else capi.volume_subflow_planes(p["flow"], T, H, W, p["tper"])
        fields = dict(gx=p["gx"], gy=p["gy"], gt=p["gt"], data=p["data"], state=p["state"], weight=p["weight"], boundary=vr._boundary(p), smooth_x=p["sx"],
                      smooth_y=p["sy"], smooth_t=p["smt"], flow_x=fx, flow_y=fy)
        for name, a in fields.items():
            if a is not None:
                dev.append(inst.to_device(np.ascontiguousarray(a, np.float32)))
                setattr(jobs[k], name, dev[-1])
        dev.append(inst.to_device(np.full(p["data"].shape, SENTINEL, np.float32)))
        jobs[k].out = dev[-1]
    return jobs, dev


def _run_batch(inst, probs, pen, rounds=srb.ROUNDS):
    p0 = probs[0]
    jobs, dev = _device_jobs(inst, probs)
    try:
        rc = inst.volume_subflow_robust_device(_params(p0, pen, rounds), capi.poisson_layout_of(p0["data"][0]), jobs, allow_job_errors=True)
        codes = [j.rc for j in jobs]
        outs = [inst.from_device(j.out, p0["data"].shape, np.float32) for j in jobs]
    finally:
        for q in dev:
            inst.free(q)
    return rc, codes, outs


def _check_members(probs, outs, chunks, pen, rounds=srb.ROUNDS):
    """every member of every chunk against the restatement's rounds under the chunk's means (the iterate before the last: the
    restatement's, the library's own stays on the device)"""
    for members in chunks:
        rels = []
        chunk = vsr.irls_f32([probs[k] for k in members], pen, rounds, rels=rels)
        assert max(rels) <= 1e-5, "every round of the reference stops by its rule"
        for k, (u32, its) in zip(members, chunk):
            y = srb.Yardstick(probs[k], pen, rounds, u32=u32, iters32=its)
            err, res = y.measure(u32[-2], outs[k])
            eb, _ = y.bounds()
            print(f"VOLUME_SUBFLOW_ROBUST batch member {k}: ERR {err:.3e} (irls_f32 {y.err32:.3e}, bound {eb:.3e})")
            assert err <= eb, (k, err, eb)
            assert_copied_bits(probs[k], outs[k])


@pytest.mark.parametrize("at", [1, 0])
def test_a_bad_weight_fails_its_volume_only(inst, at):
    """the two that stay run as a chunk of two: their bytes are those of the call with those two alone (the chunk's means), and the
    transposed links follow the volumes when the refused one leaves from the front: round 0's set-up builds them again"""
    trio, pen = srb.batch_trio()
    bad = dict(trio[at], weight=trio[at]["weight"].copy())
    where = tuple(np.argwhere(vw.kinds(bad["sides"], bad["periodic"], bad["state"]) == vw.UNKNOWN)[5])
    bad["weight"][where] = np.nan
    probs = list(trio)
    probs[at] = bad
    stay = [k for k in range(3) if k != at]
    rc, codes, outs = _run_batch(inst, probs, pen)
    assert rc == capi.SC_ERR_BAD_ARG and codes == [capi.SC_ERR_BAD_ARG if k == at else capi.SC_OK for k in range(3)], (rc, codes)
    assert (outs[at] == np.float32(SENTINEL)).all(), "the refused volume's out was written"
    rc2, codes2, outs2 = _run_batch(inst, [probs[k] for k in stay], pen)
    assert rc2 == capi.SC_OK
    for k, alone in zip(stay, outs2):
        assert outs[k].tobytes() == alone.tobytes(), "a member's bytes are those of the call without the refused volume"
    _check_members(probs, outs, [stay], pen)


def test_a_flow_where_the_first_volume_has_none_is_refused(inst):
    trio, pen = srb.batch_trio()
    none = dict(trio[0], flow=None)
    for probs in ([none, trio[1]], [trio[1], none]):
        rc, codes, outs = _run_batch(inst, probs, pen, 2)
        assert rc == capi.SC_ERR_BAD_ARG and codes == [capi.SC_OK, capi.SC_ERR_BAD_ARG], (rc, codes)
        assert (outs[1] == SENTINEL).all(), "a refused volume must not be written"
    # exactly one of the two arrays, in the device call and in the host call
    jobs, dev = _device_jobs(inst, [trio[0], trio[1]])
    try:
        jobs[1].flow_y = None
        rc = inst.volume_subflow_robust_device(_params(trio[0], pen, 2), capi.poisson_layout_of(trio[0]["data"][0]), jobs, allow_job_errors=True)
        assert rc == capi.SC_ERR_BAD_ARG and [j.rc for j in jobs] == [capi.SC_OK, capi.SC_ERR_BAD_ARG]
    finally:
        for q in dev:
            inst.free(q)
    import ctypes as C
    p = trio[0]
    T, H, W, _ = p["data"].shape
    fx, fy = capi.volume_subflow_planes(p["flow"], T, H, W, True)
    out = np.full(p["data"].shape, SENTINEL, np.float32)
    params, lay = _params(p, pen, 2), capi.poisson_layout_of(p["data"][0])
    ptr = lambda a: None if a is None else np.ascontiguousarray(a, np.float32).ctypes.data
    for one in ((fx, None), (None, fy)):
        rc = inst.L.sc_hip_volume_subflow_robust(inst.h, C.byref(params), C.byref(lay), ptr(p["gx"]), ptr(p["gy"]), ptr(p["gt"]), ptr(p["data"]),
                                                 ptr(p["state"]), ptr(p["weight"]), ptr(p["sx"]), ptr(p["sy"]), ptr(p["smt"]), ptr(one[0]), ptr(one[1]),
                                                 ptr(p["boundary"]), ptr(out))
        assert rc == capi.SC_ERR_BAD_ARG and (out == SENTINEL).all()


@pytest.mark.parametrize("name", ["flow_x", "flow_y"])
def test_a_flow_array_that_overlaps_out_is_refused(inst, name):
    """a flow array may share no float of its own length with out's span -- here its last float is out's first"""
    p = srb.make_input("free_lt", 9, 7, 3, 4, 1.0, "scatter", "constant", "t", "periodic", True, "half", seed=30)
    pen = srb.penalties(p, (1.0, 1.0, 2.0), 1e-2)
    T, H, W, C = p["data"].shape
    plane = capi.volume_subflow_planes(p["flow"], T, H, W, True)[0 if name == "flow_x" else 1].ravel()
    for at, want in ((plane.size - 1, capi.SC_ERR_BAD_ARG), (plane.size, capi.SC_OK)):
        jobs, dev = _device_jobs(inst, [p])
        host = np.full(plane.size + p["data"].size + 8, SENTINEL, np.float32)
        host[:plane.size] = plane
        block = inst.to_device(host)
        dev.append(block)
        try:
            setattr(jobs[0], name, block)
            jobs[0].out = block + 4 * at
            inst.volume_subflow_robust_device(_params(p, pen, 2), capi.poisson_layout_of(p["data"][0]), jobs, allow_job_errors=True)
            after = inst.from_device(block, host.shape, np.float32)
            assert jobs[0].rc == want, (at, jobs[0].rc)
        finally:
            for q in dev:
                inst.free(q)
        if want != capi.SC_OK:
            assert np.array_equal(after, host), "a refused volume must not be written"
        else:
            assert np.array_equal(after[:at], host[:at]) and (after[at + p["data"].size:] == SENTINEL).all()
            assert after[at:at + p["data"].size].tobytes() == solve(inst, p, pen, 2).tobytes()


_NINE_BAD = 2


def nine_volumes():
    """nine volumes of 8 frames x 3 channels (24 planes: a chunk holds 8 volumes, the ninth runs in a second one), volume _NINE_BAD with
    a NaN weight: it leaves the first chunk, whose transposed links are built again for the seven that stay"""
    pats = ("hole", "scatter", "keyframes", "split", "all")
    flows = ("half", "random", "pan", "collapse", "edge", "axis", "zero", "whole")
    probs = [srb.make_input("neumann", 7, 5, 3, 8, 1.0, pats[k % 5], "sparse", "xyt", "periodic", True, flows[k % 8], seed=50 + k,
                            **(dict(amount=2) if flows[k % 8] in ("whole", "random") else {})) for k in range(9)]
    bad = dict(probs[_NINE_BAD], weight=probs[_NINE_BAD]["weight"].copy())
    where = tuple(np.argwhere(vw.kinds(bad["sides"], bad["periodic"], bad["state"]) == vw.UNKNOWN)[3])
    bad["weight"][where] = np.nan
    probs[_NINE_BAD] = bad
    return probs, srb.penalties(probs[0], (1.0, 1.0, 2.0), 1e-2)


def test_nine_volumes_run_in_two_chunks(inst):
    probs, pen = nine_volumes()
    rc, codes, outs = _run_batch(inst, probs, pen, 2)
    assert rc == capi.SC_ERR_BAD_ARG and codes == [capi.SC_ERR_BAD_ARG if k == _NINE_BAD else capi.SC_OK for k in range(9)], (rc, codes)
    assert (outs[_NINE_BAD] == np.float32(SENTINEL)).all(), "the refused volume's out was written"
    _check_members(probs, outs, [[k for k in range(8) if k != _NINE_BAD], [8]], pen, 2)


# ---- 8. what it is for -----------------------------------------------------------------------------------------------------------------
def test_tv_denoise_video_along_the_subpixel_flow_beats_the_rounded_call_on_a_slow_pan():
    """a smooth texture that pans by (0.5, 0.5) pixels per frame, noise of sigma 0.1: np.rint rounds the flow to zero, so the rounded call
    compares a surface point with its neighbour half a pixel on and blurs the motion; along the bilinear link the point meets itself.
    An inequality at the same tau, not a threshold.  The float64 rounds (tests/test_volume_subflow_robust_host.py): rms error 0.0826
    along the sub-pixel flow, 0.1078 rounded, a factor 1.31."""
    T, H, W = 6, 20, 24
    clean, noisy = srb.panning_texture(T, H, W)
    flow = srb.pan_flow(T, H, W)
    rms = lambda u: float(np.sqrt(np.mean((u.astype(np.float64) - clean) ** 2)))
    sub, rounded = pkg.tv_denoise_video(noisy, flow=flow, subpixel=True, **srb.DENOISE), pkg.tv_denoise_video(noisy, flow=flow, **srb.DENOISE)
    print(f"VOLUME_SUBFLOW_ROBUST denoise: rms error along the sub-pixel flow {rms(sub):.4f}, rounded {rms(rounded):.4f}, of the noisy frames {rms(noisy):.4f}")
    assert rms(sub) < rms(rounded)


def test_l1_along_the_subpixel_flow_ignores_gross_temporal_outliers():
    """gt along the bilinear links of a pan of (0.5, 0.5) with outliers of +-4: p_time = 1 lands closer to the truth than p_time = 2.  The
    float64 rounds: 0.074 of the range against 0.240, a factor 3.23."""
    T, H, W = 5, 16, 24
    p, truth = srb.subpixel_outlier_problem(T, H, W)
    gx, gy, gt = p["gx"][..., 0], p["gy"][..., 0], p["gt"][..., 0]
    known, values = p["state"][..., 0] == 1, p["data"][..., 0]
    unk = ~known
    err = lambda u: float(np.abs(u.astype(np.float64) - truth[..., 0])[unk].max()) / p["range"]
    run = lambda r: pkg.integrate_gradients_video(gx, gy, gt, known, values, p=1.0, p_time=r, eps=1e-3 * p["range"], flow=p["flow"], subpixel=True,
                                                  max_rounds=8, round_tol=-1.0)
    l1, l2 = err(run(1.0)), err(run(2.0))
    print(f"VOLUME_SUBFLOW_ROBUST outliers along the sub-pixel flow: p_time 1 {l1:.3e} of the range, p_time 2 {l2:.3e}")
    assert l1 < l2


# ---- 9. the Python wrappers ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loop", [False, True])
def test_the_python_calls_are_the_c_calls_they_document(inst, loop):
    T, H, W = 6, 20, 24
    _, frames = srb.panning_texture(T, H, W)
    flow = srb.pan_flow(T, H, W, (2.25, -0.75), loop=loop)
    zero = np.zeros_like(frames)
    got = pkg.tv_denoise_video(frames, 4.0, tau=0.5, p=1.0, p_time=1.0, q=2.0, eps=1e-2, loop=loop, max_rounds=3, round_tol=-1.0, flow=flow, subpixel=True)
    want = inst.volume_subflow_robust(zero, zero, frames, np.zeros(frames.shape, np.float32), flow, np.full(frames.shape, 4.0, np.float32), tau=0.5,
                                      loop=loop, neumann=True, p_grad=1.0, eps_grad=1e-2, p_time=1.0, eps_time=1e-2, p_data=2.0, eps_data=1e-2,
                                      max_rounds=3, round_tol=-1.0)
    assert got.shape == frames.shape and np.array_equal(bits(got), bits(want))
    rounded = pkg.tv_denoise_video(frames, 4.0, tau=0.5, p=1.0, p_time=1.0, q=2.0, eps=1e-2, loop=loop, max_rounds=3, round_tol=-1.0, flow=flow)
    rwant = inst.volume_flow_robust(zero, zero, frames, np.zeros(frames.shape, np.float32), flow, np.full(frames.shape, 4.0, np.float32), tau=0.5,
                                    loop=loop, neumann=True, p_grad=1.0, eps_grad=1e-2, p_time=1.0, eps_time=1e-2, p_data=2.0, eps_data=1e-2,
                                    max_rounds=3, round_tol=-1.0)
    assert np.array_equal(bits(rounded), bits(rwant)), "the default keeps the rounding and the bytes"
    assert not np.array_equal(bits(got), bits(rounded)), "the unrounded flow changes the answer"
    p, _ = srb.subpixel_outlier_problem(T, H, W)
    gx, gy, gt = p["gx"][..., 0], p["gy"][..., 0], p["gt"][..., 0]
    if loop:
        gt = np.concatenate([gt, np.zeros_like(gt[:1])])
    known, values = p["state"][..., 0] == 1, p["data"][..., 0]
    got = pkg.integrate_gradients_video(gx, gy, gt, known, values, p=1.0, p_time=1.0, eps=1e-3, loop=loop, max_rounds=3, round_tol=-1.0, flow=flow,
                                        subpixel=True)
    want = inst.volume_subflow_robust(gx, gy, values, known.astype(np.float32), flow, None, gt=gt, tau=1.0, loop=loop, neumann=True, p_grad=1.0,
                                      eps_grad=1e-3, p_time=1.0, eps_time=1e-3, max_rounds=3, round_tol=-1.0)
    assert np.array_equal(bits(got), bits(want))
    got = pkg.integrate_gradients_video(gx, gy, gt, p=1.0, p_time=2.0, eps=1e-3, anchor=1e-2, loop=loop, max_rounds=2, round_tol=-1.0, flow=flow,
                                        subpixel=True)
    want = inst.volume_subflow_robust(gx, gy, np.zeros_like(gx), np.zeros(gx.shape, np.float32), flow, np.full(gx.shape, 1e-2, np.float32), gt=gt, tau=1.0,
                                      loop=loop, neumann=True, p_grad=1.0, eps_grad=1e-3, p_time=2.0, eps_time=1e-3, max_rounds=2, round_tol=-1.0)
    assert np.array_equal(bits(got), bits(want))
    got = pkg.volume_robust_solve(gx, gy, values, known.astype(np.uint8), gt=gt, loop=loop, p=1.0, p_time=1.0, max_rounds=2, round_tol=-1.0, flow=flow,
                                  subpixel=True)
    want = inst.volume_subflow_robust(gx, gy, values, known.astype(np.float32), flow, None, gt=gt, tau=1.0, loop=loop, neumann=True, max_rounds=2,
                                      round_tol=-1.0)
    assert np.array_equal(bits(got), bits(want))
