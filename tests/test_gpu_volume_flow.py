"""GPU tests of the flow volume solve (sc_hip_volume_flow, sc_hip_volume_flow_device) through capi: WLS volume solves whose temporal links
follow a caller's whole-numbered flow.

1. against the float64 solve (tests/volume_flow_np.py) on tests/volume_flow_bounds.py's matrix through the host call -- volume_bounds'
   borders, sizes, frames, channels, states, weights and forms, volume_wls_bounds' links and times, the seven flows zero / pan / pan1 /
   split / random / collapse / far: ERR and RES within the bounds, the iteration count within twice the reference iteration's plus the
   polling period, out's bits at KNOWN and OUTSIDE pixels data's and on the Dirichlet lines boundary's.
2. ties: a flow of zeros (-0.0 among them) gives the bytes and the sweep count of sc_hip_volume_wls, for the three forms, free and
   periodic time; so does no flow; two runs of a collapse and of a random call give the same bytes.
3. equivariance: under periodic x and y, a constant pan and every state 0 the answer is the straight-link answer of the input with frame
   t rolled back by t pans, rolled forward again.
4. tiling: shapes where sc_hip_pcg_plan puts a frame boundary inside a band, a link's ends in different bands and in different
   256-column groups; split and collapse against the exact solve at each.
5. the device call: HWC and CHW with padded rows, a frame stride with a gap, guard frames around every array -- the dense flow arrays at
   their own length --, NaN in every element the header says is not read: nothing but the named elements of out is written, out may
   be data.
6. batches: two volumes around one whose flow has a fractional value (SC_ERR_BAD_ARG, its out untouched), a volume with a flow where the
   first has none and the reverse, exactly one flow array (device and host call), a flow array that overlaps out, nine volumes in two chunks.
7. volume_wls_solve, inpaint_video, poisson_clone_video and interpolate_constraints_video with flow= against the float64 solve;
   inpaint_video recovers a texture that moves under a static hole where the straight-link call does not."""
from __future__ import annotations

import functools

import numpy as np
import pytest

from seamlesscloneoptimization_amd import capi, seamless_clone

import volume_flow_bounds as fb
import volume_flow_np as vf
import volume_wls_bounds as wb

pytestmark = pytest.mark.gpu

L, G = capi.SC_POISSON_LAPLACIAN, capi.SC_POISSON_GUIDANCE
SENTINEL = -7.25
POLL = capi.SC_WEIGHTED_POLL


@pytest.fixture(scope="module")
def inst():
    i = capi.Instance(0)
    yield i
    i.destroy()


def boundary_of(p):
    return p["boundary"] if vf.has_dirichlet(p["sides"], p["periodic"]) else None


def solve(inst, p, form="lap", **kw):
    return inst.volume_flow(p["data"], p["state"], weight=p["weight"], boundary=boundary_of(p), tau=p["tau"], free_sides=p["sides"],
                            periodic=p["periodic"], **fb.call_args(p, form), **kw)


def solve_straight(inst, p, form="lap"):
    return inst.volume_wls(p["data"], p["state"], p["weight"], boundary=boundary_of(p), tau=p["tau"], free_sides=p["sides"], periodic=p["periodic"],
                           **wb.call_args(p, form))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_copied_bits(p, out):
    """out at KNOWN and OUTSIDE pixels is data, on the Dirichlet lines boundary, bit for bit"""
    k = vf.kinds(p["sides"], p["periodic"], p["state"])
    out = out.reshape(k.shape)
    held = (k == vf.KNOWN) | (k == vf.OUTSIDE)
    assert np.array_equal(bits(out)[held], bits(p["data"].reshape(k.shape))[held]), "KNOWN and OUTSIDE pixels must be data's bits"
    line = k == vf.DIRICHLET
    assert np.array_equal(bits(out)[line], bits(p["boundary"].reshape(k.shape))[line]), "Dirichlet lines must be boundary's bits"
    assert np.isfinite(out[k == vf.UNKNOWN]).all(), "an unread element's NaN reached the answer"


def assert_yardstick(tag, p, form, out, y=None):
    """out lies within the yardstick's ERR and RES bounds for this input"""
    y = y or fb.Yardstick(p, form)
    assert y.rel32 <= 1e-5 and 2 * y.iters32 + POLL <= fb.MAX_ITERS, "the reference iteration must stay within the call's budget"
    bad, err, res = y.check(out)
    print(f"VOLUME_FLOW {tag}: ERR {err:.3g} (pcg_f32 {y.err32:.3g}) RES {res:.3g} (pcg_f32 {y.res32:.3g}) pcg_f32 iterations {y.iters32}")
    assert not bad, bad


# ---- 1. against the exact solve ------------------------------------------------------------------------------------------------
_CASES = fb.matrix()
_IDS = [f"{b}-{W}x{H}x{C}x{T}-tau{tau:g}-{p}-{wk}-{f}-{ln}-{tm}-{fl}" for b, H, W, C, T, tau, p, wk, f, ln, tm, fl in _CASES]


@pytest.mark.parametrize("i", range(len(_CASES)), ids=_IDS)
def test_against_the_exact_solve(inst, i):
    H, W = _CASES[i][1:3]
    p, form, y = fb.matrix_case(i)
    assert y.rel32 <= 1e-5 and y.max_sweeps() <= fb.MAX_ITERS, "the reference iteration must stay within the call's budget on every input"
    out = solve(inst, p, form)
    info = inst.info()
    bad, err, res = y.check(out)
    print(f"VOLUME_FLOW {_IDS[i]}: ERR {err:.3g} (pcg_f32 {y.err32:.3g}) RES {res:.3g} (pcg_f32 {y.res32:.3g}) sweeps {info.sweeps} "
          f"(pcg_f32 {y.iters32}) rel {info.rel_residual:.3g}")
    assert (info.method, info.converged, info.W, info.H) == (capi.SC_METHOD_FFT, 1, W, H)
    assert info.sweeps <= y.max_sweeps(), (info.sweeps, y.iters32)
    assert not bad, bad
    assert_copied_bits(p, out)


# ---- 2. ties ------------------------------------------------------------------------------------------------------------------------
def _zeros_with_minus_zero(p):
    f = np.zeros_like(p["flow"])
    f[:, ::2, 1::3] = -0.0
    return f


@pytest.mark.parametrize("time", fb.TIMES)
@pytest.mark.parametrize("form", fb.FORMS)
def test_a_flow_of_zeros_gives_the_bytes_and_sweeps_of_the_wls_call(inst, form, time):
    p = fb.nan_unread(fb.make_input("free_lt", 23, 17, 3, 4, 1.7, "scatter", "sparse", "xyt", time, "zero", seed=4))
    want = solve_straight(inst, p, form)
    sweeps = inst.info().sweeps
    got = solve(inst, dict(p, flow=_zeros_with_minus_zero(p)), form)
    assert got.tobytes() == want.tobytes() and inst.info().sweeps == sweeps
    # ... and without link arrays, where the straight call runs its plain statistics and set-up
    q = dict(p, sx=None, sy=None, smt=None)
    want = solve_straight(inst, q, form)
    sweeps = inst.info().sweeps
    got = solve(inst, dict(q, flow=_zeros_with_minus_zero(q)), form)
    assert got.tobytes() == want.tobytes() and inst.info().sweeps == sweeps


@pytest.mark.parametrize("time", fb.TIMES)
@pytest.mark.parametrize("form", fb.FORMS)
def test_no_flow_gives_the_bytes_and_sweeps_of_the_wls_call(inst, form, time):
    p = fb.nan_unread(fb.make_input("periodic_x", 23, 17, 3, 4, 0.6, "hole", "constant", "xyt", time, "zero", seed=5))
    want = solve_straight(inst, p, form)
    sweeps = inst.info().sweeps
    got = solve(inst, dict(p, flow=None), form)
    assert got.tobytes() == want.tobytes() and inst.info().sweeps == sweeps


@pytest.mark.parametrize("flow", ["collapse", "random"])
def test_two_runs_give_the_same_bytes(inst, flow):
    p = fb.nan_unread(fb.make_input("periodic_x", 47, 33, 3, 5, 1.0, "scatter", "sparse", "xyt", "periodic", flow))
    a, b = solve(inst, p, "gt"), solve(inst, p, "gt")
    assert a.tobytes() == b.tobytes()


# ---- 3. equivariance ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("time", fb.TIMES)
def test_a_constant_pan_is_the_straight_call_on_rolled_frames(inst, time):
    """periodic x and y, every state 0, a sparse weight, flow = a constant pan (dx, dy): frame t rolled back by t pans turns every link
    into a straight one (under periodic time the wrapping link too when T pans are a whole number of periods: 6 frames x (3, 2) on
    18 x 12).  The rolled straight answer is held to the flow input's yardstick, ERR and RES, as the flow call's own answer is: within
    the bounds, not to the byte, because the sums run in another order."""
    T, H, W, C, pan = 6, 12, 18, 3, (3, 2)
    p = fb.make_input("periodic_xy", H, W, C, T, 1.0, "all", "sparse", "xyt", time, "zero", seed=8)
    p["flow"] = np.broadcast_to(np.float32(pan), p["flow"].shape).copy()
    p["links"] = fb.links_of(p)
    y = fb.Yardstick(p, "gt")
    out = solve(inst, p, "gt")
    assert_yardstick(f"pan {time}", p, "gt", out, y)
    back = lambda a: a if a is None else np.stack([np.roll(a[t], (-t * pan[1], -t * pan[0]), (0, 1)) for t in range(a.shape[0])])
    q = {n: (back(a) if isinstance(a, np.ndarray) and n not in ("flow",) else a) for n, a in p.items() if n != "links"}
    straight = solve_straight(inst, q, "gt")
    forward = np.stack([np.roll(straight[t], (t * pan[1], t * pan[0]), (0, 1)) for t in range(T)])
    bad, err, res = y.check(forward)
    print(f"VOLUME_FLOW pan {time}: the rolled straight answer against the flow input's yardstick: ERR {err:.3g} (bound {y.bounds()[0]:.3g}) "
          f"RES {res:.3g} (bound {y.bounds()[1]:.3g})")
    assert not bad, bad
    assert_copied_bits(p, forward)


# ---- 4. tiling ----------------------------------------------------------------------------------------------------------------------
# (border, H, W, T, what the shape is there for)
_TILINGS = [("neumann", 47, 33, 5, "seam_in_band"), ("neumann", 47, 33, 5, "ends_in_other_bands"), ("neumann", 9, 300, 3, "ends_in_other_groups")]


@pytest.mark.parametrize("flow", ["split", "collapse"])
@pytest.mark.parametrize("case", _TILINGS, ids=[f"{c[4]}-{c[2]}x{c[1]}x{c[3]}" for c in _TILINGS])
def test_links_across_the_tiling(inst, case, flow):
    border, H, W, T, what = case
    args = (dict(column=256, amount=5) if flow == "split" else dict(column=280)) if W > 256 else {}          # (collapse: onto column 280)
    p = fb.make_input(border, H, W, 3, T, 1.0, "scatter", "sparse", "t", "free", flow, seed=11, **args)
    plan = capi.pcg_plan(W, H, G | capi.border_bits(p["sides"], False, p["periodic"]), T)
    ny, nx, rows = plan["ny"] // T, plan["nx"], plan["rows"]
    fwd, _ = p["links"]
    src = np.flatnonzero(fwd.reshape(-1) >= 0)
    dst = fwd.reshape(-1)[src]
    if what == "seam_in_band":
        assert any(0 < (t * ny) % rows for t in range(1, T)), ("a frame boundary strictly inside a band", plan)
    elif what == "ends_in_other_bands":
        assert plan["bands"] > 1 and ((src // nx) // rows != (dst // nx) // rows).any(), ("a link whose ends lie in different bands", plan)
    else:
        assert plan["cg"] > 1 and ((src % nx) // 256 != (dst % nx) // 256).any(), ("a link whose ends lie in different column groups", plan)
    out = solve(inst, p, "gt")
    assert_yardstick(f"tiling {what} {flow}", p, "gt", out)
    assert_copied_bits(p, out)


# ---- 5. the device call -------------------------------------------------------------------------------------------------------------
def _layout_views(name, T, H, W, fill):
    """(backing array filled with `fill`, its T x H x W x 3 view): a guard frame before and after, a gap between the frames"""
    if name == "hwc":
        back = np.full((T + 2, H + 2, W, 3), fill, np.float32)          # two rows between the frames
        return back, back[1:-1, :H]
    back = np.full((T + 2, 3, H + 1, W + 5), fill, np.float32)          # CHW, padded rows, a row between the planes
    return back, back[1:-1, :, :H, :W].transpose(0, 2, 3, 1)


_FIELDS = ("data", "state", "weight", "gx", "gy", "gt", "boundary", "smooth_x", "smooth_y", "smooth_t")
_NAMES = dict(smooth_x="sx", smooth_y="sy", smooth_t="smt")


def _flow_planes(p):
    """(flow_x, flow_y) with NaN where the header says the flow is not read: off the work rectangle"""
    T, H, W = p["state"].shape[:3]
    fx, fy = capi.volume_flow_planes(p["flow"], T, H, W, p["tper"])
    rows, cols = vf.unknowns(p["sides"], p["periodic"], H, W)
    read = np.zeros((H, W), bool)
    read[rows, cols] = True
    return tuple(np.where(read[None], a, np.float32(np.nan)).astype(np.float32) for a in (fx, fy))


@pytest.mark.parametrize("alias", ["none", "data"])
@pytest.mark.parametrize("layout", ["hwc", "chw_padded"])
def test_device_layouts_write_only_named_elements(inst, layout, alias):
    T, H, W = 4, 23, 17
    p = fb.nan_unread(fb.make_input("free_lt", H, W, 3, T, 1.3, "scatter", "sparse", "xyt", "periodic", "random", seed=3))          # Dirichlet lines right and bottom
    arrays = {}
    for name in _FIELDS + ("out",):
        back, view = _layout_views(layout, T, H, W, np.nan if name in ("gx", "gy", "gt", "smooth_x", "smooth_y", "smooth_t") else SENTINEL)
        if name != "out":
            view[...] = p[_NAMES.get(name, name)]          # (gt and smooth_t: T frames under periodic time)
        arrays[name] = (back, view)
    for name, plane in zip(("flow_x", "flow_y"), _flow_planes(p)):          # dense whatever the layout, a guard frame on either side
        back = np.full((T + 2, H, W), np.nan, np.float32)
        back[1:-1] = plane
        arrays[name] = (back, back[1:-1])
    lay = capi.poisson_layout_of(arrays["data"][1][0])
    stride = arrays["data"][1].strides[0] // 4
    assert stride > (H - 1) * lay.row_stride + (W - 1) * lay.col_stride + 2 * lay.channel_stride + 1, "the frames leave a gap"
    off = lambda name: arrays[name][1].__array_interface__["data"][0] - arrays[name][0].__array_interface__["data"][0]
    dev = {name: inst.to_device(back) for name, (back, _) in arrays.items()}
    try:
        jobs = capi.Instance.make_volume_flow_jobs(1)
        j = jobs[0]
        for name in _FIELDS + ("flow_x", "flow_y"):
            setattr(j, name, dev[name] + off(name))
        target = "out" if alias == "none" else alias
        j.out = dev[target] + off(target)
        kind = G | capi.border_bits(p["sides"], False, p["periodic"])
        rc = inst.volume_flow_device(capi.VolumeWlsParams(kind, T, stride, 1.3, 1, 0.0, 0, 0.0, 0.0, 0.0), lay, jobs)
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
    assert_copied_bits(p, got)
    assert_yardstick(f"device {layout} out={alias}", p, "gt", got)


# ---- 6. batches ---------------------------------------------------------------------------------------------------------------------
def _device_jobs(inst, probs, form="lap"):
    """VolumeFlowJob array of the inputs on dense device arrays, each with an out full of SENTINEL; (jobs, pointers to free)"""
    jobs = capi.Instance.make_volume_flow_jobs(len(probs))
    dev = []
    for k, p in enumerate(probs):
        T, H, W = p["state"].shape[:3]
        fx, fy = (None, None) if p["flow"] is None else (p["fx"], p["fy"]) if "fx" in p else capi.volume_flow_planes(p["flow"], T, H, W, p["tper"])
        fields = dict(wb.vb.call_args(p, form), data=p["data"], state=p["state"], weight=p["weight"], boundary=boundary_of(p), smooth_x=p["sx"],
                      smooth_y=p["sy"], smooth_t=p["smt"], flow_x=fx, flow_y=fy)
        for name, a in fields.items():
            if a is not None:
                dev.append(inst.to_device(np.ascontiguousarray(a, np.float32)))
                setattr(jobs[k], name, dev[-1])
        dev.append(inst.to_device(np.full(p["data"].shape, SENTINEL, np.float32)))
        jobs[k].out = dev[-1]
    return jobs, dev


def _params(p0, form):
    T, H, W, C = p0["data"].shape
    kind = (L if form == "lap" else G) | capi.border_bits(p0["sides"], False, p0["periodic"])
    return capi.VolumeWlsParams(kind, T, H * W * C, p0["tau"], 1 if p0["tper"] else 0, 0.0, 0, 0.0, 0.0, 0.0)


def _run_batch(inst, probs, form="lap"):
    p0 = probs[0]
    jobs, dev = _device_jobs(inst, probs, form)
    try:
        rc = inst.volume_flow_device(_params(p0, form), capi.poisson_layout_of(p0["data"][0]), jobs, allow_job_errors=True)
        codes = [j.rc for j in jobs]
        outs = [inst.from_device(j.out, p0["data"].shape, np.float32) for j in jobs]
    finally:
        for q in dev:
            inst.free(q)
    return rc, codes, outs


def _check_members(probs, outs, chunks, form):
    for members in chunks:
        means = fb.chunk_means([probs[k] for k in members])
        for k in members:
            y = fb.Yardstick(probs[k], form, means=means)
            bad, err, res = y.check(outs[k])
            print(f"VOLUME_FLOW batch member {k}: ERR {err:.3g} (pcg_f32 {y.err32:.3g}) RES {res:.3g} (pcg_f32 {y.res32:.3g})")
            assert not bad, (k, bad)
            assert_copied_bits(probs[k], outs[k])


@functools.lru_cache(maxsize=None)
def _trio():
    return [fb.make_input("free_lt", 23, 17, 3, 4, 1.0, pat, "constant", "xyt", "periodic", flow, seed=20 + k)
            for k, (pat, flow) in enumerate((("hole", "split"), ("scatter", "random"), ("keyframes", "pan")))]


@pytest.mark.parametrize("at", [1, 0])
def test_a_fractional_flow_fails_its_volume_only(inst, at):
    """the two that stay run as a chunk of two: their bytes are those of the call with those two alone (the chunk's means), and the
    link planes follow the volumes when the refused one leaves from the front"""
    probs = list(_trio())
    T, H, W = probs[at]["state"].shape[:3]
    fx, fy = capi.volume_flow_planes(probs[at]["flow"], T, H, W, True)
    fx = fx.copy()
    fx[1, H // 2, W // 2] = 0.5
    probs[at] = dict(probs[at], fx=fx, fy=fy)
    stay = [k for k in range(3) if k != at]
    rc, codes, outs = _run_batch(inst, probs, "gt")
    assert rc == capi.SC_ERR_BAD_ARG and codes == [capi.SC_ERR_BAD_ARG if k == at else capi.SC_OK for k in range(3)], (rc, codes)
    assert (outs[at] == SENTINEL).all(), "a refused volume must not be written"
    rc2, codes2, outs2 = _run_batch(inst, [probs[k] for k in stay], "gt")
    assert rc2 == capi.SC_OK
    for k, alone in zip(stay, outs2):
        assert outs[k].tobytes() == alone.tobytes(), "a member's bytes are those of the call without the refused volume"
    _check_members(probs, outs, [stay], "gt")


def test_a_flow_where_the_first_volume_has_none_is_refused(inst):
    probs = _trio()
    none = dict(probs[0], flow=None)
    rc, codes, outs = _run_batch(inst, [none, probs[1]], "gt")
    assert rc == capi.SC_ERR_BAD_ARG and codes == [capi.SC_OK, capi.SC_ERR_BAD_ARG], (rc, codes)
    assert (outs[1] == SENTINEL).all(), "a refused volume must not be written"
    want = _run_straight_batch(inst, [none], "gt")
    assert outs[0].tobytes() == want[0].tobytes(), "without a flow the call runs sc_hip_volume_wls's launches"
    rc, codes, outs = _run_batch(inst, [probs[1], none], "gt")
    assert rc == capi.SC_ERR_BAD_ARG and codes == [capi.SC_OK, capi.SC_ERR_BAD_ARG], (rc, codes)
    assert (outs[1] == SENTINEL).all()
    # exactly one of the two arrays
    T, H, W = probs[1]["state"].shape[:3]
    fx, fy = capi.volume_flow_planes(probs[1]["flow"], T, H, W, True)
    jobs, dev = _device_jobs(inst, [probs[0], probs[1]], "gt")
    try:
        jobs[1].flow_y = None
        rc = inst.volume_flow_device(_params(probs[0], "gt"), capi.poisson_layout_of(probs[0]["data"][0]), jobs, allow_job_errors=True)
        assert rc == capi.SC_ERR_BAD_ARG and [j.rc for j in jobs] == [capi.SC_OK, capi.SC_ERR_BAD_ARG]
    finally:
        for q in dev:
            inst.free(q)


def test_the_host_call_refuses_exactly_one_flow_array(inst):
    import ctypes as C
    p = _trio()[0]
    T, H, W, _ = p["data"].shape
    fx, fy = capi.volume_flow_planes(p["flow"], T, H, W, True)
    out = np.full(p["data"].shape, SENTINEL, np.float32)
    params = _params(p, "lap")
    lay = capi.poisson_layout_of(p["data"][0])
    ptr = lambda a: None if a is None else a.ctypes.data
    for one in ((fx, None), (None, fy)):
        rc = inst.L.sc_hip_volume_flow(inst.h, C.byref(params), C.byref(lay), None, None, None, ptr(p["lap"]), ptr(p["data"]), ptr(p["state"]),
                                       ptr(p["weight"]), ptr(p["sx"]), ptr(p["sy"]), ptr(p["smt"]), ptr(one[0]), ptr(one[1]), ptr(p["boundary"]),
                                       ptr(out))
        assert rc == capi.SC_ERR_BAD_ARG and (out == SENTINEL).all()


def _run_straight_batch(inst, probs, form):
    p0 = probs[0]
    jobs = capi.Instance.make_volume_wls_jobs(len(probs))
    dev = []
    try:
        for k, p in enumerate(probs):
            fields = dict(wb.vb.call_args(p, form), data=p["data"], state=p["state"], weight=p["weight"], boundary=boundary_of(p), smooth_x=p["sx"],
                          smooth_y=p["sy"], smooth_t=p["smt"])
            for name, a in fields.items():
                if a is not None:
                    dev.append(inst.to_device(np.ascontiguousarray(a, np.float32)))
                    setattr(jobs[k], name, dev[-1])
            dev.append(inst.to_device(np.full(p["data"].shape, SENTINEL, np.float32)))
            jobs[k].out = dev[-1]
        inst.volume_wls_device(_params(p0, form), capi.poisson_layout_of(p0["data"][0]), jobs)
        return [inst.from_device(j.out, p0["data"].shape, np.float32) for j in jobs]
    finally:
        for q in dev:
            inst.free(q)


@pytest.mark.parametrize("name", ["flow_x", "flow_y"])
def test_a_flow_array_that_overlaps_out_is_refused(inst, name):
    """a flow array may share no float of its own length with out's span -- here its last float is out's first"""
    p = fb.make_input("free_lt", 9, 7, 3, 4, 1.0, "scatter", "constant", "t", "periodic", "pan1", seed=30)
    T, H, W, C = p["data"].shape
    plane = capi.volume_flow_planes(p["flow"], T, H, W, True)[0 if name == "flow_x" else 1].ravel()
    for at, want in ((plane.size - 1, capi.SC_ERR_BAD_ARG), (plane.size, capi.SC_OK)):
        jobs, dev = _device_jobs(inst, [p], "gt")
        host = np.full(plane.size + p["data"].size + 8, SENTINEL, np.float32)
        host[:plane.size] = plane
        block = inst.to_device(host)
        dev.append(block)
        try:
            setattr(jobs[0], name, block)
            jobs[0].out = block + 4 * at
            inst.volume_flow_device(_params(p, "gt"), capi.poisson_layout_of(p["data"][0]), jobs, allow_job_errors=True)
            after = inst.from_device(block, host.shape, np.float32)
            assert jobs[0].rc == want, (at, jobs[0].rc)
        finally:
            for q in dev:
                inst.free(q)
        if want != capi.SC_OK:
            assert np.array_equal(after, host), "a refused volume must not be written"
        else:
            assert np.array_equal(after[:at], host[:at]) and (after[at + p["data"].size:] == SENTINEL).all()
            assert_yardstick(f"{name} ends where out begins", p, "gt", after[at:at + p["data"].size].reshape(p["data"].shape))


def test_nine_volumes_run_in_two_chunks(inst):
    """8 frames x 3 channels are 24 planes: a chunk holds 8 volumes, the ninth runs in a second one"""
    pats = ("hole", "scatter", "keyframes", "split", "all")
    flows = ("split", "random", "pan", "collapse", "far", "pan1", "zero")
    probs = [fb.make_input("neumann", 7, 5, 3, 8, 1.0, pats[k % 5], "sparse", "xyt", "periodic", flows[k % 7], seed=50 + k, **(dict(amount=2) if flows[k % 7] in ("split", "random") else {}))
             for k in range(9)]
    rc, codes, outs = _run_batch(inst, probs)
    assert rc == capi.SC_OK and codes == [capi.SC_OK] * 9, (rc, codes)
    _check_members(probs, outs, [list(range(8)), [8]], "lap")


# ---- 7. the Python entry points ---------------------------------------------------------------------------------------------------------
def _moving_video(T, H, W, C, pan, seed):
    """a texture that moves by `pan` = (dx, dy) pixels per frame (it wraps), float32 T x H x W x C"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    base = 2.0 + np.sin(x / 1.7) * np.cos(y / 2.3) + 0.6 * rng.standard_normal((H, W))
    frames = np.stack([np.roll(base, (t * pan[1], t * pan[0]), (0, 1)) for t in range(T)])
    return np.ascontiguousarray(np.broadcast_to(frames[..., None], (T, H, W, C)) * (1 + 0.1 * np.arange(C)), np.float32)


def _problem(v, state, flow, tau, weight=None, sx=None, sy=None, smt=None, data=None, **guidance):
    shape = v.shape
    full = lambda a: None if a is None else np.ascontiguousarray(np.broadcast_to(a.reshape(a.shape + (1,) * (len(shape) - a.ndim)), a.shape[:1] + shape[1:]), np.float32)
    p = dict(sides="lrtb", periodic="", tper=False, tau=tau, state=full(state.astype(np.float32)), data=v if data is None else data, weight=full(weight),
             sx=full(sx), sy=full(sy), smt=full(smt), boundary=None, lap=np.zeros_like(v), gx=None, gy=None, gt=None, flow=np.rint(flow).astype(np.float32))
    p.update(guidance)
    p["links"] = fb.links_of(p)
    return p


def test_volume_wls_solve_with_a_flow_against_the_exact_solve():
    p = fb.make_input("periodic_x", 23, 17, 3, 5, 0.5, "scatter", "sparse", "xyt", "periodic", "random", seed=7)
    flow = p["flow"] + np.float32(0.25)          # (the Python layer rounds)
    out = seamless_clone.volume_wls_solve(p["data"], p["state"], gx=p["gx"], gy=p["gy"], gt=p["gt"], weight=p["weight"], smooth_x=p["sx"],
                                          smooth_y=p["sy"], smooth_t=p["smt"], boundary=p["boundary"], tau=0.5, loop=True, neumann=False, free_sides="",
                                          periodic="x", flow=flow)
    assert_yardstick("volume_wls_solve(flow=)", p, "gt", out)
    assert_copied_bits(p, out)


def test_inpaint_video_follows_a_moving_texture():
    """a texture that moves 2 pixels per frame under a hole that stands still: along the flow every hidden surface point is visible in
    another frame, so the flow call recovers it; the straight links tie it to other surface points"""
    T, H, W, C, pan = 6, 20, 24, 1, (2, 0)
    truth = _moving_video(T, H, W, C, pan, 1)
    holes = np.zeros((T, H, W), bool)
    holes[:, 7:13, 9:15] = True
    frames = np.where(holes[..., None], np.float32(0), truth)
    flow = np.broadcast_to(np.float32(pan), (T - 1, H, W, 2))
    got = seamless_clone.inpaint_video(frames, holes, tau=4.0, flow=flow)
    plain = seamless_clone.inpaint_video(frames, holes, tau=4.0)
    p = _problem(frames, np.where(holes, 0, 1), flow, 4.0)
    assert_yardstick("inpaint_video(flow=)", p, "lap", got)
    scale = float(np.abs(truth[holes]).max())
    err, err_plain = (float(np.abs(a.astype(np.float64) - truth)[holes].max()) / scale for a in (got, plain))
    print(f"VOLUME_FLOW inpaint_video: ERR against the moving truth {err:.3g} with the flow, {err_plain:.3g} without")
    assert err < err_plain, (err, err_plain)
    assert np.array_equal(bits(got)[~holes], bits(frames)[~holes])


def test_poisson_clone_video_with_a_flow_against_the_exact_solve():
    T, H, W, C, pan = 4, 19, 23, 3, (1, -1)
    srcs, dsts = _moving_video(T, H, W, C, pan, 2), _moving_video(T, H, W, C, (0, 0), 3)
    masks = np.zeros((T, H, W), bool)
    for t in range(T):
        masks[t, 6 - t:12 - t, 5 + t:13 + t] = True          # the mask moves with the source
    flow = np.broadcast_to(np.float32(pan), (T - 1, H, W, 2))
    out = seamless_clone.poisson_clone_video(srcs, dsts, masks, tau=1.5, flow=flow)
    gx, gy = np.zeros_like(srcs), np.zeros_like(srcs)
    for t in range(T):
        gx[t], gy[t] = seamless_clone._forward_differences(srcs[t])
    partner, inside = seamless_clone._along_flow(srcs, np.asarray(flow), False)
    both = masks[:-1] & inside & seamless_clone._along_flow(masks, np.asarray(flow), False)[0]
    gt = np.where(both[..., None], partner - srcs[:-1], np.float32(0)).astype(np.float32)
    assert both.any() and np.abs(gt).max() < 1e-6, "along its own motion the source does not change"
    p = _problem(dsts, np.where(masks, 0, 1), flow, 1.5, gx=gx, gy=gy, gt=gt, lap=None)
    assert_yardstick("poisson_clone_video(flow=)", p, "gt", out)


@pytest.mark.parametrize("hard", [True, False])
def test_interpolate_constraints_video_with_a_flow_against_the_exact_solve(hard):
    T, H, W, C, pan = 4, 19, 23, 3, (2, 1)
    guide = _moving_video(T, H, W, 1, pan, 4)
    values = _moving_video(T, H, W, C, pan, 5)
    known = np.random.default_rng(6).random((T, H, W)) < 0.05
    known[1:3] = False                                      # two frames are filled through time alone
    flow = np.broadcast_to(np.float32(pan), (T - 1, H, W, 2))
    sigma = 0.3
    out = seamless_clone.interpolate_constraints_video(values, known, guide, edge_sigma=sigma, tau=0.3, hard=hard, strength=2.0, flow=flow)          # (links over three decades: a larger tau leaves the call's budget)
    dx, dy, _ = seamless_clone._video_abs_differences(guide, False)
    g = np.asarray(guide, np.float64)
    dt = np.sqrt(((seamless_clone._along_flow(g, np.asarray(flow), False)[0] - g[:-1]) ** 2).sum(3))
    sx, sy, smt = ((np.exp(-d * d / (2.0 * sigma * sigma)) + 1e-3).astype(np.float32) for d in (dx, dy, dt))
    if hard:
        p = _problem(values, np.where(known, 1, 0), flow, 0.3, sx=sx, sy=sy, smt=smt)
        assert np.array_equal(bits(out)[known], bits(values)[known])
    else:
        d = np.where(known[:, :, :, None], values, np.float32(0)).astype(np.float32)
        p = _problem(values, np.zeros((T, H, W)), flow, 0.3, weight=np.where(known, np.float32(2), np.float32(0)), sx=sx, sy=sy, smt=smt, data=d)
    assert_yardstick(f"interpolate_constraints_video(flow=, hard={hard})", p, "lap", out)
