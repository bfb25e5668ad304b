"""GPU tests of the sub-pixel flow volume solve (sc_hip_volume_subflow, sc_hip_volume_subflow_device) through capi: WLS volume solves
whose temporal links are bilinear stencils along a caller's real-valued flow.

1. against the float64 solve (tests/volume_subflow_np.py) on tests/volume_subflow_bounds.py's matrix through the host call --
   volume_bounds' borders, sizes, frames, channels, states, weights and forms, volume_wls_bounds' links and times, the eight flows zero /
   half / pan / axis / random / whole / collapse / edge: ERR and RES within the bounds, the iteration count within twice the reference
   iteration's plus the polling period, out's bits at KNOWN and OUTSIDE pixels data's and on the Dirichlet lines boundary's.
2. ties and determinism: no flow gives the bytes and the sweep count of sc_hip_volume_wls; two runs of a random and of a collapse call
   give the same bytes; on a whole pan and on a zero flow the new call and sc_hip_volume_flow pass the same yardstick.
3. tiling: shapes where sc_hip_pcg_plan puts a frame boundary inside a band, a link's taps in two bands, in two 256-column groups,
   wrapping on a periodic axis; collapse and random against the exact solve at each.
4. the device call: HWC and CHW with padded rows, a frame stride with a gap, guard frames around every array, NaN in every element the
   header says is not read: nothing but the named elements of out is written, out may be data.
5. batches: a volume with a flow where the first has none and the reverse, exactly one flow array, a flow array that overlaps out, nine
   volumes in two chunks, a fractional value accepted where sc_hip_volume_flow refuses it; the link storage of one volume is one
   volume's.
6. volume_wls_solve, inpaint_video, poisson_clone_video and interpolate_constraints_video with subpixel=True against the float64 solve;
   with the default they give the rounded call's bytes.
7. motion: inpaint_video(flow=, subpixel=True) recovers a texture that moves half a pixel per frame under a static hole better than
   the rounded call (tests/test_volume_subflow_host.py holds the float64 solves to a factor 1.5)."""
from __future__ import annotations

import functools

import numpy as np
import pytest

from seamlesscloneoptimization_amd import capi, seamless_clone

import volume_flow_bounds as fb
import volume_subflow_bounds as sb
import volume_subflow_np as vs
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
    return p["boundary"] if vs.has_dirichlet(p["sides"], p["periodic"]) else None


def solve(inst, p, form="lap", **kw):
    return inst.volume_subflow(p["data"], p["state"], weight=p["weight"], boundary=boundary_of(p), tau=p["tau"], free_sides=p["sides"],
                               periodic=p["periodic"], **sb.call_args(p, form), **kw)


def solve_straight(inst, p, form="lap"):
    return inst.volume_wls(p["data"], p["state"], p["weight"], boundary=boundary_of(p), tau=p["tau"], free_sides=p["sides"], periodic=p["periodic"],
                           **wb.call_args(p, form))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_copied_bits(p, out):
    """out at KNOWN and OUTSIDE pixels is data, on the Dirichlet lines boundary, bit for bit"""
    k = vs.kinds(p["sides"], p["periodic"], p["state"])
    out = out.reshape(k.shape)
    held = (k == vs.KNOWN) | (k == vs.OUTSIDE)
    assert np.array_equal(bits(out)[held], bits(p["data"].reshape(k.shape))[held]), "KNOWN and OUTSIDE pixels must be data's bits"
    line = k == vs.DIRICHLET
    assert np.array_equal(bits(out)[line], bits(p["boundary"].reshape(k.shape))[line]), "Dirichlet lines must be boundary's bits"
    assert np.isfinite(out[k == vs.UNKNOWN]).all(), "an unread element's NaN reached the answer"


def assert_yardstick(tag, p, form, out, y=None):
    """out lies within the yardstick's ERR and RES bounds for this input"""
    y = y or sb.Yardstick(p, form)
    assert y.rel32 <= 1e-5 and 2 * y.iters32 + POLL <= sb.MAX_ITERS, "the reference iteration must stay within the call's budget"
    bad, err, res = y.check(out)
    print(f"VOLUME_SUBFLOW {tag}: ERR {err:.3g} (pcg_f32 {y.err32:.3g}) RES {res:.3g} (pcg_f32 {y.res32:.3g}) pcg_f32 iterations {y.iters32}")
    assert not bad, bad


# ---- 1. against the exact solve ------------------------------------------------------------------------------------------------
_CASES = sb.matrix()
_IDS = [f"{b}-{W}x{H}x{C}x{T}-tau{tau:g}-{p}-{wk}-{f}-{ln}-{tm}-{fl}" for b, H, W, C, T, tau, p, wk, f, ln, tm, fl in _CASES]


@pytest.mark.parametrize("i", range(len(_CASES)), ids=_IDS)
def test_against_the_exact_solve(inst, i):
    H, W = _CASES[i][1:3]
    p, form, y = sb.matrix_case(i)
    assert y.rel32 <= 1e-5 and y.max_sweeps() <= sb.MAX_ITERS, "the reference iteration must stay within the call's budget on every input"
    out = solve(inst, p, form)
    info = inst.info()
    bad, err, res = y.check(out)
    print(f"VOLUME_SUBFLOW {_IDS[i]}: ERR {err:.3g} (pcg_f32 {y.err32:.3g}) RES {res:.3g} (pcg_f32 {y.res32:.3g}) sweeps {info.sweeps} "
          f"(pcg_f32 {y.iters32}) rel {info.rel_residual:.3g}")
    assert (info.method, info.converged, info.W, info.H) == (capi.SC_METHOD_FFT, 1, W, H)
    assert info.sweeps <= y.max_sweeps(), (info.sweeps, y.iters32)
    assert not bad, bad
    assert_copied_bits(p, out)


# ---- 2. ties and determinism ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("time", sb.TIMES)
@pytest.mark.parametrize("form", sb.FORMS)
def test_no_flow_gives_the_bytes_and_sweeps_of_the_wls_call(inst, form, time):
    q = wb.nan_unread(sb.make_input("periodic_x", 23, 17, 3, 4, 0.6, "hole", "constant", "xyt", time, "zero", seed=5))          # (without a flow every straight link is read)
    want = solve_straight(inst, q, form)
    sweeps = inst.info().sweeps
    got = solve(inst, dict(q, flow=None), form)
    assert got.tobytes() == want.tobytes() and inst.info().sweeps == sweeps


@pytest.mark.parametrize("flow", ["collapse", "random"])
def test_two_runs_give_the_same_bytes(inst, flow):
    p = sb.nan_unread(sb.make_input("periodic_x", 47, 33, 3, 5, 1.0, "scatter", "sparse", "xyt", "periodic", flow))
    a, b = solve(inst, p, "gt"), solve(inst, p, "gt")
    assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("flow", ["pan1", "zero"])
def test_on_a_whole_flow_without_collisions_both_calls_pass_the_same_yardstick(inst, flow):
    """a whole-numbered flow without collisions: sc_hip_volume_flow's matching keeps every candidate, the two calls solve one system, and
    each is held to the exact solve of it -- to the bounds, not to the byte (the product form rounds differently)"""
    q = fb.make_input("neumann", 23, 17, 3, 4, 1.0, "scatter", "sparse", "xyt", "free", flow, seed=6)
    p = dict(q, links=sb.links_of(q))
    y = sb.Yardstick(p, "gt")
    yf = fb.Yardstick(q, "gt")
    assert np.abs(y.want - yf.want).max() <= 1e-9 * np.abs(yf.want).max(), "the two restatements solve the same system"
    new = solve(inst, p, "gt")
    old = inst.volume_flow(q["data"], q["state"], weight=q["weight"], boundary=boundary_of(q), tau=q["tau"], free_sides=q["sides"],
                           periodic=q["periodic"], **fb.call_args(q, "gt"))
    for tag, out in (("volume_subflow", new), ("volume_flow", old)):
        assert_yardstick(f"{flow} {tag}", p, "gt", out, y)
        bad, _, _ = yf.check(out)
        assert not bad, (tag, bad)


# ---- 3. tiling ----------------------------------------------------------------------------------------------------------------------
# (border, H, W, T, what the shape is there for)
_TILINGS = [("neumann", 47, 33, 5, "seam_in_band"), ("neumann", 47, 33, 5, "taps_in_two_bands"), ("neumann", 9, 300, 3, "taps_in_two_groups"),
            ("periodic_xy", 9, 14, 3, "taps_wrap")]


def tiling_input(case, flow):
    """the input of one tiling case, its premise asserted (host arithmetic only: tests/test_volume_subflow_host.py runs it too)"""
    border, H, W, T, what = case
    sides, periodic = {b[0]: b[1:] for b in sb.BORDERS}[border]
    plan = capi.pcg_plan(W, H, G | capi.border_bits(sides, False, periodic), T)
    ny, nx, rows = plan["ny"] // T, plan["nx"], plan["rows"]
    args = {}
    if flow == "collapse":          # onto a point whose taps straddle the seam the case is about
        if W > 256:
            args["column"] = 256          # the point (255.5, .): taps in columns 255 and 256
        if what == "taps_wrap":
            args["column"] = 0            # the point (-0.5, .): taps in the last column and in column 0
        if what == "taps_in_two_bands":
            args["row"] = next(r for r in range(1, ny) if (ny + r) % rows == 0)          # rows r - 1 and r of frame 1 lie in two bands
    p = sb.make_input(border, H, W, 3, T, 1.0, "scatter", "sparse", "t", "free", flow, seed=11, **args)
    idx, _ = p["links"]
    has = idx >= 0
    first = np.where(has, idx, np.iinfo(np.int64).max).min(-1)
    last = np.where(has, idx, -1).max(-1)
    linked = has.any(-1)
    if what == "seam_in_band":
        assert any(0 < (t * ny) % rows for t in range(1, T)), ("a frame boundary strictly inside a band", plan)
    elif what == "taps_in_two_bands":
        assert plan["bands"] > 1 and ((first // nx) // rows != (last // nx) // rows)[linked].any(), ("a link whose taps lie in two bands", plan)
    elif what == "taps_in_two_groups":
        assert plan["cg"] > 1 and ((first % nx) // 256 != (last % nx) // 256)[linked].any(), ("a link whose taps straddle columns 255 / 256", plan)
    else:
        assert ((last % nx) - (first % nx) > 1)[linked].any(), "a link whose taps wrap around a periodic axis"
    return p


@pytest.mark.parametrize("flow", ["collapse", "random"])
@pytest.mark.parametrize("case", _TILINGS, ids=[f"{c[4]}-{c[2]}x{c[1]}x{c[3]}" for c in _TILINGS])
def test_links_across_the_tiling(inst, case, flow):
    p = tiling_input(case, flow)
    out = solve(inst, p, "gt")
    assert_yardstick(f"tiling {case[4]} {flow}", p, "gt", out)
    assert_copied_bits(p, out)


# ---- 4. the device call -------------------------------------------------------------------------------------------------------------
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
    fx, fy = capi.volume_subflow_planes(p["flow"], T, H, W, p["tper"])
    rows, cols = vs.unknowns(p["sides"], p["periodic"], H, W)
    read = np.zeros((H, W), bool)
    read[rows, cols] = True
    return tuple(np.where(read[None], a, np.float32(np.nan)).astype(np.float32) for a in (fx, fy))


@pytest.mark.parametrize("alias", ["none", "data"])
@pytest.mark.parametrize("layout", ["hwc", "chw_padded"])
def test_device_layouts_write_only_named_elements(inst, layout, alias):
    T, H, W = 4, 23, 17
    p = sb.nan_unread(sb.make_input("free_lt", H, W, 3, T, 1.3, "scatter", "sparse", "xyt", "periodic", "random", seed=3))          # Dirichlet lines right and bottom
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
        rc = inst.volume_subflow_device(capi.VolumeWlsParams(kind, T, stride, 1.3, 1, 0.0, 0, 0.0, 0.0, 0.0), lay, jobs)
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


# ---- 5. batches ---------------------------------------------------------------------------------------------------------------------
def _device_jobs(inst, probs, form="lap"):
    """VolumeFlowJob array of the inputs on dense device arrays, each with an out full of SENTINEL; (jobs, pointers to free)"""
    jobs = capi.Instance.make_volume_flow_jobs(len(probs))
    dev = []
    for k, p in enumerate(probs):
        T, H, W = p["state"].shape[:3]
        fx, fy = (None, None) if p["flow"] is None else capi.volume_subflow_planes(p["flow"], T, H, W, p["tper"])
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


def _run_batch(inst, probs, form="lap", call="volume_subflow_device"):
    p0 = probs[0]
    jobs, dev = _device_jobs(inst, probs, form)
    try:
        rc = getattr(inst, call)(_params(p0, form), capi.poisson_layout_of(p0["data"][0]), jobs, allow_job_errors=True)
        codes = [j.rc for j in jobs]
        outs = [inst.from_device(j.out, p0["data"].shape, np.float32) for j in jobs]
    finally:
        for q in dev:
            inst.free(q)
    return rc, codes, outs


def _check_members(probs, outs, chunks, form):
    for members in chunks:
        means = sb.chunk_means([probs[k] for k in members])
        for k in members:
            y = sb.Yardstick(probs[k], form, means=means)
            bad, err, res = y.check(outs[k])
            print(f"VOLUME_SUBFLOW batch member {k}: ERR {err:.3g} (pcg_f32 {y.err32:.3g}) RES {res:.3g} (pcg_f32 {y.res32:.3g})")
            assert not bad, (k, bad)
            assert_copied_bits(probs[k], outs[k])


@functools.lru_cache(maxsize=None)
def _trio():
    return [sb.make_input("free_lt", 23, 17, 3, 4, 1.0, pat, "constant", "xyt", "periodic", flow, seed=20 + k)
            for k, (pat, flow) in enumerate((("hole", "half"), ("scatter", "random"), ("keyframes", "pan")))]


def test_a_fractional_flow_is_accepted_where_the_flow_call_refuses_it(inst):
    """three volumes with fractional flows run as one chunk here; sc_hip_volume_flow_device refuses each of them and writes nothing"""
    probs = list(_trio())
    rc, codes, outs = _run_batch(inst, probs, "gt")
    assert rc == capi.SC_OK and codes == [capi.SC_OK] * 3, (rc, codes)
    _check_members(probs, outs, [[0, 1, 2]], "gt")
    rc, codes, outs = _run_batch(inst, probs, "gt", call="volume_flow_device")
    assert rc == capi.SC_ERR_BAD_ARG and codes == [capi.SC_ERR_BAD_ARG] * 3, (rc, codes)
    assert all((o == SENTINEL).all() for o in outs), "a refused volume must not be written"


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
    jobs, dev = _device_jobs(inst, [probs[0], probs[1]], "gt")
    try:
        jobs[1].flow_y = None
        rc = inst.volume_subflow_device(_params(probs[0], "gt"), capi.poisson_layout_of(probs[0]["data"][0]), jobs, allow_job_errors=True)
        assert rc == capi.SC_ERR_BAD_ARG and [j.rc for j in jobs] == [capi.SC_OK, capi.SC_ERR_BAD_ARG]
    finally:
        for q in dev:
            inst.free(q)


def test_the_host_call_refuses_exactly_one_flow_array(inst):
    import ctypes as C
    p = _trio()[0]
    T, H, W, _ = p["data"].shape
    fx, fy = capi.volume_subflow_planes(p["flow"], T, H, W, True)
    out = np.full(p["data"].shape, SENTINEL, np.float32)
    params = _params(p, "lap")
    lay = capi.poisson_layout_of(p["data"][0])
    ptr = lambda a: None if a is None else a.ctypes.data
    for one in ((fx, None), (None, fy)):
        rc = inst.L.sc_hip_volume_subflow(inst.h, C.byref(params), C.byref(lay), None, None, None, ptr(p["lap"]), ptr(p["data"]), ptr(p["state"]),
                                          ptr(p["weight"]), ptr(p["sx"]), ptr(p["sy"]), ptr(p["smt"]), ptr(one[0]), ptr(one[1]), ptr(p["boundary"]),
                                          ptr(out))
        assert rc == capi.SC_ERR_BAD_ARG and (out == SENTINEL).all()


@pytest.mark.parametrize("name", ["flow_x", "flow_y"])
def test_a_flow_array_that_overlaps_out_is_refused(inst, name):
    """a flow array may share no float of its own length with out's span -- here its last float is out's first"""
    p = sb.make_input("free_lt", 9, 7, 3, 4, 1.0, "scatter", "constant", "t", "periodic", "half", seed=30)
    T, H, W, C = p["data"].shape
    plane = capi.volume_subflow_planes(p["flow"], T, H, W, True)[0 if name == "flow_x" else 1].ravel()
    for at, want in ((plane.size - 1, capi.SC_ERR_BAD_ARG), (plane.size, capi.SC_OK)):
        jobs, dev = _device_jobs(inst, [p], "gt")
        host = np.full(plane.size + p["data"].size + 8, SENTINEL, np.float32)
        host[:plane.size] = plane
        block = inst.to_device(host)
        dev.append(block)
        try:
            setattr(jobs[0], name, block)
            jobs[0].out = block + 4 * at
            inst.volume_subflow_device(_params(p, "gt"), capi.poisson_layout_of(p["data"][0]), jobs, allow_job_errors=True)
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
    probs = [sb.make_input("neumann", 7, 5, 3, 8, 1.0, pats[k % 5], "sparse", "xyt", "periodic", sb.FLOWS[k % 8], seed=50 + k,
                           **(dict(amount=2) if sb.FLOWS[k % 8] in ("whole", "random") else {})) for k in range(9)]
    rc, codes, outs = _run_batch(inst, probs)
    assert rc == capi.SC_OK and codes == [capi.SC_OK] * 9, (rc, codes)
    _check_members(probs, outs, [list(range(8)), [8]], "lap")


def _arena_after(call):
    """the bytes a fresh instance's arena holds after `call(inst)`: sc_run_info.device_bytes of a small clone behind it"""
    from oracle import oracle_np
    dst, patch, mask, cx, cy = oracle_np.synth_inputs(96, 64, margin=32)
    inst = capi.Instance(0)
    try:
        call(inst)
        inst.run(patch, dst.copy(), mask, cx, cy, sync=True)
        return int(inst.info().device_bytes)
    finally:
        inst.destroy()


def test_the_link_storage_is_that_of_the_call_s_volumes():
    """one volume of two single-channel frames -- an optical-flow pair -- holds the links of one volume, not of the 96 a chunk of such
    volumes could hold: 48 bytes per pixel and frame, 64 more while they are built, rho | LT 8.  The arena grows by
    doubling, hence the factor 2, and in slabs of up to 32 MiB for its small pieces, hence the slack"""
    T, H, W = 2, 512, 512
    rng = np.random.default_rng(3)
    data = rng.standard_normal((T, H, W, 1)).astype(np.float32)
    state = np.zeros((T, H, W, 1), np.float32)
    weight = np.ones((T, H, W, 1), np.float32)
    lap = np.zeros_like(data)
    flow = np.full((T - 1, H, W, 2), 0.5, np.float32)
    straight = _arena_after(lambda inst: inst.volume_wls(data, state, weight, lap=lap, tau=1.0, neumann=True))
    subflow = _arena_after(lambda inst: inst.volume_subflow(data, state, flow, weight, lap=lap, tau=1.0, neumann=True))
    n = T * H * W
    print(f"VOLUME_SUBFLOW arena: {straight} bytes behind the straight call, {subflow} behind the sub-pixel call, {n} elements")
    assert subflow - straight <= 2 * (48 + 64 + 8) * n + (64 << 20), (straight, subflow)


# ---- 6. the Python entry points ---------------------------------------------------------------------------------------------------------
_moving_video = sb.moving_video


def _problem(v, state, flow, tau, weight=None, sx=None, sy=None, smt=None, data=None, **guidance):
    shape = v.shape
    full = lambda a: None if a is None else np.ascontiguousarray(np.broadcast_to(a.reshape(a.shape + (1,) * (len(shape) - a.ndim)), a.shape[:1] + shape[1:]), np.float32)
    p = dict(sides="lrtb", periodic="", tper=False, tau=tau, state=full(state.astype(np.float32)), data=v if data is None else data, weight=full(weight),
             sx=full(sx), sy=full(sy), smt=full(smt), boundary=None, lap=np.zeros_like(v), gx=None, gy=None, gt=None, flow=np.asarray(flow, np.float32))
    p.update(guidance)
    p["links"] = sb.links_of(p)
    return p


def test_volume_wls_solve_with_a_subpixel_flow_against_the_exact_solve():
    p = sb.make_input("periodic_x", 23, 17, 3, 5, 0.5, "scatter", "sparse", "xyt", "periodic", "random", seed=7)
    kw = dict(gx=p["gx"], gy=p["gy"], gt=p["gt"], weight=p["weight"], smooth_x=p["sx"], smooth_y=p["sy"], smooth_t=p["smt"], boundary=p["boundary"],
              tau=0.5, loop=True, neumann=False, free_sides="", periodic="x", flow=p["flow"])
    out = seamless_clone.volume_wls_solve(p["data"], p["state"], subpixel=True, **kw)
    assert_yardstick("volume_wls_solve(flow=, subpixel=True)", p, "gt", out)
    assert_copied_bits(p, out)
    # the default still rounds: the bytes of the call on the rounded flow
    inst = capi.Instance(0)
    try:
        want = inst.volume_flow(p["data"], p["state"], np.rint(p["flow"]), weight=p["weight"], smooth_x=p["sx"], smooth_y=p["sy"], smooth_t=p["smt"],
                                gx=p["gx"], gy=p["gy"], gt=p["gt"], boundary=p["boundary"], tau=0.5, loop=True, periodic="x")
    finally:
        inst.destroy()
    for got in (seamless_clone.volume_wls_solve(p["data"], p["state"], **kw), seamless_clone.volume_wls_solve(p["data"], p["state"], subpixel=False, **kw)):
        assert got.tobytes() == want.tobytes()


def test_inpaint_video_follows_a_texture_that_moves_half_a_pixel():
    truth, holes, frames, flow = sb.motion_case()
    tau = sb.MOTION_TAU
    got = seamless_clone.inpaint_video(frames, holes, tau=tau, flow=flow, subpixel=True)
    rounded = seamless_clone.inpaint_video(frames, holes, tau=tau, flow=flow)
    assert rounded.tobytes() == seamless_clone.inpaint_video(frames, holes, tau=tau, flow=np.rint(flow)).tobytes(), "the default rounds the flow"
    p = _problem(frames, np.where(holes, 0, 1), flow, tau)
    assert_yardstick("inpaint_video(flow=, subpixel=True)", p, "lap", got)
    rms = lambda a: float(np.sqrt(((a.astype(np.float64) - truth)[holes] ** 2).mean()))
    err, err_rounded = rms(got), rms(rounded)
    print(f"VOLUME_SUBFLOW inpaint_video: rms error against the moving truth {err:.3g} with the sub-pixel flow, {err_rounded:.3g} with the rounded one")
    assert err < err_rounded, (err, err_rounded)
    assert np.array_equal(bits(got)[~holes], bits(frames)[~holes])


def test_poisson_clone_video_with_a_subpixel_flow_against_the_exact_solve():
    T, H, W, C, pan = 4, 19, 23, 3, (0.5, -0.25)
    srcs, dsts = _moving_video(T, H, W, C, pan, 2), _moving_video(T, H, W, C, (0, 0), 3)
    masks = np.zeros((T, H, W), bool)
    masks[:, 5:13, 6:15] = True
    flow = np.broadcast_to(np.float32(pan), (T - 1, H, W, 2))
    out = seamless_clone.poisson_clone_video(srcs, dsts, masks, tau=1.5, flow=flow, subpixel=True)
    gx, gy = np.zeros_like(srcs), np.zeros_like(srcs)
    for t in range(T):
        gx[t], gy[t] = seamless_clone._forward_differences(srcs[t])
    # the temporal guidance: the source's difference along the bilinear link where the source and all its taps lie in the mask
    state = np.where(masks, 0, 1)
    p = _problem(dsts, state, flow, 1.5, gx=gx, gy=gy, gt=None, lap=None)
    idx, b = p["links"]
    s64 = srcs.astype(np.float64).reshape(-1, C)
    inside = (idx >= 0).any(-1)
    partner = sum(b[..., k, None].astype(np.float64) * s64[np.where(idx[..., k] >= 0, idx[..., k], 0)].reshape(srcs.shape) for k in range(4))
    mflat = masks.reshape(-1)
    all_in = masks & inside
    for k in range(4):
        all_in &= (idx[..., k] < 0) | mflat[np.where(idx[..., k] >= 0, idx[..., k], 0)]
    gt = np.where(all_in[..., None], partner - srcs, 0.0)[:-1].astype(np.float32)
    assert all_in[:-1].any()
    p["gt"] = gt
    assert_yardstick("poisson_clone_video(flow=, subpixel=True)", p, "gt", out)
    default = seamless_clone.poisson_clone_video(srcs, dsts, masks, tau=1.5, flow=flow)
    assert default.tobytes() == seamless_clone.poisson_clone_video(srcs, dsts, masks, tau=1.5, flow=np.rint(flow)).tobytes()


@pytest.mark.parametrize("hard", [True, False])
def test_interpolate_constraints_video_with_a_subpixel_flow_against_the_exact_solve(hard):
    T, H, W, C, pan = 4, 19, 23, 3, (1.5, 0.25)
    guide = _moving_video(T, H, W, 1, pan, 4)
    values = _moving_video(T, H, W, C, pan, 5)
    known = np.random.default_rng(6).random((T, H, W)) < 0.05
    known[1:3] = False                                      # two frames are filled through time alone
    flow = np.broadcast_to(np.float32(pan), (T - 1, H, W, 2))
    sigma = 0.3
    out = seamless_clone.interpolate_constraints_video(values, known, guide, edge_sigma=sigma, tau=0.3, hard=hard, strength=2.0, flow=flow, subpixel=True)
    dx, dy, _ = seamless_clone._video_abs_differences(guide, False)
    g = np.asarray(guide, np.float64)
    # the guide's difference along the bilinear link, from the restatement's own taps (reflecting borders: the work rectangle is the frame);
    # where a pixel holds no link the difference is 0 -- the element is not read
    idx, b = vs.taps("lrtb", "", False, (T, H, W), np.asarray(flow))
    gflat = g.reshape(-1, g.shape[3])
    partner = sum(b[..., k, None].astype(np.float64) * gflat[np.where(idx[..., k] >= 0, idx[..., k], 0)].reshape(g.shape) for k in range(4))
    dt = np.sqrt((np.where((idx >= 0).any(-1)[..., None], partner - g, 0.0)[:-1] ** 2).sum(3))
    sx, sy, smt = ((np.exp(-d * d / (2.0 * sigma * sigma)) + 1e-3).astype(np.float32) for d in (dx, dy, dt))
    if hard:
        p = _problem(values, np.where(known, 1, 0), flow, 0.3, sx=sx, sy=sy, smt=smt)
        assert np.array_equal(bits(out)[known], bits(values)[known])
    else:
        d = np.where(known[:, :, :, None], values, np.float32(0)).astype(np.float32)
        p = _problem(values, np.zeros((T, H, W)), flow, 0.3, weight=np.where(known, np.float32(2), np.float32(0)), sx=sx, sy=sy, smt=smt, data=d)
    assert_yardstick(f"interpolate_constraints_video(flow=, subpixel=True, hard={hard})", p, "lap", out)
    kw = dict(edge_sigma=sigma, tau=0.3, hard=hard, strength=2.0)
    default = seamless_clone.interpolate_constraints_video(values, known, guide, flow=flow, **kw)
    assert default.tobytes() == seamless_clone.interpolate_constraints_video(values, known, guide, flow=np.rint(flow), **kw).tobytes()
