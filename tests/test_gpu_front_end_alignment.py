"""Every reader of a clone's input bytes, bit for bit, at every byte alignment, inside guard bands.

The walk of tests/front_end_cases.py through sc_hip_front_end_device: the scan, the erodes and the fused pre-process run where the
caller's bytes lie -- mask, patch and destination each at its own base offset and row padding inside ONE device allocation, 4096 guard
bytes around every image -- in every launch form a clone can take: solo, on a predicted box (the scan riding in the pre-process launch,
the tiles eroding the mask themselves), same-size group, size class.  Every case runs twice, with 0x00 and with 0xFF in the guard bands
and the row padding; both runs must give the same values and both must equal the restatement on the dense content, with
np.array_equal: the mask is bytes, U0 byte values, lap an integer in [-1020, 1020] (exact in float16), and the grey blend holds the
equality test_opencv_grey_mask_semantics holds.  A stray read shows as a wrong value, never as a fault.

One test per reader and form; each judges its reader alone (front_end_cases.py says how the walks keep the readers apart).
tests/test_front_end_alignment_host.py checks from the geometry alone that the walk reaches what these tests claim."""
import numpy as np
import pytest

import front_end_cases as fc

pytestmark = pytest.mark.gpu


class FrontEnd:
    """An instance of its own and one device allocation that every case's buffer is uploaded into."""

    def __init__(self):
        from seamlesscloneoptimization_amd import capi
        self.capi = capi
        self.inst = capi.Instance(0)
        self.raw, self.cap, self.state = None, 0, None
        self.calls = 0

    def close(self):
        if self.raw:
            self.inst.free(self.raw)
        self.inst.destroy()

    def base(self, n):
        if n > self.cap:
            if self.raw:
                self.inst.free(self.raw)
            self.cap = max(n, 4 << 20)
            self.raw = self.inst.malloc(self.cap + 4096)
        return (self.raw + 4095) // 4096 * 4096          # (guard bands are multiples of 4096: an image's address mod 16 is its o)

    def configure(self, mode, grey, method=None):
        state = (mode, grey, method)
        if state != self.state:
            self.inst.set_clone_mode(mode)
            self.inst.set_solver(method=self.capi.SC_METHOD_AUTO if method is None else method, flags=self.capi.SC_FLAG_OPENCV_GREY_MASK if grey else 0)
            self.state = state

    def place(self, case, fill):
        """The case's buffer on the device: (host copy, plan, jobs)."""
        buf, plan = fc.build_arena(case, fill)
        d = self.base(buf.size)
        self.inst._check(self.inst.L.sc_hip_memcpy_h2d(self.inst.h, d, buf.ctypes.data, buf.size))
        jobs = (self.capi.BatchJob * len(case.members))()
        for j, m, ((bm, sm), (bf, sf), (bb, sb)) in zip(jobs, case.members, plan):
            mh, mw = m.c.mask.shape
            br, bc = m.c.dst.shape[:2]
            j.face, j.face_cols, j.face_rows, j.face_step = d + bf, mw, mh, sf
            j.body, j.body_cols, j.body_rows, j.body_step = d + bb, bc, br, sb
            j.mask, j.mask_cols, j.mask_rows, j.mask_step = d + bm, mw, mh, sm
            j.centerX, j.centerY, j.body_restore = m.c.cx, m.c.cy, None
        return buf, plan, jobs

    def run(self, case, fill):
        self.configure(case.mode, case.grey)
        _, _, jobs = self.place(case, fill)
        self.calls += 1
        return self.inst.front_end_device(jobs, case.form, case.storage, [m.guess for m in case.members] if case.form == 1 else None, case.fields)


@pytest.fixture(scope="module")
def fe():
    from oracle import oracle_c
    oracle_c.build()
    f = FrontEnd()
    yield f
    f.close()


def _geo_dict(a):
    return dict(zip(("x0", "y0", "W", "H", "ltx", "lty"), (int(v) for v in a)))


def check(fe, case, what):
    """Runs `case` with both fills and judges `what` of it: 'rect' (rectangle, code, geo), 'M' (the eroded mask of the ROI the launch ran
    on), 'rhs' (B and lap).  Raises with the case's placements, residues and the first pixel that differs."""
    res = {fill: fe.run(case, fill) for fill in (0x00, 0xFF)}
    for k, m in enumerate(case.members):
        want = fc.expected(case, m)
        for fill, rs in res.items():
            r, bad = rs[k], []
            if "rect" in what:
                if r["rect_dev"] != want["rect"] or r["rect_host"] != want["rect"]:
                    bad.append("rectangle: device copy %s, pinned mailbox %s, want %s" % (r["rect_dev"], r["rect_host"], want["rect"]))
                if r["rc"] != want["rc"]:
                    bad.append("member code %d, want %d" % (r["rc"], want["rc"]))
                if want["geo"] is not None and not np.array_equal(r["geo"], want["geo"]):
                    bad.append("geo %s, want %s" % (r["geo"], want["geo"]))
            if "M" in what:
                assert r["M"] is not None, fc.describe(case, k, fill) + ": no eroded mask came back (code %d)" % r["rc"]
                bad.append(fc.first_difference("M", r["M"], fc.restate_M(m.c, _geo_dict(r["geo"]), case.grey)))
            if "rhs" in what:
                bad.append(fc.first_difference("lap", r["lap"], want["lap"]))
                bad.append(fc.first_difference("B", r["B"], None if case.storage & 4 else want["B"]))
            bad = [b for b in bad if b]
            if bad:
                raise AssertionError(fc.describe(case, k, fill) + "\n  " + "\n  ".join(bad))
        a, b = res[0x00][k], res[0xFF][k]
        for name in ("rect_dev", "rect_host", "rc", "geo", "M", "B", "lap"):
            same = a[name] == b[name] if not isinstance(a[name], np.ndarray) else np.array_equal(a[name], b[name])
            assert same, fc.describe(case, k) + ": %s depends on what lies in the guard bands and the row padding" % name


# ---- the scan ----------------------------------------------------------------------------------------------------------------------------
def test_scan_solo(fe):
    """k_mask_bbox at every a0 for each extreme pixel, one and two workgroup columns, the trimmed dwords at both row ends against
    non-zero border bytes; the empty interior, the single pixel (SC_ERR_EMPTY_MASK, the rectangle still exact), the all-255 mask."""
    for case in fc.scan_cases():
        check(fe, case, ("rect",))


def test_scan_riding(fe):
    """k_preprocess<.., BB>: the scan as extra workgroup rows, tile grids 1, 2, 3 wide against scans of 1, 2, 5 workgroups, on a right
    guess and on a wrong one: the rectangle is the true one, geo the guessed box's."""
    for case in fc.riding_cases():
        check(fe, case, ("rect",))


def test_scan_group(fe):
    """k_mask_bbox_group + k_mask_bbox_fold_group: three masks of one size; seventeen of differing sizes (two launches, the parts advance,
    workgroups beyond a member's own grid leave neutral parts)."""
    for case in fc.group_scan_cases():
        check(fe, case, ("rect",))


# ---- the erodes --------------------------------------------------------------------------------------------------------------------------
def test_erode_solo(fe):
    """k_mask_erode3 at every (address mod 4, step mod 4), holes across every word, wave and strip seam and at ring distances 2, 3, 4."""
    for case in fc.erode_cases()["solo"]:
        check(fe, case, ("M",))


def test_erode_in_tile(fe):
    """preprocess_block<.., ER = true>: the tiles of a launch on a predicted box erode the mask themselves; 255 beside the box."""
    for case in fc.erode_cases()["tile"]:
        check(fe, case, ("M",))


def test_erode_group(fe):
    """k_mask_erode3_group<16>: same-size members at different placements, size classes of three sizes."""
    for case in fc.erode_cases()["group"]:
        check(fe, case, ("M",))


def test_erode_grey(fe):
    """k_mask_erode_min7 (SC_FLAG_OPENCV_GREY_MASK): grey values across its 64 x 16 tiles' seams."""
    for case in fc.erode_cases()["grey"]:
        check(fe, case, ("M",))


# ---- the pre-process ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", [0, 1, 3])
@pytest.mark.parametrize("mode", [fc.NORMAL, fc.MIXED, fc.MONO])
def test_preprocess_solo(fe, mode, storage):
    """k_preprocess<HF, HU, .., MODE>: every staged-row origin mod 16 of patch and destination, the ROI against each destination edge."""
    for case in fc.pre_solo_cases(mode, storage):
        check(fe, case, ("rhs",))


def test_preprocess_solo_predicted(fe):
    """k_preprocess<.., BB = true>: the same tiles behind riding scan rows, taking the eroded mask from LDS, in every mode and storage."""
    combos = [(m, s) for m in (fc.NORMAL, fc.MIXED, fc.MONO) for s in (0, 1, 3)]
    for i, c in enumerate(fc.pre_solo_cases()):
        m, = c.members
        mode, storage = combos[i % len(combos)]
        check(fe, fc.Case("pre", 1, [fc.Member(m.c, m.pm, m.pf, m.pb, fc.true_rect(m.c))], mode, storage), ("rhs",))


def test_preprocess_solo_grey(fe):
    """k_preprocess<false, false, GREY>: OpenCV's fractional blend on a grey eroded mask, equal to the C restatement."""
    for case in fc.erode_cases()["grey"]:
        check(fe, case, ("rhs",))
    for case in fc.pre_solo_cases(grey=True)[::3]:          # ... and bit-identical to the select on 0 / 255 masks
        check(fe, case, ("rhs",))


def test_preprocess_group(fe):
    """k_preprocess_group in its NORMAL, MIXED and MONOCHROME instantiations, float / float16 / no U0 stored."""
    for case in fc.pre_group_cases():
        check(fe, case, ("rhs",))


def test_preprocess_size_class(fe):
    """k_preprocess_group with j.W > 0: members of three sizes inside fields laid out for the largest."""
    for case in fc.pre_class_cases():
        check(fe, case, ("rhs",))


def test_hook_refuses_what_no_launcher_instantiates(fe):
    case = fc.pre_solo_cases()[20]
    fe.configure(fc.NORMAL, False)
    _, _, jobs = fe.place(case, 0)
    for form, storage in ((0, 2), (0, 7), (1, 7), (0, 5), (2, 2), (4, 0)):
        with pytest.raises(fe.capi.SeamlessCloneError):
            fe.inst.front_end_device(jobs, form, storage, [fc.true_rect(case.members[0].c)])


# ---- the production calls hand the pointers through as the hook does ------------------------------------------------------------------------
def _placed_members(sizes, odd):
    from oracle import oracle_np
    ms = []
    for k, (W, H) in enumerate(sizes):
        dst, patch, mask, cx, cy = oracle_np.synth_inputs(W, H, seed_dst=31 + k, seed_patch=57 + k, margin=24)
        c = fc.Content("clone %dx%d #%d" % (W, H, k), mask, patch, dst, cx, cy)
        pl = [fc.Place(5 + 4 * k, 3), fc.Place(7 + k, 1 + k), fc.Place(3 + 2 * k, 2)] if odd else [fc.Place(0, 0)] * 3
        ms.append(fc.Member(c, *pl))
    return ms


def _destinations(fe, case, call):
    fe_buf, plan, jobs = fe.place(case, 0xFF)
    call(jobs)
    fe.inst.sync()
    after = fe.inst.from_device(fe.base(fe_buf.size), (fe_buf.size,))
    outs = [fc.views(after, m, offs)[2].copy() for m, offs in zip(case.members, plan)]
    for m, offs, out in zip(case.members, plan, outs):          # nothing but the destinations' pixels changed
        v = fc.views(after, m, offs)[2]
        v[...] = m.c.dst
    assert np.array_equal(after, fe_buf)
    return outs


@pytest.mark.parametrize("method", ["default", "fft"])
def test_run_device_reads_mask_and_patch_where_they_lie(fe, method):
    """sc_hip_run_device on a 130 x 70 ROI: mask, patch and destination at odd bases and steps give the bytes of the same content
    placed dense and aligned."""
    capi = fe.capi
    outs = {}
    for odd in (False, True):
        case = fc.Case("run_device", 0, _placed_members([(130, 70)], odd))
        fe.state = None
        fe.configure(fc.NORMAL, False, capi.SC_METHOD_FFT if method == "fft" else capi.SC_METHOD_AUTO)

        def call(jobs):
            j = jobs[0]
            rc = fe.inst.L.sc_hip_run_device(fe.inst.h, j.face, j.face_cols, j.face_rows, j.face_step, j.body, j.body_cols, j.body_rows, j.body_step,
                                             j.mask, j.mask_cols, j.mask_rows, j.mask_step, j.centerX, j.centerY, True)
            fe.inst._check(rc)
        outs[odd], = _destinations(fe, case, call)
        info = fe.inst.info()
        assert (info.W, info.H) == (130, 70)
    m = case.members[0]
    assert np.array_equal(outs[False], outs[True]) and (outs[True] != m.c.dst).mean() > 0.2
    fe.state = None


def test_run_device_batch_reads_mask_and_patch_where_they_lie(fe):
    """sc_hip_run_device_batch, three members of 300 x 194 as one group: the same, member by member."""
    outs = {}
    for odd in (False, True):
        case = fc.Case("run_device_batch", 2, _placed_members([(300, 194)] * 3, odd))
        fe.state = None
        fe.configure(fc.NORMAL, False)

        def call(jobs):
            fe.inst.run_device_batch(jobs)
            assert all(j.rc == 0 for j in jobs)
        outs[odd] = _destinations(fe, case, call)
        assert fe.inst.info().group_members == 3
    for a, b, m in zip(outs[False], outs[True], case.members):
        assert np.array_equal(a, b) and (a != m.c.dst).mean() > 0.2
    fe.state = None
