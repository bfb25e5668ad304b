"""sc_batch_job.body_restore against the caller's own full copy: a group restores only the FRAME of a destination whose ROI interior its
clone writes and reads the ROI from the restore source (csrc/sc_batch.cpp), so every case here runs twice -- with body_restore set, and
with body_restore = NULL after a full copy_d2d of the same source -- into allocations pre-filled with 0xA5 (a byte nobody restored
shows), and the two must agree over the WHOLE allocation, guard bands in front of and behind the image included.

Shapes: the smallest at which the first level-0 launch's tiling (232 x 52 exact, 8-row bands, 4 pixels per lane) and the frame copy
(16-byte chunks, runs between interior rows) can go wrong.  A handful of cases' SHA-256 are compared with
tests/golden/roi_in_place_digests.json, which this same file recorded on the commit BEFORE the frame-only restore
(SC_RECORD_ROI_DIGESTS=<file> writes them to that file instead of comparing)."""
import hashlib
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 256          # bytes of 0xA5 in front of and behind every destination (a multiple of 16: the image keeps its alignment)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "roi_in_place_digests.json")
RECORD_TO = os.environ.get("SC_RECORD_ROI_DIGESTS")


def digest_is_the_recorded_one(name, arrays):
    h = hashlib.sha256()
    for g in arrays:
        h.update(g.tobytes())
    if RECORD_TO:
        d = json.load(open(RECORD_TO)) if os.path.exists(RECORD_TO) else {}
        d[name] = h.hexdigest()
        json.dump(d, open(RECORD_TO, "w"), indent=1, sort_keys=True)
        return
    assert json.load(open(GOLDEN))[name] == h.hexdigest(), "%s: not the bytes of the commit before the frame-only restore" % name


def ring_ramp(W, H, period=32, band=2, seed=5):
    """patch and mask of tests/test_gpu_round4.py's ring_ramp_inputs: rings of inward ramps, whose solution leaves the 16-bit field's range"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H + 2, 0:W + 2]
    ph = (np.hypot(yy - (H + 1) / 2.0, xx - (W + 1) / 2.0) / period) % 1.0
    patch = np.clip(255.0 * (1.0 - ph)[:, :, None] + rng.normal(0.0, 3.0, (H + 2, W + 2, 3)), 0, 255).astype(np.uint8)
    return patch, np.where((ph * period < band) | (ph * period > period - band), 0, 255).astype(np.uint8)


@pytest.fixture(scope="module")
def inst():
    from seamlesscloneoptimization_amd import capi
    i = capi.Instance(0)
    i.set_solver(method=capi.SC_METHOD_MULTIGRID)
    yield i
    i.destroy()


def fresh_instance(**solver):
    from seamlesscloneoptimization_amd import capi
    i = capi.Instance(0)
    i.set_solver(method=capi.SC_METHOD_MULTIGRID, **solver)
    return i


def member(W, H, seed, a=0, pad=0, margin=32, mask=None, patch=None):
    """One clone of a W x H ROI at ltx = 16 + a, lty = 16 of a (H + margin) x (W + margin) destination whose rows are 3 cols + pad bytes
    apart (the padding holds random bytes too: it is part of what a restore copies)."""
    rng = np.random.default_rng([seed, W, H])
    rows, cols = H + margin, W + margin
    step = 3 * cols + pad
    yy, xx = np.mgrid[0:rows, 0:cols]
    img = np.clip((128.0 + 60.0 * np.sin(2 * np.pi * xx / cols) * np.cos(2 * np.pi * yy / rows))[:, :, None] + rng.normal(0.0, 12.0, (rows, cols, 3)), 0, 255).astype(np.uint8)
    dst = rng.integers(0, 256, (rows, step), dtype=np.uint8)
    dst[:, :3 * cols] = img.reshape(rows, 3 * cols)
    if patch is None:
        yy, xx = np.mgrid[0:H + 2, 0:W + 2]
        patch = np.clip((110.0 + 50.0 * np.cos(3 * np.pi * xx / W))[:, :, None] + rng.normal(0.0, 20.0, (H + 2, W + 2, 3)), 0, 255).astype(np.uint8)
    if mask is None:
        mask = np.full((H + 2, W + 2), 255, np.uint8)
    return dict(dst=dst, cols=cols, patch=patch, mask=mask, cx=16 + a + W // 2, cy=16 + H // 2, off=0, share=None)


def run_batch(inst, members, restore):
    """The members through ONE sc_hip_run_device_batch.  restore: body_restore is set; else the caller copies the source over the
    destination itself first.  Returns (codes, sc_run_info, the destinations' whole allocations)."""
    from seamlesscloneoptimization_amd import capi
    jobs = capi.Pool.make_jobs(len(members))
    held, boxes = [], []
    for k, (j, m) in enumerate(zip(jobs, members)):
        dst = m["dst"]
        f, s, k_mask = inst.to_device(m["patch"]), inst.to_device(dst), inst.to_device(m["mask"])
        held += [f, s, k_mask]
        if m["share"] is None:
            n = GUARD + m["off"] + dst.nbytes + GUARD
            base = inst.to_device(np.full(n, 0xA5, np.uint8))
            boxes.append((base, n, base + GUARD + m["off"]))
        else:
            boxes.append((None, 0, boxes[m["share"]][2]))
        body = boxes[k][2]
        if not restore and m["share"] is None:
            inst.copy_d2d_async(body, s, dst.nbytes)
        j.face, j.face_cols, j.face_rows, j.face_step = f, m["patch"].shape[1], m["patch"].shape[0], 3 * m["patch"].shape[1]
        j.body, j.body_cols, j.body_rows, j.body_step = body, m["cols"], dst.shape[0], dst.shape[1]
        j.mask, j.mask_cols, j.mask_rows, j.mask_step = k_mask, m["mask"].shape[1], m["mask"].shape[0], m["mask"].shape[1]
        j.centerX, j.centerY, j.body_restore = m["cx"], m["cy"], (s if restore else None)
    try:
        inst.run_device_batch(jobs)
        info = inst.info()
        out = [inst.from_device(base, (n,)) for base, n, _ in boxes if base is not None]
    finally:
        inst.sync()
        for p in held + [b[0] for b in boxes if b[0] is not None]:
            inst.free(p)
    return [j.rc for j in jobs], info, out


def both_ways(inst, members, name=None, inst_plain=None):
    """with body_restore, and with the caller's own copy: the same codes, the same bytes everywhere.  Returns the restore run's info."""
    rc, info, got = run_batch(inst, members, True)
    rc0, info0, want = run_batch(inst_plain or inst, members, False)
    assert rc == rc0 and (info.sweeps, info.field_retry, info.group_members, info.group_ragged) == (info0.sweeps, info0.field_retry, info0.group_members, info0.group_ragged)
    for k, (g, w) in enumerate(zip(got, want)):
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, "%s: destination %d differs at %d bytes, first at allocation byte %d" % (name, k, bad.size, bad[0])
        assert (g[:GUARD] == 0xA5).all() and (g[-GUARD:] == 0xA5).all(), "a guard band was written"
    first = members[0]["dst"].reshape(-1)
    assert not np.array_equal(got[0][GUARD + members[0]["off"]:][:first.size], first), "the clone wrote nothing"
    if name:
        digest_is_the_recorded_one(name, got)
    return info


SWEEP = [(237, 60), (300, 194), (466, 110), (301, 194), (302, 194), (303, 194)]


@pytest.mark.parametrize("W,H", SWEEP)
def test_tiling_sweep_groups_of_three(inst, W, H):
    """groups of three same-size members at every 3 ltx mod 4 and at steps 3 cols + {0, 1, 2, 3}"""
    for a in range(4):
        for pad in range(4):
            members = [member(W, H, 10 * k + a + 4 * pad, a=a, pad=pad) for k in range(3)]
            info = both_ways(inst, members, "sweep %dx%d a=%d pad=%d" % (W, H, a, pad) if (a, pad) in ((0, 0), (3, 1)) and W in (237, 300) else None)
            assert info.group_members == 3 and info.group_ragged == 0


def test_one_size_class(inst):
    members = [member(300, 194, 1), member(280, 180, 2, a=1, pad=1), member(320, 200, 3, a=2, pad=3)]
    info = both_ways(inst, members, "size class")
    assert info.group_members == 3 and info.group_ragged == 1


def test_a_wrong_guess_comes_back_restored_and_cloned_alone():
    """one member's mask has an empty inner border column: the device's box is not the predicted one, the group's output launch skips
    the member, and it is repeated alone -- on a destination whose interior rows the group never restored"""
    mask = np.full((196, 302), 255, np.uint8)
    mask[:, 1] = 0
    members = [member(300, 194, 1), member(300, 194, 2, a=1, mask=mask), member(300, 194, 3, a=2, pad=2)]
    a, b = fresh_instance(), fresh_instance()
    try:
        info = both_ways(a, members, "wrong guess", inst_plain=b)
        assert info.group_members == 3
    finally:
        a.destroy(); b.destroy()


def test_a_saturating_member_repeats_the_group_on_float_fields(inst):
    W, H = 640, 560
    patch, mask = ring_ramp(W, H)
    members = [member(W, H, 1), member(W, H, 2, a=1, pad=1, patch=patch, mask=mask), member(W, H, 3, a=3)]
    info = both_ways(inst, members, "saturating member")
    assert info.field_retry == 1 and info.group_members == 3


def test_max_sweeps_1():
    a = fresh_instance(max_sweeps=1)
    try:
        info = both_ways(a, [member(300, 194, k, a=k, pad=k) for k in range(3)], "max_sweeps 1")
        assert info.sweeps == 1 and info.group_members == 3
    finally:
        a.destroy()


def test_two_jobs_sharing_one_body(inst):
    """two disjoint ROIs of one destination (and one source) and a member of its own: the shared destination is restored whole"""
    W, H = 300, 194
    wide = member(W, H, 1, margin=32 + W + 8)
    second = dict(wide, cx=wide["cx"] + W + 8, share=0, patch=member(W, H, 5)["patch"])
    info = both_ways(inst, [wide, second, member(W, H, 2, a=1)], "shared body")
    assert info.group_members == 3


@pytest.mark.parametrize("off", [1, 4, 8])
def test_a_misaligned_body(inst, off):
    members = [member(300, 194, 1), dict(member(300, 194, 2, a=1, pad=1), off=off), member(300, 194, 3, a=2)]
    assert both_ways(inst, members).group_members == 3


def test_n_1_and_a_single_run_device_clone_at_the_same_alignments(inst):
    """a call of one member runs it alone after a full restore; sc_hip_run_device behind the caller's own copy gives the same bytes"""
    for a in range(4):
        for pad in range(4):
            m = member(300, 194, a + 4 * pad, a=a, pad=pad)
            both_ways(inst, [m], "n=1 a=%d pad=%d" % (a, pad) if (a, pad) == (1, 3) else None)
            _, _, (got,) = run_batch(inst, [m], True)
            dst = m["dst"]
            f, s, k_mask = inst.to_device(m["patch"]), inst.to_device(dst), inst.to_device(m["mask"])
            base = inst.to_device(np.full(2 * GUARD + dst.nbytes, 0xA5, np.uint8))
            try:
                inst.copy_d2d_async(base + GUARD, s, dst.nbytes)
                rc = inst.L.sc_hip_run_device(inst.h, f, m["patch"].shape[1], m["patch"].shape[0], 3 * m["patch"].shape[1], base + GUARD, m["cols"], dst.shape[0], dst.shape[1],
                                              k_mask, m["mask"].shape[1], m["mask"].shape[0], m["mask"].shape[1], m["cx"], m["cy"], True)
                assert rc == 0
                single = inst.from_device(base, (2 * GUARD + dst.nbytes,))
            finally:
                for p in (f, s, k_mask, base):
                    inst.free(p)
            assert np.array_equal(single, got)


def test_no_speculate():
    from seamlesscloneoptimization_amd import capi
    a = fresh_instance(flags=capi.SC_FLAG_NO_SPECULATE)
    try:
        info = both_ways(a, [member(300, 194, k, a=k, pad=k) for k in range(3)], "no speculate")
        assert info.group_members == 3
    finally:
        a.destroy()
