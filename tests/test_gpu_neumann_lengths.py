"""The Neumann DCT solve (SC_POISSON_NEUMANN: k_mix with both axes of kind 1, k_fft_build kind 1, k_poisson_mean) at every transform length class, on both
sides of every launch-shape cut, through the table cache with both kinds, at its size limits and over what it must never read
(the GPU side of tests/test_neumann_lengths_host.py).

Float32 transforms are held to the float32 restatement on the same input -- measured <= max(FACTOR x solve_f32's, FLOOR) for the
residual ratio RES and the error ERR -- and double transforms to float32 ulps: tests/direct_bounds.py says what the quantities
are and where the constants come from.  The older bounds of tests/test_gpu_neumann.py (3e-2 R, 1e-6 R, the mean) hold as well.
Lines NEULEN / NEULOW / NEUCUT / NEULIM carry the measured values beside the restatement's."""
import numpy as np
import pytest

import direct_np as dn
from direct_bounds import NEUMANN
from test_direct_lengths_host import fft_M
from test_neumann_lengths_host import JOBS_MAX, mean_parts, neumann_classes, tiny

Yardstick = NEUMANN.yardstick

pytestmark = pytest.mark.gpu

from seamlesscloneoptimization_amd import capi  # noqa: E402

from test_gpu_neumann import BOUND, MEAN_BOUND, Dev, _batch, _layout_views  # noqa: E402

PREC = {"f32": 0, "f64": capi.SC_FLAG_FFT_FP64}
OLD = {"f32": BOUND["fft32"], "f64": BOUND["fft64"]}


@pytest.fixture()
def inst():
    i = capi.Instance(0)
    yield i
    i.destroy()


def _configure(inst, prec):
    inst.set_solver(method=capi.SC_METHOD_FFT, flags=(inst.default_opts().flags & ~capi.SC_FLAG_FFT_FP64) | PREC[prec])


def _rough(W, H, C, seed):
    """[(name, gx, gy, boundary)]: the reconstruction of a white-noise image, and a random guidance field with a random boundary"""
    rng = np.random.default_rng(seed)
    img = rng.uniform(-50, 300, (H, W, C)).astype(np.float32)
    fx, fy = dn.forward_differences(img)
    b = rng.uniform(-100, 400, (H, W, C)).astype(np.float32)
    gx = rng.normal(0, 20, (H, W, C)).astype(np.float32)
    gy = rng.normal(0, 20, (H, W, C)).astype(np.float32)
    return [("reconstruction", fx, fy, img), ("random", gx, gy, b)]


def _solve_and_check(inst, gx, gy, b, precs, tag, fails, rough=True, laplacian=True, old=True):
    """One input under each precision: GUIDANCE (and LAPLACIAN fed numpy's divergence: the same bits), RES / ERR against the
    yardstick, the older bounds.  Appends to fails; returns {prec: (err, res)} and the yardstick."""
    lap = dn.divergence(gx, gy)
    mean = dn.mean_of(b) if b is not None else None
    y = Yardstick("lrtb", "", 0.0, None, lap, b)
    got = {}
    for prec in precs:
        _configure(inst, prec)
        out = inst.poisson(b, gx=gx, gy=gy, neumann=True)
        i = inst.info()
        if not (i.method == capi.SC_METHOD_FFT and i.converged == 1 and (i.W, i.H) == (gx.shape[1], gx.shape[0])):
            fails.append((tag, prec, "info", i.method, i.W, i.H))
        if laplacian and not np.array_equal(inst.poisson(b, lap=lap, neumann=True), out):
            fails.append((tag, prec, "LAPLACIAN differs from GUIDANCE"))
        if not np.isfinite(out).all():
            fails.append((tag, prec, "not finite"))
            continue
        bad, err, res = y.check(out, prec == "f64", rough and (prec == "f32" or "reconstruction" in tag))
        fails.extend((tag, prec) + t for t in bad)
        merr = float(np.abs(out.astype(np.float64).mean(axis=(0, 1)) - (mean if mean is not None else 0.0)).max()) / y.R
        if old and not err <= OLD[prec]:
            fails.append((tag, prec, "old ERR bound", err, OLD[prec]))
        if not merr <= MEAN_BOUND:
            fails.append((tag, prec, "mean", merr, MEAN_BOUND))
        got[prec] = (err, res)
    return got, y


def _fmt(got, y):
    s = "f32 RES %.2e (x%.1f) ERR %.2e (x%.1f) / solve_f32 %.2e %.2e" % (
        got["f32"][1], got["f32"][1] / max(y.res32, 1e-300), got["f32"][0], got["f32"][0] / max(y.err32, 1e-300), y.res32, y.err32) if "f32" in got else "f32 -"
    if "f64" in got:
        s += " | f64 RES %.2e ERR %.2f ulp" % (got["f64"][1], got["f64"][0] * y.R / float(np.spacing(np.float32(y.R))))
    return s


# ---------------------------------------------------------------------------------------------------- every length class
def test_every_length_class_at_both_ends(inst):
    """Every class of the DCT kind (float: all, M <= 16384; double: M <= 8192) at n_lo and n_hi -- n_hi is the tight end, M = 2n or
    2n - 1 -- along x (n x 9) and along y (9 x n), C = 3, a rough reconstruction and a random guidance field, both forms."""
    cls64 = {c[0] for c in neumann_classes(True)}
    fails = []
    print("\nNEULEN M r n axis input | f32 RES (x restatement) ERR (x restatement) / solve_f32 RES ERR | f64 RES, ERR in ulps")
    for M, r, lo, hi in neumann_classes(False):
        for n in sorted({lo, hi}):
            for axis in "xy":
                W, H = (n, 9) if axis == "x" else (9, n)
                assert fft_M(n) == M and tiny(W, H, False)
                precs = ("f32", "f64") if M in cls64 else ("f32",)
                for what, gx, gy, b in _rough(W, H, 3, seed=1000 * n + (axis == "y")):
                    got, y = _solve_and_check(inst, gx, gy, b, precs, (M, n, axis, what), fails)
                    print("NEULEN M=%5d r=%d n=%4d %s %-14s | %s" % (M, r, n, axis, what, _fmt(got, y)))
    assert not fails, fails


# ------------------------------------------------------------------------------------------------------------- low modes
def _low_mode_sizes():
    tops = [c[3] for c in neumann_classes(False)[-6:]]
    return [(n, 9) for n in tops] + [(9, n) for n in tops] + [(8192, 64), (2050, 1030)]


def test_low_modes_on_smooth_images(inst):
    """smooth_image's reconstruction (modes k, l <= 4, where the restatement's own ERR is 1000 times below its ERR on a rough image:
    tests/test_neumann_lengths_host.py) at the tight end of the six largest float classes, at 8192 x 64 and at 2050 x 1030: a wrong
    low coefficient -- X'_0, the first twiddles, the lowest denominators -- is an error of the size of the image here."""
    fails = []
    print("\nNEULOW W x H | f32 ERR (x restatement) ...")
    for W, H in _low_mode_sizes():
        C = 3 if W * H < 1 << 20 else 2
        sm = dn.smooth_image(H, W, C, seed=W + 3 * H)
        fx, fy = dn.forward_differences(sm)
        precs = ("f32", "f64") if max(W, H) <= 4096 else ("f32",)
        got, y = _solve_and_check(inst, fx, fy, sm, precs, (W, H, "smooth"), fails, rough=False)
        print("NEULOW %4dx%-4d C=%d | %s" % (W, H, C, _fmt(got, y)))
    assert not fails, fails


# ------------------------------------------------------------------------------------------- the tiny / transposed cut
CUT_CASES = [(1024, 1024, "f32"), (1025, 1024, "f32"), (1024, 1025, "f32"), (1024, 512, "f64"), (1024, 513, "f64"), (513, 1024, "f64"),
             (3000, 400, "f32"), (400, 3000, "f32"), (3000, 400, "f64"), (400, 3000, "f64")]


@pytest.mark.parametrize("W,H,prec", CUT_CASES)
def test_both_sides_of_the_transposed_store_cut(inst, W, H, prec):
    """plane x sizeof(T) <= 4 MiB: stored transposed by the transform launches; above: two k_fft_transpose launches with planes = C."""
    is_tiny = tiny(W, H, prec == "f64")
    assert is_tiny == ((W, H, prec) in ((1024, 1024, "f32"), (1024, 512, "f64")))
    fails = []
    for C in (1, 4):
        what, gx, gy, b = _rough(W, H, C, seed=W * 7 + H * 13 + C)[0]
        got, y = _solve_and_check(inst, gx, gy, b, (prec,), (W, H, C, what), fails, laplacian=(C == 1))
        print("NEUCUT %4dx%-4d C=%d %s | %s" % (W, H, C, "tiny" if is_tiny else "transposed", _fmt(got, y)))
    assert not fails, fails


def _members(m, H, W, C, seed, offset=0.0, none_at=lambda k: False):
    rng = np.random.default_rng(seed)
    ps = []
    for k in range(m):
        b = ((offset + k + rng.uniform(-1, 1, (H, W, C))) if offset else rng.uniform(-50, 300, (H, W, C))).astype(np.float32)
        ps.append((None if none_at(k) else b, rng.normal(0, 15, (H, W, C)).astype(np.float32), rng.normal(0, 15, (H, W, C)).astype(np.float32)))
    return ps


def _batch_against_solo(inst, ps, prec):
    """One sc_hip_poisson_device call over ps: every member's bits are its solo run's, nothing outside the outputs' spans changed.
    Returns (outputs, info)."""
    H, W, C = ps[0][1].shape
    _configure(inst, prec)
    rc, outs, jobs, info, dev, full, ids = _batch(inst, ps)
    try:
        assert rc == capi.SC_OK and all(j.rc == capi.SC_OK for j in jobs)
        written = np.zeros(full.size, bool)
        for (_, _, _, ko) in ids:
            off = dev.parts[ko][0] // 4
            written[off:off + H * W * C] = True
        assert np.array_equal(full[~written], dev.host[~written]), "something outside the outputs' spans changed"
    finally:
        dev.free()
    for k, (b, gx, gy) in enumerate(ps):
        solo = inst.poisson(b, gx=gx, gy=gy, neumann=True)
        assert np.array_equal(outs[k], solo), (k, len(ps), float(np.abs(outs[k] - solo).max()))
    return outs, info


@pytest.mark.parametrize("m,W,H,C,prec", [(2, 1100, 1000, 2, "f32"), (17, 1100, 1000, 1, "f32"), (2, 1000, 530, 2, "f64"),
                                          (17, 1000, 530, 1, "f64")])
def test_batches_above_the_cut_equal_their_solo_runs(inst, m, W, H, C, prec):
    """planes = C m > C through the two transposes; 17 members: a second chunk of one member.  Work planes 2 x 4 (8) bytes x W H C m
    <= 150 MB."""
    assert not tiny(W, H, prec == "f64") and 2 * (8 if prec == "f64" else 4) * W * H * C * m < 1 << 30
    ps = _members(m, H, W, C, seed=m + W, none_at=lambda k: k % 3 == 1)
    outs, info = _batch_against_solo(inst, ps, prec)
    assert info.method == capi.SC_METHOD_FFT and info.group_members == m
    b, gx, gy = ps[m - 1]                                   # the last member (the second chunk's at 17) against the yardstick
    y = Yardstick("lrtb", "", 0.0, None, dn.divergence(gx, gy), b)
    bad, err, res = y.check(outs[m - 1], prec == "f64", prec == "f32")          # (random guidance: no RES bound in double)
    assert not bad, (bad, err, res)


# --------------------------------------------------------------------------------------------------- chunks and mean parts
@pytest.mark.parametrize("C", [1, 4])
@pytest.mark.parametrize("H", [255, 256, 257, 513])
def test_chunks_of_16_members_and_the_mean_parts(inst, H, C):
    """Batches of 16 .. 49 members (one to four launches of PoissonJobs::MAX members, the offset parts + p0 np into the partial sums)
    at H on both sides of the cap of 256 parts (257: one part of two rows; 513: two or three rows per part); boundaries 1e4 + k + [-1, 1],
    every third member without boundary, the first member of the second chunk among them."""
    W = 12
    assert mean_parts(H) == min(H, 256)
    for m in (16, 17, 32, 33, 49):
        none_at = lambda k: k % 3 == 1          # noqa: E731
        assert none_at(JOBS_MAX)
        ps = _members(m, H, W, C, seed=H + m, offset=1e4, none_at=none_at)
        for prec in (("f32", "f64") if m == 17 else ("f32",)):
            outs, info = _batch_against_solo(inst, ps, prec)
            per = capi.SC_POISSON_MAX_PLANES // C
            last = m - per * ((m - 1) // per)
            assert info.group_members == (last if last > 1 else 0), (m, C, info.group_members)
            if C == 4 and m == 49:
                assert per == 48 and last == 1              # the call crossed SC_POISSON_MAX_PLANES: a chunk of 48 and one of 1
            for k, (b, gx, gy) in enumerate(ps):
                mean = np.zeros(C) if b is None else dn.mean_of(b)
                want = dn.solve_free(dn.divergence(gx, gy), b)
                R = float(np.abs(want).max())
                got = outs[k].astype(np.float64)
                assert np.abs(got.mean(axis=(0, 1)) - mean).max() <= MEAN_BOUND * R, (m, k, prec, b is None)
                assert np.abs(got - want).max() <= OLD[prec] * R, (m, k, prec)


# ------------------------------------------------------------------------------------------- the cache with two kinds
class _Lru:
    """FftState::dims as fft_build_dim keeps it: 8 entries keyed (n, double, kind), one tick counter, the first least recently used
    entry other than `keep` is the victim, a buffer grows and never shrinks."""

    def __init__(self):
        self.tick = 0
        self.slots = [dict(key=None, used=0, cap=0, hist=[], evictions=0) for _ in range(8)]
        self.kept_with_full_cache = 0

    def _dim(self, n, dbl, kind, keep=None):
        victim = None
        for d in self.slots:
            if d["key"] == (n, dbl, kind):
                self.tick += 1
                d["used"] = self.tick
                return d, True
            if d is not keep and (victim is None or d["used"] < victim["used"]):
                victim = d
        if victim["key"] is not None:
            victim["evictions"] += 1
        M = fft_M(n)
        need = (16 if dbl else 8) * (4 * M + 1 + (n + 1 if kind else 0))
        victim["hist"].append((n, dbl, kind, M, need > victim["cap"]))
        victim["cap"] = max(victim["cap"], need)
        self.tick += 1
        victim.update(key=(n, dbl, kind), used=self.tick)
        return victim, False

    def solve(self, a, b, dbl, kind):
        full = all(d["key"] is not None for d in self.slots)
        da, hit_a = self._dim(a, dbl, kind)
        db, hit_b = self._dim(b, dbl, kind, da)
        assert da["key"] == (a, dbl, kind)                  # the first direction's entry survived the second's build
        if full and hit_a and not hit_b:
            self.kept_with_full_cache += 1


def _dirichlet(i, n_w, n_h, prec, seed):
    """SC_METHOD_FFT field solve with n_w x n_h unknowns (a Dirichlet ring around them)"""
    rng = np.random.default_rng(seed)
    B = rng.integers(0, 256, (2, n_h + 2, n_w + 2)).astype(np.float32)
    lap = np.zeros_like(B)
    lap[:, 1:-1, 1:-1] = rng.integers(-600, 601, (2, n_h, n_w)).astype(np.float32)
    _configure(i, prec)
    i.field_load(B, lap)
    i.field_solve()
    return i.field_store()


def _neumann(i, W, H, prec, seed):
    rng = np.random.default_rng(seed)
    g = rng.normal(0, 10, (2, H, W, 2)).astype(np.float32)
    b = rng.uniform(-50, 300, (H, W, 2)).astype(np.float32)
    _configure(i, prec)
    return i.poisson(b, gx=g[0], gy=g[1], neumann=True)


def _run_sequence(seq):
    """Every step on one instance and on a fresh one: the same bits."""
    used = capi.Instance(0)
    try:
        for k, (kind, a, b, prec) in enumerate(seq):
            fn = _neumann if kind else _dirichlet
            got = fn(used, a, b, prec, seed=900 + k)
            fresh = capi.Instance(0)
            try:
                want = fn(fresh, a, b, prec, seed=900 + k)
            finally:
                fresh.destroy()
            assert np.isfinite(got).all() and np.array_equal(got, want), (k, kind, a, b, prec, float(np.abs(got - want).max()))
    finally:
        used.destroy()


def _model(seq):
    lru = _Lru()
    for kind, a, b, prec in seq:
        lru.solve(a, b, prec == "f64", kind)
    return lru


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("n", [640, 512, 96, 1280])
def test_cache_dirichlet_then_neumann_of_the_same_length(prec, n):
    """(a) n unknowns under Dirichlet, n pixels under Neumann, Dirichlet again, Neumann again: both kinds take M = fft_len(n), n the
    tight end of its class (M = 2n), two entries of one (n, precision)."""
    assert fft_M(n) == 2 * n
    _run_sequence([(0, n, 9, prec), (1, n, 9, prec), (0, n, 9, prec), (1, n, 9, prec), (1, 9, n, prec), (0, 9, n, prec)])


EVICT_SEQUENCE = [(1, 300, 200, "f32"), (1, 100, 100, "f32"), (1, 40, 7, "f64"), (1, 640, 9, "f32"), (1, 9, 512, "f64"), (1, 130, 31, "f32"),
                  (1, 33, 17, "f32"), (1, 50, 60, "f64"), (1, 70, 80, "f32"), (1, 21, 9, "f32"), (1, 21, 45, "f32"), (1, 300, 200, "f32"),
                  (1, 100, 100, "f64"), (1, 45, 21, "f32"), (1, 640, 640, "f32"), (1, 300, 200, "f32")]


def test_cache_neumann_sequence_evicts_every_entry():
    """(b) more than 8 distinct (length, precision) pairs: every entry is evicted, evicted sizes come back, W == H, and a solve whose
    first direction is cached and whose second is new while the cache is full (the first must survive: `keep`)."""
    lru = _model(EVICT_SEQUENCE)
    assert all(d["evictions"] >= 1 for d in lru.slots) and lru.kept_with_full_cache >= 1
    assert any(a == b for _, a, b, _ in EVICT_SEQUENCE) and EVICT_SEQUENCE[-1] == EVICT_SEQUENCE[0]
    _run_sequence(EVICT_SEQUENCE)


GROW_SEQUENCE = [(0, 640, 640, "f32")] + [(1, n, n, "f32") for n in (20, 24, 28, 36, 44, 52, 60)] + \
                [(1, 640, 640, "f32"),                       # the DCT tables of n = 640 into the entry that held the DST's: n + 1 elements more, same M
                 (1, 4096, 24, "f32"),                      # M = 64 -> 8192 in one entry
                 (0, 640, 640, "f32")] + [(1, n, n, "f32") for n in (68, 76, 84, 92, 100)] + \
                [(1, 30, 30, "f32"),                        # M = 64 in the entry that holds 8192's buffer
                 (1, 4096, 30, "f32"), (1, 24, 4096, "f32")]


def test_cache_entry_grows_shrinks_and_changes_kind():
    """(c) one entry from a short M to a long one and back, and an entry that held the DST tables of n reused for the DCT tables of the
    same n and M, which need n + 1 more elements: the model says which entry each step lands in."""
    lru = _model(GROW_SEQUENCE)
    hists = [d["hist"] for d in lru.slots]
    assert any((a[0], a[1], a[3]) == (b[0], b[1], b[3]) and a[2] == 0 and b[2] == 1 and b[4] for h in hists for a, b in zip(h, h[1:])), hists
    assert any(a[3] <= 128 and b[3] == 8192 and c[3] <= 128 and b[4] and not c[4] for h in hists for a, b, c in zip(h, h[1:], h[2:])), hists
    _run_sequence(GROW_SEQUENCE)


# ------------------------------------------------------------------------------------------------- limits and refusals
def test_limits_and_the_instance_after_a_refusal(inst):
    """One pixel past the top of either precision: SC_ERR_BAD_SIZE and an untouched output; the same instance then solves the top
    size within the class walk's bounds.  2 x 2, 2 x 8192 and 8192 x 2 are solved, to RES and ERR relative to the restatement -- a
    finding: the float32 reconstruction at 8192 x 2 reaches 3.6e-2 R (26 x the restatement's 1.4e-3; RES 9.3e-7, 3 x), above the 3e-2 R
    that holds from 8192 x 8 (2.1e-2) up: two rows damp the long side's lowest modes even less than the 64 of DESIGN.md section 4's
    finding; the older bound is not applied to the two strips of 2 x 8192."""
    fails = []
    for prec, top in (("f32", 8192), ("f64", 4096)):
        for W, H in ((top + 1, 8), (8, top + 1)):
            _configure(inst, prec)
            g = np.random.default_rng(W).normal(0, 10, (H, W, 1)).astype(np.float32)
            out = np.full_like(g, -7.25)
            for kw in (dict(gx=g, gy=g), dict(lap=g)):
                with pytest.raises(capi.SeamlessCloneError) as e:
                    inst.poisson(None, out=out, neumann=True, **kw)
                assert e.value.code == capi.SC_ERR_BAD_SIZE and np.all(out == -7.25), (prec, W, H)
            Wt, Ht = (top, 8) if W > H else (8, top)
            for what, gx, gy, b in _rough(Wt, Ht, 3, seed=Wt + 2 * Ht):
                got, y = _solve_and_check(inst, gx, gy, b, (prec,), (Wt, Ht, what), fails)
                print("NEULIM %4dx%-4d %-14s | %s" % (Wt, Ht, what, _fmt(got, y)))
    for W, H in ((2, 2), (2, 8192), (8192, 2), (2, 4096), (4096, 2)):
        for what, gx, gy, b in _rough(W, H, 3, seed=W + 2 * H):
            got, y = _solve_and_check(inst, gx, gy, b, ("f32", "f64") if max(W, H) <= 4096 else ("f32",), (W, H, what), fails, old=max(W, H) <= 4096)
            print("NEULIM %4dx%-4d %-14s | %s" % (W, H, what, _fmt(got, y)))
    assert not fails, fails


# --------------------------------------------------------------------------------------------------- what is never read
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("kind", ["padded", "rgba"])
def test_padding_and_the_unused_float_are_never_read(inst, kind, prec):
    """NaN in the padding columns / the fourth float of boundary, gx, gy and lap, and in gx's last column and gy's last row: finite
    outputs with the bits of the clean run, the output's own padding untouched."""
    H, W, C = 67, 131, 3
    rng = np.random.default_rng(21)
    b = rng.uniform(-50, 300, (H, W, C)).astype(np.float32)
    gx = rng.normal(0, 10, (H, W, C)).astype(np.float32)
    gy = rng.normal(0, 10, (H, W, C)).astype(np.float32)
    lap = dn.divergence(gx, gy)
    _configure(inst, prec)
    ref = inst.poisson(b, gx=gx, gy=gy, neumann=True)
    assert np.isfinite(ref).all()
    dirty_x, dirty_y = gx.copy(), gy.copy()
    dirty_x[:, -1] = np.nan
    dirty_y[-1] = np.nan
    make = _layout_views(H, W, C, kind, np.nan)
    (vb, bb), (vx, bx), (vy, by), (vl, bl) = make(b), make(dirty_x), make(dirty_y), make(lap)
    for buf in (bb, bx, by, bl):
        assert np.isnan(buf).sum() >= (5 * H * C if kind == "padded" else H * W)
    for kw in (dict(gx=vx, gy=vy), dict(lap=vl)):
        vo, obuf = _layout_views(H, W, C, kind, -7.25)()
        got = inst.poisson(vb, out=vo, neumann=True, **kw)
        assert got is vo and np.isfinite(vo).all() and np.array_equal(np.array(vo), ref), (kind, prec, list(kw))
        named = np.ones(obuf.shape, bool)
        if kind == "padded":
            named[:, W:] = False
        else:
            named[:, :, C:] = False
        assert np.all(obuf[~named] == -7.25)
