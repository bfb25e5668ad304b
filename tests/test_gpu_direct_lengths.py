"""The direct solvers at every transform length, plane layout and parity fold (the GPU side of tests/test_direct_lengths_host.py).

SC_METHOD_FFT at both ends of every length class its precision supports, along each axis, with the float tables and the exact ones;
the size limits and what an instance does after a refusal; both plane layouts (three launches up to 4 MiB per channel, five with two
transposes above); SC_METHOD_AUTO's strips end to end; the transform-table cache through a sequence that evicts every entry; and
SC_METHOD_DST's parity fold across its 128-row tiles.  Field-level references are the C port's direct solve (double transforms); the
float32 bound is relative to the port's own float32 transforms on the same input (DESIGN.md §4 holds the measured table)."""
import numpy as np
import pytest

from test_direct_lengths_host import dst_padded_half, fft_M, fft_max_M, length_classes

pytestmark = pytest.mark.gpu

# Bounds set from one MI355X run of this file: float transforms 1.5e-4 ... 4.4e-4 scaled, 0.8x ... 5.0x the port's float32
# transforms (the ratio peaks where the port's transforms are unusually exact: 3e-5 at n = 1); double transforms at most 2 ulps.
F32_FACTOR, F32_FLOOR = 4.0, 4e-4          # float transforms: scaled error <= max(4 x the port's float32 transforms, 4e-4)
F64_ULPS = 4                                # double transforms: within 4 float32 ulps of max|want|
STRIP_SHARE_DIRECT, STRIP_SHARE_MG = 5e-5, 2.5e-3    # AUTO strips end to end: differing channels (measured <= 2.4e-5 / 1.2e-3)


@pytest.fixture(scope="module")
def oracles():
    from oracle import oracle_np, oracle_c
    oracle_c.build()
    return oracle_np, oracle_c


@pytest.fixture()
def inst():
    from seamlesscloneoptimization_amd import capi
    i = capi.Instance(0)
    yield i
    i.destroy()


def _nt(oc):
    return min(8, oc.max_threads())


def _field(W, H, seed):
    """A W x H field (ring included): random Dirichlet ring / body in [0, 255], integer right-hand side in [-600, 600]."""
    rng = np.random.default_rng(seed)
    B = rng.integers(0, 256, (3, H, W)).astype(np.float32)
    lap = np.zeros((3, H, W), np.float32)
    lap[:, 1:-1, 1:-1] = rng.integers(-600, 601, (3, H - 2, W - 2)).astype(np.float32)
    return B, lap


def _solve(inst, B, lap, method, flags):
    inst.set_solver(method=method, flags=flags)
    inst.field_load(B, lap)
    inst.field_solve()
    got = inst.field_store()
    i = inst.info()
    assert i.method == method and i.converged == 1
    ring_ok = (np.array_equal(got[:, 0, :], B[:, 0, :]) and np.array_equal(got[:, -1, :], B[:, -1, :]) and
               np.array_equal(got[:, :, 0], B[:, :, 0]) and np.array_equal(got[:, :, -1], B[:, :, -1]))
    assert ring_ok, ("the Dirichlet ring changed", B.shape, method, flags)
    return got


def _ulp(x):
    return float(np.spacing(np.float32(x)))


class _Ref:
    """The port's answers for one field: double transforms with either denominator, and its float32 transforms' scaled error."""

    def __init__(self, oc, B, lap):
        self.oc, self.g = oc, oc.fold(B, lap)
        self._want, self._e32 = {}, {}

    def want(self, exact):
        if exact not in self._want:
            self._want[exact] = self.oc.solve_dst(self.g, _nt(self.oc), exact_den=exact)
        return self._want[exact]

    def scale(self, exact):
        return max(1.0, float(np.abs(self.want(exact)).max()) / 500.0)

    def err32(self, exact):
        if exact not in self._e32:
            u32 = self.oc.solve_dst(self.g, _nt(self.oc), exact_den=exact, internals="f32")
            self._e32[exact] = float(np.abs(u32 - self.want(exact)).max()) / self.scale(exact)
        return self._e32[exact]


def _check_fft(inst, ref, B, lap, fp64):
    """SC_METHOD_FFT on one field with both denominators against the port.  Returns [(exact, err, bound, oracle-f32 err)]: the
    scaled error for float transforms, the absolute one in float32 ulps of max|want| for double transforms."""
    from seamlesscloneoptimization_amd import capi
    rows = []
    for exact in (False, True):
        flags = (capi.SC_FLAG_FFT_FP64 if fp64 else 0) | (capi.SC_FLAG_EXACT_TABLES if exact else 0)
        got = _solve(inst, B, lap, capi.SC_METHOD_FFT, flags)
        want = ref.want(exact)
        d = float(np.abs(got[:, 1:-1, 1:-1] - want).max())
        if fp64:
            rows.append((exact, d / _ulp(np.abs(want).max()), F64_ULPS, ref.err32(exact)))
        else:
            e32 = ref.err32(exact)
            rows.append((exact, d / ref.scale(exact), max(F32_FACTOR * e32, F32_FLOOR), e32))
    return rows


# ---------------------------------------------------------------------------------------------------- every length class
def test_fft_every_length_class_at_both_ends(inst, oracles):
    """Every transform length class (float M <= 16384, double M <= 8192) at n_lo and n_hi -- n_hi is the tight end, M = 2n or 2n + 1 --
    along x ((n+2) x 9) and along y (9 x (n+2)), float tables and SC_FLAG_EXACT_TABLES.  One line per (length, n, axis)."""
    _, oc = oracles
    cls64 = {c[0] for c in length_classes(True)}
    fails = []
    print("\nFFT lengths: M r n axis | float: err(ft) err(exact) / oracle-f32 (ft, exact) | double: ulps(ft) ulps(exact)")
    for M, r, lo, hi in length_classes(False):
        for n in sorted({lo, hi}):
            for axis in "xy":
                W, H = (n + 2, 9) if axis == "x" else (9, n + 2)
                B, lap = _field(W, H, seed=1000 * n + (axis == "y"))
                ref = _Ref(oc, B, lap)
                f32 = _check_fft(inst, ref, B, lap, False)
                f64 = _check_fft(inst, ref, B, lap, True) if M in cls64 else []
                line = "FFTLEN M=%5d r=%d n=%4d %s | f32 %.2e %.2e / %.2e %.2e" % (M, r, n, axis, f32[0][1], f32[1][1], f32[0][3], f32[1][3])
                line += (" | f64 %.2f %.2f ulp" % (f64[0][1], f64[1][1])) if f64 else " | f64 -"
                print(line)
                for prec, rows in (("f32", f32), ("f64", f64)):
                    for exact, err, bound, _ in rows:
                        if not err <= bound:
                            fails.append((M, n, axis, prec, "exact" if exact else "float-tables", err, bound))
    assert not fails, fails


# ----------------------------------------------------------------------------------------------------------- size limits
def test_fft_size_limits_and_the_instance_after_a_refusal(inst, oracles):
    """8193 unknowns (float) and 4097 (double) along either axis: SC_ERR_BAD_SIZE, and the same instance then solves 8192 / 4096
    correctly.  SC_METHOD_AUTO takes the direct solve for a narrow strip 4096 unknowns long and the cycles at 4097."""
    from seamlesscloneoptimization_amd import capi
    _, oc = oracles
    for fp64, top in ((False, 8192), (True, 4096)):
        assert fft_M(top) == fft_max_M(fp64) and fft_M(top + 1) > fft_max_M(fp64)
        flags = capi.SC_FLAG_FFT_FP64 if fp64 else 0
        for axis in "xy":
            shape = lambda n: (n + 2, 9) if axis == "x" else (9, n + 2)     # noqa: E731
            B, lap = _field(*shape(top + 1), seed=top + 1)
            inst.set_solver(method=capi.SC_METHOD_FFT, flags=flags)
            inst.field_load(B, lap)
            with pytest.raises(capi.SeamlessCloneError) as e:
                inst.field_solve()
            assert e.value.code == capi.SC_ERR_BAD_SIZE, (fp64, axis, e.value)
            B, lap = _field(*shape(top), seed=top)              # the same instance, the largest supported size
            got = _solve(inst, B, lap, capi.SC_METHOD_FFT, flags)
            want = oc.solve_dst(oc.fold(B, lap), _nt(oc))
            d = float(np.abs(got[:, 1:-1, 1:-1] - want).max())
            if fp64:
                assert d <= F64_ULPS * _ulp(np.abs(want).max()), (axis, d)
            else:
                e32 = float(np.abs(oc.solve_dst(oc.fold(B, lap), _nt(oc), internals="f32") - want).max())
                assert d <= max(F32_FACTOR * e32, F32_FLOOR * max(1.0, float(np.abs(want).max()) / 500.0)), (axis, d, e32)
    # SC_METHOD_AUTO: a narrow strip up to 4096 unknowns long is solved directly, one unknown longer by the cycles
    for n, method in ((4096, capi.SC_METHOD_FFT), (4097, capi.SC_METHOD_MULTIGRID)):
        for W, H in ((n + 2, 102), (102, n + 2)):
            assert capi.auto_takes_direct(W - 2, H - 2) == (method == capi.SC_METHOD_FFT)
            B, lap = _field(W, H, seed=n)
            inst.set_solver(method=capi.SC_METHOD_AUTO, flags=0)
            inst.field_load(B, lap)
            inst.field_solve(allow_not_converged=True)
            assert inst.info().method == method, (W, H, inst.info().method)


# --------------------------------------------------------------------------------------------------------- plane layouts
LAYOUT_CASES = [(1026, 514, True), (1027, 514, True), (2050, 514, False), (2051, 514, False)] + \
               [(W, H, fp64) for W, H in ((4000, 140), (140, 4000), (1100, 1000)) for fp64 in (False, True)]


@pytest.mark.parametrize("W,H,fp64", LAYOUT_CASES)
def test_fft_both_plane_layouts(inst, oracles, W, H, fp64):
    """Both sides of the 4 MiB per channel switch between the three-launch form and the five-launch form with two transposes, w or
    h not a multiple of 64 on the transposed side, field level against the port."""
    _, oc = oracles
    tiny = (W - 2) * (H - 2) * (8 if fp64 else 4) <= 4 << 20
    assert tiny == ((W, H) in ((1026, 514), (2050, 514)) or (not fp64 and (W, H) in ((4000, 140), (140, 4000))))
    B, lap = _field(W, H, seed=W * 7 + H)
    ref = _Ref(oc, B, lap)
    rows = _check_fft(inst, ref, B, lap, fp64)
    print("LAYOUT %dx%d %s %s: %s" % (W, H, "f64" if fp64 else "f32", "tiny" if tiny else "transposed",
                                     ", ".join("%s %.3g (bound %.3g)" % ("exact" if x else "ft", e, b) for x, e, b, _ in rows)))
    for exact, err, bound, _ in rows:
        assert err <= bound, (W, H, fp64, exact, err, bound)


def _jobs(pi, items):
    from seamlesscloneoptimization_amd import capi
    jobs = capi.Pool.make_jobs(len(items))
    keep = []
    for j, (dst, patch, mask, cx, cy) in zip(jobs, items):
        fp, b, b0, m = pi.to_device(patch), pi.to_device(dst), pi.to_device(dst), pi.to_device(mask)
        keep.append((fp, b, b0, m))
        j.face, j.face_cols, j.face_rows, j.face_step = fp, patch.shape[1], patch.shape[0], 3 * patch.shape[1]
        j.body, j.body_cols, j.body_rows, j.body_step = b, dst.shape[1], dst.shape[0], 3 * dst.shape[1]
        j.mask, j.mask_cols, j.mask_rows, j.mask_step = m, mask.shape[1], mask.shape[0], mask.shape[1]
        j.centerX, j.centerY, j.body_restore = cx, cy, b0
    return jobs, keep


@pytest.mark.parametrize("fp64", [False, True])
def test_fft_group_at_a_transposed_size_equals_the_solo_runs(oracles, fp64):
    """A pool group of four 1100 x 1000 clones (12 channels through the five-launch form) against each clone alone."""
    from seamlesscloneoptimization_amd import capi
    o, oc = oracles
    flags = capi.SC_FLAG_FFT_FP64 if fp64 else 0
    N = 4
    items = [o.synth_inputs(1100, 1000, seed_dst=310 + k, seed_patch=330 + k, margin=20) for k in range(N)]
    pool = capi.Pool(0, 1, group=N, method=capi.SC_METHOD_FFT, flags=flags)
    solo = capi.Instance(0)
    try:
        pi = pool.instances[0]
        jobs, keep = _jobs(pi, items)
        pool.run(jobs, device_resident=True)
        assert pi.info().method == capi.SC_METHOD_FFT and pi.field_shape()[0] == 3 * N
        solo.set_solver(method=capi.SC_METHOD_FFT, flags=flags)
        for k, ((dst, patch, mask, cx, cy), (fp, b, b0, m)) in enumerate(zip(items, keep)):
            got = pi.from_device(b, dst.shape)
            alone = dst.copy()
            assert solo.run(patch, alone, mask, cx, cy) == 0
            assert np.array_equal(got, alone), (k, int(np.abs(got.astype(np.int16) - alone).max()))
            if k == 0:
                want = oc.seamless_clone(dst, patch, mask, cx, cy, _nt(oc))
                assert int(np.abs(got.astype(np.int16) - want).max()) <= 1
        for t in keep:
            for p in t:
                pi.free(p)
    finally:
        solo.destroy()
        pool.close()


# ----------------------------------------------------------------------------------------------------------- AUTO strips
def _strip_cases():
    out = []
    for L in (2600, 3074, 3600, 4096):
        for a in (58, 128, 140, 141):
            out += [(L, a), (a, L)]
    return out + [(2598, 168)]                  # a 2600 x 170 ROI: direct by the area rule


def test_auto_strips_end_to_end(oracles):
    """Whole clones through the DEFAULT options at strip sizes (unknowns w x h) with M = 6144 and 8192 along and 58 ... 141 across,
    against the float-table port: the method auto_takes_direct names, max <= 1, and a differing share below STRIP_SHARE_DIRECT /
    STRIP_SHARE_MG.  The 1500 x 130 ROI's share is printed beside them: the longer strips' are up to 3.4x its (1 / den amplifies the
    rounding of the lowest modes ~ n^2), so it is a yardstick, not the bound."""
    from seamlesscloneoptimization_amd import capi
    o, oc = oracles
    inst = capi.Instance(0)
    try:
        def one(w, h, seed):
            dst, patch, mask, cx, cy = o.synth_inputs(w + 2, h + 2, margin=16, seed_dst=seed, seed_patch=seed + 1)
            want = oc.seamless_clone(dst, patch, mask, cx, cy, min(16, oc.max_threads()))
            body = dst.copy()
            assert inst.run(patch, body, mask, cx, cy) == 0
            i = inst.info()
            assert (i.W, i.H) == (w + 2, h + 2)
            d = np.abs(body.astype(np.int16) - want.astype(np.int16))
            return i.method, int(d.max()), float((d > 0).sum()) / (3.0 * w * h)
        m0, mx0, share0 = one(1498, 128, 5)
        assert m0 == capi.SC_METHOD_FFT and mx0 <= 1
        print("\nSTRIP 1498x128 (reference): method %d max %d share %.3e" % (m0, mx0, share0))
        bad = []
        for k, (w, h) in enumerate(_strip_cases()):
            method, mx, share = one(w, h, 40 + 2 * k)
            direct = capi.auto_takes_direct(w, h)
            print("STRIP %dx%d: method %d (%s) max %d share %.3e" % (w, h, method, "direct" if direct else "multigrid", mx, share))
            if method != (capi.SC_METHOD_FFT if direct else capi.SC_METHOD_MULTIGRID) or mx > 1 or \
                    share > (STRIP_SHARE_DIRECT if direct else STRIP_SHARE_MG):
                bad.append((w, h, method, mx, share))
        assert not bad, (share0, bad)
    finally:
        inst.destroy()


# ----------------------------------------------------------------------------------------------------------- table cache
class _LruModel:
    """sc_fft.hip's two LRUs as the library keeps them (fft_build_dim, fft_fxy: one tick counter, the first least recently used
    entry is the victim, a buffer grows and never shrinks): what a sequence of solves does to them."""

    def __init__(self):
        self.tick = 0
        self.dims = [dict(n=0, dbl=False, used=0, cap=0, evicted=False) for _ in range(8)]
        self.fxy = [dict(key=None, used=0, evicted=False) for _ in range(4)]
        self.grew_to_max = self.small_in_large = False
        self.revisits_of_evicted = 0
        self.gone = set()

    def _dim(self, n, dbl, keep):
        victim = None
        for d in self.dims:
            if d["n"] == n and d["dbl"] == dbl:
                self.tick += 1
                d["used"] = self.tick
                return d
            if d is not keep and (victim is None or d["used"] < victim["used"]):
                victim = d
        if (n, dbl) in self.gone:
            self.revisits_of_evicted += 1
        if victim["n"]:
            victim["evicted"] = True
            self.gone.add((victim["n"], victim["dbl"]))
        M = fft_M(n)
        need = (16 if dbl else 8) * (4 * M + 1)
        if M == 16384 and 0 < victim["cap"] < need:
            self.grew_to_max = True
        if victim["cap"] >= 16 * 4 * 8192 and M <= 1024:
            self.small_in_large = True
        victim["cap"] = max(victim["cap"], need)
        self.tick += 1
        victim.update(n=n, dbl=dbl, used=self.tick)
        return victim

    def solve(self, w, h, dbl):
        dw = self._dim(w, dbl, None)
        self._dim(h, dbl, dw)
        victim = None
        for f in self.fxy:
            if f["key"] == (w, h):
                self.tick += 1
                f["used"] = self.tick
                return
            if victim is None or f["used"] < victim["used"]:
                victim = f
        if victim["key"] is not None:
            victim["evicted"] = True
        self.tick += 1
        victim.update(key=(w, h), used=self.tick)


CACHE_SEQUENCE = [  # unknowns (w, h), double transforms
    (300, 200, False), (300, 200, True), (100, 100, False), (100, 100, True), (40, 7, False),
    (8000, 9, False), (300, 200, False), (4000, 9, True), (130, 130, True), (9, 8000, False),
    (60, 3000, False), (2500, 9, True), (20, 20, False), (33, 17, True), (50, 60, False), (70, 80, True),
    (21, 9, True), (300, 200, True), (100, 100, False), (8000, 9, False), (40, 7, False), (4000, 9, True),
    (45, 46, False), (45, 46, True), (100, 100, True), (9, 21, True), (6001, 9, False), (300, 200, False),
]


def test_fft_table_cache_across_precisions_and_large_lengths(oracles):
    """One instance through CACHE_SEQUENCE -- float and double solves of the same n, an entry grown from a small length to M = 16384
    and a large buffer reused for a small one, every FftDim (8) and FftFxy (4) entry evicted and evicted sizes revisited, square
    sizes -- byte-identical at every step to a fresh instance on the same input."""
    from seamlesscloneoptimization_amd import capi
    _, oc = oracles
    model = _LruModel()
    for w, h, dbl in CACHE_SEQUENCE:
        model.solve(w, h, dbl)
    assert all(d["evicted"] for d in model.dims) and all(f["evicted"] for f in model.fxy)
    assert model.grew_to_max and model.small_in_large and model.revisits_of_evicted >= 4
    assert any(w == h for w, h, _ in CACHE_SEQUENCE)
    seq = capi.Instance(0)
    try:
        for k, (w, h, dbl) in enumerate(CACHE_SEQUENCE):
            B, lap = _field(w + 2, h + 2, seed=500 + k)
            flags = capi.SC_FLAG_FFT_FP64 if dbl else 0
            got = _solve(seq, B, lap, capi.SC_METHOD_FFT, flags)
            fresh = capi.Instance(0)
            try:
                want = _solve(fresh, B, lap, capi.SC_METHOD_FFT, flags)
            finally:
                fresh.destroy()
            assert np.array_equal(got, want), (k, w, h, dbl, float(np.abs(got - want).max()))
            if k % 9 == 0:          # and the fresh answer is the right one
                ref = oc.solve_dst(oc.fold(B, lap), _nt(oc))
                assert float(np.abs(got[:, 1:-1, 1:-1] - ref).max()) <= 2e-3 * max(1.0, float(np.abs(ref).max()) / 500.0), (k, w, h)
    finally:
        seq.destroy()


# ------------------------------------------------------------------------------------------------------- DST parity fold
def _dst_sizes():
    ns = set(range(253, 259)) | set(range(509, 515)) | set(range(1021, 1027))
    for n in range(2, 1101):
        if dst_padded_half(n) != dst_padded_half(n - 1):
            ns |= {n - 1, n}
    return sorted(ns)


def test_dst_parity_fold_across_tiles(inst, oracles):
    """SC_METHOD_DST with m = ceil(n/2) = 127 ... 129, 255 ... 257, 511 ... 513 in both parities and on each side of every change of the
    padded half size up to n = 1100, along each axis: against the port within F64_ULPS float32 ulps, and byte-identical to
    SC_METHOD_FFT with SC_FLAG_FFT_FP64 (DESIGN.md §4's claim, measured at every one of these sizes)."""
    from seamlesscloneoptimization_amd import capi
    _, oc = oracles
    worst = 0.0
    for n in _dst_sizes():
        for axis in "xy":
            W, H = (n + 2, 9) if axis == "x" else (9, n + 2)
            B, lap = _field(W, H, seed=7000 + 2 * n + (axis == "y"))
            for exact in (False, True):
                flags = capi.SC_FLAG_EXACT_TABLES if exact else 0
                want = oc.solve_dst(oc.fold(B, lap), _nt(oc), exact_den=exact)
                ulp = _ulp(np.abs(want).max())
                got = _solve(inst, B, lap, capi.SC_METHOD_DST, flags)
                fft = _solve(inst, B, lap, capi.SC_METHOD_FFT, flags | capi.SC_FLAG_FFT_FP64)
                e_ref = float(np.abs(got[:, 1:-1, 1:-1] - want).max()) / ulp
                worst = max(worst, e_ref)
                assert e_ref <= F64_ULPS, (n, axis, exact, e_ref)
                assert np.array_equal(got, fft), (n, axis, exact, float(np.abs(got - fft).max()) / ulp)
    print("DST fold: worst %.2f ulp against the port, byte-identical to FFT+FP64" % worst)


def test_dst_odd_in_both_directions_end_to_end(inst, oracles):
    """A 259 x 517-unknown clone (odd n both ways, m = 130 and 259: the middle point beyond the first tile) through SC_METHOD_DST."""
    from seamlesscloneoptimization_amd import capi
    o, oc = oracles
    dst, patch, mask, cx, cy = o.synth_inputs(261, 519, margin=24, seed_dst=259, seed_patch=517)
    want = oc.seamless_clone(dst, patch, mask, cx, cy, _nt(oc))
    inst.set_solver(method=capi.SC_METHOD_DST)
    body = dst.copy()
    assert inst.run(patch, body, mask, cx, cy) == 0
    i = inst.info()
    assert i.method == capi.SC_METHOD_DST and (i.W, i.H) == (261, 519)
    assert int(np.abs(body.astype(np.int16) - want).max()) <= 1
    assert not np.array_equal(body, dst)
