"""The multigrid cycle walk without a GPU (tests/mg_cycle_cases.py, tests/mg_cycle_bounds.py; the device side: tests/test_gpu_mg_cycles.py).

1. Every shape is pinned to the regime it is there for, through sc_hip_cycle0_plan -- the functions the level-0 kernel and its launcher
   evaluate, on the library's own ladder -- and oracle/mg_np.py's ladder is held against the library's.
2. The inputs stay inside the 16-bit field's range, the default spec computes what it always did (tests/golden/mg_cycles_spec.npz).
3. Sharpness: a bound that a defective cycle meets is worth nothing.  The float32 restatement is mutated here (never in oracle/) the way a
   kernel goes wrong at a seam, and every mutation must miss the bounds of the device test by a factor of two:
       m1x / m1y   the first column / row of the last tile (the last interior one where that tile holds the ring alone) misses the last
                   half-step of a level-0 smoothing call
       m2          the level-0 restriction's last coarse column x 0.9
       m3          tw1 and tw2 swapped in the prolongation
       m4          m1x on level 1's own launch (the level1_seams shapes)
   at n = 1 in the first cycle, at n = 2 in the second cycle only, and at n = 3 (the shapes of cases.N3) in the third only, against the bound
   itself.  The seam mutations are judged by the float routes' bounds -- the field hooks and the SC_FLAG_FLOAT_L1 clone, the runs that are there
   to catch them (mg_cycle_bounds.py) -- and at n = 1 by the format routes' as well; from the second cycle on the format routes' own
   bound carries E_fmt besides, and what it is there to catch is a wrong load or store: m5, every float16 store truncating instead of
   rounding, must exceed the kept field's format bound at n = 1 and n = 2, and m6, the 16-bit store without its rounding half, the
   bytes' at n = 3 (the 16-bit field exists from n = 2 on; its full cycle from n = 3), on every shape that composes level 1; the
   unmutated restatement with the formats must meet both bounds at every budget.  A converged
   solve forgets each of them (oracle/mg_np.py's cycle has an exact residual); one, two and three cycles do not."""
import contextlib
import os

import numpy as np
import pytest

import mg_cycle_bounds as mb
import mg_cycle_cases as cases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mg_cycles_spec.npz")


def plans(name):
    """the plan hook's answers for the shape's three level-0 launch forms: first launch (2 sweeps), full cycle (4, prolongs), judged (2, prolongs)"""
    from seamlesscloneoptimization_amd import capi
    W, H = cases.shape(name)
    first = capi.cycle0_plan(W, H, 2)
    comp = bool(first["composes"])
    return first, capi.cycle0_plan(W, H, 4, True, comp), capi.cycle0_plan(W, H, 2, True, comp)


def verdicts(plan):
    from seamlesscloneoptimization_amd import capi
    return {capi.CYCLE0_INNER[v] for v in plan["inner"].ravel()}


# ---------------------------------------------------------------------------------------------------------------- 1. regimes
@pytest.mark.parametrize("name", cases.NAMES)
def test_shape_is_in_its_regime(name):
    from oracle import mg_np
    from seamlesscloneoptimization_amd import capi
    cls, W, H = cases.SHAPES[name]
    first, full, judged = plans(name)
    for p, T in ((first, 2), (full, 4), (judged, 2)):
        assert (p["xstep"], p["ystep"], p["hx"], p["hy"], p["waves"], p["rows"]) == (cases.XSTEP, cases.YSTEP[T], 12, 2 * T + 2, 8, 8), name
        assert (p["nbx"], p["nby"]) == (-(-W // cases.XSTEP), -(-H // cases.YSTEP[T])), name
        assert p["inner"].shape == (p["nby"], p["nbx"], 8)
    last_cols = W - cases.XSTEP * (full["nbx"] - 1)
    last_rows = {T: H - cases.YSTEP[T] * (-(-H // cases.YSTEP[T]) - 1) for T in (2, 4)}
    # ---- the ladder: the library's own against the numpy spec's
    levels = mg_np.build_levels(W, H)
    assert first["levels"] == len(levels)
    assert (first["n1x"], first["n1y"]) == (levels[0][0].nc, levels[0][1].nc)
    if len(levels) > 1:
        assert (first["n2x"], first["n2y"]) == (levels[1][0].nc, levels[1][1].nc)
    assert first["bottom"] == mg_np.bottom_level(levels), (name, first["bottom"], mg_np.bottom_level(levels))
    assert bool(first["composes"]) == mg_np.composes_level1(levels), name
    composed = bool(first["composes"])
    tail = first["tail"]
    # ---- the class
    if cls == "last_cols_1":
        assert full["nbx"] == 2 and 1 <= last_cols <= 5 and last_cols == W - 232
    elif cls == "last_cols_2":
        assert full["nbx"] == 3 and 1 <= last_cols <= 5 and last_cols == W - 464
    elif cls == "whole_tiles":
        assert last_cols in (cases.XSTEP - 1, cases.XSTEP) and full["nbx"] == (1 if W < 233 else 2)
    elif cls == "inner_cols":
        want = cases.INNER_COLS[name]
        tile1 = {capi.CYCLE0_INNER[v] for v in full["inner"][:, 1, :].ravel()}
        assert tile1 - {"y_first", "y_last", "l1_y_first", "l1_y_last", "l2_y"} == {want}, (name, tile1)
        assert ("inner" in verdicts(full)) == (want == "inner")
        # the three column conditions, evaluated here for column tile 1 (xw = 232 - 12): equality where the docstring says so
        xw = cases.XSTEP - 12
        l0, l1, l2 = (W - 2) - (xw + 255), first["n1x"] - (((xw + 252) >> 1) + 2), first["n2x"] - (((xw + 252) >> 2) + 1)
        assert {"cols_476": l0 == -1, "cols_477": l0 == 0 and l1 == -1, "cols_478": l1 == 0 and l2 == -1, "cols_479": l2 == 0 and l1 == 0}[name], (l0, l1, l2)
        assert composed
    elif cls == "level1_seams":
        assert composed
    elif cls == "last_rows":
        assert W == 236 and last_cols == 4
        # a last row tile of 0 .. 4 rows beyond one (H < 88) or two whole tiles, at the full cycle's step or at the two-sweep launches'
        over = {T: (H - cases.YSTEP[T]) % cases.YSTEP[T] for T in (2, 4)}
        whole = {T: (H - over[T]) // cases.YSTEP[T] for T in (2, 4)}
        assert any(over[T] <= 4 and whole[T] == (1 if H < 88 else 2) for T in (2, 4)), (name, over, whole)
        assert all(last_rows[T] == (over[T] or cases.YSTEP[T]) for T in (2, 4) if over[T] <= 4)
    elif cls == "inner_rows":
        assert W == 482 and composed
        assert capi.CYCLE0_INNER[full["inner"][1, 1, 2]] == cases.INNER_ROWS[name], (name, full["inner"][1, 1])
        y0 = 1 * cases.YSTEP[4] - 10 + 2 * 8
        Jb = (y0 >> 1) - 1
        y, l1, l2 = (H - 2) - (y0 + 7), first["n1y"] - (Jb + 5), first["n2y"] - ((Jb >> 1) + 4)
        assert {"inner_rows_58": y == -1, "inner_rows_59": y == 0 and l1 == -1, "inner_rows_60": l1 == 0 and l2 < 0, "inner_rows_66": l2 == -1,
                "inner_rows_67": l2 == 0}[name], (y, l1, l2)
    elif cls == "hierarchy":
        n1 = (levels[1][0].n, levels[1][1].n)
        facts = {"ladder_512x60": tail == 2 and levels[2][0].n == 127 and first["bottom"] == 3,
                 "ladder_516x60": tail == 3 and levels[2][0].n == 128 and levels[3][0].n <= 127 and first["bottom"] == 4,
                 "ladder_131x60": max(n1) == 64 and first["bottom"] == 1 and not composed and mg_np.direct_level(levels) == 1,
                 "ladder_132x60": max(n1) == 65 and tail == 2 and first["bottom"] == 3 and composed,
                 "ladder_195x60": max(n1) == 96 and tail == 2 and first["bottom"] == 3 and composed,
                 "ladder_196x60": max(n1) == 97 and tail == 2 and first["bottom"] == 3 and composed,
                 "ladder_300x9": mg_np.direct_level(levels) is None and not composed and len(levels) == 2,
                 "ladder_60x236": composed and full["nby"] == 6 and full["nbx"] == 1}
        assert facts[name], name
    elif cls == "both_seams":
        assert full["nbx"] == 3 and full["nby"] == 3 and "inner" in verdicts(full) and "inner" in verdicts(judged) and composed
    # a wave that prolongs never passes where the same wave without the coarse conditions fails
    plain = capi.cycle0_plan(W, H, 4)["inner"]
    assert not ((full["inner"] == 0) & (plain != 0)).any()


def test_level1_seam_shapes_pack_as_listed():
    """level 1's own launch (four sweeps from a zero correction): a tile owns 232 columns; the last column tile of several planes shares a
    workgroup where the plan says so (sc_hip_coarse_tile_plan; K planes per packed workgroup)"""
    from seamlesscloneoptimization_amd import capi
    for name, (width, packed) in cases.LEVEL1_SEAMS.items():
        W, H = cases.shape(name)
        p = capi.cycle0_plan(W, H, 2)
        assert p["n1x"] + 2 == width, name
        for rows in (12, 28):                      # the two band heights of the float16 level-1 launch (R = 4, 6: 8 R - 2 (2 x 4 + 2))
            full, lps, K, blocks = capi.coarse_tile_plan(p["n1x"] + 2, p["n1y"] + 2, 3, 232, 12, rows)
            assert (K > 1) == packed and full == 1, (name, full, lps, K)
            assert lps == (8 if packed else 64), (name, lps)


def test_every_branch_of_coarsen_1d_is_reached():
    seen = {}
    for name in cases.NAMES:
        for (l, d), b in cases.branches(name).items():
            seen.setdefault((l, b), []).append(name)
    want = {(0, "odd"), (0, "even_keep")} | {(l, b) for l in (1, 2) for b in ("odd", "even_keep", "even_drop")}
    assert set(seen) == want, want - set(seen)            # (level 0's last interval is one spacing: nothing to drop there)


def test_the_plan_hook_refuses_what_no_launch_has():
    from seamlesscloneoptimization_amd import capi
    for bad in ((2, 60, 2, 0, 0), (236, 60, 0, 0, 0), (236, 60, 6, 0, 0), (236, 60, 4, 0, 1), (5, 5, 4, 1, 1), (300, 4, 2, 1, 0)):
        with pytest.raises(capi.SeamlessCloneError):
            capi.cycle0_plan(*bad)


# ---------------------------------------------------------------------------------------------------------------- 2. inputs, default spec
@pytest.mark.parametrize("name", cases.NAMES)
def test_clone_inputs_stay_inside_the_16_bit_field(name):
    """[-256, 768) is what the 16-bit field holds; the spec's iterates must lie well inside it, or the device would repeat the clone on float
    fields (info.field_retry) and the walk would judge another path"""
    first = plans(name)[0]
    for n in cases.budgets(name):
        for c in cases.channels(name, n):
            kinds = ("u64", "u64_fast") if first["composes"] else ("u64",)
            for kind in kinds:
                u = mb.solve(name, "clone", c, n, kind)
                assert -200.0 < u.min() and u.max() < 700.0, (name, n, c, kind, float(u.min()), float(u.max()))


def test_default_spec_is_bit_for_bit_what_it_was():
    """oracle/mg_np.py with every new option at its default, against arrays its previous text computed (tests/golden/mg_cycles_spec.npz)"""
    from oracle import mg_np
    g = np.load(GOLDEN)
    U, F = cases.noise_fields("cols_236")
    B, lap = cases.clone_inputs("cols_236")[5:7]
    got = {"fused_3": mg_np.solve(U[0], F[0], cycles=3), "unfused_1": mg_np.solve(U[0], F[0], cycles=1, fused=False),
           "half_2": mg_np.solve(B[1], lap[1], cycles=2, level1_half=True), "fast_3": mg_np.solve(B[1], lap[1], cycles=3, level1_half=True, field_q16=True)}
    assert sorted(got) == sorted(g.files)
    for k, v in got.items():
        assert v.dtype == np.float32 and np.array_equal(v, g[k]), k


def test_twin_and_restatement_are_the_same_cycle():
    """the twin in double and the float32 restatement differ from the default spec by rounding only, on both schedules and with the formats"""
    for name in ("cols_236", "ladder_131x60"):
        for fused in (True, False):
            spec = mb.solve(name, "fields", 0, 1, "spec", fused)
            assert mb.interior_max(mb.solve(name, "fields", 0, 1, "u64", fused) - spec) < 1e-3
            assert mb.interior_max(mb.solve(name, "fields", 0, 1, "u32", fused) - spec) < 1e-3
            assert mb.solve(name, "fields", 0, 1, "u64", fused).dtype == np.float64
    assert 1e-3 < mb.e_fmt("cols_236", 1, 1, False) < 0.2 and mb.e_fmt("ladder_131x60", 1, 1, False) == 0.0


# ---------------------------------------------------------------------------------------------------------------- 3. sharpness
@contextlib.contextmanager
def mutated(name, kind, cycle):
    """oracle/mg_np.py with one mutation `kind` active in cycle `cycle` (0-based) of a solve of the shape's plane and in no other"""
    from oracle import mg_np
    W, H = cases.shape(name)
    levels = mg_np.build_levels(W, H)
    first, full, _ = plans(name)
    state = {"cycle": -1}
    rb_gen, restrict, prolong, vcycle = mg_np.rb_gen, mg_np.restrict, mg_np.prolong, mg_np.vcycle

    def on(level_n):
        return state["cycle"] == cycle and level_n

    def skip_last_half_step(U, F, dx, dy, sweeps, out, x=None, y=None):
        # the points the last half-step updates (x + y odd) keep what they held after sweeps - 1 sweeps
        before = rb_gen(U, F, dx, dy, sweeps - 1) if sweeps > 1 else U.astype(np.float32)
        yy, xx = np.mgrid[0:U.shape[0], 0:U.shape[1]]
        m = ((xx + yy) & 1) == 1
        m &= (xx == x) if x is not None else (yy == y)
        m[0, :] = m[-1, :] = False; m[:, 0] = m[:, -1] = False
        out = out.copy()
        out[m] = before[m]
        return out

    def rb(U, F, dx, dy, sweeps=1, omega=1.0, dtype=np.float32):
        out = rb_gen(U, F, dx, dy, sweeps, omega, dtype)
        level0 = (dx.n, dy.n) == (W - 2, H - 2)
        level1 = len(levels) > 1 and (dx.n, dy.n) == (levels[1][0].n, levels[1][1].n)
        # (a last tile of one column / row holds the ring alone: the seam's last interior line then)
        if kind == "m1x" and on(level0):
            return skip_last_half_step(U, F, dx, dy, sweeps, out, x=min(cases.XSTEP * (full["nbx"] - 1), W - 2))
        if kind == "m1y" and on(level0):
            return skip_last_half_step(U, F, dx, dy, sweeps, out, y=min(cases.YSTEP[4] * (full["nby"] - 1), H - 2))
        if kind == "m4" and on(level1):
            return skip_last_half_step(U, F, dx, dy, sweeps, out, x=min(cases.XSTEP, dx.n))
        return out

    def rs(R, dx, dy, dtype=np.float32):
        out = restrict(R, dx, dy, dtype)
        if kind == "m2" and on(dx.n == W - 2 and dy.n == H - 2):
            out = out.copy()
            out[:, dx.nc] *= np.float32(0.9)
        return out

    def pr(E, dx, dy, dtype=np.float32):
        if kind == "m3" and on(True):
            sx, sy = (type("Swapped", (), dict(vars(d), tw1=d.tw2, tw2=d.tw1)) for d in (dx, dy))
            return prolong(E, sx, sy, dtype)
        return prolong(E, dx, dy, dtype)

    def vc(lv, l, *a, **k):
        if l == 0:
            state["cycle"] += 1
        return vcycle(lv, l, *a, **k)

    mg_np.rb_gen, mg_np.restrict, mg_np.prolong, mg_np.vcycle = rb, rs, pr, vc
    try:
        yield
    finally:
        mg_np.rb_gen, mg_np.restrict, mg_np.prolong, mg_np.vcycle = rb_gen, restrict, prolong, vcycle


def applies(name, kind):
    from oracle import mg_np
    W, H = cases.shape(name)
    levels = mg_np.build_levels(W, H)
    first, full, _ = plans(name)
    if kind == "m1x":
        return full["nbx"] > 1
    if kind == "m1y":
        return full["nby"] > 1
    if kind == "m2":
        return True
    if kind == "m3":            # a tail with the points: some level the cycle prolongs to has one or two fine points beyond its last coarse one
        d = mg_np.direct_level(levels)
        upto = d if d is not None else len(levels) - 1
        return any(float(dim.tw1) != float(dim.tw2) for l in range(upto) for dim in levels[l])
    if kind == "m4":
        return name in cases.LEVEL1_SEAMS and cases.LEVEL1_SEAMS[name][0] > cases.XSTEP
    raise KeyError(kind)


def mutant_distance(name, route, c, n, kind, cycle, half=False):
    """D of the mutated float32 restatement's iterate n"""
    from oracle import mg_np
    U0, F = mb.plane(name, route, c)
    with mutated(name, kind, cycle):
        u = mg_np.solve(U0, F, cycles=n, residual_f32=True, direct_f32=True, level1_half=half)
    return mb.interior_max(u - mb.solve(name, route, c, n, "u64_half" if half else "u64"))


def worst_bound(name, c, n):
    """the largest bound any route of the device test applies to the clone's plane at budget n"""
    composes = bool(plans(name)[0]["composes"])
    return max(mb.format_bound(name, c, n, fast) for fast in ((False, True) if composes and n > 1 else (False,)))


@pytest.mark.parametrize("name", cases.NAMES)
def test_first_cycle_mutations_miss_the_bounds_twice_over(name):
    c = cases.NAMES.index(name) % 3
    kinds = [k for k in ("m1x", "m1y", "m2", "m3", "m4") if applies(name, k)]
    assert "m2" in kinds and ("m1x" in kinds or "m1y" in kinds), (name, kinds)
    if name in ("cols_464", "cols_470", "cols_472"):          # (232 columns, cols_462: one whole tile, no seam)
        assert "m4" in kinds
    for kind in kinds:
        d_fields = mutant_distance(name, "fields", 0, 1, kind, 0)
        d_clone = mutant_distance(name, "clone", c, 1, kind, 0)
        b_fields, b_clone = mb.float_bound(name, "fields", 0, 1), worst_bound(name, c, 1)
        print("%s %s n=1: fields D %.3g bound %.3g, clone D %.3g bound %.3g" % (name, kind, d_fields, b_fields, d_clone, b_clone))
        assert d_fields > 2.0 * b_fields, (name, kind, d_fields, b_fields)
        assert d_clone > 2.0 * b_clone, (name, kind, d_clone, b_clone)


@pytest.mark.parametrize("name", cases.NAMES)
def test_second_cycle_seam_mutation_misses_the_bounds_twice_over(name):
    c = cases.channels(name, 2)[0]
    kinds = [k for k in ("m1x", "m1y") if applies(name, k)]
    assert kinds
    for kind in kinds:
        d_fields = mutant_distance(name, "fields", 0, 2, kind, 1)
        d_clone = mutant_distance(name, "clone", c, 2, kind, 1)
        b_fields, b_clone = mb.float_bound(name, "fields", 0, 2), mb.float_bound(name, "clone", c, 2)
        print("%s %s n=2: fields D %.3g bound %.3g, clone D %.3g bound %.3g (format routes: %.3g)" % (name, kind, d_fields, b_fields, d_clone, b_clone, worst_bound(name, c, 2)))
        assert d_fields > 2.0 * b_fields, (name, kind, d_fields, b_fields)
        assert d_clone > 2.0 * b_clone, (name, kind, d_clone, b_clone)


@pytest.mark.parametrize("name", cases.N3)
def test_third_cycle_shapes_are_sharp(name):
    """a shape runs three cycles only if the seam mutation in the third cycle alone still exceeds the bound"""
    c = cases.channels(name, 3)[0]
    kinds = [k for k in ("m1x", "m1y") if applies(name, k)]
    for kind in kinds:
        d_fields = mutant_distance(name, "fields", 0, 3, kind, 2)
        d_clone = mutant_distance(name, "clone", c, 3, kind, 2)
        b_fields, b_clone = mb.float_bound(name, "fields", 0, 3), mb.float_bound(name, "clone", c, 3)
        print("%s %s n=3: fields D %.3g bound %.3g, clone D %.3g bound %.3g (format routes: %.3g)" % (name, kind, d_fields, b_fields, d_clone, b_clone, worst_bound(name, c, 3)))
        assert d_fields > b_fields, (name, kind, d_fields, b_fields)
        assert d_clone > b_clone, (name, kind, d_clone, b_clone)


def test_three_cycles_run_in_every_class():
    assert {cases.SHAPES[n][0] for n in cases.N3} == set(cases.CLASSES)


# ---- the format routes' bound: a wrong store
def f16_truncating(a, dtype=np.float32):
    """m5: float16 toward zero instead of to nearest"""
    h = a.astype(np.float16)
    over = np.abs(h.astype(np.float64)) > np.abs(a.astype(np.float64))
    return np.where(over, np.nextafter(h, np.float16(0)), h).astype(dtype)


def q16_without_the_half(a, dtype=np.float32):
    """m6: code = trunc(64 u + 16384) instead of trunc(64 u + 16384.5)"""
    t = (a.astype(dtype) * dtype(64.0) + dtype(16384.0)).astype(dtype)
    code = np.clip(np.trunc(np.clip(t, 0.0, 65535.0)), 0, 65535).astype(dtype)
    return (code * dtype(0.015625) - dtype(256.0)).astype(dtype)


def format_mutant_distance(name, c, n, attr, fn, fast):
    from oracle import mg_np
    U0, F = mb.plane(name, "clone", c)
    old = getattr(mg_np, attr)
    setattr(mg_np, attr, fn)
    try:
        u = mg_np.solve(U0, F, cycles=n, residual_f32=True, direct_f32=True, level1_half=True, field_q16=fast)
    finally:
        setattr(mg_np, attr, old)
    return mb.interior_max(u - mb.solve(name, "clone", c, n, "u64_fast" if fast else "u64_half"))


@pytest.mark.parametrize("name", cases.NAMES)
def test_format_bounds_hold_for_the_restatement_and_catch_a_wrong_store(name):
    if not plans(name)[0]["composes"]:
        assert all(mb.e_fmt(name, 0, n, True) == 0.0 for n in (1, 2))          # no format beyond the exact float16 inputs: the float bound
        return
    c = cases.NAMES.index(name) % 3
    for n in (1, 2, 3):
        for fast in (False, True):
            clean = mb.interior_max(mb.solve(name, "clone", c, n, "u32_fast" if fast else "u32_half") - mb.solve(name, "clone", c, n, "u64_fast" if fast else "u64_half"))
            assert clean <= mb.format_bound(name, c, n, fast), (name, n, fast, clean, mb.format_bound(name, c, n, fast))
    for n in (1, 2):
        d, b = format_mutant_distance(name, c, n, "_f16", f16_truncating, False), mb.format_bound(name, c, n, False)
        print("%s m5 n=%d: D %.3g bound %.3g" % (name, n, d, b))
        assert d > b, (name, "m5", n, d, b)
    d, b = format_mutant_distance(name, c, 3, "_q16", q16_without_the_half, True), mb.format_bound(name, c, 3, True)
    print("%s m6 n=3: D %.3g bound %.3g" % (name, d, b))
    assert d > b, (name, "m6", 3, d, b)
