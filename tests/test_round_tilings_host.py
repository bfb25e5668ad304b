"""CPU tests behind tests/test_gpu_round_tilings.py: its matrices cover what they are there for, every case's restatement alone stays
inside the conditions the GPU tests rely on, and the bounds are sharp at these shapes -- a round rebuilt in numpy with one deliberate
tiling mistake misses the GPU test's bound by a factor of 10 at least (the factors are printed)."""
from __future__ import annotations

import numpy as np
import pytest

from seamlesscloneoptimization_amd import capi

import bounded_bounds as bb
import region_np
import region_robust_bounds as gr
import region_robust_np as rr
import robust_coupled_np as rc
import round_tilings_bounds as tb
import volume_coupled_np as vc
import volume_robust_bounds as rb
import volume_robust_np as vr
import volume_wls_np as vw

S, T, J = vc.SPACE, vc.TIME, vc.CHANNELS
G = capi.SC_POISSON_GUIDANCE
SHARP = 10.0


def plan_of(shape, border):
    ny, nx, frames = tb.SHAPES[shape]
    H, W = tb.image_size(border, ny, nx)
    sides, periodic = tb.BORDERS[border]
    return capi.pcg_plan(W, H, G | capi.border_bits(sides, False, periodic), frames)


# ---- the matrices ------------------------------------------------------------------------------------------------------------------------
def test_the_volume_matrix_covers_every_coupling_border_and_time_at_every_shape():
    m = tb.volume_matrix()
    assert 22 <= len(m) <= 26 and len(set(m)) == len(m)
    assert {c[0] for c in m} == {"stacked_frames", "long_time", "wide_frames"}
    for shape in tb.VOLUME_SHAPES:
        rows = [c for c in m if c[0] == shape]
        assert {c[3] for c in rows} == {0, S, S | T, J, S | J, S | T | J}, shape
        assert {c[1] for c in rows} == set(tb.VOLUME_BORDERS[shape]) >= {"neumann", "free_lt"}, shape
        assert {c[2] for c in rows} == {"free", "periodic"}, shape
        assert {(c[1], c[2]) for c in rows} >= {(b, t) for b in ("neumann", "free_lt") for t in ("free", "periodic")} or shape == "wide_frames"
        # every form is effective under its exponents, a form with TIME is one penalty, CHANNELS has channels to couple
        for c in rows:
            assert vc.effective(c[3], c[5] + (0, 0, 0), c[4]) == c[3] and (not c[3] & T or c[5][0] == c[5][1]), c
        # ... whose states differ between the channels
        joint = [i for i, c in enumerate(m) if c[0] == shape and c[3] & J]
        assert any((lambda s: (s != s[..., :1]).any())(tb.volume_input(*m[i][:3], m[i][4], m[i][7])["state"]) for i in joint), shape
        for border in tb.VOLUME_BORDERS[shape]:
            missing = [name for name, ok in tb.regime(shape, plan_of(shape, border)) if not ok]
            assert not missing, (shape, border, missing)
    assert any(c[:2] == ("wide_frames", "periodic_x") for c in m), "the wrap across the outer groups"
    for shape in ("stacked_frames", "long_time"):
        assert any(c[0] == shape and c[2] == "periodic" for c in m), "the wrap's owner in frame T - 1"
    # stacked frames with three channels: exactly one chunk of 192 planes
    assert all(c[4] * tb.SHAPES[c[0]][2] == 192 for c in m if c[0] == "stacked_frames")
    assert {c[6] for c in m} == set(tb.EPS) and {c[7] for c in m} == set(tb.TAUS)


def test_the_region_and_bounded_matrices_cover_their_axes():
    m = tb.region_matrix()
    assert len(m) == 12 and len(set(m)) == len(m)
    for shape in tb.PLANE_SHAPES:
        rows = [c for c in m if c[0] == shape]
        assert {c[1] for c in rows} == {"neumann", "frame", "periodic_xy"} and {c[2] for c in rows} == {"scatter", "split"}
        assert {c[3] for c in rows} == {0, rr.ISO, rr.JOINT, rr.ISO | rr.JOINT} and all(c[4][0] < 2 for c in rows)
        for border in tb.REGION_BORDERS + tb.BOUNDED_BORDERS:
            missing = [name for name, ok in tb.regime(shape, plan_of(shape, border)) if not ok]
            assert not missing, (shape, border, missing)
    assert all(m[i][0] == "many_parts" for i in tb.CAPPED) and {m[i][3] for i in tb.CAPPED} == {0, rr.ISO | rr.JOINT}
    b = tb.bounded_matrix()
    assert len(b) == 8
    for shape in tb.PLANE_SHAPES:
        rows = [c for c in b if tb.bounded_shape(c) == shape]
        assert {c[0] for c in rows} == set(tb.BOUNDED_BORDERS) and {c[8] for c in rows} == {"both", "arrays"} and {c[4] for c in rows} == {"scatter", "split"}
    # the refusal test's case, and a part 200 with an UNKNOWN and a KNOWN pixel in it
    case = next(c for c in b if tb.bounded_shape(c) == "many_parts" and c[8] == "arrays" and c[0] == "frame")
    p, _ = bb.case_input(case, True, False)
    plan = plan_of("many_parts", "frame")
    k = region_np.kinds(p["sides"], p["periodic"], p["state"])[plan["y0"] + 200 * plan["rows"]:plan["y0"] + 201 * plan["rows"]]
    assert (k == region_np.UNKNOWN).any() and (k == region_np.KNOWN).any() and plan["bands"] > 200


# ---- the restatement alone stays inside the GPU tests' conditions ---------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(tb.volume_matrix())), ids=[tb.volume_id(c) for c in tb.volume_matrix()])
def test_every_inner_solve_of_the_volume_restatement_ends_before_max_iters(i):
    p, pen, coupling, y = tb.volume_case(i)
    assert len(y.iters32) == tb.ROUNDS + 1 and max(y.iters32) < 400, y.iters32
    assert all(e > 0 and r > 0 for e, r in y.fig32), "no floor is needed: the restatement's figures are not 0"
    q = rb.nan_unread(p)
    want = np.sum(y.energy(y.exact[-1]))
    got = np.sum(vc.energy(q, pen, y.exact[-1], coupling) if coupling else vr.energy(q, pen, y.exact[-1]))
    assert got == want, "the energy reads an element the header says is not read"


@pytest.mark.parametrize("i", range(len(tb.region_matrix())), ids=[tb.region_id(c) for c in tb.region_matrix()])
def test_every_inner_solve_of_the_region_restatement_ends_before_max_iters(i):
    p, pen, coupling, y = tb.region_case(i)
    assert len(y.iters32) == tb.ROUNDS + 1 and max(y.iters32) < 400, y.iters32
    assert all(e > 0 and r > 0 for e, r in y.fig32)


@pytest.mark.parametrize("case", tb.bounded_matrix(), ids=[bb.case_id(c) for c in tb.bounded_matrix()])
def test_the_bounded_reference_converges(case):
    p, y = bb.case_input(case)
    assert y.rounds <= bb.MAX_REFERENCE_ROUNDS and y.rounds32 <= y.max_rounds() and max(y.iters32) < 400, (y.rounds, y.rounds32, y.iters32)
    outside, near = tb.violated(p, y)
    n = int(y.unk.sum())
    assert 0.4 * n <= outside <= 0.6 * n and near <= 0.01 * n, "the bounds sit at the quartiles: half of the unconstrained answer is outside"


def test_the_batches_inner_solves_end_before_max_iters():
    for n, frames, coupling in ((17, 2, S | J), (9, 8, S | T | J)):
        probs = tb.batch_inputs(n, frames)
        pen = rb.penalties(probs[0], (1.0, 1.0, 2.0), 1e-2)
        chunk = vc.irls_f32(probs[:8] if frames == 8 else probs, pen, tb.ROUNDS, coupling)
        assert max(max(its) for _, its in chunk) < 400
        assert np.array_equal(probs[-1]["data"], np.float32(3) * probs[0]["data"]) and probs[-1]["range"] > 2.9 * probs[0]["range"]


# ---- sharpness ---------------------------------------------------------------------------------------------------------------------------
def _volume_args(P, links):
    """volume_wls_np's args of a round with these (s_x, s_y, s_t, w'): volume_robust_np.round_args' second half"""
    sx, sy, smt, w = links
    lap = vw.divergence(*vr._head(P), sx, sy, smt, 1.0, P["gx"], P["gy"], P["gt"])
    data = P["data"] if P["weight"] is not None else np.where(vw.kinds(P["sides"], P["periodic"], P["state"]) == vw.UNKNOWN, np.float32(0), vr._f32(P["data"]))
    return vr._head(P) + (w, sx, sy, smt, 1.0, data, lap)


def _missed(tag, y, mutated):
    """by how much round 1's iterate of a mutated system misses the GPU test's bound: the larger of ERR / its bound, RES / its bound"""
    err, res = y.measure(y.exact[0], mutated, 1)
    eb, rb_ = y.bounds(1)
    factor = max(err / eb, res / rb_)
    print(f"SHARP {tag}: ERR {err:.3e} (bound {eb:.3e}) RES {res:.3e} (bound {rb_:.3e}): misses by a factor of {factor:.1f}")
    return factor


def test_a_back_link_read_from_the_wrong_frame_misses_the_bound():
    """stacked frames, uncoupled: in the first row of one band -- band 100 starts at row 9 of frame 27 -- the back link's rho taken
    from frame t instead of t - 1 (the link changed as a whole: the mistaken value on both of its ends)"""
    i = next(i for i, c in enumerate(tb.volume_matrix()) if c[0] == "stacked_frames" and c[1] == "neumann" and c[3] == 0)
    p, pen, coupling, y = tb.volume_case(i)
    plan = plan_of("stacked_frames", "neumann")
    ny = tb.SHAPES["stacked_frames"][0]
    t, row = divmod(100 * plan["rows"], ny)
    assert t > 0 and 0 < row < ny - 1, "the band starts inside a frame"
    sx, sy, st, w = vr.reweigh(p, pen, y.exact[0], np.float64)
    st = st.copy()
    st[t - 1, row] = st[t, row]
    mutated = vr._thwc(vw.solve_exact(_volume_args(p, (sx, sy, st, w)), vr._boundary(p)))
    unchanged = vr._thwc(vw.solve_exact(_volume_args(p, vr.reweigh(p, pen, y.exact[0], np.float64)), vr._boundary(p)))
    assert np.array_equal(unchanged, y.exact[1]), "the round as rebuilt here is the yardstick's own"
    assert _missed("the back link's rho from frame t, one row of one band", y, mutated) >= SHARP


def test_a_west_link_read_one_short_of_its_owner_misses_the_bound():
    """wide frames, SPACE: the west link of column 256 -- the first of the second column group; its owner, column 255, lies in the
    first -- takes the rho one element short of the owner's, column 254's (the link changed as a whole)"""
    i = next(i for i, c in enumerate(tb.volume_matrix()) if c[0] == "wide_frames" and c[1] == "neumann" and c[3] == S)
    p, pen, coupling, y = tb.volume_case(i)
    assert plan_of("wide_frames", "neumann")["cg"] == 3
    sx, sy, st, w = vc.reweigh(p, pen, y.exact[0], coupling, np.float64)
    sx = sx.copy()
    sx[:, :, 255] = sx[:, :, 254]
    mutated = vr._thwc(vw.solve_exact(_volume_args(p, (sx, sy, st, w)), vr._boundary(p)))
    assert _missed("the west link's rho at the group boundary from column 254", y, mutated) >= SHARP


@pytest.mark.parametrize("i", tb.CAPPED, ids=[tb.region_id(tb.region_matrix()[i]) for i in tb.CAPPED])
def test_a_part_left_out_of_s_bar_misses_the_capped_bound(i):
    """many parts: part 117 of 234 left out of the sum of the live links.  s-bar only steers the preconditioner: the converged rounds
    cannot see it (the factor printed first), the capped round does"""
    shape, border, pattern, coupling, exps, epsf = tb.region_matrix()[i]
    p = tb.region_input(shape, border, pattern)
    pen = gr.penalties(p, exps, epsf)
    plan = plan_of(shape, border)
    assert plan["cg"] * plan["bands"] == 234
    rows = slice(plan["y0"] + 117 * plan["rows"], plan["y0"] + 118 * plan["rows"])
    u0 = tb.capped_start(p)
    args = rr.round_args(p, pen, u0, coupling)
    lx, ly = region_np.live_links(p["sides"], p["periodic"], p["state"])
    total = float(args[4][lx].astype(np.float64).sum() + args[5][ly].astype(np.float64).sum())
    part = float(args[4][rows][lx[rows]].astype(np.float64).sum() + args[5][rows][ly[rows]].astype(np.float64).sum())
    factor = 1.0 - part / total
    assert 0.9 < factor < 1.0
    u64, bound = tb.capped_bound(p, pen, coupling, u0)
    d = tb.distance(p, tb.capped_round(p, pen, coupling, u0, np.float32, factor), u64)
    print(f"SHARP {tb.region_id(tb.region_matrix()[i])}: part 117 holds {part / total:.3%} of the links' sum; capped D {d:.3e} (bound {bound:.3e}): "
          f"misses by a factor of {d / bound:.1f}")
    assert d / bound >= SHARP


def test_a_part_left_out_of_esum_exceeds_energy_rel():
    """many parts, both couplings: the gradient energy of part 117 alone, against ENERGY_REL of the whole"""
    i = next(i for i, c in enumerate(tb.region_matrix()) if c[0] == "many_parts" and c[3] == rr.ISO | rr.JOINT)
    p, pen, coupling, y = tb.region_case(i)
    plan = plan_of("many_parts", tb.region_matrix()[i][1])
    rows = slice(plan["y0"] + 117 * plan["rows"], plan["y0"] + 118 * plan["rows"])
    u = y.exact[-1]
    mx, _, hx, _ = rr.magnitudes(p, u, coupling, np.float64)
    share = np.where(hx, rc._psi(pen[0], pen[2], mx), 0.0)[:, :, 0]          # (joint: the image's magnitude, counted once)
    whole = float(np.sum(rr.energy(p, pen, u, coupling)))
    data_term = whole - float(share.sum())
    assert data_term >= 0 and abs(float(share.sum()) + data_term - whole) <= 1e-12 * whole
    rel = float(share[rows].sum()) / whole
    print(f"SHARP esum: part 117 holds {rel:.3e} of the energy (ENERGY_REL {gr.ENERGY_REL:.1e}): {rel / gr.ENERGY_REL:.0f} times the bound")
    assert rel >= SHARP * gr.ENERGY_REL
