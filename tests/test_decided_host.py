"""CPU side of tests/test_gpu_decided_channels.py: the launch decisions of the float-table correction (sc_lowmode.hip) restated in
Python, the proof that the GPU file's shapes reach both sides of each of them, and a self-test of the decided-channel check
(tests/decided_np.py) on the oracle alone.  Every restatement names the C++ function it mirrors; a retune of one of their thresholds
makes a coverage assertion below fail here, on the CPU, instead of quietly dropping a branch from the GPU tests."""
import numpy as np
import pytest

import decided_np as dn

LM_HAT, LM_KB, LM_RS = 8, 32, 4         # sc_lowmode.hip: node spacing, modes per register block, row splits the parts buffer holds
PARTS_SUM_FROM = 32                     # sc_lowmode.hip lowmode_nodes: k_lm_parts_sum adds the projection's parts from 32 parts on
K_CAP = 256                             # sc_lowmode.hip lowmode_count: at most 256 modes per direction


def lowmode_count(n):
    """sc_lowmode.hip lowmode_count: ceil(n / 64) modes, at least 8, a multiple of 8, at most n and at most 256"""
    k = (n + 63) // 64
    k = (max(k, 8) + 7) & ~7
    return min(k, n, K_CAP)


def projection_splits(nxt, nkb):
    """sc_lowmode.hip lowmode_projection_splits: as few row splits as fill the chip, at most LM_RS"""
    nrs = 1
    while nrs < LM_RS and nxt * nrs * nkb * 3 < 192:
        nrs *= 2
    return nrs


def round_up(v, m):
    return (v + m - 1) // m * m


def lm_geometry(W, H):
    """sc_lowmode.hip lm_prepare / lowmode_nodes for one W x H field (ring included)"""
    Kx, Ky = lowmode_count(W - 2), lowmode_count(H - 2)
    Kxp, Kyp = round_up(Kx, LM_KB), round_up(Ky, LM_KB)
    nx, ny = ((W - 2) >> 3) + 2, ((H - 2) >> 3) + 2
    nxt, nkb = (nx + 63) // 64, Kyp // LM_KB
    nrs = projection_splits(nxt, nkb)
    nparts = nxt * nrs
    return dict(Kx=Kx, Ky=Ky, Kxp=Kxp, Kyp=Kyp, nx=nx, ny=ny, nxt=nxt, nrs=nrs, nparts=nparts, parts_sum=nparts >= PARTS_SUM_FROM)


# ---- the GPU cases ------------------------------------------------------------------------------------------------------------
# W - 2 and H - 2 at every residue mod 8 (H's residue a permutation of W's), one plane count each
RESIDUE_FIELDS = [(2 + 8 * (40 + 8 * r) + r, 2 + 8 * (30 + 3 * r) + (5 * r + 3) % 8, (1, 2, 3, 6, 16, 3, 2, 1)[r]) for r in range(8)]
# (W, H, C) of the correction at every launch geometry (test_correction_at_every_launch_geometry)
FIELD_CASES = RESIDUE_FIELDS + [
    (32260, 40, 1),        # one row split, 64 parts: k_lm_parts_sum; Kx at the cap
    (16400, 64, 2),        # two row splits, 66 parts; Kx at the cap
    (3700, 600, 3),        # four row splits, exactly 32 parts: k_lm_parts_sum
    (2048, 2048, 6),       # four row splits, 20 parts: the expansion adds them itself
    (4096, 4096, 1),       # 36 parts, 64 modes per direction
    (514, 515, 2),         # n = 512 | 513: K = 8 | 16
    (1027, 1026, 3),       # n = 1025 | 1024: K = 24 | 16
    (9, 7, 1),             # n = 7 | 5: K = n
]
# (W, H, C, post-smoothing sweeps) of the correction from the cell shares a solve's last launch left (k_lm_bands_to_cells).  The judged
# launch of a solve through the hooks has `post` sweeps, and the fused level-0 form takes post = 1 or 2 (sc_multigrid.cpp fused_level0):
# the tilings of 1 and 2 sweeps.  The 4-sweep tiling (post + pre: the early correction of a clone's output) is not reachable from the
# hooks; the end-to-end tests of tests/test_gpu_decided_channels.py cover it.
BANDS_CASES = [(300, 105, 3, 2), (300, 105, 3, 1), (517, 300, 1, 2), (517, 300, 2, 1), (260, 1025, 2, 2), (260, 1025, 6, 1), (70, 53, 3, 2),
               (70, 53, 3, 1)]
# end to end: multigrid clones at every residue of W - 2 and H - 2, the shapes of test_output_and_restriction_variants_agree, wide,
# 4096^2 and one size of lowmode_early_kind 3 (plan_size "conditional")
MG_RESIDUE_SHAPES = [(730 + r, 562 + (5 * r + 3) % 8) for r in range(8)]
VARIANT_SHAPES = [(9, 9), (64, 71), (233, 59), (240, 53), (57, 40), (249, 60), (505, 118), (517, 400), (1030, 1000), (1856, 1700), (2048, 2048)]
BIG_SHAPES = [(3700, 600), (4096, 4096), (3120, 3120)]
# size classes: n = 512 | 513 and 1024 | 1025 in one class (a K step inside it); a class with a saturating member (field_retry)
CLASSES = [[(514, 600), (515, 610)], [(1026, 1026), (1027, 1027)]]
SATURATING_CLASS = [(640, 560), (652, 571), (625, 583)]


def decision_sides():
    sides = set()
    for W, H, C in FIELD_CASES:
        g = lm_geometry(W, H)
        sides.add(("parts_sum", g["parts_sum"]))
        sides.add(("splits", g["nrs"]))
        sides.add(("Kx_cap", g["Kx"] == K_CAP))
        sides.add(("K_is_n", g["Kx"] == W - 2))
        sides.add(("C", C))
        sides.add(("wres", (W - 2) % 8))
        sides.add(("hres", (H - 2) % 8))
    return sides


def test_restatements_match_the_library_and_the_numpy_correction():
    from oracle import lowmode_np
    from seamlesscloneoptimization_amd import capi
    for n in list(range(1, 40)) + [511, 512, 513, 1023, 1024, 1025, 4094, 15872, 15873, 16000, 32258]:
        assert lowmode_count(n) == lowmode_np.lowmode_count(n), n
    # the planner's export (sc_hip_plan_size) of the class-eligible sizes: modes, column tiles, row splits
    for W, H in [(2048, 2048), (1030, 1000), (514, 514), (515, 515), (3120, 3120), (730, 565)]:
        p, g = capi.plan_size(W, H), lm_geometry(W, H)
        assert p["eligible"] == 1, (W, H)
        assert (p["Kxp"], p["Kyp"], p["column_tiles"], p["row_splits"]) == (g["Kxp"], g["Kyp"], g["nxt"], g["nrs"]), (W, H, p, g)


def test_gpu_cases_reach_every_side():
    s = decision_sides()
    for side in [("parts_sum", True), ("parts_sum", False), ("splits", 1), ("splits", 2), ("splits", 4), ("Kx_cap", True), ("Kx_cap", False),
                 ("K_is_n", True)] + [("C", c) for c in (1, 2, 3, 6, 16)] + [("wres", r) for r in range(8)] + [("hres", r) for r in range(8)]:
        assert side in s, side
    assert lm_geometry(3700, 600)["nparts"] == PARTS_SUM_FROM and lm_geometry(4096, 4096)["nparts"] == 36
    assert {lowmode_count(512), lowmode_count(513), lowmode_count(1024), lowmode_count(1025)} == {8, 16, 24}
    assert {(W - 2) % 8 for W, _ in MG_RESIDUE_SHAPES} == set(range(8)) and {(H - 2) % 8 for _, H in MG_RESIDUE_SHAPES} == set(range(8))
    assert {(H - 2) % 8 for _, H, _, _ in BANDS_CASES} != {0} and {p for *_, p in BANDS_CASES} == {1, 2}


def test_classes_hold_their_k_step_and_their_saturating_member():
    """planner export: each class is one size class (kind 2, or 3: on another hierarchy than the solo run), across a K step"""
    from seamlesscloneoptimization_amd import capi
    for sizes in CLASSES + [SATURATING_CLASS]:
        g, k = capi.plan_groups(sizes)
        assert len(set(g)) == 1 and set(k) <= {2, 3}, (sizes, g, k)
    for sizes in CLASSES:
        assert len({(lowmode_count(W - 2), lowmode_count(H - 2)) for W, H in sizes}) == 2, sizes


def test_boundaries_and_bounds():
    u = np.array([-3.0, 0.2, 0.7, 1.0, 1.02, 254.99, 255.0, 256.5, 100.5])
    assert np.allclose(dn.boundary_distance(u), [4.0, 0.8, 0.3, 0.0, 0.02, 0.01, 0.0, 1.5, 0.5])
    assert dn.to_bytes(u).tolist() == [0, 0, 0, 1, 1, 254, 255, 255, 100]
    assert np.allclose(dn.crossed_bound([100.95, 100.95, 0.5, 254.9, 100.5], [101, 99, 1, 255, 100]), [0.05, 0.95, 0.5, 0.1, 0.0])


def test_the_check_flags_what_the_statistics_accept():
    """A +0.3 bump on one 8 x 8 cell of a 2048^2 float-table solution, truncated: image_diff_stats' max <= 1, percent < 0.5 accepts the
    bytes; the decided-channel check at the multigrid delta rejects them, and passes the unbumped bytes."""
    from oracle import oracle_c, oracle_np
    from seamlesscloneoptimization_amd import compare
    oracle_c.build()
    dst, patch, mask, cx, cy = oracle_np.synth_inputs(2048, 2048, margin=16)
    case = dn.clone_case(oracle_c, dst, patch, mask, cx, cy, nthreads=min(16, oracle_c.max_threads()))
    want = oracle_c.seamless_clone(dst, patch, mask, cx, cy, nthreads=min(16, oracle_c.max_threads()))
    assert np.array_equal(case.want(), want)
    und, mism, bound = dn.check(case, want, dn.DELTA_MG, "oracle")
    assert mism == 0 and bound == 0.0 and 0.1 < und < 0.2          # 2 x 0.08 of every unit interval
    u = case.u.copy()
    # an 8 x 8 cell (field rows and columns 8k ... 8k + 7) away from the clamps, where the bump moves bytes
    k = next(k for k in range(64, 255) if 2.0 < u[:, 8 * k - 1:8 * k + 7, 8 * k - 1:8 * k + 7].min() and u[:, 8 * k - 1:8 * k + 7, 8 * k - 1:8 * k + 7].max() < 253.0)
    u[:, 8 * k - 1:8 * k + 7, 8 * k - 1:8 * k + 7] += np.float32(0.3)
    bumped = case.dst.copy()
    y0, x0 = case.lty + 1, case.ltx + 1
    bumped[y0:y0 + case.H - 2, x0:x0 + case.W - 2] = np.moveaxis(dn.to_bytes(u), 0, 2)
    s = compare.image_diff_stats(want, bumped)
    assert s["max"] <= 1 and s["percent"] < 0.5 and s["max"] == 1
    with pytest.raises(AssertionError, match="decided channels"):
        dn.check(case, bumped, dn.DELTA_MG, "bumped")
    outside = want.copy()
    outside[case.lty, case.ltx + 5, 1] ^= 1                        # the ring belongs to the destination
    with pytest.raises(AssertionError, match="outside the ROI interior"):
        dn.check(case, outside, dn.DELTA_MG, "ring")
