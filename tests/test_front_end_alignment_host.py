"""(host arithmetic only) The front-end alignment walk reaches what tests/test_gpu_front_end_alignment.py claims.

From the walk's geometry alone (tests/front_end_cases.py restates the kernels' address arithmetic): every residue of every
re-alignment, every seam of every tiling, every launch form.  And the restatement of a placed view -- the images read back out of the
case's one buffer -- equals the restatement of the dense content, so placing moves bytes and nothing else."""
import numpy as np

import front_end_cases as fc


def test_scan_walk_meets_every_row_offset_and_grid():
    """For each of the scan's two extreme pixels every a0 in 0..15; rows whose a0 differs from their neighbour's; one and two workgroup
    columns, the last pixels found by either; the empty interior, the single pixel and the all-255 mask."""
    cases = fc.scan_cases()
    a0 = [set(), set()]
    widths, heights, pads, kinds, changing, cols, wgcol = set(), set(), set(), set(), 0, set(), set()
    for c in cases:
        m, = c.members
        mh, mw = m.c.mask.shape
        widths.add(mw); heights.add(mh); pads.add(m.pm.pad); kinds.add(c.note)
        for k, (x, y) in enumerate(m.c.marks):
            a0[k].add(fc.scan_a0(m, y))
            assert 1 <= x <= mw - 2 and 1 <= y <= mh - 2
        changing += len({fc.scan_a0(m, y) for y in range(1, mh - 1)}) > 1
        cols.add((mw, fc.scan_grid(mw, mh)[0]))
        wgcol |= {(mw, (x + fc.scan_a0(m, y)) // (fc.BB_CHUNK * fc.BB_CHUNKS)) for x, y in m.c.marks}      # the workgroup column that finds the pixel
        if m.c.marks:                                                  # the border lines carry non-zero bytes the rectangle ignores
            assert m.c.mask[0].all() and m.c.mask[-1].all() and m.c.mask[:, 0].all() and m.c.mask[:, -1].all()
            xs, ys = [p[0] for p in m.c.marks], [p[1] for p in m.c.marks]
            assert fc.true_rect(m.c) == (min(xs), max(xs), min(ys), max(ys))
    assert a0[0] == set(range(16)) and a0[1] == set(range(16)), a0
    assert widths == set(fc.SCAN_W) and heights == set(fc.SCAN_H) and pads == set(fc.SCAN_PAD)
    assert kinds >= {"zero", "single", "full"} and changing > len(cases) // 2
    # from mw = 1010 the launch has two workgroup columns; at mw = 1025 the last pixels move into the second with a0 > 0
    assert {(1009, 1), (1010, 2), (1025, 2), (1040, 2)} <= cols and {(1025, 0), (1025, 1), (1040, 1), (1010, 0)} <= wgcol
    # where the extremes sit: both sides of the first 16-byte chunk and of the first workgroup row, and against both ends
    marks = [(x, y, c.members[0].c.mask.shape[1], c.members[0].c.mask.shape[0]) for c in cases for x, y in c.members[0].c.marks]
    xs, ys = {p[0] for p in marks}, {p[1] for p in marks}
    assert xs >= {1, 2, 14, 15, 16, 17} and ys >= {1, 3, 4, 15, 16}, (sorted(xs), sorted(ys))
    assert {mw - x for x, _, mw, _ in marks if mw >= 1009} >= {2, 3} and {mh - y for _, y, _, mh in marks if mh >= 33} >= {2}
    zero = [c.members[0] for c in cases if c.note == "zero"][0]
    assert fc.true_rect(zero.c) == (zero.c.mask.shape[1] - 1, 0, zero.c.mask.shape[0] - 1, 0)
    single = [c.members[0] for c in cases if c.note == "single"][0]
    r = fc.true_rect(single.c)
    assert r[0] == r[1] and fc.geo_of(r, 0, 0) is None


def test_riding_and_group_scans_meet_every_grid_combination():
    """Riding: tile grids 1, 2, 3 wide against scans of 1, 2, 5 workgroups, some riding workgroups idle, a right and a wrong guess
    (one column short) of each.  Group: three masks of one size; seventeen of differing sizes -- a second launch, grids smaller than the launch's."""
    seen, idle = set(), 0
    for c in fc.riding_cases():
        m, = c.members
        mh, mw = m.c.mask.shape
        g = fc.run_geo(c, m)
        gx = (g["W"] + fc.P4_TW - 1) // fc.P4_TW
        sx, sy = fc.scan_grid(mw, mh)
        rows = (sx * sy + gx - 1) // gx
        idle += rows * gx > sx * sy
        right = m.guess == fc.true_rect(m.c)
        if not right:
            assert m.guess[1] == fc.true_rect(m.c)[1] - 1 and m.guess[::2] == fc.true_rect(m.c)[::2]
        seen.add((gx, sx * sy, right))
    assert seen == {(a, b, r) for a in (1, 2, 3) for b in (1, 2, 5) for r in (True, False)}, sorted(seen)
    assert idle >= 4
    big = [c for c in fc.group_scan_cases() if len(c.members) == 17]
    assert len(big) == 2
    for c in big:
        grids = {fc.scan_grid(*m.c.mask.shape[::-1]) for m in c.members}
        assert len(grids) >= 4 and max(g[0] for g in grids) == 2 and len({m.c.mask.shape for m in c.members}) >= 8
        assert len({fc.scan_a0(m, 1) for m in c.members}) >= 8
    assert any(len(c.members) == 3 and len({m.c.mask.shape for m in c.members}) == 1 and len({m.pm for m in c.members}) == 3 for c in fc.group_scan_cases())


def _erode_table(cases):
    pairs, base, sizes, holes = set(), set(), set(), set()
    for c in cases:
        for m in c.members:
            g = fc.run_geo(c, m)
            sizes.add((g["W"], g["H"]))
            base.add(((m.pm.o + g["x0"]) % 4, m.mstep % 4))
            pairs |= {(fc.erode_shift(m, g, y), m.mstep % 4) for y in range(g["H"])}
            holes |= {(x, y, g["W"], g["H"]) for x, y in m.c.marks}
    return pairs, base, sizes, holes


def test_erode_walk_meets_every_shift_seam_and_ring():
    """Every (address mod 4, step mod 4) in the solo, the in-tile and the group walk; holes on both sides of every word, wave, strip and
    tile seam and at ring distances 2, 3 and 4 from each side; ROIs whose window ends at the mask's last column and row, and at column 1."""
    walks = fc.erode_cases()
    every = {(a, s) for a in range(4) for s in range(4)}
    for name in ("solo", "tile", "group"):
        pairs, base, sizes, holes = _erode_table(walks[name])
        assert pairs == every, (name, sorted(every - pairs))
        if name != "tile":
            assert sizes == set(fc.ER_SIZES), name
            assert {b[0] for b in base} == {0, 1, 2, 3} and {b[1] for b in base} == {0, 1, 2, 3}
        xs, ys = {h[0] for h in holes}, {h[1] for h in holes}
        assert xs >= {2, 3, 4, 7, 8, 127, 128, 255, 256} and ys >= {2, 3, 4, 7, 8, 15, 16, 31, 32}, (name, sorted(xs), sorted(ys))
        right = {W - 1 - x for x, _, W, _ in holes}
        below = {H - 1 - y for _, y, _, H in holes}
        assert right >= {2, 3, 4} and below >= {2, 3, 4}, (name, sorted(right)[:6], sorted(below)[:6])
    for c in walks["solo"]:
        m, = c.members
        g = fc.run_geo(c, m)
        # the erode of the scan's ROI is the port's whole mask stage
        assert np.array_equal(fc.restate_M(m.c, g), fc.oracle_np.mask_stage(m.c.mask, m.c.cx, m.c.cy)["M"])
    full = [c.members[0] for c in walks["solo"] if c.members[0].c.mask.all() is np.True_ or c.members[0].c.mask[0, 0] == 255]
    assert len(full) == len(walks["solo"]) // 2
    for m in full:          # x0 = y0 = 1, the ROI's last column and row are the interior's last, and 255 lies beside the ROI
        g = fc.geo_of(fc.true_rect(m.c), m.c.cx, m.c.cy)
        mh, mw = m.c.mask.shape
        assert (g["x0"], g["y0"], g["x0"] + g["W"], g["y0"] + g["H"]) == (1, 1, mw - 1, mh - 1)
    # in the tile: the library's own guess (the interior of an all-255 mask) and boxes with 255 beside them, where the ring test alone zeroes M
    short = 0
    for c in walks["tile"]:
        m, = c.members
        g = fc.run_geo(c, m)
        beside = m.c.mask[g["y0"]:g["y0"] + g["H"], g["x0"] + g["W"]]
        short += bool((beside == 255).all())
    assert short >= len(walks["tile"]) // 2
    # groups: same-size members at different placements, size classes of three sizes
    assert sum(c.form == 3 for c in walks["group"]) >= 4
    for c in walks["group"]:
        wh = {(fc.run_geo(c, m)["W"], fc.run_geo(c, m)["H"]) for m in c.members}
        assert len(wh) == (1 if c.form == 2 else 3) and len({(m.pm, m.c.mask.shape) for m in c.members}) == len(c.members)
    # grey: minimum-filter tiles are 64 x 16; values 1..254 across 63 | 64 and 15 | 16
    gs = {(fc.run_geo(c, c.members[0])["W"], fc.run_geo(c, c.members[0])["H"]) for c in walks["grey"]}
    assert any(W > fc.G7_TW and H > fc.G7_TH for W, H in gs) and all(0 < fc.restate_M(c.members[0].c, fc.run_geo(c, c.members[0]), True).max() < 255 for c in walks["grey"] if min(fc.run_geo(c, c.members[0])["W"], fc.run_geo(c, c.members[0])["H"]) > 9)
    assert {(m.pm.o + fc.run_geo(c, m)["x0"]) % 4 for c in walks["grey"] for m in c.members} == {0, 1, 2, 3}


def _pre_table(cases):
    body, face, base_b, base_f, diff, rows_b, rows_f, sizes, edges, pads = set(), set(), set(), set(), set(), 0, 0, set(), set(), set()
    for c in cases:
        for m in c.members:
            g = fc.run_geo(c, m)
            org = fc.stage_origins(m, g)
            body |= {v[0] for v in org.values()}
            face |= {v[1] for v in org.values()}
            rb, rf = (m.pb.o + 3 * g["ltx"]) % 16, (m.pf.o + 3 * g["x0"]) % 16
            base_b.add(rb); base_f.add(rf); diff.add((rb - rf) % 16)
            # adjacent staged rows whose origins differ in their low two bits: the row above must be re-aligned by ITS origin
            rows_b += any((org[(0, y)][0] ^ org[(0, y - 1)][0]) & 3 for y in range(1, g["H"]))
            rows_f += any((org[(0, y)][1] ^ org[(0, y - 1)][1]) & 3 for y in range(1, g["H"]))
            sizes.add((g["W"], g["H"]))
            br, bc = m.c.dst.shape[:2]
            edges |= {k for k, v in (("left", g["ltx"] == 0), ("right", g["ltx"] + g["W"] == bc), ("top", g["lty"] == 0), ("bottom", g["lty"] + g["H"] == br)) if v}
            pads |= {m.pb.pad, m.pf.pad}
    return body, face, base_b, base_f, diff, rows_b, rows_f, sizes, edges, pads


def test_preprocess_walk_meets_every_origin_and_edge():
    """Every staged-row origin mod 16 for the destination and for the patch, each base residue independently of the other, adjacent
    rows with different origins, the ROI against each edge of its destination, every size, in the solo, the group and the class walk."""
    all16 = set(range(16))
    body, face, base_b, base_f, diff, rows_b, rows_f, sizes, edges, pads = _pre_table(fc.pre_solo_cases())
    assert body == all16 and face == all16 and base_b == all16 and base_f == all16
    assert len(diff) >= 8 and rows_b >= 16 and rows_f >= 16
    assert sizes == set(fc.PRE_SIZES) and {w for w, _ in sizes} == set(fc.PRE_W) and {h for _, h in sizes} == set(fc.PRE_H)
    assert edges == {"left", "right", "top", "bottom"} and pads == set(fc.PRE_PAD)
    for walk in (fc.pre_group_cases(), fc.pre_class_cases()):
        body, face, _, _, diff, rows_b, rows_f, sizes, edges, _ = _pre_table(walk)
        assert body == all16 and face == all16 and len(diff) >= 4 and rows_b and rows_f and edges == {"left", "right", "top", "bottom"}
    forms = {(c.mode, c.storage) for c in fc.pre_group_cases()}
    assert forms == {(m, s) for m in (fc.NORMAL, fc.MIXED, fc.MONO) for s in (0, 1, 3, 7)}
    assert {(c.mode, c.storage) for c in fc.pre_class_cases()} >= {(m, s) for m in (fc.NORMAL, fc.MIXED, fc.MONO) for s in (0, 7)}
    for c in fc.pre_group_cases():
        assert len({(fc.run_geo(c, m)["W"], fc.run_geo(c, m)["H"]) for m in c.members}) == 1 and len({(m.pf, m.pb) for m in c.members}) == 3
    for c in fc.pre_class_cases():
        ws = sorted(fc.run_geo(c, m)["W"] for m in c.members)
        assert ws[0] < fc.P4_TW and any(w == fc.P4_TW + 1 for w in ws) or ws[0] < 8, ws
    assert any(any(fc.run_geo(c, m)["W"] == fc.P4_TW + 1 for m in c.members) and min(fc.run_geo(c, m)["W"] for m in c.members) < 8 for c in fc.pre_class_cases())
    # the pre-process walk has nothing on the mask's border and nothing beside the ROI: its tests judge the pre-process alone
    for c in fc.pre_solo_cases():
        m, = c.members
        g = fc.run_geo(c, m)
        z = m.c.mask.copy()
        z[g["y0"]:g["y0"] + g["H"], g["x0"]:g["x0"] + g["W"]] = 0
        assert not z.any()


def test_buffers_keep_every_image_inside_guard_bands():
    """One buffer per case; every image GUARD bytes from the buffer's ends and from its neighbours; base address mod 16 = o."""
    for c in fc.scan_cases()[::9] + fc.riding_cases() + fc.group_scan_cases() + fc.erode_cases()["group"] + fc.pre_class_cases() + fc.pre_solo_cases()[::5]:
        plan, n = fc.arena_plan(c)
        spans = []
        for m, offs in zip(c.members, plan):
            for (base, step), img, pl in zip(offs, (m.c.mask, m.c.patch, m.c.dst), (m.pm, m.pf, m.pb)):
                assert base % 4096 == pl.o and pl.o < 16
                spans.append((base, base + img.shape[0] * step))
        spans.sort()
        assert spans[0][0] >= fc.GUARD and n - spans[-1][1] >= fc.GUARD and n % 4096 == 0
        assert all(b[0] - a[1] >= fc.GUARD for a, b in zip(spans, spans[1:]))


def test_restatement_of_a_placed_view_is_the_dense_restatement():
    """The images read back through the placement's strided views, with 0x00 and with 0xFF around them, restate to what the dense content
    restates to: rectangle, eroded mask, right-hand side in every mode."""
    picks = fc.scan_cases()[::23] + fc.riding_cases()[::5] + fc.erode_cases()["solo"][::11] + fc.erode_cases()["tile"][3::13] + fc.erode_cases()["grey"][::7]
    picks += fc.pre_solo_cases()[::6] + fc.pre_solo_cases(fc.MIXED, 1)[1::9] + fc.pre_solo_cases(fc.MONO, 3)[2::9] + fc.pre_class_cases()[::5]
    n = 0
    for c in picks:
        for fill in (0x00, 0xFF):
            buf, plan = fc.build_arena(c, fill)
            for m, offs in zip(c.members, plan):
                vm, vf, vb = fc.views(buf, m, offs)
                assert not vm.flags["C_CONTIGUOUS"] or m.pm.pad == 0
                placed = fc.Content(m.c.key + " placed", vm, vf, vb, m.c.cx, m.c.cy)
                want = fc.expected(c, m)
                assert fc.true_rect(placed) == want["rect"]
                g = fc.run_geo(c, fc.Member(placed, m.pm, m.pf, m.pb, m.guess))
                assert (g is None) == (want["geo"] is None)
                if g is None or not c.fields:
                    continue
                assert np.array_equal(fc.geo_array(g), want["geo"])
                M = fc.restate_M(placed, g, c.grey)
                B, lap = fc.restate_rhs(placed, g, M, c.mode, c.grey)
                assert np.array_equal(M, want["M"]) and np.array_equal(B, want["B"]) and np.array_equal(lap, want["lap"])
                n += 1
    assert n >= 60
