"""The walk of the multigrid cycle's tile seams: the shapes, the regime each is there for, the inputs and the budgets
(tests/test_gpu_mg_cycles.py runs them on the device, tests/test_mg_cycles_host.py pins every shape to its regime through
sc_hip_cycle0_plan and checks that the bounds of tests/mg_cycle_bounds.py are sharp).

Sizes are FIELD sizes, ring included, as the field hooks and k_cycle0's Uin.W take them.  A level-0 tile owns 232 columns
(256 - 2 x 12 halo columns) and 64 - 2 (2 T + 2) rows: 52 for the launches of two sweeps (the first launch, a judged cycle), 44 for
the full cycle's four.  Every number below was read off capi.cycle0_plan (the functions the kernel and its launcher evaluate) and
oracle/mg_np.py's ladder, and the host test holds the two against each other shape by shape.

Classes (SHAPES: name -> (class, W, H)):
  last_cols_1      one column seam, a last column tile of 1 .. 5 columns                                    W = 233 .. 237
  last_cols_2      two column seams, the same                                                               W = 465 .. 469
  whole_tiles      a whole number of column tiles, and one column short                                     W = 231, 232, 463, 464
  inner_cols       the wave-uniform `inner` test (restated for the host beside cycle0_plan, csrc/sc_cycle0.hip) of column tile 1 on both sides of each of its three
                   column conditions: 476 fails level 0's (xw + 255 <= W - 2), 477 meets it with equality and fails level 1's, 478 meets
                   level 1's with equality and fails level 2's, 479 meets all three (level 2's with equality).  H = 60 has wave rows that
                   pass every row condition, so at 479 some waves take the mask-free forms and at 476 .. 478 none does
  level1_seams     level 1's own launch at its column seam: level-1 fields of 232 (W = 462: one whole tile, nothing packed), 233, 236 and 237
                   columns (W = 464, 470, 472: a last column tile of 1, 4, 5 columns, which sc_hip_coarse_tile_plan packs)
  last_rows        the row seams with W = 236: heights 44 .. 48 and 52 .. 56 (one seam at the 44- and the 52-row step, a last row tile of 0 .. 4
                   rows), 88 .. 91 and 104 .. 107 (two seams)
  inner_rows       the row conditions of `inner` with W = 482: wave 2 of row tile 1 in a full cycle (rows 50 .. 57) fails y0 + R - 1 <= H - 2 at
                   H = 58, meets it with equality at 59 and fails level 1's last-row condition there, meets that with equality at 60 and
                   fails level 2's, which 66 fails and 67 meets with equality.  (y0 >= 1 depends on the wave alone: y0 = -10 + 8 wave is even,
                   waves 0 and 1 of the first row tile fail it at every height, and so does every shape here)
  hierarchy        both sides of the ladder's decisions: a level >= 2 with 127 unknowns (512: the tail level is 2) and with 128 (516: it is 3);
                   level 1 with 64 unknowns (131: solved directly, nothing composed) and with 65 (132: smoothed on the composed schedule with
                   the tail pair below); 96 and 97 (195, 196: composed both -- the numpy spec solved level 1 directly up to 96 until this walk);
                   a thin ROI without a direct level (300 x 9); 60 x 236: the transposed ladder
  both_seams       482 x 106: seams in both directions and waves that take the mask-free forms
coarsen_1d's three branches at levels 0, 1 and 2 are reached by the union of the shapes (level 0 has a last interval of exactly one
spacing, so only two of them exist there); the host test lists which shape reaches which.

Budgets: n = 1 and n = 2 cycles on every shape; n = 3 on the shapes of N3 (one per class at least: the sharpness condition of the host test
decides which).  n = 1 judges every channel of a clone, n = 2 and n = 3 one, rotating with the shape."""
import functools

import numpy as np

SMALL = 60

SHAPES = {}
for _w in (233, 234, 235, 236, 237):
    SHAPES["cols_%d" % _w] = ("last_cols_1", _w, SMALL)
for _w in (465, 466, 467, 468, 469):
    SHAPES["cols_%d" % _w] = ("last_cols_2", _w, SMALL)
for _w in (231, 232, 463):
    SHAPES["cols_%d" % _w] = ("whole_tiles", _w, SMALL)
SHAPES["cols_464"] = ("whole_tiles", 464, SMALL)            # ... and level 1's field of 233 columns (level1_seams)
for _w in (476, 477, 478, 479):
    SHAPES["cols_%d" % _w] = ("inner_cols", _w, SMALL)
for _w in (462, 470, 472):
    SHAPES["cols_%d" % _w] = ("level1_seams", _w, SMALL)
for _h in (44, 45, 46, 47, 48, 52, 53, 54, 55, 56, 88, 89, 90, 91, 104, 105, 106, 107):
    SHAPES["rows_%d" % _h] = ("last_rows", 236, _h)
for _h in (58, 59, 60, 66, 67):
    SHAPES["inner_rows_%d" % _h] = ("inner_rows", 482, _h)
for _w, _h in ((512, SMALL), (516, SMALL), (131, SMALL), (132, SMALL), (195, SMALL), (196, SMALL), (300, 9), (SMALL, 236)):
    SHAPES["ladder_%dx%d" % (_w, _h)] = ("hierarchy", _w, _h)
SHAPES["both_482x106"] = ("both_seams", 482, 106)
NAMES = list(SHAPES)
CLASSES = sorted({c for c, _, _ in SHAPES.values()})

LEVEL1_SEAMS = {"cols_462": (232, False), "cols_464": (233, True), "cols_470": (236, True), "cols_472": (237, True)}      # level-1 field width, packed

# the column / row tile sizes the classes are built on (asserted against the plan hook)
XSTEP, YSTEP = 232, {2: 52, 4: 44}

# name -> the first failing condition (capi.CYCLE0_INNER) of column tile 1's waves in a full composed cycle (sweeps 4), as a set over the waves
# that pass every row condition somewhere in the launch; "inner": some wave takes the mask-free forms
INNER_COLS = {"cols_476": "x_last", "cols_477": "l1_x", "cols_478": "l2_x", "cols_479": "inner"}
# name -> verdict of wave 2 of row tile 1, column tile 1, in a full composed cycle
INNER_ROWS = {"inner_rows_58": "y_last", "inner_rows_59": "l1_y_last", "inner_rows_60": "l2_y", "inner_rows_66": "l2_y", "inner_rows_67": "inner"}

# the shapes that also run three cycles (tests/test_mg_cycles_host.py: each is sharp there), one per class at least
N3 = ("cols_236", "cols_468", "cols_463", "cols_479", "cols_470", "rows_47", "rows_90", "inner_rows_59", "ladder_516x60", "ladder_132x60", "both_482x106")


def shape(name):
    return SHAPES[name][1], SHAPES[name][2]


def budgets(name):
    return (1, 2, 3) if name in N3 else (1, 2)


def channels(name, n):
    """the channels of a clone judged after n cycles: all at n = 1, one -- rotating with the shape -- after that"""
    return (0, 1, 2) if n == 1 else ((NAMES.index(name) + n) % 3,)


def coarsen_branch(n, a):
    """which branch of coarsen_1d (oracle/mg_np.py, csrc/sc_mg_levels.cpp) a direction with n unknowns and last interval a takes"""
    return "odd" if n % 2 == 1 else "even_keep" if a >= 1.0 else "even_drop"


def branches(name):
    """{(level, direction): branch} for levels 0, 1, 2 of the shape's ladder, where the level is coarsened at all"""
    from oracle import mg_np
    W, H = shape(name)
    out = {}
    for l, (dx, dy) in enumerate(mg_np.build_levels(W, H)[:3]):
        if dx.nc > 0:
            out[l, "x"] = coarsen_branch(dx.n, dx.alpha)
            out[l, "y"] = coarsen_branch(dy.n, dy.alpha)
    return out


@functools.lru_cache(maxsize=None)
def noise_fields(name):
    """route (a): the noise fields of test_multigrid_cycles_follow_the_spec, one plane (U with its ring, F zero on the ring)"""
    W, H = shape(name)
    rng = np.random.default_rng(W)
    U = rng.uniform(0, 255, (1, H, W)).astype(np.float32)
    F = np.zeros((1, H, W), np.float32)
    F[:, 1:-1, 1:-1] = rng.normal(0, 30, (1, H - 2, W - 2)).astype(np.float32)
    U.setflags(write=False); F.setflags(write=False)
    return U, F


MARGIN = 16


@functools.lru_cache(maxsize=None)
def clone_inputs(name):
    """routes (b) and (c): a clone whose initial error is smooth and large, so that the second cycle still moves the field -- a flat
    destination (128, noise sigma 4), a patch of one long wave (127 + 110 sin(2.3 pi x / W + 0.4) cos(1.7 pi y / H + 0.9), noise sigma 6), the
    mask all 255.  Returns (dst, patch, mask, cx, cy, B, lap, (ltx, lty)): B the initial field with its Dirichlet ring and lap the right-hand
    side, 3 x H x W float32 each, from oracle_np.mask_stage and build_rhs; (ltx, lty) the ROI's corner in the destination."""
    from oracle import oracle_np
    W, H = shape(name)
    rng = np.random.default_rng([W, H, 11])
    Hd, Wd = H + MARGIN, W + MARGIN
    dst = np.clip(128.0 + rng.normal(0.0, 4.0, (Hd, Wd, 3)), 0, 255).astype(np.uint8)
    yy, xx = np.mgrid[0:H + 2, 0:W + 2]
    wave = 127.0 + 110.0 * np.sin(2.3 * np.pi * xx / W + 0.4) * np.cos(1.7 * np.pi * yy / H + 0.9)
    patch = np.clip(wave[:, :, None] + rng.normal(0.0, 6.0, (H + 2, W + 2, 3)), 0, 255).astype(np.uint8)
    mask = np.full((H + 2, W + 2), 255, np.uint8)
    cx, cy = Wd // 2, Hd // 2
    geo = oracle_np.mask_stage(mask, cx, cy)
    assert (geo["W"], geo["H"]) == (W, H), (geo["W"], geo["H"], W, H)
    B, lap = oracle_np.build_rhs(dst, patch, geo)[:2]
    B = np.ascontiguousarray(np.moveaxis(B, 2, 0), np.float32)
    lap = np.ascontiguousarray(np.moveaxis(lap, 2, 0), np.float32)
    for a in (dst, patch, mask, B, lap):
        a.setflags(write=False)
    return dst, patch, mask, cx, cy, B, lap, (geo["ltx"], geo["lty"])
