"""Placements and the walk of the front-end alignment sweep (plain data and arithmetic, no GPU).

The front end of a clone -- the bounding-box scan, the erodes, the fused pre-process -- reads the caller's mask, patch and destination
bytes where they lie.  A Case is a launch form of sc_hip_front_end_device with one or more Members; a Member is dense Content (mask,
patch, destination, centre) and one placement (o, pad) per image.  build_arena puts every image of a case into ONE buffer: per image a
4096-aligned region of GUARD bytes, the base offset o, rows `cols * ch + pad` bytes apart, GUARD bytes behind; guard bands and row
padding hold the fill byte (0x00 and 0xFF: "outside" and "inside the mask" to the erode, zero and non-zero to the scan).  The
restatements run on the dense content (oracle_np, oracle_c, clone_modes_np); the geometry models below (scan_a0, erode_shift,
stage_origin ...) restate the kernels' address arithmetic so that tests/test_front_end_alignment_host.py can say from the walk alone
which residues and seams every reader meets.

Which reader a test judges:
  scan   the raw rectangle (device copy = pinned mailbox = bounding_box of the zero-bordered mask), the member's code and geo
  erode  M against three erode3x3 (grey: erode_min7) of the mask bytes of the ROI the launch ran on
  pre    B and lap against build_rhs of the dense content
so a wrong value in one reader fails that reader's tests and no other's: the scan walk alone has non-zero bytes on the mask's border,
the erode walk alone has 255 beside the ROI (all-255 masks, guessed boxes smaller than the mask's), the pre-process walk has neither.
"""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

from oracle import oracle_np

GUARD = 4096
NORMAL, MIXED, MONO = 1, 2, 3
SC_ERR_EMPTY_MASK = -3

# ---- the kernels' tiling (csrc/sc_kernels.hip)
BB_CHUNK, BB_CHUNKS, BB_WG_ROWS = 16, 64, 16            # scan: bytes per lane, lanes per row of a workgroup, rows per workgroup
ER_WAVE, ER_ROWS_SOLO, ER_ROWS_GROUP = 256, 8, 16       # erode: columns per wave, rows per lane solo / in a group
P4_TW, P4_TH = 128, 16                                  # pre-process tile (the in-tile erode's too)
G7_TW, G7_TH = 64, 16                                   # grey erode tile


@dataclass(frozen=True)
class Place:
    o: int
    pad: int


@dataclass
class Content:
    key: str
    mask: np.ndarray        # (mh, mw)
    patch: np.ndarray       # (mh, mw, 3)
    dst: np.ndarray         # (br, bc, 3)
    cx: int
    cy: int
    marks: tuple = ()       # scan: the two extreme pixels (x, y); erode: the holes (x, y) in ROI coordinates


@dataclass
class Member:
    c: Content
    pm: Place
    pf: Place
    pb: Place
    guess: tuple = None     # form 1: the rectangle {x0, x1, y0, y1} the member is launched on

    @property
    def mstep(self):
        return self.c.mask.shape[1] + self.pm.pad

    @property
    def fstep(self):
        return 3 * self.c.patch.shape[1] + self.pf.pad

    @property
    def bstep(self):
        return 3 * self.c.dst.shape[1] + self.pb.pad


@dataclass
class Case:
    reader: str
    form: int
    members: list
    mode: int = NORMAL
    storage: int = 0
    grey: bool = False
    fields: bool = True
    note: str = ""


# ---- geometry ------------------------------------------------------------------------------------------------------------------
def true_rect(c):
    return tuple(int(v) for v in oracle_np.bounding_box(oracle_np.zero_mask_border(c.mask)))


def geo_of(rect, cx, cy):
    """geo_from_rect: None where the rectangle gives no usable ROI."""
    x0, x1, y0, y1 = rect
    if not (x1 - x0 > 0 and y1 - y0 > 0):
        return None
    W, H = x1 - x0 + 1, y1 - y0 + 1
    return dict(x0=x0, y0=y0, W=W, H=H, ltx=cx - (W >> 1), lty=cy - (H >> 1))


def run_geo(case, m):
    """The ROI the launches of `case` run member m on: the guessed box in form 1, else the scan's."""
    return geo_of(m.guess if case.form == 1 else true_rect(m.c), m.c.cx, m.c.cy)


def geo_array(g):
    return np.array([g[k] for k in ("x0", "y0", "W", "H", "ltx", "lty")], np.int32)


def scan_a0(m, y):
    """mask_bbox_block: the row's offset from the 16-byte boundary below it."""
    return (m.pm.o + y * m.mstep) % 16


def scan_grid(mw, mh):
    chunks = (mw + 15 + 15) // 16
    return (chunks + BB_CHUNKS - 1) // BB_CHUNKS, (mh + BB_WG_ROWS - 1) // BB_WG_ROWS


def erode_shift(m, g, y):
    """mask_erode3_block / the ER copy: address mod 4 of byte x - 3 of ROI row y for a lane's x = 0 mod 4."""
    return (m.pm.o + (y + g["y0"]) * m.mstep + g["x0"] - 3) % 4


def stage_origin(o, step, ox, oy, y, tx0):
    """p4_stage: offset of the first staged byte (pixel tx0 - 1 of ROI row y) from the 16-byte boundary below it; the ROI's origin is
    pixel (ox, oy) of an image at base offset o."""
    return (o + (oy + y) * step + 3 * ox + 3 * (tx0 - 1)) % 16


def stage_origins(m, g):
    """{(tile column, staged row y): (body origin, patch origin)} over every tile of the ROI (rows -1 and H are not read)."""
    out = {}
    for tx0 in range(0, g["W"], P4_TW):
        for y in range(g["H"]):
            out[(tx0, y)] = (stage_origin(m.pb.o, m.bstep, g["ltx"], g["lty"], y, tx0), stage_origin(m.pf.o, m.fstep, g["x0"], g["y0"], y, tx0))
    return out


# ---- restatements on the dense content --------------------------------------------------------------------------------------------
def restate_M(c, g, grey=False):
    """The eroded mask of ROI g of the mask's own bytes.  For the scan's ROI this is oracle_np.mask_stage's M (the ROI lies inside the
    zeroed border); for a guessed box it is the erode 'on the guessed crop'."""
    M = np.ascontiguousarray(c.mask[g["y0"]:g["y0"] + g["H"], g["x0"]:g["x0"] + g["W"]])
    if grey:
        return oracle_np.erode_min7(M)
    for _ in range(3):
        M = oracle_np.erode3x3(M)
    return M


def restate_rhs(c, g, M, mode=NORMAL, grey=False):
    """(B, lap) as [3][H][W] float32: oracle_c.build_rhs for NORMAL and grey, clone_modes_np.build_rhs for MIXED and MONOCHROME."""
    if mode == NORMAL or grey:
        from oracle import oracle_c
        return oracle_c.build_rhs(c.dst, c.patch, geo_array(g), M, opencv_grey=grey)
    import clone_modes_np as cm
    B, lap, _ = cm.build_rhs(c.dst, c.patch, dict(g, M=M), mode)
    return np.ascontiguousarray(B.transpose(2, 0, 1)), np.ascontiguousarray(lap.transpose(2, 0, 1))


_memo = {}


def expected(case, m):
    """dict(rect, rc, geo, M, B, lap) of member m under `case`, from the dense content (cached per content, box, mode)."""
    key = (m.c.key, m.guess if case.form == 1 else None, case.mode, case.grey, case.fields)
    if key not in _memo:
        rect = true_rect(m.c)
        g = run_geo(case, m)
        e = dict(rect=rect, rc=0 if geo_of(rect, m.c.cx, m.c.cy) else SC_ERR_EMPTY_MASK, geo=None if g is None else geo_array(g), M=None, B=None, lap=None)
        if case.fields and g is not None:
            e["M"] = restate_M(m.c, g, case.grey)
            e["B"], e["lap"] = restate_rhs(m.c, g, e["M"], case.mode, case.grey)
        _memo[key] = e
    return _memo[key]


# ---- one allocation per case ---------------------------------------------------------------------------------------------------------
def arena_plan(case):
    """Per member [(base, step)] of mask, patch, destination inside the case's buffer, and the buffer's size."""
    cursor, plan = 0, []
    for m in case.members:
        offs = []
        for img, pl, ch in ((m.c.mask, m.pm, 1), (m.c.patch, m.pf, 3), (m.c.dst, m.pb, 3)):
            rows, cols = img.shape[:2]
            step = cols * ch + pl.pad
            base = cursor + GUARD + pl.o
            offs.append((base, step))
            cursor = (base + rows * step + GUARD + 4095) // 4096 * 4096
        plan.append(offs)
    return plan, cursor


def views(buf, m, offs):
    """The member's three images as strided views into buf."""
    mh, mw = m.c.mask.shape
    br, bc = m.c.dst.shape[:2]
    (bm, sm), (bf, sf), (bb, sb) = offs
    return (np.ndarray((mh, mw), np.uint8, buf, bm, (sm, 1)), np.ndarray((mh, mw, 3), np.uint8, buf, bf, (sf, 3, 1)),
            np.ndarray((br, bc, 3), np.uint8, buf, bb, (sb, 3, 1)))


def build_arena(case, fill):
    plan, n = arena_plan(case)
    buf = np.full(n, fill, np.uint8)
    for m, offs in zip(case.members, plan):
        vm, vf, vb = views(buf, m, offs)
        vm[...] = m.c.mask
        vf[...] = m.c.patch
        vb[...] = m.c.dst
    return buf, plan


def describe(case, k, fill=None):
    m = case.members[k]
    g = run_geo(case, m)
    s = "%s form %d mode %d storage %d%s%s, member %d (%s): mask (o %d, pad %d) patch (o %d, pad %d) destination (o %d, pad %d)" % (
        case.reader, case.form, case.mode, case.storage, " grey" if case.grey else "", "" if fill is None else " fill 0x%02X" % fill, k, m.c.key,
        m.pm.o, m.pm.pad, m.pf.o, m.pf.pad, m.pb.o, m.pb.pad)
    s += "; mask %dx%d step mod 16 = %d" % (m.c.mask.shape[1], m.c.mask.shape[0], m.mstep % 16)
    if g:
        s += "; ROI %dx%d at mask (%d, %d), destination (%d, %d); erode address mod 4 = %d, step mod 4 = %d; origins mod 16: patch %d, destination %d" % (
            g["W"], g["H"], g["x0"], g["y0"], g["ltx"], g["lty"], erode_shift(m, g, 0), m.mstep % 4,
            stage_origin(m.pf.o, m.fstep, g["x0"], g["y0"], 0, 1), stage_origin(m.pb.o, m.bstep, g["ltx"], g["lty"], 0, 1))
    return s + ("; " + case.note if case.note else "")


def first_difference(name, got, want):
    """None, or where `got` first differs from `want`: the pixel, its word (4 pixels) and the lane that serves it."""
    if got is None or want is None:
        return None if got is want else "%s: %s" % (name, "missing" if got is None else "not expected")
    if got.shape != want.shape:
        return "%s: shape %s, want %s" % (name, got.shape, want.shape)
    bad = np.argwhere(got != want)
    if not bad.size:
        return None
    idx = tuple(int(v) for v in bad[0])
    y, x = idx[-2], idx[-1]
    return "%s: %d values differ; first at %sx %d y %d: got %s, want %s; word %d (lane %d of a 64-word wave, lane %d of a %d-pixel tile), tile row %d" % (
        name, len(bad), "" if len(idx) == 2 else "channel %d " % idx[0], x, y, got[idx], want[idx], x // 4, (x // 4) % 64, (x % P4_TW) // 4, P4_TW, y % P4_TH)


# ---- contents ------------------------------------------------------------------------------------------------------------------------
def _images(rng, mw, mh, bc, br, blank=False):
    if blank:
        return np.zeros((mh, mw, 3), np.uint8), np.zeros((br, bc, 3), np.uint8)
    return rng.integers(0, 256, (mh, mw, 3), dtype=np.uint8), rng.integers(0, 256, (br, bc, 3), dtype=np.uint8)


SCAN_W = [3, 4, 17, 18, 33, 1009, 1010, 1025, 1040]
SCAN_H = [3, 5, 17, 33, 40]
SCAN_PAD = [0, 1, 3, 7, 13]
SCAN_VALS = [1, 128, 255]


def scan_content(mw, mh, t, kind="two"):
    """A mask that is zero except two pixels (kind 'two'), one ('single'), none ('zero') or all 255 ('full'), with non-zero bytes on
    its four border lines, which the scan must ignore.  marks: the pixels that set (x0, y0) and (x1, y1) -- or (x0, y1) and (x1, y0)."""
    rng = np.random.default_rng(7000 + 31 * t + mw)
    mask = np.zeros((mh, mw), np.uint8)
    xs = sorted({x for x in (1, 2, 14, 15, 16, 17, mw - 3, mw - 2) if 1 <= x <= mw - 2})
    ys = sorted({y for y in (1, 3, 4, 15, 16, mh - 2) if 1 <= y <= mh - 2})
    far = [x for x in (mw - 3, mw - 2, 16, 17) if x in xs]          # the far pixel: against the row's end, or just behind the first chunk
    xa, xb = sorted((xs[t % len(xs)], far[t % len(far)]))
    ya, yb = ys[(t // 2) % len(ys)], ys[(5 * t + 2) % len(ys)]
    marks = ()
    if kind == "two":
        mask[ya, xa], mask[yb, xb] = SCAN_VALS[t % 3], SCAN_VALS[(t + 1) % 3]
        marks = ((xa, ya), (xb, yb))
    elif kind == "single":
        mask[ya, xa] = SCAN_VALS[t % 3]
        marks = ((xa, ya), (xa, ya))
    elif kind == "full":
        mask[:] = 255
    if kind != "full":
        mask[0, :], mask[-1, :] = rng.integers(1, 256, mw), rng.integers(1, 256, mw)
        mask[:, 0], mask[:, -1] = rng.integers(1, 256, mh), rng.integers(1, 256, mh)
    patch, dst = _images(rng, mw, mh, mw + 2, mh + 2, blank=True)
    return Content("scan %s %dx%d #%d" % (kind, mw, mh, t), mask, patch, dst, (mw + 2) // 2, (mh + 2) // 2, marks)


def roi_content(key, W, H, x0=1, y0=1, r=1, b=1, l=2, t=1, dr=3, db=2, holes=(), full=False, grey=False, seed=0):
    """A mask of (x0 + W + r) x (y0 + H + b) pixels that is 255 on the ROI [x0, x0 + W) x [y0, y0 + H) -- everywhere with `full`, grey
    values 1..254 with `grey` -- and zero elsewhere, with holes (x, y, value) in ROI coordinates; a random patch; a random destination
    with l / dr columns and t / db rows around the ROI."""
    rng = np.random.default_rng(9000 + seed)
    mw, mh = x0 + W + r, y0 + H + b
    mask = np.full((mh, mw), 255, np.uint8) if full else np.zeros((mh, mw), np.uint8)
    mask[y0:y0 + H, x0:x0 + W] = rng.integers(1, 255, (H, W), dtype=np.uint8) if grey else 255
    for x, y, v in holes:
        mask[y0 + y, x0 + x] = v
    patch, dst = _images(rng, mw, mh, l + W + dr, t + H + db)
    return Content(key, mask, patch, dst, l + (W >> 1), t + (H >> 1), tuple((x, y) for x, y, _ in holes))


# ---- the scan's walk -------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def scan_cases():
    cases = []
    configs = [(mw, SCAN_H[i % 5]) for i, mw in enumerate(SCAN_W)]
    for i, (mw, mh) in enumerate(configs):
        c = scan_content(mw, mh, i)
        for o in range(16):
            pl = Place(o, SCAN_PAD[(o + i) % 5])
            cases.append(Case("scan", 0, [Member(c, pl, Place(0, 0), Place(0, 0))], fields=False))
    for i, (mw, mh) in enumerate([(1040, 40), (1010, 33), (1009, 3), (3, 40), (18, 17), (1025, 5)], 20):
        c = scan_content(mw, mh, i)
        for o in (1, 6, 11, 15):
            cases.append(Case("scan", 0, [Member(c, Place(o, SCAN_PAD[(o + i) % 5]), Place(0, 0), Place(0, 0))], fields=False))
    for i, kind in enumerate(("zero", "single", "full"), 40):
        for j, (mw, mh) in enumerate([(17, 5), (1010, 17), (33, 33)]):
            c = scan_content(mw, mh, i + 3 * j, kind)
            for o, pad in ((5, 3), (15, 13)):
                cases.append(Case("scan", 0, [Member(c, Place(o, pad), Place(0, 0), Place(0, 0))], fields=False, note=kind))
    return cases


RIDE_W = {1: 100, 2: 200, 3: 259}          # tile grids 1, 2, 3 wide: the guessed box's width
RIDE_MH = {1: 12, 2: 20, 5: 70}            # scans of 1, 2, 5 workgroups: the mask's height


@lru_cache(maxsize=None)
def riding_cases():
    """Form 1: the scan as extra workgroup rows of the pre-process launch, on a right guess and on one a column short."""
    cases = []
    for gi, (gx, W) in enumerate(RIDE_W.items()):
        for si, (nb, mh) in enumerate(RIDE_MH.items()):
            mw = W + 2
            c = roi_content("ride %dx%d" % (mw, mh), W, mh - 2, seed=100 + 3 * gi + si)
            c.mask[0, :] = c.mask[-1, :] = 77          # border bytes the scan ignores
            c.mask[:, 0] = c.mask[:, -1] = 200
            rect = (1, mw - 2, 1, mh - 2)
            for k, guess in enumerate((rect, (1, mw - 3, 1, mh - 2))):
                q = 4 * gi + 2 * si + k
                cases.append(Case("scan", 1, [Member(c, Place((5 * q + 1) % 16, SCAN_PAD[q % 5]), Place((3 * q) % 16, q % 4), Place((7 * q + 2) % 16, (q + 1) % 4), guess)],
                                  note="tile grid %d wide, scan of %d workgroups, %s guess" % (gx, nb, "wrong" if k else "right")))
    return cases


@lru_cache(maxsize=None)
def group_scan_cases():
    cases = []
    for rep in range(2):          # three masks of one size at three placements
        for i, (mw, mh) in enumerate([(33, 17), (1010, 33), (18, 5)]):
            ms = [Member(scan_content(mw, mh, 60 + 3 * i + k), Place((5 * k + 3 * rep + i) % 16, SCAN_PAD[(k + rep) % 5]), Place(0, 0), Place(0, 0)) for k in range(3)]
            cases.append(Case("scan", 2, ms, fields=False, note="three masks of one size"))
    for rep in range(2):          # seventeen masks of differing sizes: a second launch, workgroups outside the smaller masks' grids
        ms = [Member(scan_content(SCAN_W[(i + rep) % 9], SCAN_H[(2 * i + rep) % 5], 80 + i, "two" if i % 6 else "full"), Place((7 * i + rep) % 16, SCAN_PAD[(i + rep) % 5]), Place(0, 0), Place(0, 0))
              for i in range(17)]
        cases.append(Case("scan", 2, ms, fields=False, note="seventeen masks of differing sizes"))
    return cases


# ---- the erodes' walk ------------------------------------------------------------------------------------------------------------------
ER_SIZES = list(zip([7, 8, 9, 255, 256, 257, 260], [7, 8, 9, 32, 33, 64, 65])) + [(260, 7), (7, 65), (257, 33), (256, 65), (9, 32)]
ER_PLACES = 8


def _holes(W, H, k):
    """One (small ROIs) or three single non-255 pixels (values 254 and 0) of case k: ring distances 2, 3, 4 from each side, and both sides of every
    word (4), wave (256), strip (8, 16, 32, 64 rows) and tile (128 x 16) seam the ROI has."""
    xs = sorted({x for x in (2, 3, 4, W - 5, W - 4, W - 3, 7, 8, 127, 128, 255, 256) if 2 <= x <= W - 3})
    ys = sorted({y for y in (2, 3, 4, H - 5, H - 4, H - 3, 7, 8, 15, 16, 31, 32, 63, 64) if 2 <= y <= H - 3})
    n = 1 if min(W, H) < 32 else 3
    return tuple((xs[(3 * k + 5 * i) % len(xs)], ys[(2 * k + 3 * i + 1) % len(ys)], (254, 0)[(k + i) % 2]) for i in range(n))


@lru_cache(maxsize=None)
def erode_members():
    """ER_PLACES members per ROI size.  Even k: an all-255 mask (the border too: the columns beside the ROI are 255, which is what makes
    the ring test at the ROI's right edge visible; x0 = y0 = 1 and x0 + W = mw - 1, y0 + H = mh - 1); odd k: the ROI inside a zero
    mask with margins.  (o + x0) mod 4 and step mod 4 take every residue over a size's members."""
    out = {}
    for s, (W, H) in enumerate(ER_SIZES):
        ms = []
        for k in range(ER_PLACES):
            full = k % 2 == 0
            x0, y0, r, b = (1, 1, 1, 1) if full else ((2, 3, 4, 6)[(k // 2 + s) % 4], (2, 5, 1, 3)[(k // 2) % 4], (1, 2, 5, 1)[(k // 2 + s) % 4], (1, 3, 1, 2)[(k // 2) % 4])
            c = roi_content("erode %dx%d #%d%s" % (W, H, k, " all-255" if full else ""), W, H, x0, y0, r, b, holes=() if k == 0 else _holes(W, H, k + s + 1), full=full, seed=200 + 8 * s + k)
            mw = x0 + W + r
            want_step = (k + s) % 4                      # step mod 4
            pad = (want_step - mw) % 4 + (4 if k >= 6 else 0)
            o = ((k // 2 + k + s) - x0) % 4 + 4 * ((k + s) % 4)
            ms.append(Member(c, Place(o, pad), Place((3 * k + s) % 16, (k + 1) % 4), Place((5 * k + 2 * s + 1) % 16, (k + 2) % 4)))
        out[(W, H)] = ms
    return out


@lru_cache(maxsize=None)
def erode_cases():
    members = erode_members()
    solo = [Case("erode", 0, [m]) for ms in members.values() for m in ms]
    # in the tile: launched on the mask's interior (all-255 masks: the library's own guess) and on a box one column and one row short
    tile = []
    for (W, H), ms in members.items():
        for k, m in enumerate(ms):
            mh, mw = m.c.mask.shape
            g = geo_of(true_rect(m.c), m.c.cx, m.c.cy)
            x0, x1, y0, y1 = g["x0"], g["x0"] + W - 1, g["y0"], g["y0"] + H - 1
            guess = (x0, x1, y0, y1) if k % 4 < 2 or W < 9 or H < 9 else (x0 + (k // 4), x1 - 1, y0, y1 - (k // 4))
            tile.append(Case("erode", 1, [Member(m.c, m.pm, m.pf, m.pb, guess)], note="guess %s" % (guess,)))
    group = []
    for (W, H), ms in members.items():
        group.append(Case("erode", 2, [ms[0], ms[2], ms[6]], note="three all-255 masks, one ROI size"))
        group.append(Case("erode", 2, [ms[5], ms[3], ms[7], ms[1]], note="four members of one ROI size"))
    for a, b, c in ((0, 3, 6), (1, 4, 10), (7, 2, 5), (8, 9, 11)):
        sz = [ER_SIZES[a], ER_SIZES[b], ER_SIZES[c]]
        group.append(Case("erode", 3, [members[z][(2 * i + a) % ER_PLACES] for i, z in enumerate(sz)], note="size class %s" % (sz,)))
    grey = []
    for s, (W, H) in enumerate([(130, 33), (65, 17), (9, 9), (64, 16), (129, 32)]):
        for k in range(4):
            c = roi_content("grey %dx%d #%d" % (W, H, k), W, H, (1, 2, 3, 4)[k], (1, 2, 1, 3)[k], (1, 3, 2, 1)[k], (1, 1, 2, 1)[k], grey=True, seed=400 + 4 * s + k)
            grey.append(Case("erode", 0, [Member(c, Place((5 * k + s) % 16, (k + s) % 4), Place((3 * k + 1) % 16, k % 4), Place((7 * k + s) % 16, (k + 2) % 4))], grey=True))
    return dict(solo=solo, tile=tile, group=group, grey=grey)


# ---- the pre-process's walk ------------------------------------------------------------------------------------------------------------
PRE_W = [3, 4, 5, 127, 128, 129, 130, 257, 259]
PRE_H = [3, 15, 16, 17, 33]
PRE_SIZES = [(w, PRE_H[i % 5]) for i, w in enumerate(PRE_W)] + [(130, 33), (259, 33), (4, 16), (128, 15), (129, 17)]
PRE_PAD = [0, 1, 2, 3, 5, 11]
PRE_PLACES = 4


@lru_cache(maxsize=None)
def pre_members():
    """PRE_PLACES members per ROI size; member q of the walk has (o_face + 3 x0) mod 16 = 5 q and (o_body + 3 ltx) mod 16 = 7 q + 3 + size,
    so each residue class is met independently of the other; the ROI touches the destination's left / right / top / bottom edge in turn."""
    out = {}
    for s, (W, H) in enumerate(PRE_SIZES):
        ms = []
        for k in range(PRE_PLACES):
            q = PRE_PLACES * s + k
            l, dr = ((0, 3), (2, 0), (5, 1), (0, 0))[k]
            t, db = ((1, 0), (0, 2), (0, 0), (2, 1))[(k + s) % 4]
            x0, y0, r, b = (1, 2, 3, 4)[(k + s) % 4], (1, 3, 1, 2)[k], (1, 2, 1, 3)[k], (1, 1, 2, 1)[(k + s) % 4]
            holes = _holes(W, H, k + s + 1) if min(W, H) >= 9 else ()
            c = roi_content("pre %dx%d #%d" % (W, H, k), W, H, x0, y0, r, b, l, t, dr, db, holes=holes, seed=600 + q)
            pf = Place((5 * q - 3 * x0) % 16, PRE_PAD[q % 6])
            pb = Place((7 * q + 3 + s - 3 * l) % 16, PRE_PAD[(q + 2) % 6])
            ms.append(Member(c, Place((3 * q + 1) % 16, q % 4), pf, pb))
        out[(W, H)] = ms
    return out


def pre_solo_cases(mode=NORMAL, storage=0, grey=False):
    return [Case("pre", 0, [m], mode, storage, grey) for ms in pre_members().values() for m in ms]


PRE_GROUP_FORMS = [(NORMAL, 0), (MIXED, 1), (MONO, 3), (NORMAL, 7), (MIXED, 0), (MONO, 1), (NORMAL, 3), (MIXED, 7), (MONO, 0), (NORMAL, 1), (MIXED, 3), (MONO, 7), (NORMAL, 7)]
PRE_CLASSES = [[(5, 16), (129, 17), (127, 17)], [(4, 15), (129, 3), (257, 16)], [(3, 3), (130, 33), (128, 15)], [(259, 17), (4, 16), (129, 17)]]


def pre_group_cases():
    """Form 2: three members of one size at three placements, every mode and storage word in turn."""
    members = pre_members()
    return [Case("pre", 2, [ms[(i + k) % PRE_PLACES] for k in range(3)], *PRE_GROUP_FORMS[i % len(PRE_GROUP_FORMS)]) for i, ms in enumerate(members.values())]


def pre_class_cases():
    """Form 3: size classes of three sizes -- one member smaller than a tile, one a tile's width plus one -- in every mode and storage word."""
    members = pre_members()
    cases = []
    for i, sizes in enumerate(PRE_CLASSES):
        for j in range(3):
            mode, storage = PRE_GROUP_FORMS[(3 * i + j) % len(PRE_GROUP_FORMS)]
            cases.append(Case("pre", 3, [members[z][(i + j + k) % PRE_PLACES] for k, z in enumerate(sizes)], mode, storage, note="size class %s" % (sizes,)))
    return cases
