"""The column tiling of the coarse multigrid launches (coarse_tile_plan, csrc/sc_common.h), through the GPU-free lookup
sc_hip_coarse_tile_plan: the same two functions the launchers size their grids with and the kernels decode their workgroup number with.

Where the last column tile of a level needs at most half a wave, one workgroup serves that tile of K planes, a slot of 64 / K lanes each.
For every field width 3 .. 4200, plane counts 1, 2, 3, 5, 9, 48, 96 and both kernels' (useful width, halo) -- (232, 12) on the way down
(k_cycle0's coarse forms), (248, 4) on the way up (k_rb_tb's) --
  * every (row tile, plane, column) is owned by exactly one (workgroup, lane), and that lane is not a halo lane of its slot;
  * every slot carries at least `halo` columns beyond the columns it owns on each side that has a neighbouring tile;
  * the launch never has more workgroups than the unpacked tiling, and exactly as many where nothing is packed (K < 2), for a size
    class and when the unpacked tiling is asked for (SC_LEGACY_UNPACKED_TILES);
  * slot origins are multiples of 4 (float4 loads)."""
import numpy as np
import pytest

from seamlesscloneoptimization_amd import capi

KERNELS = ((232, 12), (248, 4))
ROWS = 36           # rows a tile owns: 8 waves of 6 rows at depth 2 on the way down
PLANES = (1, 2, 3, 5, 9, 48, 96)


def check(W, C, uw, hx, H):
    nbx, nby, hq = -(-W // uw), -(-H // ROWS), hx // 4
    unpacked = capi.coarse_tile_plan(W, H, C, uw, hx, ROWS, unpacked=True)
    assert unpacked == (nbx, 64, 1, nbx * nby * C), (W, C, uw, unpacked)
    assert capi.coarse_tile_plan(W, H, C, uw, hx, ROWS, size_class=True) == unpacked, (W, C, uw)
    (full, lps, K, blocks), (by, wlps, plane, x) = capi.coarse_tile_plan(W, H, C, uw, hx, ROWS, lanes=True)
    assert by.shape == (blocks,) and x.shape == (blocks, 64)
    assert blocks <= unpacked[3] and (K >= 2 or blocks == unpacked[3]), (W, C, uw, blocks, unpacked)
    assert blocks == nby * (full * C + (nbx - full) * -(-C // K)) and full in (nbx, nbx - 1) and (full == nbx) == (K == 1), (W, C, uw)
    assert K * lps == 64 and by.shape == (blocks,), (W, C, uw, K, lps)
    # the lanes the residue tile needs, halos included; it is packed exactly when they fit half a wave, into the smallest power of two
    need = -(-(W - (nbx - 1) * uw + 2 * hx) // 4)
    spans = []
    assert (K >= 2) == (need <= 32) and (K == 1 or lps // 2 < need <= lps), (W, C, uw, need, lps)
    # a workgroup is 64 / wlps slots of wlps lanes: one plane per slot (the first one real), 4 columns per lane from the slot's origin
    assert ((wlps == 64) | (wlps == lps)).all(), (W, C, uw)
    for n in np.unique(wlps):
        w = wlps == n
        xs, ps = x[w].reshape(-1, 64 // n, n), plane[w].reshape(-1, 64 // n, n)
        assert (xs == xs[:, :, :1] + 4 * np.arange(n)).all() and (xs[:, :, 0] % 4 == 0).all(), (W, C, uw, n)
        assert (ps == ps[:, :1, :1] + np.arange(64 // n)[None, :, None]).all() and (ps[:, 0, 0] >= 0).all() and (ps[:, 0, 0] < C).all(), (W, C, uw, n)
        # what a slot owns: its lanes but the first and last hq, as far as the field goes; nothing of it lies left of the field
        org, pl, row = xs[:, :, 0].ravel(), ps[:, :, 0].ravel(), np.repeat(by[w], 64 // n)
        lo, hi = org + hx, np.minimum(org + 4 * (n - hq), W)
        live = (pl < C) & (hi > lo)
        assert (lo >= 0).all(), (W, C, uw, n)
        spans.append(np.stack([row[live] * C + pl[live], lo[live], hi[live]], axis=1))
        # halos: hx columns left of the first owned column unless that is column 0 (always: lo - org), and hx columns right of the last
        # owned one unless that is the ring column W - 1
        assert ((lo == 0) | (lo - org >= hx)).all() and ((hi == W) | (org + 4 * n - hi >= hx)).all(), (W, C, uw, n)
    # every (row tile, plane) is covered by its spans exactly once: sorted, they tile [0, W)
    t = np.concatenate(spans)
    t = t[np.lexsort((t[:, 1], t[:, 0]))]
    first = np.r_[True, t[1:, 0] != t[:-1, 0]]
    last = np.r_[first[1:], True]
    assert (np.unique(t[:, 0]) == np.arange(nby * C)).all(), (W, C, uw)
    assert (t[first, 1] == 0).all() and (t[last, 2] == W).all() and (t[1:, 1][~first[1:]] == t[:-1, 2][~last[:-1]]).all(), (W, C, uw)


@pytest.mark.parametrize("uw,hx", KERNELS)
@pytest.mark.parametrize("C", PLANES)
def test_every_column_has_one_owner(C, uw, hx):
    for W in range(3, 4201):
        check(W, C, uw, hx, ROWS + 1 if C <= 9 else ROWS)         # two row tiles where that stays cheap


def test_flagship_levels():
    """The plans the issue's table lists for a 2048^2 ROI in groups of 16 (48 planes): level widths 1025, 513, 257."""
    down = lambda W, rows: capi.coarse_tile_plan(W, W, 48, 232, 12, rows)
    up = lambda W, rows: capi.coarse_tile_plan(W, W, 48, 248, 4, rows)
    assert down(1025, 76)[:3] == (4, 32, 2) and down(513, 36)[:3] == (2, 32, 2) and down(257, 36)[:3] == (1, 16, 4)
    assert up(513, 40)[:3] == (2, 8, 8) and up(257, 40)[:3] == (1, 8, 8)
    assert down(1025, 76)[3] == 14 * (4 * 48 + 24) and up(257, 40)[3] == 7 * (48 + 6)


def test_bad_facts_are_refused():
    for bad in (dict(W=0), dict(C_=0), dict(useful=200), dict(halo=6), dict(rows=0)):
        kw = dict(W=100, H=100, C_=3, useful=232, halo=12, rows=36)
        kw.update(bad)
        with pytest.raises(capi.SeamlessCloneError):
            capi.coarse_tile_plan(**kw)
