"""CPU checks of the whole-image edits' restatement (tests/photo_edits_np.py) on hand-built images, and of the Python surface
that needs no GPU (the EditParams layout, the constants, the cv2-shaped functions' mask handling)."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from seamlesscloneoptimization_amd import capi, seamless_clone
import photo_edits_np as pe


def _step(H=12, W=20, at=10):
    img = np.zeros((H, W, 3), np.uint8)
    img[:, at:] = 255
    return img


def test_edit_params_layout_and_constants():
    assert ctypes.sizeof(capi.EditParams) == 9 * 4
    assert (capi.SC_EDIT_COLOR_CHANGE, capi.SC_EDIT_ILLUMINATION_CHANGE, capi.SC_EDIT_TEXTURE_FLATTENING) == (1, 2, 3)
    for name in ("sc_hip_edit", "sc_hip_edit_device", "sc_hip_default_edit_params", "sc_hip_edit_rhs", "sc_hip_canny"):
        assert name in capi.declared_symbols()


def test_vertical_step_gives_one_pixel_edge_column():
    cls, edges = pe.canny(_step(at=10), 30, 45, 3)
    cols = np.nonzero(edges.any(axis=0))[0]
    assert list(cols) == [9]
    assert edges[:, 9].all()
    assert (cls[:, 9] == 2).all()


def test_swapped_thresholds_are_the_same():
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (23, 31, 3), dtype=np.uint8)
    for k in (3, 5, 7):
        a = pe.canny_classes(img, 40, 120, k)
        b = pe.canny_classes(img, 120, 40, k)
        assert np.array_equal(a, b)


def test_weak_chain_joined_to_strong_seed_becomes_edge_and_detached_does_not():
    cls = np.zeros((9, 16), np.uint8)
    cls[2, 2:8] = 1
    cls[2, 8] = 2                    # seed at the end of the first chain
    cls[3, 9] = 1                    # diagonal neighbour of the seed: 8-connected
    cls[6, 2:12] = 1                 # a chain that touches no strong pixel
    e = pe.hysteresis(cls)
    assert e[2, 2:9].all() and e[3, 9]
    assert not e[6].any()


def test_aperture_7_saturates():
    img = _step(H=16, W=24, at=12)
    dx, _ = pe.sobel(img[:, :, 0], 7)
    assert dx.max() == 32767
    dx5, _ = pe.sobel(img[:, :, 0], 5)
    assert dx5.max() < 32767


def test_illumination_beta_zero_is_colour_change_identity():
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (30, 40, 3), dtype=np.uint8)
    mask = np.zeros((30, 40), np.uint8)
    mask[5:25, 8:33] = 255
    mask[10:20, 15:20] = 128
    _, lap_c, _ = pe.build_rhs(img, mask, pe.COLOR, red_mul=1.0, green_mul=1.0, blue_mul=1.0)
    _, lap_i, _ = pe.build_rhs(img, mask, pe.ILLUMINATION, alpha=0.7, beta=0.0)
    assert np.array_equal(lap_c, lap_i)


@pytest.mark.parametrize("op", [pe.COLOR, pe.ILLUMINATION, pe.TEXTURE])
def test_empty_mask_solves_back_to_src(op):
    rng = np.random.default_rng(7)
    img = rng.integers(0, 256, (33, 47, 3), dtype=np.uint8)
    out = pe.edit(img, np.zeros((33, 47), np.uint8), op)
    assert np.abs(out.astype(int) - img).max() <= 1


def test_whole_image_erode_ignores_the_outside():
    m = np.full((10, 12), 255, np.uint8)
    assert (pe.erode_whole(m) == 255).all()
    m[5, 6] = 0
    e = pe.erode_whole(m)
    assert (e[2:9, 3:10] == 0).all() and e[0, 0] == 255


def test_colour_change_scales_the_field_inside_the_mask():
    img = np.tile(np.arange(0, 200, 10, dtype=np.uint8)[None, :, None], (16, 1, 3))
    mask = np.zeros((16, 20), np.uint8)
    mask[:, :] = 255
    _, lap, (GX, _) = pe.build_rhs(img, mask, pe.COLOR, red_mul=2.0, green_mul=1.0, blue_mul=0.5)
    assert GX[5, 5, 2] == 20 and GX[5, 5, 1] == 10 and GX[5, 5, 0] == 5
    assert lap[:, 0].max() == 0 and lap[:, -1].max() == 0


def test_three_channel_mask_goes_through_the_grey_formula():
    m3 = np.zeros((4, 5, 3), np.uint8)
    m3[1, 2] = (10, 200, 90)
    g = seamless_clone._edit_mask(m3, (4, 5, 3))
    assert g.shape == (4, 5) and g[1, 2] == pe.grey_bgr(m3)[1, 2] and g[0, 0] == 0
    with pytest.raises(ValueError):
        seamless_clone._edit_mask(np.zeros((4, 6), np.uint8), (4, 5, 3))
