"""Whole-image gradient edits on the MI355X (sc_hip_edit: cv::colorChange, cv::illuminationChange, cv::textureFlattening).

PARITY UNPINNED: OpenCV is not available to compare against and the reference has no fixture of these functions; the library is
checked against the restatement in tests/photo_edits_np.py -- Canny's class and edge maps, the eroded mask and the right-hand
side of colour change and texture flattening bit for bit, illumination change's right-hand side within powf's error, whole
edits within one grey level -- and tied to itself by identities."""
import ctypes
import os

import numpy as np
import pytest

import photo_edits_np as pe

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _jpg(name):
    from PIL import Image
    return np.ascontiguousarray(np.asarray(Image.open(os.path.join(GOLDEN, name)).convert("RGB"))[:, :, ::-1])


def _rand(W, H, seed):
    """A smooth random image with some texture: gradients of every size, edges of every strength."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = 128 + 60 * np.sin(xx / 7.0 + seed)[:, :, None] * np.cos(yy / 5.0)[:, :, None] * np.array([1.0, 0.6, -0.8])
    img = base + rng.normal(0, 18, (H, W, 3))
    img[(xx // 9 + yy // 7) % 5 == 0] += 70
    return np.clip(img, 0, 255).astype(np.uint8)


def _ellipse(W, H, cx=None, cy=None, a=None, b=None, value=255):
    yy, xx = np.mgrid[0:H, 0:W]
    cx = W / 2 if cx is None else cx
    cy = H / 2 if cy is None else cy
    a = W / 3 if a is None else a
    b = H / 3 if b is None else b
    m = np.zeros((H, W), np.uint8)
    m[((xx - cx) / a) ** 2 + ((yy - cy) / b) ** 2 <= 1] = value
    return m


def _dmax(a, b):
    return int(np.abs(a.astype(np.int16) - b.astype(np.int16)).max())


def _off_by_one(a, b):
    return int((np.abs(a.astype(np.int16) - b.astype(np.int16)) == 1).sum())


@pytest.fixture(scope="module")
def inst():
    from seamlesscloneoptimization_amd import capi
    i = capi.Instance(0)
    yield i
    i.destroy()


def _new(**solver):
    from seamlesscloneoptimization_amd import capi
    i = capi.Instance(0)
    if solver:
        i.set_solver(**solver)
    return i


# ---- Canny ------------------------------------------------------------------------------------------------------------------------
CANNY_IMAGES = ["r9x8", "r37x29", "r131x45", "airplane.jpg", "sky.jpg"]
THRESHOLDS = [(30, 45), (120, 40), (60.7, 60.2), (0, 0)]
_IMG_CACHE = {}


def _image(name):
    if name not in _IMG_CACHE:
        if name.endswith(".jpg"):
            _IMG_CACHE[name] = _jpg(name)
        else:
            W, H = (int(v) for v in name[1:].split("x"))
            _IMG_CACHE[name] = _rand(W, H, W * 7 + H)
    return _IMG_CACHE[name]


@pytest.mark.parametrize("name", CANNY_IMAGES)
@pytest.mark.parametrize("k", [3, 5, 7])
@pytest.mark.parametrize("low,high", THRESHOLDS)
def test_canny_maps_are_bit_exact(inst, name, k, low, high):
    img = _image(name)
    cls, edges, counts = inst.canny(img, low, high, k)
    want_cls, want_edges = pe.canny(img, low, high, k)
    assert np.array_equal(cls, want_cls), int((cls != want_cls).sum())
    assert np.array_equal(edges, want_edges), int((edges != want_edges).sum())
    assert counts[0] >= 4 and counts[1] >= 1


def test_canny_flat_image(inst):
    img = np.full((50, 70, 3), 77, np.uint8)
    for k in (3, 5, 7):
        cls, edges, _ = inst.canny(img, 0, 0, k)
        assert not cls.any() and not edges.any()


def test_canny_padded_step(inst):
    img = _rand(83, 41, 5)
    wide = np.zeros((41, 100, 3), np.uint8)
    wide[:, :83] = img
    cls, edges, _ = inst.canny(wide[:, :83], 20, 90, 5)
    want_cls, want_edges = pe.canny(img, 20, 90, 5)
    assert np.array_equal(cls, want_cls) and np.array_equal(edges, want_edges)


def _serpentine(W=700, H=420, pitch=24, band=8):
    """A snake-shaped band of grey 40 on black crossing the image back and forth; one end of it is white.  Its boundary is a long
    chain of weak pixels (magnitude 160 at aperture 3) with strong ones (> 1000) only near the white end."""
    img = np.zeros((H, W, 3), np.uint8)
    rows = list(range(10, H - band - 10, pitch))
    for i, y in enumerate(rows):
        img[y:y + band, 10:W - 10] = 40
        if i + 1 < len(rows):
            x = W - 10 - band if i % 2 == 0 else 10
            img[y:rows[i + 1] + band, x:x + band] = 40
    img[rows[0]:rows[0] + band, 10:40] = 255
    return img


def test_hysteresis_runs_several_rounds_across_many_tiles(inst):
    img = _serpentine()
    cls, edges, counts = inst.canny(img, 100, 600, 3)
    want_cls, want_edges = pe.canny(img, 100, 600, 3)
    assert np.array_equal(cls, want_cls)
    assert np.array_equal(edges, want_edges), int((edges != want_edges).sum())
    # the chain's far end is reached: edge pixels in the last band, hundreds of tiles away from the seed
    assert edges[-60:].any()
    assert (want_cls == 2).sum() < (want_edges > 0).sum() // 10
    assert counts[1] >= 2, counts           # more than one batch of launches
    print("serpentine: %d hysteresis launches, %d mailbox reads" % counts)


# ---- the eroded mask and the right-hand side -----------------------------------------------------------------------------------
def _masks(W, H):
    out = {}
    m = np.zeros((H, W), np.uint8)
    m[: H // 2, : W // 3] = 255                       # touches the top and left edges and the corner
    out["corner"] = m
    m = np.zeros((H, W), np.uint8)
    m[H // 4:, W // 2:] = 255                         # bottom and right edges
    out["bottom_right"] = m
    out["ellipse"] = _ellipse(W, H)
    g = _ellipse(W, H, value=255)
    g[g > 0] = (np.arange(int((g > 0).sum())) * 37 % 256).astype(np.uint8)
    out["grey"] = g
    out["empty"] = np.zeros((H, W), np.uint8)
    out["full"] = np.full((H, W), 255, np.uint8)
    return out


RHS_SIZES = [(9, 8), (37, 29), (131, 45), (258, 19)]


@pytest.mark.parametrize("W,H", RHS_SIZES)
def test_eroded_mask_is_bit_exact(inst, W, H):
    from seamlesscloneoptimization_amd import capi
    img = _rand(W, H, 11)
    for name, mask in _masks(W, H).items():
        M, _ = inst.edit_rhs(inst.edit_params(capi.SC_EDIT_COLOR_CHANGE), img, mask)
        assert np.array_equal(M, pe.erode_whole(mask)), name


@pytest.mark.parametrize("W,H", RHS_SIZES + [(300, 194)])
@pytest.mark.parametrize("op", ["color", "texture"])
def test_rhs_is_bit_exact(inst, W, H, op):
    from seamlesscloneoptimization_amd import capi
    img = _rand(W, H, 13) if (W, H) != (300, 194) else _image("airplane.jpg")
    for name, mask in _masks(W, H).items():
        if op == "color":
            kw = dict(red_mul=2.5, green_mul=1.0, blue_mul=0.3)
            p = inst.edit_params(capi.SC_EDIT_COLOR_CHANGE, **kw)
            _, want, _ = pe.build_rhs(img, mask, pe.COLOR, **kw)
        else:
            kw = dict(low_threshold=20.0, high_threshold=70.0, kernel_size=5)
            p = inst.edit_params(capi.SC_EDIT_TEXTURE_FLATTENING, **kw)
            _, want, _ = pe.build_rhs(img, mask, pe.TEXTURE, **kw)
        _, lap = inst.edit_rhs(p, img, mask)
        assert np.array_equal(lap, want), (name, int((lap != want).sum()))


@pytest.mark.parametrize("W,H", RHS_SIZES + [(300, 194)])
@pytest.mark.parametrize("alpha,beta", [(0.2, 0.4), (1.5, 0.9), (0.5, 0.0)])
def test_illumination_rhs_within_powf_error(inst, W, H, alpha, beta):
    """The device's powf and the host's differ in the last bits.  Every term of lap is |Q| m-weighted and scaled by
    alpha^beta |Q|^-beta; a relative error of 2^-20 per term (eight float32 ulps: powf's error is a few) plus one ulp of each
    of the three additions bounds the difference: tol = 2^-20 (|Gx(q)| + |Gx(q - x)| + |Gy(q)| + |Gy(q - y)|) + 4 ulp(|lap|)."""
    from seamlesscloneoptimization_amd import capi
    img = _rand(W, H, 17) if (W, H) != (300, 194) else _image("airplane.jpg")
    for name, mask in _masks(W, H).items():
        p = inst.edit_params(capi.SC_EDIT_ILLUMINATION_CHANGE, alpha=alpha, beta=beta)
        _, lap = inst.edit_rhs(p, img, mask)
        _, want, (GX, GY) = pe.build_rhs(img, mask, pe.ILLUMINATION, alpha=alpha, beta=beta)
        mag = np.zeros_like(want)
        s = (np.abs(GX[1:-1, 1:-1]) + np.abs(GX[1:-1, :-2]) + np.abs(GY[1:-1, 1:-1]) + np.abs(GY[:-2, 1:-1]))
        mag[:, 1:-1, 1:-1] = np.moveaxis(s, 2, 0)
        tol = mag * 2.0 ** -20 + 4 * np.spacing(np.abs(want))
        assert np.isfinite(lap).all()
        assert (np.abs(lap - want) <= tol).all(), (name, float(np.abs(lap - want).max()))
        if beta == 0.0:
            assert np.array_equal(lap, want)


# ---- whole edits -----------------------------------------------------------------------------------------------------------------
OPS = {"color": (1, dict(red_mul=1.6, green_mul=0.8, blue_mul=1.2)),
       "illumination": (2, dict(alpha=0.3, beta=0.5)),
       "texture": (3, dict(low_threshold=25.0, high_threshold=60.0, kernel_size=3))}
METHODS = ["auto", "multigrid", "dst", "fft", "fft_fp64"]


def _solver(method):
    from seamlesscloneoptimization_amd import capi
    return {"auto": dict(method=capi.SC_METHOD_AUTO), "multigrid": dict(method=capi.SC_METHOD_MULTIGRID),
            "dst": dict(method=capi.SC_METHOD_DST), "fft": dict(method=capi.SC_METHOD_FFT),
            "fft_fp64": dict(method=capi.SC_METHOD_FFT, flags=capi.SC_FLAG_FFT_FP64)}[method]


def _want(img, mask, op):
    code, kw = OPS[op]
    return pe.edit(img, mask, code, **kw)


@pytest.mark.parametrize("op", list(OPS))
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("W,H,mask_kind", [(301, 203, "ellipse"), (258, 131, "grey"), (97, 60, "rect")])
def test_edit_within_one_grey_level(op, method, W, H, mask_kind):
    img = _rand(W, H, W + H)
    mask = {"ellipse": _ellipse(W, H), "grey": _masks(W, H)["grey"], "rect": _masks(W, H)["corner"]}[mask_kind]
    want = _want(img, mask, op)
    i = _new(**_solver(method))
    try:
        code, kw = OPS[op]
        out = i.edit(i.edit_params(code, **kw), img, mask)
        info = i.info()
    finally:
        i.destroy()
    d = _dmax(out, want)
    print("%s %s %dx%d %s: max %d, %d off by one, method %d, field_retry %d" % (op, method, W, H, mask_kind, d, _off_by_one(out, want),
                                                                          info.method, info.field_retry))
    assert d <= 1
    assert (info.W, info.H, info.x0, info.y0, info.ltx, info.lty) == (W, H, 0, 0, 0, 0)
    assert np.array_equal(out[0], img[0]) and np.array_equal(out[-1], img[-1])
    assert np.array_equal(out[:, 0], img[:, 0]) and np.array_equal(out[:, -1], img[:, -1])


@pytest.mark.parametrize("op", list(OPS))
def test_sky_auto_takes_multigrid(op):
    from seamlesscloneoptimization_amd import capi
    img = _image("sky.jpg")
    H, W = img.shape[:2]
    mask = _ellipse(W, H, a=W / 4, b=H / 4)
    want = _want(img, mask, op)
    i = _new()
    try:
        code, kw = OPS[op]
        out = i.edit(i.edit_params(code, **kw), img, mask)
        info = i.info()
    finally:
        i.destroy()
    print("sky %s: max %d, %d off by one, field_retry %d" % (op, _dmax(out, want), _off_by_one(out, want), info.field_retry))
    assert info.method == capi.SC_METHOD_MULTIGRID
    assert _dmax(out, want) <= 1


def test_colour_change_past_the_16_bit_field():
    """red_mul = 2.5 on a bright image: the solution may leave the multigrid fast path's 16-bit field range (it did not here), in which case
    the edit is repeated on float fields (field_retry); either way the result is within one grey level."""
    from seamlesscloneoptimization_amd import capi
    W, H = 1100, 900
    img = _rand(W, H, 3)
    img[:, :, 2] = np.clip(img[:, :, 2].astype(int) + 60, 0, 255).astype(np.uint8)
    mask = _ellipse(W, H, a=W / 2.5, b=H / 2.5)
    want = pe.color_change(img, mask, red_mul=2.5, green_mul=1.0, blue_mul=1.0)
    i = _new(method=capi.SC_METHOD_MULTIGRID)
    try:
        out = i.edit(i.edit_params(capi.SC_EDIT_COLOR_CHANGE, red_mul=2.5), img, mask)
        info = i.info()
    finally:
        i.destroy()
    print("red_mul 2.5: max %d, %d off by one, field_retry %d" % (_dmax(out, want), _off_by_one(out, want), info.field_retry))
    assert _dmax(out, want) <= 1


# ---- identities ----------------------------------------------------------------------------------------------------------------------
def test_colour_change_one_equals_illumination_beta_zero(inst):
    from seamlesscloneoptimization_amd import capi
    img = _rand(211, 143, 2)
    mask = _masks(211, 143)["grey"]
    a = inst.edit(inst.edit_params(capi.SC_EDIT_COLOR_CHANGE), img, mask)
    b = inst.edit(inst.edit_params(capi.SC_EDIT_ILLUMINATION_CHANGE, alpha=0.37, beta=0.0), img, mask)
    assert np.array_equal(a, b)


@pytest.mark.parametrize("op", list(OPS))
def test_empty_mask_returns_src(inst, op):
    img = _rand(150, 91, 4)
    code, kw = OPS[op]
    out = inst.edit(inst.edit_params(code, **kw), img, np.zeros((91, 150), np.uint8))
    assert _dmax(out, img) <= 1


@pytest.mark.parametrize("op", list(OPS))
def test_in_place_equals_out_of_place_and_padded_rows(inst, op):
    code, kw = OPS[op]
    W, H = 123, 77
    img = _rand(W, H, 6)
    mask = _ellipse(W, H)
    ref = inst.edit(inst.edit_params(code, **kw), img, mask)
    same = img.copy()
    inst.edit(inst.edit_params(code, **kw), same, mask, dst=same)
    assert np.array_equal(same, ref)
    # padded steps for src, mask and dst; the bytes behind cols * 3 of each dst row stay as they were
    wsrc = np.zeros((H, W + 9, 3), np.uint8)
    wsrc[:, :W] = img
    wmask = np.zeros((H, W + 13), np.uint8)
    wmask[:, :W] = mask
    wdst = np.full((H, W + 5, 3), 0xA5, np.uint8)
    inst.edit(inst.edit_params(code, **kw), wsrc[:, :W], wmask[:, :W], dst=wdst[:, :W])
    assert np.array_equal(wdst[:, :W], ref)
    assert (wdst[:, W:] == 0xA5).all()


@pytest.mark.parametrize("op", list(OPS))
def test_host_equals_device(inst, op):
    code, kw = OPS[op]
    W, H = 157, 101
    img = _rand(W, H, 8)
    mask = _masks(W, H)["grey"]
    ref = inst.edit(inst.edit_params(code, **kw), img, mask)
    d_src = inst.to_device(img)
    d_mask = inst.to_device(mask)
    d_dst = inst.to_device(np.full_like(img, 0x3C))
    try:
        inst.edit_device(inst.edit_params(code, **kw), d_src, (H, W), d_mask, d_dst, sync=True)
        out = inst.from_device(d_dst, img.shape)
        inst.edit_device(inst.edit_params(code, **kw), d_src, (H, W), d_mask, d_src, sync=False)      # in place on the device
        inst.sync()
        out_in_place = inst.from_device(d_src, img.shape)
    finally:
        for p in (d_src, d_mask, d_dst):
            inst.free(p)
    assert np.array_equal(out, ref)
    assert np.array_equal(out_in_place, ref)


def test_clone_after_an_edit_is_unchanged():
    from oracle import oracle_np
    from seamlesscloneoptimization_amd import capi
    dst, patch, mask, cx, cy = oracle_np.synth_inputs(300, 200, margin=32)
    i = _new(method=capi.SC_METHOD_MULTIGRID)
    try:
        i.set_clone_mode(capi.SC_MIXED_CLONE)
        before = dst.copy()
        i.run(patch, before, mask, cx, cy)
        opts = bytes(i.get_solver())
        img = _rand(640, 480, 9)
        for code, kw in OPS.values():
            i.edit(i.edit_params(code, **kw), img, _ellipse(640, 480))
        assert i.clone_mode == capi.SC_MIXED_CLONE
        assert bytes(i.get_solver()) == opts
        after = dst.copy()
        i.run(patch, after, mask, cx, cy)
    finally:
        i.destroy()
    assert np.array_equal(before, after)


def test_error_codes(inst):
    from seamlesscloneoptimization_amd import capi
    L = inst.L
    img = _rand(20, 10, 1)
    mask = np.zeros((10, 20), np.uint8)
    out = np.zeros_like(img)

    def call(p, src=img, cols=20, rows=10, ss=60, m=mask, ms=20, d=out, ds=60):
        return L.sc_hip_edit(inst.h, ctypes.byref(p), src.ctypes.data if src is not None else None, cols, rows, ss,
                             m.ctypes.data if m is not None else None, ms, d.ctypes.data if d is not None else None, ds)

    ok = inst.edit_params(capi.SC_EDIT_COLOR_CHANGE)
    assert call(ok) == capi.SC_OK
    for op in (0, 4, -1):
        assert call(inst.edit_params(op)) == capi.SC_ERR_BAD_ARG
    assert call(ok, src=None) == capi.SC_ERR_BAD_ARG
    assert call(ok, m=None) == capi.SC_ERR_BAD_ARG
    assert call(ok, d=None) == capi.SC_ERR_BAD_ARG
    assert L.sc_hip_edit(inst.h, None, img.ctypes.data, 20, 10, 60, mask.ctypes.data, 20, out.ctypes.data, 60) == capi.SC_ERR_BAD_ARG
    assert call(inst.edit_params(capi.SC_EDIT_COLOR_CHANGE, red_mul=float("nan"))) == capi.SC_ERR_BAD_ARG
    assert call(inst.edit_params(capi.SC_EDIT_ILLUMINATION_CHANGE, beta=float("inf"))) == capi.SC_ERR_BAD_ARG
    assert call(inst.edit_params(capi.SC_EDIT_TEXTURE_FLATTENING, low_threshold=float("nan"))) == capi.SC_ERR_BAD_ARG
    assert call(inst.edit_params(capi.SC_EDIT_TEXTURE_FLATTENING, kernel_size=4)) == capi.SC_ERR_BAD_ARG
    assert call(ok, cols=2) == capi.SC_ERR_BAD_SIZE
    assert call(ok, rows=2) == capi.SC_ERR_BAD_SIZE
    assert call(ok, ss=59) == capi.SC_ERR_BAD_SIZE
    assert call(ok, ms=19) == capi.SC_ERR_BAD_SIZE
    assert call(ok, ds=59) == capi.SC_ERR_BAD_SIZE
    assert call(ok) == capi.SC_OK


# ---- Python ------------------------------------------------------------------------------------------------------------------------
def test_cv2_shaped_functions_on_sky_with_a_three_channel_mask():
    import seamlesscloneoptimization_amd as pkg
    img = _image("sky.jpg")
    H, W = img.shape[:2]
    m1 = _ellipse(W, H, a=W / 5, b=H / 4)
    m3 = np.repeat(m1[:, :, None], 3, axis=2)
    keep = img.copy()
    for fn, op, kw in ((pkg.colorChange, pe.COLOR, dict(red_mul=1.5, green_mul=0.7, blue_mul=1.1)),
                       (pkg.illuminationChange, pe.ILLUMINATION, dict(alpha=0.2, beta=0.4)),
                       (pkg.textureFlattening, pe.TEXTURE, dict(low_threshold=30, high_threshold=45, kernel_size=3))):
        out = fn(img, m3, **kw)
        want = pe.edit(img, pe.grey_bgr(m3), op, **kw)
        assert out is not img and out.shape == img.shape
        assert _dmax(out, want) <= 1, fn.__name__
    assert np.array_equal(img, keep)
