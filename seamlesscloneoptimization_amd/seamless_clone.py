"""Python surface of the library: the class the reference exposes through Boost.Python
(seamlessClone-CUDA/seamlessClone-python-binding/SeamlessClone.h:54-98, implementation
SeamlessClone.cpp:60-143), rebuilt on ctypes over the C ABI.

Same method names and argument meaning:
    loadMatsInSeamlessClone(face, body, mask, centerX, centerY, gpu_id)
    seamlessClone() -> ndarray (H, W, 3) uint8        (body is blended IN PLACE as well: the
                                                       reference wraps the numpy buffer without
                                                       a copy, SeamlessClone.cpp:217, and the
                                                       clone writes into it, seamlessClone_imp.cpp:470)
    sync(), destroy(), mat2py(a), py2mat(a), loadImageInCpp_Demo(path)
Additions: setSolver(**opts), setCloneMode(mode), info(); seamlessClone(src, dst, mask, p, flags) shaped like cv2.seamlessClone;
colorChange, illuminationChange and textureFlattening shaped like their cv2 namesakes; edit_batch runs one of them over many
images through a pool (same-size images share one set of launches).
"""
from __future__ import annotations

import contextlib

import numpy as np

from . import capi


class SeamlessClone:
    def __init__(self):
        self.instance_ptr = None          # capi.Instance, created lazily like SeamlessClone.cpp:110-113
        self.bSync = False                # SeamlessClone.cpp:63
        self.face = self.body = self.mask = self.blendedMat = None
        self.centerX = self.centerY = 0
        self.gpu_id = 0
        self._opts = {}
        self._clone_mode = capi.SC_NORMAL_CLONE

    # -- reference surface --------------------------------------------------------------
    def loadMatsInSeamlessClone(self, oface, obody, omask, centerX, centerY, gpu_id):
        self.face = self.py2mat(oface)
        self.body = self.py2mat(obody)
        self.mask = self.py2mat(omask)
        self.centerX, self.centerY, self.gpu_id = int(centerX), int(centerY), int(gpu_id)

    def seamlessClone(self):
        if self.face is None:
            raise RuntimeError("loadMatsInSeamlessClone() has not been called")
        if self.instance_ptr is None:
            self.instance_ptr = capi.Instance(self.gpu_id)
            if self._opts:
                self.instance_ptr.set_solver(**self._opts)
            if self._clone_mode != capi.SC_NORMAL_CLONE:
                self.instance_ptr.set_clone_mode(self._clone_mode)
        self.instance_ptr.run(self.face, self.body, self.mask, self.centerX, self.centerY, sync=self.bSync)
        self.blendedMat = self.body       # header copy: aliases the caller's buffer (imp.cpp:470)
        return self.mat2py(self.blendedMat)

    def sync(self):
        if self.instance_ptr is not None:
            self.instance_ptr.sync()

    def destroy(self):
        if self.instance_ptr is not None:
            self.instance_ptr.destroy()
            self.instance_ptr = None

    @staticmethod
    def mat2py(mat):
        """New (rows, cols, channels) array holding a copy (SeamlessClone.cpp:120-143)."""
        a = np.asarray(mat)
        if a.ndim == 2:
            a = a[:, :, None]
        return np.array(a, copy=True, order="C")

    @staticmethod
    def py2mat(o):
        """Zero-copy view of a numpy image (SeamlessClone.cpp:145-226): uint8, HxW or HxWxC,
        rows contiguous."""
        a = np.asarray(o)
        if a.dtype != np.uint8:
            raise TypeError("image data type = %s is not supported" % a.dtype)
        if a.ndim not in (2, 3):
            raise TypeError("dimensionality (=%d) is not supported" % a.ndim)
        if a.strides[-1] != 1:
            a = np.ascontiguousarray(a)   # the reference copies in this case too (needcopy)
        return a

    def loadImageInCpp_Demo(self, imagePath):
        """cv::imread equivalent via PIL (BGR channel order like OpenCV)."""
        from PIL import Image
        rgb = np.asarray(Image.open(imagePath).convert("RGB"))
        return np.ascontiguousarray(rgb[:, :, ::-1])

    # -- additions ----------------------------------------------------------------------
    def setSolver(self, **kw):
        """Forwarded to sc_hip_set_solver (method, max_sweeps, tol, omega, ...)."""
        self._opts.update(kw)
        if self.instance_ptr is not None:
            self.instance_ptr.set_solver(**kw)

    def setCloneMode(self, mode):
        """cv2.NORMAL_CLONE (1, default), cv2.MIXED_CLONE (2) or cv2.MONOCHROME_TRANSFER (3) for the next seamlessClone()."""
        if mode not in capi.CLONE_MODES:
            raise ValueError("clone mode must be NORMAL_CLONE (1), MIXED_CLONE (2) or MONOCHROME_TRANSFER (3), not %r" % (mode,))
        self._clone_mode = int(mode)
        if self.instance_ptr is not None:
            self.instance_ptr.set_clone_mode(mode)

    def info(self):
        return self.instance_ptr.info() if self.instance_ptr is not None else None


@contextlib.contextmanager
def _instance(gpu_id, solver):
    """The instance of one call: made on gpu_id, the solver options set when any are given, destroyed on every way out."""
    inst = capi.Instance(gpu_id)
    try:
        if solver:
            inst.set_solver(**solver)
        yield inst
    finally:
        inst.destroy()


def seamlessClone(src, dst, mask, p, flags=capi.SC_NORMAL_CLONE, gpu_id=0, **solver):
    """cv2.seamlessClone-shaped convenience: returns a NEW blended image, dst untouched.  flags: cv2.NORMAL_CLONE (1),
    cv2.MIXED_CLONE (2) or cv2.MONOCHROME_TRANSFER (3)."""
    if flags not in capi.CLONE_MODES:
        raise ValueError("flags must be NORMAL_CLONE (1), MIXED_CLONE (2) or MONOCHROME_TRANSFER (3), not %r" % (flags,))
    out = np.array(dst, np.uint8, copy=True, order="C")
    with _instance(gpu_id, solver) as inst:
        if flags != capi.SC_NORMAL_CLONE:
            inst.set_clone_mode(flags)
        inst.run(np.ascontiguousarray(src), out, np.ascontiguousarray(mask), int(p[0]), int(p[1]), sync=True)
    return out


def _edit_mask(mask, shape):
    """H x W or H x W x 3 uint8 -> H x W; three channels through cvtColor(BGR2GRAY)'s integer formula for 8-bit data."""
    m = np.asarray(mask, np.uint8)
    if m.ndim == 3 and m.shape[2] == 1:
        m = m[:, :, 0]
    if m.ndim == 3:
        if m.shape[2] != 3:
            raise ValueError("mask must have one or three channels")
        i = m.astype(np.int64)
        m = ((1868 * i[..., 0] + 9617 * i[..., 1] + 4899 * i[..., 2] + 8192) >> 14).astype(np.uint8)
    if m.shape != tuple(shape[:2]):
        raise ValueError("mask must have the image's size")
    return np.ascontiguousarray(m)


def _edit(op, src, mask, gpu_id, solver, **params):
    s = np.ascontiguousarray(src, np.uint8)
    if s.ndim != 3 or s.shape[2] != 3:
        raise ValueError("src must be H x W x 3 uint8")
    m = _edit_mask(mask, s.shape)
    with _instance(gpu_id, solver) as inst:
        return inst.edit(inst.edit_params(op, **params), s, m)


def colorChange(src, mask, red_mul=1.0, green_mul=1.0, blue_mul=1.0, gpu_id=0, **solver):
    """cv2.colorChange-shaped: returns a NEW image, src untouched.  The mask is H x W or H x W x 3."""
    return _edit(capi.SC_EDIT_COLOR_CHANGE, src, mask, gpu_id, solver, red_mul=float(red_mul), green_mul=float(green_mul),
                 blue_mul=float(blue_mul))


def illuminationChange(src, mask, alpha=0.2, beta=0.4, gpu_id=0, **solver):
    """cv2.illuminationChange-shaped: returns a NEW image, src untouched."""
    return _edit(capi.SC_EDIT_ILLUMINATION_CHANGE, src, mask, gpu_id, solver, alpha=float(alpha), beta=float(beta))


def textureFlattening(src, mask, low_threshold=30, high_threshold=45, kernel_size=3, gpu_id=0, **solver):
    """cv2.textureFlattening-shaped: returns a NEW image, src untouched.  kernel_size: 3, 5 or 7."""
    return _edit(capi.SC_EDIT_TEXTURE_FLATTENING, src, mask, gpu_id, solver, low_threshold=float(low_threshold),
                 high_threshold=float(high_threshold), kernel_size=int(kernel_size))


def edit_batch(op, srcs, masks, gpu_id=0, streams=2, group=capi.SC_POOL_GROUP_AUTO, **params_and_solver):
    """One edit (capi.SC_EDIT_COLOR_CHANGE, ..._ILLUMINATION_CHANGE or ..._TEXTURE_FLATTENING) over a list of H x W x 3 uint8 images;
    returns a list of NEW images, the inputs untouched.  masks: one mask for every image, or a list with one per image (H x W or
    H x W x 3, as the cv2-shaped functions take them).  Keyword arguments named like sc_edit_params fields (red_mul, alpha,
    low_threshold, kernel_size, ...) are the edit's parameters, the others solver options (method, flags, ...).  The images go to the
    device in one copy and come back in one; a pool of `streams` instances runs them device-resident in chunks of `group` same-size
    images (SC_POOL_GROUP_AUTO: the pool's automatic size), each chunk one field of 3n channels."""
    edit_keys = {name for name, _ in capi.EditParams._fields_} - {"op"}
    params = {k: v for k, v in params_and_solver.items() if k in edit_keys}
    solver = {k: v for k, v in params_and_solver.items() if k not in edit_keys}
    imgs = [np.ascontiguousarray(s, np.uint8) for s in srcs]
    if not imgs:
        return []
    for s in imgs:
        if s.ndim != 3 or s.shape[2] != 3:
            raise ValueError("every src must be H x W x 3 uint8")
    if isinstance(masks, (list, tuple)):
        if len(masks) != len(imgs):
            raise ValueError("one mask per image, or one mask for all")
        ms = [_edit_mask(m, s.shape) for m, s in zip(masks, imgs)]
        mask_of = list(range(len(imgs)))
    else:
        ms = [_edit_mask(masks, imgs[0].shape)]
        for s in imgs[1:]:
            if s.shape != imgs[0].shape:
                raise ValueError("one mask for all images needs images of one size")
        mask_of = [0] * len(imgs)
    # one device block: sources | masks | destinations, every image at a 256-byte boundary
    def place(arrays, at):
        offs = []
        for a in arrays:
            offs.append(at)
            at += (a.nbytes + 255) // 256 * 256
        return offs, at
    src_off, at = place(imgs, 0)
    mask_off, in_bytes = place(ms, at)
    dst_off, total = place(imgs, in_bytes)
    staged = np.zeros(in_bytes, np.uint8)
    for a, o in zip(imgs + ms, src_off + mask_off):
        staged[o:o + a.nbytes] = a.reshape(-1)
    pool = capi.Pool(gpu_id, streams=streams, group=group, **solver)
    inst = pool.instances[0]
    d = None
    try:
        d = inst.malloc(total)
        inst._check(inst.L.sc_hip_memcpy_h2d(inst.h, d, staged.ctypes.data, in_bytes))
        jobs = capi.Instance.make_edit_jobs(len(imgs))
        for k, (j, s) in enumerate(zip(jobs, imgs)):
            H, W = s.shape[:2]
            j.src, j.cols, j.rows, j.src_step = d + src_off[k], W, H, 3 * W
            j.mask, j.mask_step = d + mask_off[mask_of[k]], W
            j.dst, j.dst_step = d + dst_off[k], 3 * W
        pool.edit(inst.edit_params(op, **params), jobs, device_resident=True)
        out = inst.from_device(d + in_bytes, (total - in_bytes,))
    finally:
        if d is not None:
            inst.free(d)
        pool.close()
    return [out[o - in_bytes:o - in_bytes + s.nbytes].reshape(s.shape).copy() for o, s in zip(dst_off, imgs)]


def poisson_tol(boundary, lap_scale=0.0):
    """A multigrid stop (update_tol, in the data's units) the float32 solve can reach on this problem: the corrections of float32
    V-cycles settle at ~1e-8 x max|u| x sqrt(W H) (measured), and the stop rule accepts a cycle once its
    predicted error is a tenth of update_tol, so 4e-7 x scale x sqrt(W H), at least 1e-3.  scale: max |boundary|, or lap_scale when
    that is larger (a proxy for max |u|)."""
    b = np.asarray(boundary)
    scale = max(float(np.abs(b).max()) if b.size else 0.0, float(lap_scale))
    return max(1e-3, 4e-7 * scale * float(np.sqrt(b.shape[0] * b.shape[1])))


def _direct(neumann, free_sides, periodic=""):
    """Is a call with these borders one of the direct solves that use no tol (any free side or periodic axis)?"""
    return bool(neumann) or capi.free_side_bits(free_sides) != 0 or capi.periodic_bits(periodic) != 0


def poisson_solve(boundary, gx=None, gy=None, laplacian=None, gpu_id=0, tol=None, neumann=False, free_sides="", periodic="", **solver):
    """Solve the Poisson equation on a float32 image of shape H x W or H x W x C (C 1..4) and return a NEW array: lap(u) = div (gx, gy)
    (backward differences of the guidance field) or = laplacian, with u = boundary on the one-pixel frame.  boundary's interior is
    the initial guess of the iterative methods.  tol: the multigrid stop rule in the data's units (None: poisson_tol(boundary), a
    stop float32 can reach; <= 0: the library's 1e-3); keyword arguments are solver options (method, max_sweeps, flags, ...).  The
    exact 5-point system's answer, in float32, nothing clamped.
    neumann: no boundary values -- every pixel is an unknown and the field is reflected at the border (a direct DCT solve; methods
    auto and fft).  The answer's mean per channel is boundary's; boundary may be None (mean zero).  With a laplacian, its mean is
    projected out.
    free_sides: the sides without known values, a string over "lrtb" (left, right, top, bottom) -- a region that touches the image
    edge, a strip pinned at two ends.  Their outermost pixels are unknowns and the field is reflected there; the other sides'
    outermost rows and columns keep boundary's values.  A direct solve (methods auto and fft), tol unused; "lrtb" is neumann=True.
    periodic: the axes that wrap, "x" (a 360-degree panorama), "y" or "xy" (a tileable texture): no known values along them, the pixel
    beyond either end is the one at the other end; gx's last column / gy's last row then hold the difference across the seam.  Not
    with neumann=True or a free side of the same axis (ValueError).  When the other axis has no Dirichlet line either, the answer's
    mean is boundary's, which may be None, as for neumann."""
    kind, b, gx, gy, lap, _ = capi.poisson_arrays(boundary, gx, gy, laplacian, neumann=neumann, free_sides=free_sides, periodic=periodic)
    if tol is None:
        tol = 0.0 if _direct(neumann, free_sides, periodic) else poisson_tol(b)
    with _instance(gpu_id, solver) as inst:
        return inst.poisson(b, gx=gx, gy=gy, lap=lap, tol=tol, neumann=neumann, free_sides=free_sides, periodic=periodic)


def _float_batch(members, make_jobs, call, gpu_id, solver):
    """The device side of a float32 family's batch.  members: per problem its arrays in slot order, all of one shape, each as
    (the job field that points to it, the array) -- field None: the array takes its slot, the job's pointer stays NULL.  One device
    block holds every member's arrays and, behind them, every member's out, each at a 256-byte boundary; one copy in, the device
    call, one copy back.  call(inst, layout, jobs) runs the family's device call.  Returns the members' results as new arrays."""
    fields = [[f for f, _ in m] for m in members]
    members = [[np.ascontiguousarray(a) for _, a in m] for m in members]
    n, per, ref = len(members), len(members[0]), members[0][0]
    slot = (ref.nbytes + 255) // 256 * 256
    in_bytes = slot * per * n
    staged = np.zeros(in_bytes // 4, np.float32)
    for k, arrays in enumerate(members):
        for i, a in enumerate(arrays):
            o = (k * per + i) * slot // 4
            staged[o:o + a.size] = a.reshape(-1)
    with _instance(gpu_id, solver) as inst:
        dev = inst.malloc(in_bytes + slot * n)
        try:
            inst._check(inst.L.sc_hip_memcpy_h2d(inst.h, dev, staged.ctypes.data, in_bytes))
            jobs = make_jobs(n)
            for k, j in enumerate(jobs):
                for i, f in enumerate(fields[k]):
                    if f is not None:
                        setattr(j, f, dev + (k * per + i) * slot)
                j.out = dev + in_bytes + k * slot
            call(inst, capi.poisson_layout_of(ref), jobs)
            out = inst.from_device(dev + in_bytes, (slot * n // 4,), np.float32)
        finally:
            inst.free(dev)
    return [out[k * slot // 4:k * slot // 4 + ref.size].reshape(ref.shape).copy() for k in range(n)]


def poisson_solve_batch(boundaries, gxs=None, gys=None, laplacians=None, gpu_id=0, tol=None, neumann=False, free_sides="", periodic="",
                        **solver):
    """poisson_solve over a list of same-shape problems through ONE device-resident call (sc_hip_poisson_device): the inputs go to the
    device in one copy and the results come back in one; the problems are solved as one field of n x C planes (chunks of at most
    SC_POISSON_MAX_PLANES planes).  tol: as poisson_solve's (None: the largest poisson_tol of the batch).  Returns a list of NEW
    arrays.  neumann: as poisson_solve's; boundaries may then hold None entries (mean zero).  free_sides, periodic: as poisson_solve's."""
    bs = list(boundaries)
    if not bs:
        return []
    n = len(bs)
    if (gxs is None) != (gys is None) or (gxs is None) == (laplacians is None):
        raise ValueError("give either gxs and gys or laplacians")
    fields = [gxs, gys] if gxs is not None else [laplacians]
    for f in fields:
        if len(f) != n:
            raise ValueError("one guidance field (or laplacian) per boundary")
    checked = []
    for k in range(n):
        if gxs is not None:
            kind, b, gx, gy, _, _ = capi.poisson_arrays(bs[k], gxs[k], gys[k], neumann=neumann, free_sides=free_sides, periodic=periodic)
            ins = [("gx", gx), ("gy", gy)]
        else:
            kind, b, _, _, lap, _ = capi.poisson_arrays(bs[k], lap=laplacians[k], neumann=neumann, free_sides=free_sides, periodic=periodic)
            ins = [("lap", lap)]
        if ins[0][1].shape != fields[0][0].shape:
            raise ValueError("every problem of a batch must have one shape")
        checked.append(ins + [("boundary", b) if b is not None else (None, np.zeros_like(ins[0][1]))])
    if tol is None:
        tol = 0.0 if _direct(neumann, free_sides, periodic) else max(poisson_tol(m[-1][1]) for m in checked)
    return _float_batch(checked, capi.Instance.make_poisson_jobs,
                        lambda inst, layout, jobs: inst.poisson_device(capi.PoissonParams(kind, float(tol)), layout, jobs), gpu_id, solver)


def _screened_borders(neumann, free_sides, periodic=""):
    """(neumann, free_sides) of a screened wrapper whose default is neumann=True: a free_sides given (not None) overrides that default.
    So does a periodic axis: neumann is dropped, and with free_sides None the non-periodic axis is free at both ends."""
    per = capi.periodic_bits(periodic)
    if per:
        if free_sides is None:
            free_sides = ("" if per & capi.SC_POISSON_PERIODIC_X else "lr") + ("" if per & capi.SC_POISSON_PERIODIC_Y else "tb")
        return False, free_sides
    if free_sides is None:
        return neumann, ""
    all_free = capi.free_side_bits(free_sides) == capi.SC_POISSON_FREE_ALL
    return all_free, "" if all_free else free_sides


def screened_solve(data, gx=None, gy=None, laplacian=None, lam=None, boundary=None, neumann=True, gpu_id=0, free_sides=None, periodic="",
                   **solver):
    """Screened Poisson solve on a float32 image of shape H x W or H x W x C (C 1..4); returns a NEW array u that minimises
        lam sum (u - data)^2 + sum |grad u - (gx, gy)|^2                (or with the divergence of the guidance given as laplacian),
    i.e. (A - lam) u = div g - lam data for the 5-point operator A.  neumann (the default): every pixel is an unknown, the field is
    reflected at the border.  neumann=False: u = boundary on the one-pixel frame (boundary required; only its frame is read).  A
    direct solve (methods auto and fft; flags=SC_FLAG_FFT_FP64 for double transforms); lam must be finite and > 0.
    free_sides: a string over "lrtb", the sides without known values (poisson_solve's); giving it overrides the neumann default: ""
    is the Dirichlet frame, "lrtb" the Neumann problem, anything between needs boundary for the remaining Dirichlet lines.
    periodic: the axes that wrap (poisson_solve's); it too overrides the neumann default, and with free_sides None the other axis is
    free at both ends (no boundary needed)."""
    neumann, free_sides = _screened_borders(neumann, free_sides, periodic)
    kind, d, gx, gy, lap, b, _ = capi.screened_arrays(data, gx, gy, laplacian, lam, boundary, neumann=neumann, free_sides=free_sides,
                                                      periodic=periodic)
    with _instance(gpu_id, solver) as inst:
        return inst.screened(d, gx=gx, gy=gy, lap=lap, lam=lam, boundary=b, neumann=neumann, free_sides=free_sides, periodic=periodic)


def screened_solve_batch(datas, gxs=None, gys=None, laplacians=None, lam=None, boundaries=None, neumann=True, gpu_id=0, free_sides=None,
                         periodic="", **solver):
    """screened_solve over a list of same-shape problems through ONE device-resident call (sc_hip_screened_device): one copy in, one
    copy out, the problems solved as one field of n x C planes (chunks of at most SC_POISSON_MAX_PLANES planes); every member equals
    its solo solve bit for bit.  One lam for the batch.  boundaries: one per problem when neumann=False.  free_sides, periodic: as
    screened_solve's.  Returns a list of NEW arrays."""
    neumann, free_sides = _screened_borders(neumann, free_sides, periodic)
    no_boundary = capi.no_dirichlet(capi.border_bits(free_sides, neumann, periodic))      # no side keeps a Dirichlet line
    ds = list(datas)
    n = len(ds)
    if lam is None or not np.isfinite(lam) or not lam > 0:
        raise ValueError("lam must be finite and > 0")
    if (gxs is None) != (gys is None) or (gxs is None) == (laplacians is None):
        raise ValueError("give either gxs and gys or laplacians")
    fields = [gxs, gys] if gxs is not None else [laplacians]
    if not no_boundary:
        if boundaries is None:
            raise ValueError("a Dirichlet screened solve needs boundaries (neumann=True: none)")
        fields = fields + [boundaries]
    for f in fields:
        if len(f) != n:
            raise ValueError("one guidance field (or laplacian), and one boundary under a frame, per data term")
    if not ds:
        return []
    checked = []
    for k in range(n):
        b = None if no_boundary else boundaries[k]
        if gxs is not None:
            kind, d, gx, gy, _, b, _ = capi.screened_arrays(ds[k], gxs[k], gys[k], None, lam, b, neumann=neumann, free_sides=free_sides, periodic=periodic)
            arrays = [("gx", gx), ("gy", gy), ("data", d)]
        else:
            kind, d, _, _, lap, b, _ = capi.screened_arrays(ds[k], None, None, laplacians[k], lam, b, neumann=neumann, free_sides=free_sides, periodic=periodic)
            arrays = [("lap", lap), ("data", d)]
        if d.shape != ds[0].shape:
            raise ValueError("every problem of a batch must have one shape")
        checked.append(arrays + ([] if b is None else [("boundary", b)]))
    return _float_batch(checked, capi.Instance.make_screened_jobs,
                        lambda inst, layout, jobs: inst.screened_device(capi.ScreenedParams(kind, float(lam)), layout, jobs), gpu_id, solver)


def weighted_solve(data, weight, gx=None, gy=None, laplacian=None, boundary=None, neumann=True, free_sides=None, periodic="", tol=None,
                   max_iters=None, precond_lambda=None, gpu_id=0, **solver):
    """Weighted solve on a float32 image of shape H x W or H x W x C (C 1..4); returns a NEW array u that minimises
        sum weight (u - data)^2 + sum |grad u - (gx, gy)|^2           (or with the divergence of the guidance given as laplacian;
    neither: zero guidance), i.e. (A - W) u = div g - W data, W = diag(weight), weight >= 0 of data's shape or H x W (broadcast over
    the channels).  Borders as screened_solve's: neumann (the default), free_sides, periodic; boundary on the remaining Dirichlet lines.
    Conjugate gradients on the GPU, preconditioned by the screened direct solve with the mean weight (precond_lambda overrides it);
    stops at ||r|| <= tol ||b|| (default 1e-5) or after max_iters (default 200) iterations, which raises SC_ERR_NOT_CONVERGED.  Without
    any Dirichlet line a channel needs a positive weight somewhere.  flags=SC_FLAG_FFT_FP64: the preconditioner in double."""
    neumann, free_sides = _screened_borders(neumann, free_sides, periodic)
    with _instance(gpu_id, solver) as inst:
        return inst.weighted(data, weight, gx=gx, gy=gy, lap=laplacian, boundary=boundary, neumann=neumann, free_sides=free_sides,
                             periodic=periodic, tol=tol or 0.0, max_iters=max_iters or 0, precond_lambda=precond_lambda or 0.0)


def _pcg_batch(noun, datas, boundaries, neumann, free_sides, periodic, gpu_id, solver, *, required, optional, refusal, length_why, arrays_of,
               slots, params_of, make_jobs, device_call):
    """What weighted_solve_batch, wls_solve_batch and robust_solve_batch do alike.  required, optional: the per-problem input lists
    beside datas, by the job field each fills, in the order their lengths are checked (an optional one may be None: not given);
    boundaries joins them as "boundary" when a side keeps a Dirichlet line.  refusal: the wrapper's own word against its arguments
    (None: none), raised in its place among the checks.  arrays_of(data, inputs, borders): the family's capi.*_arrays on one problem
    (inputs: its members of the lists by name, borders: neumann, free_sides, periodic as keywords) -> (kind, its checked arrays by job
    field).  slots: the order of a member's arrays in the device block (_float_batch).  params_of(kind): the call's parameters;
    device_call(inst, params, layout, jobs): the family's device call."""
    neumann, free_sides = _screened_borders(neumann, free_sides, periodic)
    no_boundary = capi.no_dirichlet(capi.border_bits(free_sides, neumann, periodic))
    ds = list(datas)
    lists = {f: list(v) for f, v in required.items()}
    n = len(ds)
    if refusal:
        raise ValueError(refusal)
    lists.update({f: v for f, v in optional.items() if v is not None})
    if not no_boundary:
        if boundaries is None:
            raise ValueError(f"a {noun} solve with a Dirichlet line needs boundaries")
        lists["boundary"] = boundaries
    for v in lists.values():
        if len(v) != n:
            raise ValueError(length_why)
    if not ds:
        return []
    checked = []
    for k in range(n):
        kind, arrays = arrays_of(ds[k], {f: v[k] for f, v in lists.items()}, dict(neumann=neumann, free_sides=free_sides, periodic=periodic))
        if arrays["data"].shape != ds[0].shape:
            raise ValueError("every problem of a batch must have one shape")
        checked.append([(f, arrays[f]) for f in slots if arrays.get(f) is not None])
    params = params_of(kind)
    return _float_batch(checked, make_jobs, lambda inst, layout, jobs: inst._check(device_call(inst, params, layout, jobs)), gpu_id, solver)


_GUIDANCE_WHY = "give gxs and gys, or laplacians, or neither"


def weighted_solve_batch(datas, weights, gxs=None, gys=None, laplacians=None, boundaries=None, neumann=True, free_sides=None, periodic="",
                         tol=None, max_iters=None, precond_lambda=None, gpu_id=0, **solver):
    """weighted_solve over a list of same-shape problems through ONE device-resident call (sc_hip_weighted_device): one copy in, one
    copy out, the problems iterated as one field of n x C planes (chunks of at most SC_POISSON_MAX_PLANES planes).  Every plane has its
    own step sizes, but the stop is joint and the automatic preconditioner constant is the chunk's mean weight: a member agrees with its
    solo solve to the stop rule's error.  Neither gxs, gys nor laplacians: zero guidance.  Returns a list of NEW arrays."""
    def arrays_of(d, a, borders):
        kind, d, w, gx, gy, lap, b, _ = capi.weighted_arrays(d, a["weight"], a.get("gx"), a.get("gy"), a.get("lap"), a.get("boundary"), **borders)
        return kind, dict(gx=gx, gy=gy, lap=lap, data=d, weight=w, boundary=b)
    return _pcg_batch("weighted", datas, boundaries, neumann, free_sides, periodic, gpu_id, solver,
                      required=dict(weight=weights), optional=dict(gx=gxs, gy=gys, lap=laplacians),
                      refusal=_GUIDANCE_WHY if (gxs is None) != (gys is None) or (gxs is not None and laplacians is not None) else None,
                      length_why="one weight, one guidance field (or laplacian) and, with a Dirichlet line, one boundary per data term",
                      arrays_of=arrays_of, slots=("gx", "gy", "lap", "data", "weight", "boundary"),
                      params_of=lambda kind: capi.WeightedParams(kind, float(tol or 0.0), int(max_iters or 0), float(precond_lambda or 0.0)),
                      make_jobs=capi.Instance.make_weighted_jobs, device_call=capi.Instance.weighted_device)


def wls_solve(data, weight, smooth_x, smooth_y, gx=None, gy=None, laplacian=None, boundary=None, neumann=True, free_sides=None, periodic="",
              tol=None, max_iters=None, precond_lambda=None, precond_smooth=None, gpu_id=0, **solver):
    """WLS solve on a float32 image of shape H x W or H x W x C (C 1..4); returns a NEW array u that minimises
        sum weight (u - data)^2 + sum smooth_x (u[y, x+1] - u[y, x] - gx)^2 + sum smooth_y (u[y+1, x] - u[y, x] - gy)^2
    (or with div(smooth g) given as laplacian; neither: zero guidance): weighted_solve with a weight on every link between two
    neighbouring pixels.  smooth_x[y, x] weighs the link (x, y) - (x + 1, y), smooth_y[y, x] the link (x, y) - (x, y + 1); float32, of
    data's shape or H x W, finite and > 0 on every link that has an unknown end (the last column / row counts only along a periodic
    axis, where it holds the link across the seam).  Borders, tol and weight as weighted_solve's; max_iters defaults to 400.  The
    preconditioner is the direct solve scaled by the mean link weight (precond_smooth overrides it) with the mean data weight over it as
    its constant (precond_lambda overrides the mean data weight)."""
    neumann, free_sides = _screened_borders(neumann, free_sides, periodic)
    with _instance(gpu_id, solver) as inst:
        return inst.wls(data, weight, smooth_x, smooth_y, gx=gx, gy=gy, lap=laplacian, boundary=boundary, neumann=neumann,
                        free_sides=free_sides, periodic=periodic, tol=tol or 0.0, max_iters=max_iters or 0,
                        precond_lambda=precond_lambda or 0.0, precond_smooth=precond_smooth or 0.0)


def wls_solve_batch(datas, weights, smooth_xs, smooth_ys, gxs=None, gys=None, laplacians=None, boundaries=None, neumann=True, free_sides=None,
                    periodic="", tol=None, max_iters=None, precond_lambda=None, precond_smooth=None, gpu_id=0, **solver):
    """wls_solve over a list of same-shape problems through ONE device-resident call (sc_hip_wls_device), as weighted_solve_batch: one
    copy in, one copy out, one joint stop, the preconditioner's two constants the chunk's means -- a member agrees with its solo solve to
    the stop rule's error.  Returns a list of NEW arrays."""
    def arrays_of(d, a, borders):
        kind, d, w, sx, sy, gx, gy, lap, b, _ = capi.wls_arrays(d, a["weight"], a["smooth_x"], a["smooth_y"], a.get("gx"), a.get("gy"), a.get("lap"),
                                                                a.get("boundary"), **borders)
        return kind, dict(gx=gx, gy=gy, lap=lap, data=d, weight=w, smooth_x=sx, smooth_y=sy, boundary=b)
    return _pcg_batch("WLS", datas, boundaries, neumann, free_sides, periodic, gpu_id, solver,
                      required=dict(weight=weights, smooth_x=smooth_xs, smooth_y=smooth_ys), optional=dict(gx=gxs, gy=gys, lap=laplacians),
                      refusal=_GUIDANCE_WHY if (gxs is None) != (gys is None) or (gxs is not None and laplacians is not None) else None,
                      length_why="one weight, one pair of link weights, one guidance field (or laplacian) and, with a Dirichlet line, one boundary "
                                 "per data term",
                      arrays_of=arrays_of, slots=("gx", "gy", "lap", "data", "weight", "smooth_x", "smooth_y", "boundary"),
                      params_of=lambda kind: capi.WlsParams(kind, float(tol or 0.0), int(max_iters or 0), float(precond_lambda or 0.0),
                                                            float(precond_smooth or 0.0)),
                      make_jobs=capi.Instance.make_wls_jobs, device_call=capi.Instance.wls_device)


def _region_validate(kind, state, weight):
    loose = capi.region_unpinned(kind, state, weight)
    if loose.any():
        raise ValueError(f"validate: {int(loose.sum())} unknown pixels lie in components that nothing pins (no known neighbour, no Dirichlet "
                         "line, no weight)")


def region_solve(data, state, gx=None, gy=None, laplacian=None, weight=None, smooth_x=None, smooth_y=None, boundary=None, neumann=True,
                 free_sides=None, periodic="", tol=None, validate=False, max_iters=None, precond_lambda=None, precond_smooth=None, gpu_id=0,
                 **solver):
    """Region solve on a float32 image of shape H x W or H x W x C (C 1..4): wls_solve's problem on a domain of any shape, with hard
    constraints at any pixel.  state (of data's shape or H x W; float32, integers or bool) holds per pixel 0 (False): solved for, 1
    (True): known, the result is data there exactly, 2: outside the domain, no link reaches the pixel (a natural border, as at a free
    side); the result is data at known and outside pixels.  weight None: no data term (otherwise read at the unknown pixels, like data);
    smooth_x, smooth_y None: every link 1.  Guidance, borders (neumann by default), tol, max_iters (400), precond_lambda, precond_smooth:
    wls_solve's.  Every connected component of unknown pixels must be pinned by a known neighbour, a Dirichlet line or a positive
    weight; the library only notices a whole channel that nothing pins -- validate=True checks every component first (a numpy flood
    fill) and raises ValueError.  Returns a NEW array."""
    neumann, free_sides = _screened_borders(neumann, free_sides, periodic)
    kind, data, state, weight, sx, sy, gx, gy, lap, b, _ = capi.region_arrays(data, state, weight, smooth_x, smooth_y, gx, gy, laplacian, boundary,
                                                                             neumann=neumann, free_sides=free_sides, periodic=periodic)
    if validate:
        _region_validate(kind, state, weight)
    with _instance(gpu_id, solver) as inst:
        return inst.region(data, state, weight, sx, sy, gx=gx, gy=gy, lap=lap, boundary=b, neumann=neumann, free_sides=free_sides,
                           periodic=periodic, tol=tol or 0.0, max_iters=max_iters or 0, precond_lambda=precond_lambda or 0.0,
                           precond_smooth=precond_smooth or 0.0)


def region_solve_batch(datas, states, gxs=None, gys=None, laplacians=None, weights=None, smooth_xs=None, smooth_ys=None, boundaries=None,
                       neumann=True, free_sides=None, periodic="", tol=None, validate=False, max_iters=None, precond_lambda=None,
                       precond_smooth=None, gpu_id=0, **solver):
    """region_solve over a list of same-shape problems through ONE device-resident call (sc_hip_region_device), as wls_solve_batch: one
    copy in, one copy out, one joint stop, the preconditioner's two constants the chunk's -- a member agrees with its solo solve to the
    stop rule's error.  weights, smooth_xs and smooth_ys: for every problem or None.  Returns a list of NEW arrays."""
    def arrays_of(d, a, borders):
        kind, d, st, w, sx, sy, gx, gy, lap, b, _ = capi.region_arrays(d, a["state"], a.get("weight"), a.get("smooth_x"), a.get("smooth_y"),
                                                                      a.get("gx"), a.get("gy"), a.get("lap"), a.get("boundary"), **borders)
        if validate:
            _region_validate(kind, st, w)
        return kind, dict(gx=gx, gy=gy, lap=lap, data=d, state=st, weight=w, smooth_x=sx, smooth_y=sy, boundary=b)
    refusal = _GUIDANCE_WHY if (gxs is None) != (gys is None) or (gxs is not None and laplacians is not None) else \
        "smooth_xs and smooth_ys go together" if (smooth_xs is None) != (smooth_ys is None) else None
    return _pcg_batch("region", datas, boundaries, neumann, free_sides, periodic, gpu_id, solver,
                      required=dict(state=states), optional=dict(gx=gxs, gy=gys, lap=laplacians, weight=weights, smooth_x=smooth_xs, smooth_y=smooth_ys),
                      refusal=refusal,
                      length_why="one state and, where given, one weight, one pair of link weights, one guidance field (or laplacian) and, with a "
                                 "Dirichlet line, one boundary per data term",
                      arrays_of=arrays_of, slots=("gx", "gy", "lap", "data", "state", "weight", "smooth_x", "smooth_y", "boundary"),
                      params_of=lambda kind: capi.RegionParams(kind, float(tol or 0.0), int(max_iters or 0), float(precond_lambda or 0.0),
                                                               float(precond_smooth or 0.0)),
                      make_jobs=capi.Instance.make_region_jobs, device_call=capi.Instance.region_device)


def _mask_of(name, mask, image):
    m = np.asarray(mask)
    if m.shape != image.shape[:2]:
        raise ValueError(f"{name} has shape {m.shape}, the image {image.shape[:2]}")
    return m.astype(bool)


def inpaint(image, hole, gpu_id=0, **solver):
    """Membrane fill of a float32 image (H x W or H x W x C): the pixels where hole (H x W, anything truthy) is set are replaced by the
    harmonic interpolation of the pixels around them -- region_solve with zero guidance, every pixel outside the hole known, reflecting
    borders where the hole touches the image's edge.  Returns a NEW array; pixels outside the hole keep their bits."""
    if not isinstance(image, np.ndarray) or image.dtype != np.float32:
        raise TypeError("image must be a float32 numpy array")
    h = _mask_of("hole", hole, image)
    if h.all():
        raise ValueError("the hole covers the whole image: nothing to fill it from")
    state = np.where(h, capi.SC_REGION_UNKNOWN, capi.SC_REGION_KNOWN).astype(np.uint8)
    return region_solve(image, state, neumann=True, gpu_id=gpu_id, **solver)


def _forward_differences(a):
    """(d/dx, d/dy) of a float32 array, of its shape: a[y, x+1] - a[y, x] and a[y+1, x] - a[y, x]; the last column / row holds 0"""
    gx, gy = np.zeros_like(a), np.zeros_like(a)
    gx[:, :-1] = a[:, 1:] - a[:, :-1]
    gy[:-1] = a[1:] - a[:-1]
    return gx, gy


def poisson_clone(src, dst, mask, mixed=False, gpu_id=0, **solver):
    """Poisson image editing (Perez, Gangnet, Blake 2003) on float32 images of one shape (H x W or H x W x C): inside mask (H x W,
    anything truthy) the result has src's forward differences, outside it is dst, bit for bit, and it is continuous across the mask's
    edge -- the region of the paper in its exact shape, solved in float32 (seamlessClone is the 8-bit clone of a patch at a position).
    mixed: per link the guidance is src's difference or dst's, whichever is larger in magnitude (mixed gradients: dst's texture shows
    through flat parts of src).  A mask that touches the image's edge gets a reflecting border there.  Returns a NEW array."""
    for name, a in (("src", src), ("dst", dst)):
        if not isinstance(a, np.ndarray) or a.dtype != np.float32:
            raise TypeError(f"{name} must be a float32 numpy array")
    if src.shape != dst.shape:
        raise ValueError(f"src has shape {src.shape}, dst {dst.shape}")
    m = _mask_of("mask", mask, dst)
    if m.all():
        raise ValueError("the mask covers the whole image: nothing of dst is left to join")
    gx, gy = _forward_differences(src)
    if mixed:
        dx, dy = _forward_differences(dst)
        gx, gy = np.where(np.abs(dx) > np.abs(gx), dx, gx), np.where(np.abs(dy) > np.abs(gy), dy, gy)
    state = np.where(m, capi.SC_REGION_UNKNOWN, capi.SC_REGION_KNOWN).astype(np.uint8)
    return region_solve(dst, state, gx=gx, gy=gy, neumann=True, gpu_id=gpu_id, **solver)


def volume_solve(data, state, gx=None, gy=None, gt=None, laplacian=None, weight=None, boundary=None, tau=1.0, neumann=True, free_sides=None,
                 periodic="", tol=None, max_iters=None, gpu_id=0, **solver):
    """Volume solve on a float32 frame stack of shape T x H x W or T x H x W x C (C 1..4, T * C <= 192): region_solve's problem with unit
    links on every frame, and every pixel joined to the same pixel of the next frame by a link of weight tau -- per channel it minimises
    sum_t [sum w (u_t - d_t)^2 + sum |grad u_t - (gx_t, gy_t)|^2] + tau sum_t sum (u_{t+1} - u_t - gt_t)^2 over the pixels whose state
    is 0, with u = data where state is 1 and no link to a pixel whose state is 2.  A known keyframe is a frame of 1s.  gt ((T - 1) x H x
    W (x C)): the wanted change from frame to frame; None: plain temporal smoothness.  laplacian: the whole right-hand side in place of
    gx, gy, gt.  Borders (neumann by default), tol, max_iters (400): region_solve's.  Returns a NEW array."""
    neumann, free_sides = _screened_borders(neumann, free_sides, periodic)
    _, data, state, weight, gx, gy, gt, lap, b = capi.volume_arrays(data, state, weight, gx, gy, gt, laplacian, boundary, tau, neumann=neumann,
                                                                     free_sides=free_sides, periodic=periodic)
    with _instance(gpu_id, solver) as inst:
        return inst.volume(data, state, weight, gx, gy, gt, lap, b, tau=tau, neumann=neumann, free_sides=free_sides, periodic=periodic,
                           tol=tol or 0.0, max_iters=max_iters or 0)


def _video_masks(name, masks, frames):
    m = np.asarray(masks)
    if m.shape != frames.shape[:3]:
        raise ValueError(f"{name} has shape {m.shape}, the frames {frames.shape[:3]}")
    return m.astype(bool)


def _flow_of(flow, frames, loop=False):
    """the rounded flow of a video as volume_flow_planes checks it ((T - 1) x H x W x 2, with loop T; (dx, dy); NaN: no link): float32"""
    fx, fy = capi.volume_flow_planes(flow, frames.shape[0], frames.shape[1], frames.shape[2], loop)
    return np.stack([fx, fy], -1)


def _along_flow(a, flow, loop=False, wrap=""):
    """(partner, inside): partner[t][p] = a[t + 1][m_t(p)], the element of the next frame (with loop: of frame 0 behind the last) that
    the rounded flow leads to from p, and where that target exists -- both components finite and the target inside the frame (an axis
    named in wrap wraps).  partner is a[t][p] itself where it does not."""
    T, H, W = a.shape[:3]
    nxt = np.roll(a, -1, 0) if loop else a[1:]
    fin = np.isfinite(flow).all(-1) & (np.abs(np.nan_to_num(flow, nan=0.0, posinf=2e6, neginf=-2e6)) <= 1e6).all(-1)
    f = np.where(fin[..., None], flow, 0).astype(np.int64)
    yy, xx = np.mgrid[0:H, 0:W]
    tx, ty = xx[None] + f[..., 0], yy[None] + f[..., 1]
    if "x" in wrap:
        tx %= W
    if "y" in wrap:
        ty %= H
    inside = fin & (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
    tt = np.arange(nxt.shape[0])[:, None, None]
    partner = nxt[tt, np.clip(ty, 0, H - 1), np.clip(tx, 0, W - 1)]
    sel = inside.reshape(inside.shape + (1,) * (a.ndim - 3))
    return np.where(sel, partner, a[:nxt.shape[0]]), inside


def _subpixel_flow_of(flow, frames, loop=False):
    """the flow of a video as volume_subflow_planes checks it, values as they are: float32 (T - 1) x H x W x 2, with loop T"""
    fx, fy = capi.volume_subflow_planes(flow, frames.shape[0], frames.shape[1], frames.shape[2], loop)
    return np.stack([fx, fy], -1)


def _subpixel_taps(flow, H, W, wrap=""):
    """sc_hip_volume_subflow's taps of a float32 flow (Tf x H x W x 2) on the whole frame: (ty, tx, b, inside) -- per tap k of 4 its row,
    its column (clipped into the frame) and its float32 weight (0: no part of the link), and where the pixel holds a link: both components
    finite and at most 1e6, every tap of non-zero weight inside the frame (an axis named in wrap wraps)"""
    flow = np.asarray(flow, np.float32)
    with np.errstate(invalid="ignore"):
        ok = (np.abs(flow) <= np.float32(1e6)).all(-1)
    f = np.where(ok[..., None], flow, np.float32(0))
    f0 = np.floor(f)
    a = f - f0
    i0 = f0.astype(np.int64)
    one = np.float32(1)
    wx, wy = (one - a[..., 0], a[..., 0]), (one - a[..., 1], a[..., 1])
    yy, xx = np.mgrid[0:H, 0:W]
    tys, txs, bs = [], [], []
    for k in range(4):
        w = wx[k & 1] * wy[k >> 1]
        tx, ty = xx[None] + i0[..., 0] + (k & 1), yy[None] + i0[..., 1] + (k >> 1)
        if "x" in wrap:
            tx %= W
        if "y" in wrap:
            ty %= H
        part = w != 0
        ok = ok & ~(part & ~((tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)))
        tys.append(np.clip(ty, 0, H - 1)); txs.append(np.clip(tx, 0, W - 1)); bs.append(w)
    return tys, txs, [np.where(ok, w, np.float32(0)) for w in bs], ok


def _along_subpixel_flow(a, flow, loop=False, wrap=""):
    """_along_flow for a real-valued flow: partner[t][p] = sum_k b_k a[t + 1][q_k(p)], the bilinear interpolation of the next frame at
    p + flow(p) with sc_hip_volume_subflow's taps, in float64; inside: where p holds a link.  partner is a[t][p] itself where it does not."""
    T, H, W = a.shape[:3]
    nxt = np.asarray(np.roll(a, -1, 0) if loop else a[1:], np.float64)
    tys, txs, bs, inside = _subpixel_taps(flow, H, W, wrap)
    tt = np.arange(nxt.shape[0])[:, None, None]
    ext = (1,) * (a.ndim - 3)
    partner = sum(b.astype(np.float64).reshape(b.shape + ext) * nxt[tt, ty, tx] for ty, tx, b in zip(tys, txs, bs))
    return np.where(inside.reshape(inside.shape + ext), partner, a[:nxt.shape[0]]), inside


def inpaint_video(frames, holes, tau=1.0, flow=None, subpixel=False, gpu_id=0, **solver):
    """Membrane fill of a float32 video (T x H x W or T x H x W x C): inpaint() with temporal links of weight tau.  The pixels where
    holes (T x H x W, anything truthy) is set are filled from the pixels around them in space and time, so a place hidden in one frame is
    filled from the frames where it is visible, and the fill does not flicker.  flow ((T - 1) x H x W x 2 of (dx, dy), rounded; NaN: no
    link): the temporal links follow it -- pixel (x, y) of frame t is joined to pixel (x + dx, y + dy) of frame t + 1 --, so a hole is
    filled from where its surface point is visible, also when the scene moves.  subpixel: the flow is not rounded -- a link joins
    (x, y) to the bilinear interpolation of frame t + 1 at (x + dx, y + dy) (volume_wls_solve's).  Returns a NEW array; pixels outside
    the holes keep their bits."""
    if not isinstance(frames, np.ndarray) or frames.dtype != np.float32:
        raise TypeError("frames must be a float32 numpy array")
    if frames.ndim not in (3, 4):
        raise ValueError("frames are T x H x W or T x H x W x C")
    h = _video_masks("holes", holes, frames)
    if h.all():
        raise ValueError("the holes cover every frame: nothing to fill them from")
    state = np.where(h, capi.SC_REGION_UNKNOWN, capi.SC_REGION_KNOWN).astype(np.uint8)
    if flow is not None:
        return volume_wls_solve(frames, state, tau=tau, neumann=True, flow=flow, subpixel=subpixel, gpu_id=gpu_id, **solver)
    return volume_solve(frames, state, tau=tau, neumann=True, gpu_id=gpu_id, **solver)


def poisson_clone_video(srcs, dsts, masks, tau=1.0, mixed=False, flow=None, subpixel=False, gpu_id=0, **solver):
    """poisson_clone on every frame of float32 videos of one shape (T x H x W or T x H x W x C), the frames joined by temporal links of
    weight tau whose guidance is srcs' difference from frame to frame where both frames' masks (T x H x W) are set, 0 elsewhere: the
    clone follows the source's change over time and does not flicker.  mixed: poisson_clone's, per frame.  flow (inpaint_video's): the
    links follow it and their guidance is srcs' difference along it, srcs[t + 1][m(p)] - srcs[t][p], where both ends are masked.
    subpixel: the flow is not rounded and the guidance is srcs' difference along the bilinear link, where the source and all its taps
    are masked.  Returns a NEW array."""
    for name, a in (("srcs", srcs), ("dsts", dsts)):
        if not isinstance(a, np.ndarray) or a.dtype != np.float32:
            raise TypeError(f"{name} must be a float32 numpy array")
    if srcs.shape != dsts.shape:
        raise ValueError(f"srcs has shape {srcs.shape}, dsts {dsts.shape}")
    if dsts.ndim not in (3, 4):
        raise ValueError("frames are T x H x W or T x H x W x C")
    m = _video_masks("masks", masks, dsts)
    if m.all():
        raise ValueError("the masks cover every frame: nothing of dsts is left to join")
    gx, gy = np.zeros_like(srcs), np.zeros_like(srcs)
    for t in range(srcs.shape[0]):
        gx[t], gy[t] = _forward_differences(srcs[t])
        if mixed:
            dx, dy = _forward_differences(dsts[t])
            gx[t], gy[t] = np.where(np.abs(dx) > np.abs(gx[t]), dx, gx[t]), np.where(np.abs(dy) > np.abs(gy[t]), dy, gy[t])
    both = (m[1:] & m[:-1]).reshape(m[1:].shape + (1,) * (srcs.ndim - 3))
    gt = np.where(both, srcs[1:] - srcs[:-1], np.float32(0)).astype(np.float32)
    state = np.where(m, capi.SC_REGION_UNKNOWN, capi.SC_REGION_KNOWN).astype(np.uint8)
    if flow is not None and subpixel:
        f = _subpixel_flow_of(flow, dsts)
        partner, inside = _along_subpixel_flow(srcs, f)
        tys, txs, bs, _ = _subpixel_taps(f, dsts.shape[1], dsts.shape[2])
        tt = np.arange(f.shape[0])[:, None, None]
        both = m[:-1] & inside
        for ty, tx, b in zip(tys, txs, bs):
            both &= (b == 0) | m[1:][tt, ty, tx]
        both = both.reshape(m[1:].shape + (1,) * (srcs.ndim - 3))
        gt = np.where(both, partner - srcs[:-1], 0.0).astype(np.float32)
        return volume_wls_solve(dsts, state, gx=gx, gy=gy, gt=gt, tau=tau, neumann=True, flow=f, subpixel=True, gpu_id=gpu_id, **solver)
    if flow is not None:
        f = _flow_of(flow, dsts)
        partner, inside = _along_flow(srcs, f)
        both = (m[:-1] & inside & _along_flow(m, f)[0]).reshape(m[1:].shape + (1,) * (srcs.ndim - 3))
        gt = np.where(both, partner - srcs[:-1], np.float32(0)).astype(np.float32)
        return volume_wls_solve(dsts, state, gx=gx, gy=gy, gt=gt, tau=tau, neumann=True, flow=f, gpu_id=gpu_id, **solver)
    return volume_solve(dsts, state, gx=gx, gy=gy, gt=gt, tau=tau, neumann=True, gpu_id=gpu_id, **solver)


def _robust_params(kind, p, q, eps_grad, eps_data, max_rounds, round_tol, tol, max_iters):
    return capi.RobustParams(kind, float(p), float(eps_grad), float(q), float(eps_data), int(max_rounds or 0), float(round_tol or 0.0),
                             float(tol or 0.0), int(max_iters or 0))


def robust_solve(gx, gy, data, weight, smooth_x=None, smooth_y=None, boundary=None, p=1.0, q=2.0, eps_grad=1e-3, eps_data=1e-3, neumann=True,
                 free_sides=None, periodic="", max_rounds=None, round_tol=None, tol=None, max_iters=None, gpu_id=0, isotropic=False,
                 joint_channels=False, **solver):
    """Robust gradient solve on a float32 image of shape H x W or H x W x C (C 1..4); returns a NEW array u that minimises
        sum weight phi_q(u - data) + sum smooth_x phi_p(u[y, x+1] - u[y, x] - gx) + sum smooth_y phi_p(u[y+1, x] - u[y, x] - gy),
        phi_r(t) = (2 / r) (t^2 + eps^2)^(r/2),      0 < p, q <= 2,
    by iteratively reweighted least squares on the GPU: the quadratic problem (wls_solve's; smooth_x, smooth_y None: every base link 1)
    and then up to max_rounds (default 15) WLS solves whose links and weights come from the previous iterate, each started from it.
    p = 1 is the anisotropic total variation of the gradient residual (one residual per link), q = 1 an L1 data term.  isotropic=True
    takes one penalty per pixel over its two forward links, psi_p(c_x t_x^2 + c_y t_y^2) with psi_p(M) = (2 / p) (M + eps^2)^(p/2) (p = 1:
    the isotropic total variation, no staircases along the axes); joint_channels=True takes one penalty over all channels of a link
    (no colour fringes at edges); both: vectorial TV, one magnitude per pixel.  They couple the gradient term only.  eps_grad,
    eps_data round the penalties off near 0 (in the data's units: a hundredth to a thousandth of its range).  With an exponent below 1
    the energy is not convex and the result is a local minimum.  round_tol (default 1e-4): stop when no channel's energy (with
    joint_channels: the image's) fell by more than that fraction in the last round; negative: run every round.  tol, max_iters: the inner solves' (wls_solve's).  Borders,
    boundary and weight as wls_solve's."""
    neumann, free_sides = _screened_borders(neumann, free_sides, periodic)
    with _instance(gpu_id, solver) as inst:
        return inst.robust(gx, gy, data, weight, smooth_x, smooth_y, boundary=boundary, neumann=neumann, free_sides=free_sides,
                           periodic=periodic, p_grad=p, eps_grad=eps_grad, p_data=q, eps_data=eps_data, max_rounds=max_rounds or 0,
                           round_tol=round_tol or 0.0, tol=tol or 0.0, max_iters=max_iters or 0, isotropic=isotropic,
                           joint_channels=joint_channels)


def robust_solve_batch(gxs, gys, datas, weights, smooth_xs=None, smooth_ys=None, boundaries=None, p=1.0, q=2.0, eps_grad=1e-3, eps_data=1e-3,
                       neumann=True, free_sides=None, periodic="", max_rounds=None, round_tol=None, tol=None, max_iters=None, gpu_id=0,
                       isotropic=False, joint_channels=False, **solver):
    """robust_solve over a list of same-shape problems through ONE device-resident call (sc_hip_robust_device), as wls_solve_batch: the
    rounds, the inner stops and the preconditioner's constants are joint, so a member agrees with its solo solve to the inner solves'
    error as the rounds carry it, not bit for bit.  Base links for every problem or for none.  isotropic, joint_channels: robust_solve's
    (channels couple within a problem, never across problems).  Returns a list of NEW arrays."""
    def arrays_of(d, a, borders):
        kind, gx, gy, d, w, sx, sy, b, _ = capi.robust_arrays(a["gx"], a["gy"], d, a["weight"], a.get("smooth_x"), a.get("smooth_y"), a.get("boundary"),
                                                              **borders, p_grad=p, eps_grad=eps_grad, p_data=q, eps_data=eps_data,
                                                              isotropic=isotropic, joint_channels=joint_channels)
        return kind, dict(gx=gx, gy=gy, data=d, weight=w, smooth_x=sx, smooth_y=sy, boundary=b)
    return _pcg_batch("robust", datas, boundaries, neumann, free_sides, periodic, gpu_id, solver,
                      required=dict(weight=weights, gx=gxs, gy=gys), optional=dict(smooth_x=smooth_xs, smooth_y=smooth_ys),
                      refusal="smooth_xs and smooth_ys go together" if (smooth_xs is None) != (smooth_ys is None) else None,
                      length_why="one weight, one guidance field, one pair of base links (or none at all) and, with a Dirichlet line, one "
                                 "boundary per data term",
                      arrays_of=arrays_of, slots=("gx", "gy", "data", "weight", "smooth_x", "smooth_y", "boundary"),
                      params_of=lambda kind: _robust_params(kind, p, q, eps_grad, eps_data, max_rounds, round_tol, tol, max_iters),
                      make_jobs=capi.Instance.make_robust_jobs, device_call=capi.Instance.robust_device)


def tv_denoise(image, lam, p=1.0, q=2.0, eps=1e-2, max_rounds=None, round_tol=None, gpu_id=0, isotropic=False, joint_channels=False,
               **solver):
    """Total-variation denoising of a float32 image (H x W or H x W x C): the image u that minimises
        lam sum phi_q(u - image) + sum phi_p(forward differences of u)
    under reflecting borders -- robust_solve with zero guidance, data = image and weight = lam.  The default p = 1, q = 2 is the
    anisotropic form of the Rudin-Osher-Fatemi model (one penalty per link); isotropic=True is ROF as usually meant: the penalty on
    the gradient's magnitude per pixel, which does not round discs into diamonds.  joint_channels=True takes the magnitude over all
    channels (with isotropic=True: vectorial TV, no colour fringes).  q = 1 gives TV-L1; p = q = 2 is plain quadratic smoothing.  lam weighs closeness to the image
    against flatness; eps (in the image's units) rounds both penalties off near 0.  Returns a NEW array."""
    if not isinstance(image, np.ndarray) or image.dtype != np.float32:
        raise TypeError("image must be a float32 numpy array")
    if not (np.isfinite(lam) and lam > 0):
        raise ValueError("lam must be finite and > 0")
    zero = np.zeros_like(image)
    return robust_solve(zero, zero, image, np.full(image.shape, lam, np.float32), p=p, q=q, eps_grad=eps, eps_data=eps, neumann=True,
                        max_rounds=max_rounds, round_tol=round_tol, gpu_id=gpu_id, isotropic=isotropic, joint_channels=joint_channels, **solver)


def integrate_gradients(gx, gy, boundary=None, p=1.0, eps=1e-3, anchor=1e-3, max_rounds=None, round_tol=None, gpu_id=0, isotropic=False,
                        joint_channels=False, **solver):
    """Integrates a float32 gradient field (gx, gy: forward differences, H x W or H x W x C) into an image with an Lp penalty on the
    residual of every link: p = 1 (the default) ignores gross outliers in the field that a least-squares integration (p = 2) would
    smear over the image.  boundary given: its outermost rows and columns are the image's (a Dirichlet frame).  None: reflecting borders,
    and the free constant is held by a data term of weight `anchor` towards 0 -- small enough to leave the shape alone, so the
    result is the integral up to (nearly) a constant.  eps rounds the penalty off near 0, in the field's units.  isotropic,
    joint_channels: robust_solve's -- one penalty on the residual vector of a pixel, of all channels, or both.  Returns a NEW array."""
    if not isinstance(gx, np.ndarray) or gx.dtype != np.float32:
        raise TypeError("gx and gy must be float32 numpy arrays")
    if boundary is None and not (np.isfinite(anchor) and anchor > 0):
        raise ValueError("anchor must be finite and > 0")
    if boundary is not None:
        return robust_solve(gx, gy, np.zeros_like(gx), np.zeros_like(gx), boundary=boundary, p=p, eps_grad=eps, neumann=False,
                            max_rounds=max_rounds, round_tol=round_tol, gpu_id=gpu_id, isotropic=isotropic, joint_channels=joint_channels, **solver)
    return robust_solve(gx, gy, np.zeros_like(gx), np.full(gx.shape, anchor, np.float32), p=p, eps_grad=eps, neumann=True,
                        max_rounds=max_rounds, round_tol=round_tol, gpu_id=gpu_id, isotropic=isotropic, joint_channels=joint_channels, **solver)


def _forward_abs_differences(a):
    """(|d/dx|, |d/dy|), H x W float64, of an H x W or H x W x C array (the root of the channels' summed squares); the last column / row,
    which has no forward neighbour, holds 0"""
    a = np.asarray(a, np.float64)
    a = a[:, :, None] if a.ndim == 2 else a
    dx, dy = np.zeros(a.shape[:2]), np.zeros(a.shape[:2])
    dx[:, :-1] = np.sqrt(((a[:, 1:] - a[:, :-1]) ** 2).sum(2))
    dy[:-1] = np.sqrt(((a[1:] - a[:-1]) ** 2).sum(2))
    return dx, dy


def wls_filter(image, lam=1.0, alpha=1.2, eps=1e-4, guide=None, gpu_id=0, **solver):
    """Edge-preserving smoothing of a float32 image (H x W or H x W x C) by weighted least squares (Farbman, Fattal, Lischinski, Szeliski
    2008): the image u that minimises sum (u - image)^2 + sum s |grad u|^2 with the link weights
        s = lam / (|forward difference of l|^alpha + eps),      l = log(luminance + 1e-6) of the image, or of `guide`,
    luminance the mean over the channels clipped at 0 -- smooth where l is flat, free to jump where l jumps.  lam sets the amount of
    smoothing, alpha how sharply it falls off at edges.  Reflecting borders; the base layer of a base / detail decomposition (the detail
    is image - result).  Returns a NEW array."""
    if not isinstance(image, np.ndarray) or image.dtype != np.float32:
        raise TypeError("image must be a float32 numpy array")
    if not (np.isfinite(lam) and lam > 0 and np.isfinite(alpha) and alpha >= 0 and np.isfinite(eps) and eps > 0):
        raise ValueError("lam and eps must be finite and > 0, alpha finite and >= 0")
    g = np.asarray(image if guide is None else guide, np.float64)
    if g.shape[:2] != image.shape[:2]:
        raise ValueError(f"guide has shape {g.shape[:2]}, the image {image.shape[:2]}")
    lum = np.log(np.maximum(g if g.ndim == 2 else g.mean(2), 0.0) + 1e-6)
    sx, sy = ((lam / (d ** alpha + eps)).astype(np.float32) for d in _forward_abs_differences(lum))
    return wls_solve(image, np.ones(image.shape[:2], np.float32), sx, sy, neumann=True, gpu_id=gpu_id, **solver)


def interpolate_constraints(values, known_mask, image_gradients=None, strength=1.0, gpu_id=0, guide=None, edge_sigma=None, hard=False, **solver):
    """Fills a float32 image (H x W or H x W x C) from the pixels where known_mask (H x W, anything truthy) is set: the weighted solve
    with weight = strength on the mask and 0 elsewhere, data = values, under reflecting borders, with zero guidance (a membrane through
    the known pixels) or image_gradients = (gx, gy), forward differences the result should have.  strength weighs closeness to the known
    values against the guidance: large values pin them.  Returns a NEW array.
    guide (H x W or H x W x C, any real dtype): the values stop spreading at the guide's edges -- the WLS solve with the link weights
    exp(-d^2 / (2 edge_sigma^2)) + 1e-3, d the guide's forward difference (over its channels: the root of the summed squares);
    edge_sigma None: a tenth of the guide's range.  Without a guide edge_sigma must be None too.
    hard: the known pixels hold exactly (region_solve with them as known pixels) instead of being pulled towards their values by a
    weight; strength is then unused, and every part of the image must contain a known pixel."""
    if not isinstance(values, np.ndarray) or values.dtype != np.float32:
        raise TypeError("values must be a float32 numpy array")
    m = np.asarray(known_mask)
    if m.shape != values.shape[:2]:
        raise ValueError(f"known_mask has shape {m.shape}, the image {values.shape[:2]}")
    if not np.isfinite(strength) or not strength > 0:
        raise ValueError("strength must be finite and > 0")
    w = np.where(m.astype(bool), np.float32(strength), np.float32(0)).astype(np.float32)
    gx, gy = (None, None) if image_gradients is None else image_gradients
    if guide is None and edge_sigma is not None:
        raise ValueError("edge_sigma needs a guide")
    if guide is not None:
        g = np.asarray(guide, np.float64)
        if g.shape[:2] != values.shape[:2]:
            raise ValueError(f"guide has shape {g.shape[:2]}, the image {values.shape[:2]}")
        sigma = 0.1 * float(g.max() - g.min()) if edge_sigma is None else float(edge_sigma)
        if not np.isfinite(sigma) or not sigma > 0:
            raise ValueError("edge_sigma must be finite and > 0 (None: a tenth of the guide's range, which must not be flat)")
        sx, sy = ((np.exp(-d * d / (2.0 * sigma * sigma)) + 1e-3).astype(np.float32) for d in _forward_abs_differences(g))
        if hard:
            return region_solve(values, m.astype(bool), gx=gx, gy=gy, smooth_x=sx, smooth_y=sy, neumann=True, gpu_id=gpu_id, **solver)
        d = np.where(m.astype(bool).reshape(m.shape + (1,) * (values.ndim - 2)), values, np.float32(0)).astype(np.float32)
        return wls_solve(d, w, sx, sy, gx=gx, gy=gy, neumann=True, gpu_id=gpu_id, **solver)
    if hard:
        return region_solve(values, m.astype(bool), gx=gx, gy=gy, neumann=True, gpu_id=gpu_id, **solver)
    return weighted_solve(np.where(m.astype(bool).reshape(m.shape + (1,) * (values.ndim - 2)), values, np.float32(0)).astype(np.float32), w,
                          gx=gx, gy=gy, neumann=True, gpu_id=gpu_id, **solver)


def gradient_filter(image, gain, lam, neumann=True, gpu_id=0, free_sides=None, periodic="", **solver):
    """Gradient-domain filtering of a float32 image (H x W or H x W x C): the image whose forward differences are `gain` times the
    input's while it stays close to the input, lam weighing the closeness -- screened_solve with data = image, guidance = gain x the
    forward differences of image, and boundary = image when neumann=False.  gain > 1 sharpens, gain < 1 flattens, gain 1 returns the
    image (to float32 rounding).  free_sides: as screened_solve's (the image itself is the boundary of the remaining Dirichlet lines).
    periodic: as screened_solve's; the forward differences then wrap along those axes.  Returns a NEW array."""
    neumann, free_sides = _screened_borders(neumann, free_sides, periodic)
    if not isinstance(image, np.ndarray) or image.dtype != np.float32:
        raise TypeError("image must be a float32 numpy array")
    if image.ndim not in (2, 3):
        raise ValueError("image is H x W or H x W x C")
    if not np.isfinite(gain):
        raise ValueError("gain must be finite")
    g = np.float32(gain)
    gx = np.zeros_like(image)
    gy = np.zeros_like(image)
    gx[:, :-1] = g * (image[:, 1:] - image[:, :-1])
    gy[:-1] = g * (image[1:] - image[:-1])
    if "x" in periodic:
        gx[:, -1] = g * (image[:, 0] - image[:, -1])
    if "y" in periodic:
        gy[-1] = g * (image[0] - image[-1])
    return screened_solve(image, gx=gx, gy=gy, lam=lam, boundary=None if neumann else image, neumann=neumann, gpu_id=gpu_id,
                          free_sides=None if neumann else free_sides, periodic=periodic, **solver)


def wrapped_forward_differences(image, axes="xy"):
    """(gx, gy) of a float32 image: forward differences, the last column of gx / row of gy holding the difference from the last pixel to
    the first along the axes named in `axes` (0 along the others): the guidance of a periodic solve that gives the image back."""
    capi.periodic_bits(axes)
    gx = np.zeros_like(image)
    gy = np.zeros_like(image)
    gx[:, :-1] = image[:, 1:] - image[:, :-1]
    gy[:-1] = image[1:] - image[:-1]
    if "x" in axes:
        gx[:, -1] = image[:, 0] - image[:, -1]
    if "y" in axes:
        gy[-1] = image[0] - image[-1]
    return gx, gy


def make_tileable(image, lam=0.0, axes="xy", gpu_id=0, **solver):
    """A copy of a float32 image (H x W or H x W x C) that tiles without a seam along `axes` ("x", "y" or "xy"): the image whose wrapped
    forward differences are the input's, except across the seam (gx's last column, gy's last row, for the named axes), where they are
    0 -- the jump between the last pixel and the first is spread over the whole image.  Solved periodically along `axes`, the other
    axis free at both ends.  lam > 0: screened_solve(image, gx, gy, lam=lam, periodic=axes), the result stays close to the image;
    lam = 0: poisson_solve(image, gx, gy, periodic=axes, free_sides=<the other axis's two sides>), which keeps the image's mean.
    lam < 0 or not finite: ValueError.  Returns a NEW array."""
    if not isinstance(image, np.ndarray) or image.dtype != np.float32:
        raise TypeError("image must be a float32 numpy array")
    if image.ndim not in (2, 3):
        raise ValueError("image is H x W or H x W x C")
    if not capi.periodic_bits(axes):
        raise ValueError('axes must name at least one of "x" and "y"')
    if lam is None or not np.isfinite(lam) or lam < 0:
        raise ValueError("lam must be finite and >= 0 (0: the unscreened solve)")
    gx, gy = wrapped_forward_differences(image, "")
    if lam > 0:
        return screened_solve(image, gx=gx, gy=gy, lam=lam, periodic=axes, gpu_id=gpu_id, **solver)
    _, free_sides = _screened_borders(False, None, axes)
    return poisson_solve(image, gx=gx, gy=gy, periodic=axes, free_sides=free_sides, gpu_id=gpu_id, **solver)


def volume_wls_solve(data, state, gx=None, gy=None, gt=None, laplacian=None, weight=None, smooth_x=None, smooth_y=None, smooth_t=None, boundary=None,
                     tau=1.0, loop=False, neumann=True, free_sides=None, periodic="", tol=None, max_iters=None, flow=None, subpixel=False, gpu_id=0,
                     **solver):
    """volume_solve with a weight on every link: per channel it minimises sum_t [sum w (u_t - d_t)^2 + sum smooth_x (d_x u_t - gx_t)^2 +
    sum smooth_y (d_y u_t - gy_t)^2] + sum_t sum tau smooth_t (u_{t+1} - u_t - gt_t)^2.  smooth_x, smooth_y (together; None: 1): T x H x
    W (x C), each at its link's low end as in region_solve.  smooth_t (None: 1) and gt: element [t] belongs to the link from frame t to
    frame t + 1, T - 1 frames.  loop: time is periodic -- frame T - 1 is linked to frame 0 (T >= 3), and smooth_t and gt hold T frames,
    the last one that link's.  Links must be finite and > 0 where they are live.  flow ((T - 1) x H x W x 2, with loop T x H x W x 2, of
    (dx, dy); rounded with np.rint, NaN kept: no link, an occlusion): the temporal link of pixel (x, y) of frame t leads to pixel (x + dx,
    y + dy) of frame t + 1 in place of (x, y) -- sc_hip_volume_flow; of several pixels with one target the first in row-major order holds
    the link; smooth_t and gt stay stored at the link's source.  Strong tau with several pixels of motion needs more iterations: raise
    max_iters.  None: straight links.  subpixel: the flow is passed on as it is (float32, not rounded) and the temporal link of pixel
    (x, y) leads to the bilinear interpolation of frame t + 1 at (x + dx, y + dy) -- sc_hip_volume_subflow: up to four taps, no matching,
    any number of links may arrive at a pixel.  Returns a NEW array."""
    neumann, free_sides = _screened_borders(neumann, free_sides, periodic)
    _, data, state, weight, smooth_x, smooth_y, smooth_t, gx, gy, gt, laplacian, boundary = capi.volume_wls_arrays(
        data, state, weight, smooth_x, smooth_y, smooth_t, gx, gy, gt, laplacian, boundary, tau, bool(loop), neumann=neumann, free_sides=free_sides,
        periodic=periodic)
    if flow is not None:
        capi.volume_flow_planes(flow, data.shape[0], data.shape[1], data.shape[2], bool(loop))      # (its shape, before a device is touched)
    with _instance(gpu_id, solver) as inst:
        if flow is not None and subpixel:
            return inst.volume_subflow(data, state, flow, weight, smooth_x, smooth_y, smooth_t, gx, gy, gt, laplacian, boundary, tau=tau,
                                       loop=bool(loop), neumann=neumann, free_sides=free_sides, periodic=periodic, tol=tol or 0.0,
                                       max_iters=max_iters or 0)
        if flow is not None:
            return inst.volume_flow(data, state, flow, weight, smooth_x, smooth_y, smooth_t, gx, gy, gt, laplacian, boundary, tau=tau,
                                    loop=bool(loop), neumann=neumann, free_sides=free_sides, periodic=periodic, tol=tol or 0.0,
                                    max_iters=max_iters or 0)
        return inst.volume_wls(data, state, weight, smooth_x, smooth_y, smooth_t, gx, gy, gt, laplacian, boundary, tau=tau, loop=bool(loop),
                               neumann=neumann, free_sides=free_sides, periodic=periodic, tol=tol or 0.0, max_iters=max_iters or 0)


def _video_of(name, a):
    if not isinstance(a, np.ndarray) or a.dtype != np.float32:
        raise TypeError(f"{name} must be a float32 numpy array")
    if a.ndim not in (3, 4):
        raise ValueError(f"{name} are T x H x W or T x H x W x C")
    return a


def _video_abs_differences(g, loop):
    """(|d/dx|, |d/dy|, |d/dt|) of a T x H x W (x C) array in float64, T x H x W each (d/dt: T - 1 frames, with loop T: the last one from
    frame T - 1 to frame 0); over the channels the root of the summed squares; where there is no forward neighbour, 0"""
    g = np.asarray(g, np.float64)
    g = g[:, :, :, None] if g.ndim == 3 else g
    per = [_forward_abs_differences(f) for f in g]
    nxt = np.roll(g, -1, 0) if loop else g[1:]
    return np.stack([p[0] for p in per]), np.stack([p[1] for p in per]), np.sqrt(((nxt - g[:nxt.shape[0]]) ** 2).sum(3))


def wls_filter_video(frames, lam=1.0, alpha=1.2, eps=1e-4, tau=1.0, guide=None, loop=False, gpu_id=0, **solver):
    """wls_filter on a float32 video (T x H x W or T x H x W x C) with the same links along time: the video u that minimises
    sum (u - frames)^2 + sum s |grad u|^2 + tau sum s_t (u_{t+1} - u_t)^2, every link lam / (|forward difference of l|^alpha + eps) in x,
    y and t, l = log(luminance + 1e-6) of the frames, or of `guide` -- the temporal link from the difference between consecutive frames'
    l.  Smooth where the video is flat in space and steady in time, free to jump at edges, cuts and moving edges: the base layer does
    not flicker.  loop: the last frame is joined to the first.  Returns a NEW array."""
    frames = _video_of("frames", frames)
    if not (np.isfinite(lam) and lam > 0 and np.isfinite(alpha) and alpha >= 0 and np.isfinite(eps) and eps > 0):
        raise ValueError("lam and eps must be finite and > 0, alpha finite and >= 0")
    g = np.asarray(frames if guide is None else guide, np.float64)
    if g.shape[:3] != frames.shape[:3]:
        raise ValueError(f"guide has shape {g.shape[:3]}, the frames {frames.shape[:3]}")
    lum = np.log(np.maximum(g if g.ndim == 3 else g.mean(3), 0.0) + 1e-6)
    sx, sy, st = ((lam / (d ** alpha + eps)).astype(np.float32) for d in _video_abs_differences(lum, loop))
    return volume_wls_solve(frames, np.zeros(frames.shape[:3], np.uint8), weight=np.ones(frames.shape[:3], np.float32), smooth_x=sx, smooth_y=sy,
                            smooth_t=st, tau=tau, loop=loop, neumann=True, gpu_id=gpu_id, **solver)


def interpolate_constraints_video(values, known_mask, guide, edge_sigma=None, tau=1.0, hard=True, loop=False, strength=1.0, flow=None,
                                  subpixel=False, gpu_id=0, **solver):
    """interpolate_constraints with a guide on a float32 video (T x H x W or T x H x W x C): the values at the pixels where known_mask
    (T x H x W) is set spread through space and time and stop at the guide's edges in both -- every link exp(-d^2 / (2 edge_sigma^2)) +
    1e-3, d the guide's forward difference in x, y or t (edge_sigma None: a tenth of the guide's range).  Scribble, colour or depth
    propagation from a few frames or a few pixels.  hard: the known pixels hold exactly; else they carry the weight `strength`.
    loop: the last frame is joined to the first.  flow (volume_wls_solve's): the temporal links follow it, and a link's d is the guide's
    difference along it, so the values travel with the scene.  subpixel (volume_wls_solve's): the flow is not rounded, and a link's d is
    the guide's difference along the bilinear link.  Returns a NEW array."""
    values = _video_of("values", values)
    m = _video_masks("known_mask", known_mask, values)
    if guide is None:
        raise ValueError("interpolate_constraints_video needs a guide")
    g = np.asarray(guide, np.float64)
    if g.shape[:3] != values.shape[:3]:
        raise ValueError(f"guide has shape {g.shape[:3]}, the frames {values.shape[:3]}")
    if not np.isfinite(strength) or not strength > 0:
        raise ValueError("strength must be finite and > 0")
    sigma = 0.1 * float(g.max() - g.min()) if edge_sigma is None else float(edge_sigma)
    if not np.isfinite(sigma) or not sigma > 0:
        raise ValueError("edge_sigma must be finite and > 0 (None: a tenth of the guide's range, which must not be flat)")
    if not m.any():
        raise ValueError("known_mask is empty: nothing to spread")
    dx, dy, dt = _video_abs_differences(g, loop)
    if flow is not None and subpixel:
        flow = _subpixel_flow_of(flow, values, loop)
        g4 = g[:, :, :, None] if g.ndim == 3 else g
        dt = np.sqrt(((_along_subpixel_flow(g4, flow, loop)[0] - g4[:flow.shape[0]]) ** 2).sum(3))
        solver = dict(solver, flow=flow, subpixel=True)
    elif flow is not None:
        flow = _flow_of(flow, values, loop)
        g4 = g[:, :, :, None] if g.ndim == 3 else g
        dt = np.sqrt(((_along_flow(g4, flow, loop)[0] - g4[:flow.shape[0]]) ** 2).sum(3))
        solver = dict(solver, flow=flow)
    sx, sy, st = ((np.exp(-d * d / (2.0 * sigma * sigma)) + 1e-3).astype(np.float32) for d in (dx, dy, dt))
    if hard:
        state = np.where(m, capi.SC_REGION_KNOWN, capi.SC_REGION_UNKNOWN).astype(np.uint8)
        return volume_wls_solve(values, state, smooth_x=sx, smooth_y=sy, smooth_t=st, tau=tau, loop=loop, neumann=True, gpu_id=gpu_id, **solver)
    d = np.where(m.reshape(m.shape + (1,) * (values.ndim - 3)), values, np.float32(0)).astype(np.float32)
    w = np.where(m, np.float32(strength), np.float32(0)).astype(np.float32)
    return volume_wls_solve(d, np.zeros(m.shape, np.uint8), weight=w, smooth_x=sx, smooth_y=sy, smooth_t=st, tau=tau, loop=loop, neumann=True,
                            gpu_id=gpu_id, **solver)


def make_loop(frames, lam=1e-2, tau=1.0, gpu_id=0, **solver):
    """A copy of a float32 clip (T x H x W or T x H x W x C, T >= 3) that loops without a seam: make_tileable along time.  The clip
    whose forward differences in x, y and t are the input's, except from the last frame to the first, where the wanted difference is 0
    -- the jump at the seam is spread over all frames.  Time is periodic, the frames' borders reflect; the result stays close to the
    input with weight lam, which also pins the solve: lam must be finite and > 0.  Only lam holds the clip's mean level: in float32 it is
    held to about 1e-7 / lam of the values' size (1e-5 at the default).  Returns a NEW array."""
    frames = _video_of("frames", frames)
    if frames.shape[0] < 3:
        raise ValueError("a loop has at least 3 frames")
    if lam is None or not np.isfinite(lam) or not lam > 0:
        raise ValueError("lam must be finite and > 0: the weight pins the solve")
    gx, gy, gt = np.zeros_like(frames), np.zeros_like(frames), np.zeros_like(frames)
    for t in range(frames.shape[0]):
        gx[t], gy[t] = _forward_differences(frames[t])
    gt[:-1] = frames[1:] - frames[:-1]          # (the wrapping link's stays 0)
    return volume_wls_solve(frames, np.zeros(frames.shape[:3], np.uint8), gx=gx, gy=gy, gt=gt, weight=np.full(frames.shape[:3], lam, np.float32),
                            tau=tau, loop=True, neumann=True, gpu_id=gpu_id, **solver)


def volume_robust_solve(gx, gy, data, state, gt=None, weight=None, smooth_x=None, smooth_y=None, smooth_t=None, boundary=None, tau=1.0, loop=False,
                        p=1.0, p_time=1.0, q=2.0, eps_grad=1e-3, eps_time=1e-3, eps_data=1e-3, neumann=True, free_sides=None, periodic="",
                        max_rounds=None, round_tol=None, tol=None, max_iters=None, gpu_id=0, isotropic=False, spacetime=False, joint_channels=False,
                        flow=None, subpixel=False, **solver):
    """volume_wls_solve with robust_solve's penalties in place of the squares: per channel it minimises over the UNKNOWN pixels
        sum weight phi_q(u - data) + sum smooth_x phi_p(d_x u - gx) + sum smooth_y phi_p(d_y u - gy) + sum tau smooth_t phi_r(u_{t+1} - u_t - gt),
        phi_e(t) = (2 / e) (t^2 + eps^2)^(e/2),      0 < p, r = p_time, q <= 2,
    by iteratively reweighted least squares on the GPU: the quadratic problem (volume_wls_solve's) and then up to max_rounds (default
    15) WLS volume solves whose links and weights come from the previous iterate, each started from it.  state, the link arrays, gt,
    loop and the borders as volume_wls_solve's; gx and gy are required (there is no laplacian form), weight None: no data term.
    round_tol (default 1e-4): stop when no channel's energy fell by more than that fraction in the last round; negative: run every
    round.  isotropic: one penalty per pixel over its x- and y-link (per frame the isotropic total variation); spacetime: ... and over
    its forward temporal link too (the space-time total variation; implies isotropic and needs p_time == p and eps_time == eps_grad);
    joint_channels: every penalty over the channels of the volume (the vectorial total variation).  With any of the three the call is
    sc_hip_volume_coupled's.  flow (volume_wls_solve's: (T - 1) x H x W x 2, with loop T, of (dx, dy), rounded; NaN: no link): every
    temporal link -- its weight, its gt, its penalty -- joins pixel (x, y) of frame t to pixel (x + dx, y + dy) of frame t + 1, and
    smooth_t and gt stay stored at the link's source; sc_hip_volume_flow_robust.  A flow goes with none of the three coupled forms here:
    volume_flow_coupled_solve has the coupled penalties along a flow.  subpixel (with a flow, and none of the coupled forms): the flow
    is passed on as it is (float32, not rounded) and a temporal link joins pixel (x, y) of frame t to the bilinear interpolation of
    frame t + 1 at (x + dx, y + dy): up to four taps, no matching, gt the wanted difference along that link;
    sc_hip_volume_subflow_robust.  Returns a NEW array."""
    neumann, free_sides = _screened_borders(neumann, free_sides, periodic)
    coupling = capi.volume_coupling(isotropic, spacetime, joint_channels)
    if subpixel:
        if flow is None:
            raise ValueError("subpixel=True needs a flow")
        if coupling:
            raise ValueError("subpixel=True goes with none of isotropic, spacetime and joint_channels: coupled penalties along a sub-pixel flow "
                             "are not offered")
    if flow is not None:
        if coupling:
            raise ValueError("flow= goes with none of isotropic, spacetime and joint_channels: coupled penalties along a flow are not offered here "
                             "(volume_flow_coupled_solve and tv_denoise_video_along_flow have them)")
        capi.volume_flow_shape(flow, np.shape(data)[0], np.shape(data)[1], np.shape(data)[2], bool(loop))       # (before a device is touched)
    if spacetime and (p_time != p or eps_time != eps_grad):
        raise ValueError("spacetime=True is one penalty over space and time: p_time must equal p and eps_time eps_grad")
    args = dict(tau=tau, loop=bool(loop), neumann=neumann, free_sides=free_sides, periodic=periodic, p_grad=p, eps_grad=eps_grad, p_time=p_time,
                eps_time=eps_time, p_data=q, eps_data=eps_data, max_rounds=max_rounds or 0, round_tol=round_tol or 0.0, tol=tol or 0.0,
                max_iters=max_iters or 0)
    with _instance(gpu_id, solver) as inst:
        if coupling:
            return inst.volume_coupled(coupling, gx, gy, data, state, weight, smooth_x, smooth_y, smooth_t, gt, boundary, **args)
        if flow is not None and subpixel:
            return inst.volume_subflow_robust(gx, gy, data, state, flow, weight, smooth_x, smooth_y, smooth_t, gt, boundary, **args)
        if flow is not None:
            return inst.volume_flow_robust(gx, gy, data, state, flow, weight, smooth_x, smooth_y, smooth_t, gt, boundary, **args)
        return inst.volume_robust(gx, gy, data, state, weight, smooth_x, smooth_y, smooth_t, gt, boundary, **args)


def volume_flow_coupled_solve(gx, gy, data, state, flow, gt=None, weight=None, smooth_x=None, smooth_y=None, smooth_t=None, boundary=None, tau=1.0,
                              loop=False, p=1.0, p_time=1.0, q=2.0, eps_grad=1e-3, eps_time=1e-3, eps_data=1e-3, neumann=True, free_sides=None,
                              periodic="", max_rounds=None, round_tol=None, tol=None, max_iters=None, gpu_id=0, isotropic=False, spacetime=False,
                              joint_channels=False, subpixel=False, **solver):
    """volume_robust_solve's coupled forms with every temporal link along `flow` ((T - 1) x H x W x 2, with loop T, of (dx, dy),
    rounded; NaN: no link): isotropic -- one penalty per pixel over its x- and y-link --, spacetime -- ... and over the temporal link
    the pixel holds, the one that leads from it to pixel (x + dx, y + dy) of frame t + 1 (implies isotropic and needs p_time == p and
    eps_time == eps_grad); a pixel that holds no link has a spatial magnitude alone, and a link that arrives at a pixel plays no part in
    that pixel's magnitude --, joint_channels -- every penalty over the channels in which its link is live.  smooth_t and gt stay stored
    at a link's source.  volume_robust_solve's other arguments and defaults.  The call is
        Instance.volume_flow_coupled(capi.volume_coupling(isotropic, spacetime, joint_channels), gx, gy, data, state, flow, weight,
                                     smooth_x, smooth_y, smooth_t, gt, boundary, ...)
    (sc_hip_volume_flow_coupled); flow None: volume_robust_solve's coupled call, none of the three: volume_robust_solve(flow=flow)'s
    bytes.  subpixel (volume_robust_solve's keyword, kept so that the two signatures stay one): True is refused -- the coupled calls
    take whole-numbered flows only.  Returns a NEW array."""
    if subpixel:
        raise ValueError("subpixel=True: coupled penalties along a sub-pixel flow are not offered (volume_robust_solve and tv_denoise_video take "
                         "subpixel=True without a coupling)")
    neumann, free_sides = _screened_borders(neumann, free_sides, periodic)
    coupling = capi.volume_coupling(isotropic, spacetime, joint_channels)
    if flow is not None:
        capi.volume_flow_shape(flow, np.shape(data)[0], np.shape(data)[1], np.shape(data)[2], bool(loop))       # (before a device is touched)
    if spacetime and (p_time != p or eps_time != eps_grad):
        raise ValueError("spacetime=True is one penalty over space and time: p_time must equal p and eps_time eps_grad")
    args = dict(tau=tau, loop=bool(loop), neumann=neumann, free_sides=free_sides, periodic=periodic, p_grad=p, eps_grad=eps_grad, p_time=p_time,
                eps_time=eps_time, p_data=q, eps_data=eps_data, max_rounds=max_rounds or 0, round_tol=round_tol or 0.0, tol=tol or 0.0,
                max_iters=max_iters or 0)
    with _instance(gpu_id, solver) as inst:
        return inst.volume_flow_coupled(coupling, gx, gy, data, state, flow, weight, smooth_x, smooth_y, smooth_t, gt, boundary, **args)


def tv_denoise_video_along_flow(frames, lam, flow, isotropic=True, spacetime=False, joint_channels=False, tau=1.0, p=1.0, p_time=1.0, q=2.0, eps=1e-2,
                                loop=False, max_rounds=None, round_tol=None, gpu_id=0, subpixel=False, **solver):
    """tv_denoise_video with its coupled forms along a flow: the video u that minimises
        lam sum phi_q(u - frames) + (the isotropic / space-time / vectorial total variation of u) with the temporal differences
        u_{t+1}(x + dx, y + dy) - u_t(x, y) over the matched pixels of `flow` (volume_flow_coupled_solve's),
    so that on a moving shot discs stay discs, colours do not fringe and the temporal term compares a surface point with itself.
    tv_denoise_video's other arguments.  The call is
        Instance.volume_flow_coupled(capi.volume_coupling(isotropic, spacetime, joint_channels), 0, 0, frames, all UNKNOWN, flow,
                                     weight=lam, p_grad=p, p_time=p_time, p_data=q, eps_grad=eps_time=eps_data=eps, neumann=True, ...)
    through volume_flow_coupled_solve, which refuses subpixel=True.  Returns a NEW array."""
    frames = _video_of("frames", frames)
    if not (np.isfinite(lam) and lam > 0):
        raise ValueError("lam must be finite and > 0")
    zero = np.zeros_like(frames)
    return volume_flow_coupled_solve(zero, zero, frames, np.zeros(frames.shape[:3], np.uint8), flow, weight=np.full(frames.shape[:3], lam, np.float32),
                                     tau=tau, loop=loop, p=p, p_time=p_time, q=q, eps_grad=eps, eps_time=eps, eps_data=eps, neumann=True,
                                     max_rounds=max_rounds, round_tol=round_tol, gpu_id=gpu_id, isotropic=isotropic, spacetime=spacetime,
                                     joint_channels=joint_channels, subpixel=subpixel, **solver)


def tv_denoise_video(frames, lam, tau=1.0, p=1.0, p_time=1.0, q=2.0, eps=1e-2, loop=False, max_rounds=None, round_tol=None, gpu_id=0, isotropic=False,
                     spacetime=False, joint_channels=False, flow=None, subpixel=False, **solver):
    """Total-variation denoising of a float32 video (T x H x W or T x H x W x C) that does not flicker: the video u that minimises
        lam sum phi_q(u - frames) + sum phi_p(forward differences of u within a frame) + tau sum phi_r(u_{t+1} - u_t),      r = p_time,
    under reflecting borders -- volume_robust_solve with zero guidance, every state unknown, data = frames and weight = lam.  p = 1 is
    the anisotropic total variation in space; p_time = 1 lets the video jump at cuts and moving edges, p_time = 2 smooths along time.
    eps (in the frames' units) rounds all three penalties off near 0.  loop: the last frame is joined to the first.  isotropic,
    spacetime, joint_channels: volume_robust_solve's coupled forms -- the total variation of the gradient's magnitude per frame (discs
    stay discs), of the space-time gradient's (a moving edge is one surface; needs p_time == p), and over all channels (no colour
    fringes).  flow (volume_robust_solve's; with none of the three coupled forms -- those along a flow:
    tv_denoise_video_along_flow): the temporal term is tau sum phi_r(u_{t+1}(x + dx,
    y + dy) - u_t(x, y)) over the matched pixels, so a panning shot is neither blurred along its motion nor left to flicker.  subpixel
    (volume_robust_solve's): the flow is not rounded and u_{t+1} is interpolated bilinearly at (x + dx, y + dy) -- a slow pan or a zoom,
    where rounding makes half the links straight again.  Returns a NEW array."""
    frames = _video_of("frames", frames)
    if not (np.isfinite(lam) and lam > 0):
        raise ValueError("lam must be finite and > 0")
    zero = np.zeros_like(frames)
    return volume_robust_solve(zero, zero, frames, np.zeros(frames.shape[:3], np.uint8), weight=np.full(frames.shape[:3], lam, np.float32), tau=tau,
                               loop=loop, p=p, p_time=p_time, q=q, eps_grad=eps, eps_time=eps, eps_data=eps, neumann=True, max_rounds=max_rounds,
                               round_tol=round_tol, gpu_id=gpu_id, isotropic=isotropic, spacetime=spacetime, joint_channels=joint_channels, flow=flow,
                               subpixel=subpixel, **solver)


def tv_inpaint_video(frames, hole, p=1.0, eps=1e-2, isotropic=True, spacetime=False, joint_channels=False, tau=1.0, loop=False, p_time=None,
                     max_rounds=None, round_tol=None, gpu_id=0, **solver):
    """Total-variation fill of a float32 video (T x H x W or T x H x W x C), the volume partner of tv_inpaint: the pixels where hole
    (T x H x W, anything truthy: a hole per frame, which may move) is set are replaced by the u that minimises
        sum phi_p(forward differences of u within a frame) + tau sum phi_r(u_{t+1} - u_t),      r = p_time (default: p),
    over the links that touch the hole, every pixel outside it held -- volume_robust_solve with zero guidance, every pixel outside the
    hole known and reflecting borders.  isotropic (the default), spacetime, joint_channels: its coupled forms.  eps (in the frames'
    units) rounds the penalties off near 0.  loop: the last frame is joined to the first.  Returns a NEW array; pixels outside the hole
    keep their bits.  (Along a flow: volume_flow_coupled_solve with zero guidance, these states and the same coupling.)"""
    frames = _video_of("frames", frames)
    h = _video_masks("hole", hole, frames)
    if h.all():
        raise ValueError("the hole covers the whole video: nothing to fill it from")
    state = np.where(h, capi.SC_REGION_UNKNOWN, capi.SC_REGION_KNOWN).astype(np.uint8)
    zero = np.zeros_like(frames)
    return volume_robust_solve(zero, zero, frames, state, tau=tau, loop=loop, p=p, p_time=p if p_time is None else p_time, eps_grad=eps, eps_time=eps,
                               neumann=True, max_rounds=max_rounds, round_tol=round_tol, gpu_id=gpu_id, isotropic=isotropic, spacetime=spacetime,
                               joint_channels=joint_channels, **solver)


def integrate_gradients_video(gx, gy, gt, known=None, values=None, p=1.0, p_time=1.0, eps=1e-3, anchor=1e-3, loop=False, tau=1.0, max_rounds=None,
                              round_tol=None, gpu_id=0, flow=None, subpixel=False, **solver):
    """Integrates a float32 video's gradient field -- gx, gy: forward differences within a frame, T x H x W (x C); gt: from a frame to
    the next, T - 1 frames (loop: T, the last one from frame T - 1 to frame 0) -- into a video with an Lp penalty on the residual of
    every link: p = p_time = 1 (the default) ignores gross outliers in the field (a bad flow vector, a shot cut, a specular frame) that
    a least-squares integration would smear over the video.  known (T x H x W, bool) and values: the pixels that hold exactly (keyframes,
    a lattice of samples).  Neither: the free constant is held by a data term of weight `anchor` towards 0, small enough to leave the
    shape alone.  Reflecting borders.  eps rounds the penalties off near 0, in the field's units.  flow (volume_robust_solve's): gt is a
    difference along the flow -- element (x, y, t) is u_{t+1}(x + dx, y + dy) - u_t(x, y), stored at the link's source.  subpixel
    (volume_robust_solve's): the flow is not rounded and gt is the difference along the bilinear link, sum_k b_k u_{t+1}(q_k) - u_t(x, y)
    (_along_subpixel_flow(u, flow)[0] - u[:-1] of a video u).  Returns a NEW array."""
    gx = _video_of("gx", gx)
    if subpixel and flow is None:
        raise ValueError("subpixel=True needs a flow")
    if (known is None) != (values is None):
        raise ValueError("known and values go together")
    if known is None:
        if not (np.isfinite(anchor) and anchor > 0):
            raise ValueError("anchor must be finite and > 0")
        return volume_robust_solve(gx, gy, np.zeros_like(gx), np.zeros(gx.shape[:3], np.uint8), gt=gt, weight=np.full(gx.shape[:3], anchor, np.float32),
                                   tau=tau, loop=loop, p=p, p_time=p_time, eps_grad=eps, eps_time=eps, neumann=True, max_rounds=max_rounds,
                                   round_tol=round_tol, gpu_id=gpu_id, flow=flow, subpixel=subpixel, **solver)
    m = _video_masks("known", known, gx)
    if not m.any():
        raise ValueError("known is empty: nothing holds the video")
    state = np.where(m, capi.SC_REGION_KNOWN, capi.SC_REGION_UNKNOWN).astype(np.uint8)
    return volume_robust_solve(gx, gy, _video_of("values", values), state, gt=gt, tau=tau, loop=loop, p=p, p_time=p_time, eps_grad=eps, eps_time=eps,
                               neumann=True, max_rounds=max_rounds, round_tol=round_tol, gpu_id=gpu_id, flow=flow, subpixel=subpixel, **solver)


def region_robust_solve(gx, gy, data, state, weight=None, smooth_x=None, smooth_y=None, boundary=None, p=1.0, q=2.0, eps_grad=1e-3, eps_data=1e-3,
                        neumann=True, free_sides=None, periodic="", max_rounds=None, round_tol=None, tol=None, max_iters=None, validate=False,
                        gpu_id=0, isotropic=False, joint_channels=False, **solver):
    """region_solve with robust_solve's penalties in place of the squares, on a float32 image of shape H x W or H x W x C (C 1..4): per
    channel it minimises over the unknown pixels
        sum weight phi_q(u - data) + sum smooth_x phi_p(d_x u - gx) + sum smooth_y phi_p(d_y u - gy),      phi_r(t) = (2 / r) (t^2 + eps^2)^(r/2),
    the sums over the links that do not touch an outside pixel and have an unknown end; u is data at known pixels and boundary on the
    Dirichlet lines.  By iteratively reweighted least squares on the GPU: the quadratic problem (region_solve's) and then up to max_rounds
    (default 15) region solves whose links and weights come from the previous iterate, each started from it.  state as region_solve's;
    gx and gy are required (there is no laplacian form); weight None: no data term; smooth_x, smooth_y None: every base link 1.
    isotropic, joint_channels: robust_solve's coupled forms over the live links.  round_tol, tol, max_iters: robust_solve's.
    validate=True checks first that every component of unknown pixels is pinned (region_solve's).  Returns a NEW array."""
    neumann, free_sides = _screened_borders(neumann, free_sides, periodic)
    if validate:
        kind, _, _, d, st, w, _, _, _, _ = capi.region_robust_arrays(gx, gy, data, state, weight, smooth_x, smooth_y, boundary, neumann=neumann,
                                                                     free_sides=free_sides, periodic=periodic, p_grad=p, eps_grad=eps_grad, p_data=q,
                                                                     eps_data=eps_data)
        _region_validate(kind, st, w)
    with _instance(gpu_id, solver) as inst:
        return inst.region_robust(gx, gy, data, state, weight, smooth_x, smooth_y, boundary=boundary, neumann=neumann, free_sides=free_sides,
                                  periodic=periodic, p_grad=p, eps_grad=eps_grad, p_data=q, eps_data=eps_data, max_rounds=max_rounds or 0,
                                  round_tol=round_tol or 0.0, tol=tol or 0.0, max_iters=max_iters or 0, isotropic=isotropic,
                                  joint_channels=joint_channels)


def region_robust_solve_batch(gxs, gys, datas, states, weights=None, smooth_xs=None, smooth_ys=None, boundaries=None, p=1.0, q=2.0, eps_grad=1e-3,
                              eps_data=1e-3, neumann=True, free_sides=None, periodic="", max_rounds=None, round_tol=None, tol=None, max_iters=None,
                              gpu_id=0, isotropic=False, joint_channels=False, **solver):
    """region_robust_solve over a list of same-shape problems through ONE device-resident call (sc_hip_region_robust_device), as
    robust_solve_batch: the rounds, the inner stops and the preconditioner's constants are joint, so a member agrees with its solo solve
    to the inner solves' error as the rounds carry it, not bit for bit.  weights, smooth_xs and smooth_ys: for every problem or None.
    Returns a list of NEW arrays."""
    def arrays_of(d, a, borders):
        kind, gx, gy, d, st, w, sx, sy, b, _ = capi.region_robust_arrays(a["gx"], a["gy"], d, a["state"], a.get("weight"), a.get("smooth_x"),
                                                                         a.get("smooth_y"), a.get("boundary"), **borders, p_grad=p, eps_grad=eps_grad,
                                                                         p_data=q, eps_data=eps_data, isotropic=isotropic, joint_channels=joint_channels)
        return kind, dict(gx=gx, gy=gy, data=d, state=st, weight=w, smooth_x=sx, smooth_y=sy, boundary=b)
    return _pcg_batch("robust region", datas, boundaries, neumann, free_sides, periodic, gpu_id, solver,
                      required=dict(state=states, gx=gxs, gy=gys), optional=dict(weight=weights, smooth_x=smooth_xs, smooth_y=smooth_ys),
                      refusal="smooth_xs and smooth_ys go together" if (smooth_xs is None) != (smooth_ys is None) else None,
                      length_why="one state, one guidance field and, where given, one weight, one pair of base links and, with a Dirichlet line, "
                                 "one boundary per data term",
                      arrays_of=arrays_of, slots=("gx", "gy", "data", "state", "weight", "smooth_x", "smooth_y", "boundary"),
                      params_of=lambda kind: _robust_params(kind, p, q, eps_grad, eps_data, max_rounds, round_tol, tol, max_iters),
                      make_jobs=capi.Instance.make_region_robust_jobs, device_call=capi.Instance.region_robust_device)


def tv_inpaint(image, hole, p=1.0, eps=1e-2, isotropic=True, joint_channels=False, max_rounds=None, round_tol=None, gpu_id=0, **solver):
    """Total-variation fill of a float32 image (H x W or H x W x C): the pixels where hole (H x W, anything truthy) is set are replaced
    by the u that minimises sum phi_p(forward differences of u) over the links that touch the hole, the pixels around it held -- edges
    run through the hole where inpaint's membrane blurs them.  region_robust_solve with zero guidance, every pixel outside the hole
    known, reflecting borders where the hole touches the image's edge.  p = 1 with isotropic=True (the default) is the total variation
    of the gradient's magnitude; joint_channels=True takes it over all channels.  eps (in the image's units) rounds the penalty off
    near 0.  Returns a NEW array; pixels outside the hole keep their bits."""
    if not isinstance(image, np.ndarray) or image.dtype != np.float32:
        raise TypeError("image must be a float32 numpy array")
    h = _mask_of("hole", hole, image)
    if h.all():
        raise ValueError("the hole covers the whole image: nothing to fill it from")
    state = np.where(h, capi.SC_REGION_UNKNOWN, capi.SC_REGION_KNOWN).astype(np.uint8)
    zero = np.zeros_like(image)
    return region_robust_solve(zero, zero, image, state, p=p, eps_grad=eps, neumann=True, max_rounds=max_rounds, round_tol=round_tol, gpu_id=gpu_id,
                               isotropic=isotropic, joint_channels=joint_channels, **solver)


def integrate_gradients_masked(gx, gy, valid, known=None, values=None, p=1.0, eps=1e-3, anchor=1e-3, max_rounds=None, round_tol=None, gpu_id=0,
                               isotropic=False, joint_channels=False, **solver):
    """integrate_gradients on a mask of valid pixels: integrates a float32 gradient field (gx, gy: forward differences, H x W or
    H x W x C) over the pixels where valid (H x W, anything truthy) is set, with an Lp penalty on the residual of every link between two
    valid pixels -- photometric-stereo normals or depth from gradients with invalid pixels and gross outliers at once.  Pixels outside
    valid are outside the domain: no link reaches them and the result holds 0 there.  known (H x W) and values: hard anchors, the
    pixels that hold exactly.  Neither: the free constant is held by a data term of weight `anchor` towards 0, as in
    integrate_gradients.  Reflecting borders.  Returns a NEW array."""
    if not isinstance(gx, np.ndarray) or gx.dtype != np.float32:
        raise TypeError("gx and gy must be float32 numpy arrays")
    v = _mask_of("valid", valid, gx)
    if not v.any():
        raise ValueError("valid is empty: nothing to integrate over")
    if (known is None) != (values is None):
        raise ValueError("known and values go together")
    state = np.where(v, capi.SC_REGION_UNKNOWN, capi.SC_REGION_OUTSIDE).astype(np.uint8)
    if known is None:
        if not (np.isfinite(anchor) and anchor > 0):
            raise ValueError("anchor must be finite and > 0")
        return region_robust_solve(gx, gy, np.zeros_like(gx), state, weight=np.full(gx.shape, anchor, np.float32), p=p, eps_grad=eps, neumann=True,
                                   max_rounds=max_rounds, round_tol=round_tol, gpu_id=gpu_id, isotropic=isotropic, joint_channels=joint_channels,
                                   **solver)
    k = _mask_of("known", known, gx) & v
    if not k.any():
        raise ValueError("known is empty inside valid: nothing holds the image")
    if not isinstance(values, np.ndarray) or values.dtype != np.float32 or values.shape != gx.shape:
        raise TypeError("values must be a float32 numpy array of gx's shape")
    state[k] = capi.SC_REGION_KNOWN
    data = np.where((v if gx.ndim == 2 else v[:, :, None]), values, np.float32(0)).astype(np.float32)
    return region_robust_solve(gx, gy, data, state, p=p, eps_grad=eps, neumann=True, max_rounds=max_rounds, round_tol=round_tol, gpu_id=gpu_id,
                               isotropic=isotropic, joint_channels=joint_channels, **solver)


def bounded_solve(data, state, lower=None, upper=None, gx=None, gy=None, laplacian=None, weight=None, smooth_x=None, smooth_y=None, boundary=None,
                  neumann=True, free_sides=None, periodic="", max_rounds=None, tol=None, validate=False, max_iters=None, precond_lambda=None,
                  precond_smooth=None, gpu_id=0, **solver):
    """region_solve under the box constraint lower <= u <= upper at every unknown pixel, on a float32 image of shape H x W or H x W x C
    (C 1..4): the minimiser of region_solve's energy among the images inside the bounds -- not the clamped unconstrained answer, which
    it differs from everywhere.  lower, upper: None (no bound on that side), a number, or a float32 array of data's shape or H x W;
    known and outside pixels and the Dirichlet lines are not constrained.  By the primal-dual active set method on the GPU: the
    unconstrained solve, then up to max_rounds (default 30) region solves with the pixels on a bound held there, each started from the
    last; it ends when the set of held pixels stops changing.  Everything else is region_solve's.  Returns a NEW array."""
    neumann, free_sides = _screened_borders(neumann, free_sides, periodic)
    kind, data, state, weight, smooth_x, smooth_y, gx, gy, laplacian, boundary = capi.bounded_arrays(
        data, state, lower, upper, weight, smooth_x, smooth_y, gx, gy, laplacian, boundary, neumann=neumann, free_sides=free_sides,
        periodic=periodic)[:10]
    if validate:
        _region_validate(kind, state, weight)
    with _instance(gpu_id, solver) as inst:
        return inst.bounded(data, state, lower, upper, weight, smooth_x, smooth_y, gx=gx, gy=gy, lap=laplacian, boundary=boundary, neumann=neumann,
                            free_sides=free_sides, periodic=periodic, max_rounds=max_rounds or 0, tol=tol or 0.0, max_iters=max_iters or 0,
                            precond_lambda=precond_lambda or 0.0, precond_smooth=precond_smooth or 0.0)


def bounded_solve_batch(datas, states, lower=None, upper=None, gxs=None, gys=None, laplacians=None, weights=None, smooth_xs=None, smooth_ys=None,
                        boundaries=None, neumann=True, free_sides=None, periodic="", max_rounds=None, tol=None, validate=False, max_iters=None,
                        precond_lambda=None, precond_smooth=None, gpu_id=0, **solver):
    """bounded_solve over a list of same-shape problems through ONE device-resident call (sc_hip_bounded_device), as region_solve_batch:
    the rounds, the inner stops and the preconditioner's constants are joint, so a member agrees with its solo solve to the stop rule's
    error.  lower, upper: None or a number for every problem, or a list of arrays, one per problem.  Returns a list of NEW arrays."""
    per_problem = {f: v for f, v in (("lower", lower), ("upper", upper)) if isinstance(v, (list, tuple))}
    scalar = {f: None if f in per_problem else v for f, v in (("lower", lower), ("upper", upper))}
    bounds = {}

    def arrays_of(d, a, borders):
        kind, d, st, w, sx, sy, gx, gy, lap, b, _, lo, hi, lo_a, hi_a = capi.bounded_arrays(
            d, a["state"], a.get("lower", scalar["lower"]), a.get("upper", scalar["upper"]), a.get("weight"), a.get("smooth_x"), a.get("smooth_y"),
            a.get("gx"), a.get("gy"), a.get("lap"), a.get("boundary"), **borders)
        if validate:
            _region_validate(kind, st, w)
        bounds["lower"], bounds["upper"] = lo, hi
        return kind, dict(gx=gx, gy=gy, lap=lap, data=d, state=st, weight=w, smooth_x=sx, smooth_y=sy, boundary=b, lower=lo_a, upper=hi_a)
    refusal = _GUIDANCE_WHY if (gxs is None) != (gys is None) or (gxs is not None and laplacians is not None) else \
        "smooth_xs and smooth_ys go together" if (smooth_xs is None) != (smooth_ys is None) else None
    return _pcg_batch("bounded", datas, boundaries, neumann, free_sides, periodic, gpu_id, solver,
                      required=dict(state=states),
                      optional=dict(gx=gxs, gy=gys, lap=laplacians, weight=weights, smooth_x=smooth_xs, smooth_y=smooth_ys, **per_problem),
                      refusal=refusal,
                      length_why="one state and, where given, one weight, one pair of link weights, one guidance field (or laplacian), one array "
                                 "per bound and, with a Dirichlet line, one boundary per data term",
                      arrays_of=arrays_of,
                      slots=("gx", "gy", "lap", "data", "state", "weight", "smooth_x", "smooth_y", "boundary", "lower", "upper"),
                      params_of=lambda kind: capi.BoundedParams(kind, float(tol or 0.0), int(max_iters or 0), float(precond_lambda or 0.0),
                                                                float(precond_smooth or 0.0), bounds["lower"], bounds["upper"],
                                                                int(max_rounds or 0)),
                      make_jobs=capi.Instance.make_bounded_jobs, device_call=capi.Instance.bounded_device)


def poisson_clone_in_range(src, dst, mask, lo=0.0, hi=1.0, mixed=False, gpu_id=0, **solver):
    """poisson_clone with the result kept inside [lo, hi] (the displayable range) wherever it is solved for: a bright patch cloned into a
    dark scene overshoots, and clamping the overshoot flattens it while the rest of the patch stays as if nothing had been cut off --
    here the excess is spread over the whole patch (bounded_solve).  Outside the mask the result is dst, bit for bit, whatever its
    range.  With bounds the unconstrained clone already satisfies, the bytes of poisson_clone.  Returns a NEW array."""
    for name, a in (("src", src), ("dst", dst)):
        if not isinstance(a, np.ndarray) or a.dtype != np.float32:
            raise TypeError(f"{name} must be a float32 numpy array")
    if src.shape != dst.shape:
        raise ValueError(f"src has shape {src.shape}, dst {dst.shape}")
    m = _mask_of("mask", mask, dst)
    if m.all():
        raise ValueError("the mask covers the whole image: nothing of dst is left to join")
    gx, gy = _forward_differences(src)
    if mixed:
        dx, dy = _forward_differences(dst)
        gx, gy = np.where(np.abs(dx) > np.abs(gx), dx, gx), np.where(np.abs(dy) > np.abs(gy), dy, gy)
    state = np.where(m, capi.SC_REGION_UNKNOWN, capi.SC_REGION_KNOWN).astype(np.uint8)
    return bounded_solve(dst, state, lo, hi, gx=gx, gy=gy, neumann=True, gpu_id=gpu_id, **solver)


def interpolate_in_range(values, known_mask, lo, hi, guide=None, edge_sigma=None, image_gradients=None, gpu_id=0, **solver):
    """interpolate_constraints with hard samples and the answer kept inside [lo, hi]: the pixels where known_mask (H x W, anything
    truthy) is set hold their values exactly, the others are filled from them -- a membrane, or along image_gradients = (gx, gy), whose
    integration may leave the range -- and stay inside the bounds (an alpha matte or a confidence map in [0, 1], a depth that is not
    negative).  guide, edge_sigma: interpolate_constraints' edge-stopping link weights.  lo, hi: numbers or arrays, bounded_solve's.
    Returns a NEW array."""
    if not isinstance(values, np.ndarray) or values.dtype != np.float32:
        raise TypeError("values must be a float32 numpy array")
    m = _mask_of("known_mask", known_mask, values)
    gx, gy = (None, None) if image_gradients is None else image_gradients
    if guide is None and edge_sigma is not None:
        raise ValueError("edge_sigma needs a guide")
    sx = sy = None
    if guide is not None:
        g = np.asarray(guide, np.float64)
        if g.shape[:2] != values.shape[:2]:
            raise ValueError(f"guide has shape {g.shape[:2]}, the image {values.shape[:2]}")
        sigma = 0.1 * float(g.max() - g.min()) if edge_sigma is None else float(edge_sigma)
        if not np.isfinite(sigma) or not sigma > 0:
            raise ValueError("edge_sigma must be finite and > 0 (None: a tenth of the guide's range, which must not be flat)")
        sx, sy = ((np.exp(-d * d / (2.0 * sigma * sigma)) + 1e-3).astype(np.float32) for d in _forward_abs_differences(g))
    return bounded_solve(values, m, lo, hi, gx=gx, gy=gy, smooth_x=sx, smooth_y=sy, neumann=True, gpu_id=gpu_id, **solver)
