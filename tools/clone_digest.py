#!/usr/bin/env python3
"""Prints one line per case, "<case name> <SHA-256>", for multigrid clones, batches, one Poisson solve and one colorChange with fixed
seeds: the smallest ROIs that reach every form of the level-0 cycle launch (csrc/sc_cycle0.hip) under every solver option that
selects one.  The hash covers the destination bytes and, from sc_run_info, sweeps, sweep_launches, field_retry and method: two
builds on the same GPU and ROCm run the same launches and compute the same bits exactly when their outputs are equal line for line.

    python tools/clone_digest.py [--root DIR] > profiles/clone_digest_<build>.txt      (--root: another checkout's built package)
"""
import argparse
import hashlib
import os
import sys

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.abspath(ap.parse_args().root))

from seamlesscloneoptimization_amd import capi  # noqa: E402


def images(W, H, seed, margin=32):
    """destination (H + margin) x (W + margin), patch and all-255 mask (H + 2) x (W + 2): a W x H ROI"""
    rng = np.random.default_rng([seed, W, H])
    Hd, Wd = H + margin, W + margin
    yy, xx = np.mgrid[0:Hd, 0:Wd]
    dst = np.clip((128.0 + 60.0 * np.sin(2 * np.pi * xx / Wd) * np.cos(2 * np.pi * yy / Hd))[:, :, None] + rng.normal(0.0, 12.0, (Hd, Wd, 3)), 0, 255).astype(np.uint8)
    yy, xx = np.mgrid[0:H + 2, 0:W + 2]
    patch = np.clip((110.0 + 50.0 * np.cos(3 * np.pi * xx / W))[:, :, None] + rng.normal(0.0, 20.0, (H + 2, W + 2, 3)), 0, 255).astype(np.uint8)
    return dst, patch, np.full((H + 2, W + 2), 255, np.uint8), Wd // 2, Hd // 2


def emit(name, data, info):
    h = hashlib.sha256(data)
    h.update(("|%d %d %d %d" % (info.sweeps, info.sweep_launches, info.field_retry, info.method)).encode())
    print(name, h.hexdigest(), flush=True)


F = capi
OPTIONS = [("defaults", {}, 0),
           ("float_field", {}, F.SC_FLAG_FLOAT_FIELD), ("float_l1", {}, F.SC_FLAG_FLOAT_L1), ("float_rhs_u0", {}, F.SC_FLAG_FLOAT_RHS | F.SC_FLAG_FLOAT_U0),
           ("no_compose_l1", {}, F.SC_FLAG_NO_COMPOSE_L1), ("keep_field", {}, F.SC_FLAG_KEEP_FIELD),
           ("level1_sweeps_3", dict(mg_level1_sweeps=3), 0), ("pre_post_1", dict(mg_pre=1, mg_post=1), 0), ("max_sweeps_1", dict(max_sweeps=1), 0),
           ("update_tol_1e-4", dict(update_tol=1e-4), 0),      # the judged cycle is rejected: the catch-up launch and the re-launch as a field
           ("tol_1e-6", dict(tol=1e-6), 0),                    # the float path with the residual stop
           ("sweeps_per_launch_1", dict(sweeps_per_launch=1), 0)]      # the unfused cycle, as a control
OPTIONS += [("legacy_%d" % bit, dict(legacy_paths=bit), F.SC_FLAG_LEGACY_PATHS)
            for bit in (F.SC_LEGACY_SEPARATE_RESTRICT, F.SC_LEGACY_BOTTOM_F32, F.SC_LEGACY_SEPARATE_TAIL)]


def configure(inst, kw=None, flags=0):
    d = inst.default_opts()
    inst.set_solver(**dict({f[0]: getattr(d, f[0]) for f in d._fields_}, method=capi.SC_METHOD_MULTIGRID, flags=d.flags | flags, **(kw or {})))


def clone(inst, name, W, H, seed):
    dst, patch, mask, cx, cy = images(W, H, seed)
    body = dst.copy()
    rc = inst.run(patch, body, mask, cx, cy, allow_not_converged=True)
    emit("%s rc=%d" % (name, rc), body.tobytes(), inst.info())


def batch(inst, name, sizes, seed):
    items = [images(W, H, seed + k) for k, (W, H) in enumerate(sizes)]
    jobs = capi.Pool.make_jobs(len(items))
    keep = []
    for j, (dst, patch, mask, cx, cy) in zip(jobs, items):
        f, b, m = inst.to_device(patch), inst.to_device(dst), inst.to_device(mask)
        keep.append((f, b, m))
        j.face, j.face_cols, j.face_rows, j.face_step = f, patch.shape[1], patch.shape[0], 3 * patch.shape[1]
        j.body, j.body_cols, j.body_rows, j.body_step = b, dst.shape[1], dst.shape[0], 3 * dst.shape[1]
        j.mask, j.mask_cols, j.mask_rows, j.mask_step = m, mask.shape[1], mask.shape[0], mask.shape[1]
        j.centerX, j.centerY = cx, cy
    rc = inst.run_device_batch(jobs)
    info = inst.info()
    out = b"".join(inst.from_device(b, it[0].shape).tobytes() for (_, b, _), it in zip(keep, items))
    for ptrs in keep:
        for p in ptrs:
            inst.free(p)
    emit("%s rc=%d members=%d ragged=%d" % (name, rc, info.group_members, info.group_ragged), out, info)


def main():
    inst = capi.Instance(0)
    try:
        for oname, kw, flags in OPTIONS:
            configure(inst, kw, flags)
            for W, H in ((300, 194), (203, 141), (100, 80)):      # level 1 composed; the same with ragged last intervals; level 1 solved directly
                clone(inst, "clone %dx%d %s" % (W, H, oname), W, H, 1)
        configure(inst)
        clone(inst, "clone 723x722 defaults", 723, 722, 2)          # a deeper ladder
        clone(inst, "clone 2048x2048 defaults", 2048, 2048, 3)      # level 1 in sixteen-wave workgroups
        batch(inst, "batch 16 x 300x194", [(300, 194)] * 16, 10)    # a same-size group
        rng = np.random.default_rng(5)
        batch(inst, "batch 8 x [280..320]x[180..200]", [(int(rng.integers(280, 321)), int(rng.integers(180, 201))) for _ in range(8)], 40)      # a size class
        rng = np.random.default_rng(6)
        H, W = 141, 203
        b, gx, gy = (rng.uniform(lo, hi, (H, W, 3)).astype(np.float32) for lo, hi in ((0, 255), (-20, 20), (-20, 20)))
        out = inst.poisson(b, gx=gx, gy=gy, allow_not_converged=True)
        emit("poisson dirichlet multigrid 203x141x3", np.ascontiguousarray(out).tobytes(), inst.info())
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        mask = np.zeros((H, W), np.uint8)
        mask[9:-11, 7:-5] = 255
        out = inst.edit(inst.edit_params(capi.SC_EDIT_COLOR_CHANGE, red_mul=1.5, green_mul=0.7, blue_mul=1.1), img, mask, allow_not_converged=True)
        emit("colorChange 203x141", out.tobytes(), inst.info())
        # a same-size group whose judged launch may write the interleaved bytes itself (C0_OUT3): by the default rule, forced, and through the splice launch
        for oname, bit in (("defaults", 0), ("forced_interleaved", getattr(F, "SC_FORCE_INTERLEAVED_OUT", None)), ("legacy_splice", getattr(F, "SC_LEGACY_SPLICE_LAUNCH", None))):
            if bit is None:      # (--root: a build from before these switches)
                continue
            configure(inst, dict(legacy_paths=bit), F.SC_FLAG_LEGACY_PATHS if bit else 0)
            batch(inst, "batch 16 x 470x300 %s" % oname, [(470, 300)] * 16, 70)
        # ... and whose first launch may read the destinations' bytes itself (C0_IN3): by the default rule, forced, and from float16 planes
        for oname, bit in (("u0_defaults", 0), ("u0_forced_bytes", getattr(F, "SC_FORCE_U0_BYTES", None)), ("u0_legacy_planes", getattr(F, "SC_LEGACY_U0_PLANES", None))):
            if bit is None:
                continue
            configure(inst, dict(legacy_paths=bit), F.SC_FLAG_LEGACY_PATHS if bit else 0)
            batch(inst, "batch 16 x 470x300 %s" % oname, [(470, 300)] * 16, 70)
    finally:
        inst.destroy()


if __name__ == "__main__":
    main()
