#!/usr/bin/env python3
"""Measures the volume solve (sc_hip_volume*).

--lengths  GPU: ERR, RES (tests/volume_bounds.py) and the iteration count beside the reference iteration's over the GPU tests' own inputs
           (tests/volume_bounds.py's matrix(): five borders x four sizes twice, frames, channels, tau, the five state patterns, the
           weights and the three forms of the right-hand side rotating; NaN in every element that is not read), the same borders and
           sizes with every state 0 under a constant weight (the reference iteration takes no step: the floors), and a length walk
           along x, along y and along the frames (Neumann and free left + top; scatter and split): one line per input, then the worst
           ratios and the worst values where the reference iteration took no step -- what RES_FACTOR / RES_FLOOR / ERR_FACTOR /
           ERR_FLOOR are set from.  Written to --lengths-out (default profiles/volume_lengths.txt).
--time     GPU: iterations and stream time (sc_run_info.ms_solve of host calls, median of --calls after --warmup) at 512^2 x 3 channels x
           16 frames and 1024^2 x 1 channel x 32 frames, Neumann borders, zero guidance, tau = 1: both keyframes known, a hole moving
           across the frames, and 1 in 30 known pixels scattered around an excluded tube.  JSON lines appended to --time-out (default
           profiles/volume_probe.json).
--kernels  GPU: one scatter volume of 512^2 x 1 x 16 frames and one scatter region image of 2048^2 x 1 -- the same number of pixels --
           each solved once, for a kernel trace taken around this process: the volume operator beside the WLS operator per unknown, the
           two transforms along the frames as a share of one application of the preconditioner.
--hash     GPU: sha256 of sc_hip_volume's out, and the iteration count, on seeded inputs -- the inputs of tests/volume_bounds.py's matrix()
           with NaN in every element that is not read, and three 384 x 256 x 3 x 8 volumes (keyframes, moving hole, scatter) -- one line
           each on standard output.  With --tree DIR the package and library of another build of this repository (tools/ab_trees.sh
           build) are loaded in place of this tree's; two such listings compare equal when the two builds write the same bytes.

    python tools/volume_probe.py --lengths --time [--calls 3] [--warmup 1]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
WALK = [2, 3, 4, 5, 8, 9, 31, 32, 33, 64, 65]
FRAME_WALK = [2, 3, 4, 7, 8, 9, 16, 17, 33, 64]


def volume_call(inst, p, form, **kw):
    import volume_bounds as vb
    import volume_np
    b = p["boundary"] if volume_np.has_dirichlet(p["sides"], p["periodic"]) else None
    return inst.volume(p["data"], p["state"], p["weight"], boundary=b, tau=p["tau"], free_sides=p["sides"], periodic=p["periodic"],
                       **vb.call_args(p, form), **kw)


def lengths(capi, inst, path):
    import volume_bounds as vb
    cases = [c + (0,) for c in vb.matrix()]
    cases += [(border, H, W, 3, vb.FRAMES[(i + j) % 4], vb.TAUS[(i + j) % 3], "none", "constant", vb.FORMS[(i + j) % 3], 0)
              for i, (border, _, _) in enumerate(vb.BORDERS) for j, (H, W) in enumerate(vb.SIZES) if not (border == "frame" and min(H, W) < 3)]
    for border in (vb.BORDERS[0][0], vb.BORDERS[2][0]):
        for i, n in enumerate(WALK):
            for pattern, wk in (("scatter", None), ("split", "sparse")):
                cases += [(border, 7, n, 3, 3, vb.TAUS[i % 3], pattern, wk, "lap", 1), (border, n, 6, 3, 4, vb.TAUS[(i + 1) % 3], pattern, wk, "gt", 1)]
        for i, T in enumerate(FRAME_WALK):
            for pattern, wk in (("scatter", None), ("keyframes", "sparse"), ("hole", None)):
                cases.append((border, 7, 9, 3 if T <= 64 else 1, T, vb.TAUS[i % 3], pattern, wk, "gt", 1))
    lines = ["# volume solve, float32: ERR, RES (tests/volume_bounds.py) and iterations beside the reference iteration's",
             "# (volume_np.pcg_f32, tol 1e-5) on the same input; one MI355X run of python tools/volume_probe.py --lengths",
             "VLEN border W H C T tau pattern weights form | ERR (x pcg_f32) RES (x pcg_f32) sweeps / pcg_f32 ERR RES iterations"]
    worst = {"err_ratio": (0, None), "res_ratio": (0, None), "err_zero": (0, None), "res_zero": (0, None), "sweeps_over": (-99, None)}
    for border, H, W, C, T, tau, pattern, wk, form, seed in cases:
        if pattern == "none":
            p = vb.make_input(border, H, W, C, T, tau, "hole", wk, seed)
            p["state"] = np.zeros_like(p["state"])
        else:
            p = vb.make_input(border, H, W, C, T, tau, pattern, wk, seed)
        p = vb.nan_unread(p)
        y = vb.Yardstick(p, form)
        out = volume_call(inst, p, form)
        sweeps = inst.info().sweeps
        err, res = y.measure(out)
        er, rr = err / y.err32 if y.err32 else float("inf"), res / y.res32 if y.res32 else float("inf")
        tag = f"{border} {W}x{H}x{C}x{T} tau {tau:g} {pattern} {wk} {form}"
        lines.append(f"VLEN {border:11s} {W:3d} {H:3d} {C} {T:3d} {tau:4g} {pattern:9s} {str(wk):9s} {form:8s} | ERR {err:.2e} (x{er:.2f}) RES {res:.2e} (x{rr:.2f}) "
                     f"sweeps {sweeps:3d} / pcg_f32 {y.err32:.2e} {y.res32:.2e} {y.iters32:3d}")
        print(lines[-1], flush=True)
        if y.iters32 == 0:
            worst["err_zero"] = max(worst["err_zero"], (err, tag))
            worst["res_zero"] = max(worst["res_zero"], (res, tag))
        else:
            worst["err_ratio"] = max(worst["err_ratio"], (er, tag))
            worst["res_ratio"] = max(worst["res_ratio"], (rr, tag))
        worst["sweeps_over"] = max(worst["sweeps_over"], (sweeps - y.max_sweeps(), tag))
    for k, (v, tag) in worst.items():
        lines.append(f"VLEN worst {k}: {v:.4g} ({tag})")
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def big_state(case, T, H, W, C):
    """float32 T x H x W x C of one timing case"""
    y, x = np.mgrid[0:H, 0:W]
    st = np.zeros((T, H, W), np.float32)
    if case == "keyframes":
        st[0], st[-1] = 1, 1
    elif case == "hole":                       # a hole 0.2 of the side across, moving from left to right
        for t in range(T):
            cx = W * (0.25 + 0.5 * t / (T - 1))
            st[t] = np.where((y - H / 2) ** 2 + (x - cx) ** 2 <= (0.1 * min(H, W)) ** 2, 0, 1)
    elif case == "scatter":
        rng = np.random.default_rng(77)
        st[...] = rng.random((T, H, W)) < 1 / 30
        st[:, (y - 0.3 * H) ** 2 + (x - 0.65 * W) ** 2 <= (0.18 * min(H, W)) ** 2] = 2
    else:
        raise ValueError(case)
    return np.ascontiguousarray(np.broadcast_to(st[:, :, :, None], (T, H, W, C)))


def big_data(T, H, W, C, rng):
    yy, xx = np.mgrid[0:H, 0:W]
    smooth = np.stack([np.sin((xx + 3 * t) / 37.0) + np.cos(yy / 53.0) for t in range(T)])[:, :, :, None] * np.ones((1, 1, 1, C))
    return (smooth + 0.05 * rng.standard_normal((T, H, W, C))).astype(np.float32)


def timing(capi, inst, path, calls, warmup):
    rng = np.random.default_rng(5)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "a") as f:
        for T, H, W, C in ((16, 512, 512, 3), (32, 1024, 1024, 1)):
            data = big_data(T, H, W, C, rng)
            lap = np.zeros((T, H, W, C), np.float32)
            for case in ("keyframes", "hole", "scatter"):
                st = big_state(case, T, H, W, C)
                ms, its = [], []
                for k in range(warmup + calls):
                    inst.volume(data, st, lap=lap, tau=1.0, neumann=True, allow_not_converged=True)
                    info = inst.info()
                    if k >= warmup:
                        ms.append(info.ms_solve)
                        its.append(info.sweeps)
                rec = dict(probe="volume", size=[W, H, C, T], tau=1.0, case=case, unknown=int((st == 0).sum()), iterations=its[-1],
                           converged=int(info.converged), rel_residual=float(info.rel_residual), ms_solve=float(np.median(ms)))
                f.write(json.dumps(rec) + "\n")
                f.flush()
                print(json.dumps(rec), flush=True)


def kernels(capi, inst):
    rng = np.random.default_rng(6)
    T, H, W = 16, 512, 512
    data = big_data(T, H, W, 1, rng)
    inst.volume(data, big_state("scatter", T, H, W, 1), lap=np.zeros_like(data), tau=1.0, neumann=True, allow_not_converged=True)
    print("volume", T, H, W, "iterations", inst.info().sweeps, flush=True)
    flat = big_data(1, 2048, 2048, 1, rng)[0]
    inst.region(flat, big_state("scatter", 1, 2048, 2048, 1)[0], lap=np.zeros_like(flat), neumann=True, allow_not_converged=True)
    print("region 2048 2048 iterations", inst.info().sweeps, flush=True)


def hashes(capi, inst):
    import hashlib
    import volume_bounds as vb
    for i, (border, H, W, C, T, tau, pattern, wk, form) in enumerate(vb.matrix()):
        p = vb.nan_unread(vb.make_input(border, H, W, C, T, tau, pattern, wk))
        out = volume_call(inst, p, form)
        print("HASH", i, border, W, H, C, T, form, inst.info().sweeps, hashlib.sha256(out.tobytes()).hexdigest(), flush=True)
    T, H, W, C = 8, 256, 384, 3
    data = big_data(T, H, W, C, np.random.default_rng(5))
    for case in ("keyframes", "hole", "scatter"):
        out = inst.volume(data, big_state(case, T, H, W, C), lap=np.zeros_like(data), tau=1.0, neumann=True, allow_not_converged=True)
        print("HASH", case, W, H, C, T, inst.info().sweeps, hashlib.sha256(out.tobytes()).hexdigest(), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lengths", action="store_true")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--hash", action="store_true")
    ap.add_argument("--tree", default=None, help="with --hash: another build of this repository whose package is loaded")
    ap.add_argument("--lengths-out", default=os.path.join(ROOT, "profiles", "volume_lengths.txt"))
    ap.add_argument("--time-out", default=os.path.join(ROOT, "profiles", "volume_probe.json"))
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    if a.tree:
        sys.path.insert(0, os.path.abspath(a.tree))
    from seamlesscloneoptimization_amd import capi
    if a.tree and not os.path.abspath(capi.__file__).startswith(os.path.abspath(a.tree) + os.sep):
        raise SystemExit(f"--tree {a.tree}: the package was loaded from {capi.__file__}")
    inst = capi.Instance(0)
    try:
        if a.lengths:
            lengths(capi, inst, a.lengths_out)
        if a.time:
            timing(capi, inst, a.time_out, a.calls, a.warmup)
        if a.kernels:
            kernels(capi, inst)
        if a.hash:
            hashes(capi, inst)
    finally:
        inst.destroy()


if __name__ == "__main__":
    main()
