#!/usr/bin/env python3
"""Measures the WLS volume solve (sc_hip_volume_wls*).

--lengths  GPU: ERR, RES (tests/volume_wls_bounds.py) and the iteration count beside the reference iteration's over the GPU tests' own
           inputs (tests/volume_wls_bounds.py's matrix(); NaN in every element that is not read), the same borders and sizes with every
           state 0 under a constant weight and constant links (the reference iteration takes no step: the floors), and a length walk
           along x, along y and along the frames (Neumann and free left + top; scatter and split; the four link forms and the two kinds
           of time rotating): one line per input, then the worst ratios and the worst values where the reference iteration took no
           step -- what RES_FACTOR / RES_FLOOR / ERR_FACTOR / ERR_FLOOR are set from.  Written to --lengths-out (default
           profiles/volume_wls_lengths.txt).
--time     GPU: iterations, stream time (sc_run_info.ms_solve) and wall time of host calls (medians of --calls after --warmup) at 512^2 x 3 channels x
           16 frames and 1024^2 x 1 channel x 32 frames, Neumann borders, zero guidance, tau = 1, 1 in 30 known pixels scattered around
           an excluded tube: unit links (sc_hip_volume's problem through this call), wls_filter_video's links from the data's own
           log-luminance (their contrast is reported), links log-uniform over two decades, each under free and under periodic time.
           JSON lines appended to --time-out (default profiles/volume_wls_probe.json).
--kernels  GPU: the two-decade case at 512^2 x 1 x 16 frames under periodic time, solved once, for a kernel trace taken around this
           process.

    python tools/volume_wls_probe.py --lengths --time [--calls 3] [--warmup 1]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
WALK = [2, 3, 4, 5, 8, 9, 31, 32, 33, 64, 65]
FRAME_WALK = [3, 4, 7, 8, 9, 16, 17, 33, 64]


def wls_call(inst, p, form, **kw):
    import volume_wls_bounds as wb
    import volume_wls_np as vw
    b = p["boundary"] if vw.has_dirichlet(p["sides"], p["periodic"]) else None
    return inst.volume_wls(p["data"], p["state"], p["weight"], boundary=b, tau=p["tau"], free_sides=p["sides"], periodic=p["periodic"],
                           **wb.call_args(p, form), **kw)


def lengths(capi, inst, path):
    import volume_wls_bounds as wb
    cases = [c + (0,) for c in wb.matrix()]
    k = 0
    for i, (border, _, _) in enumerate(wb.BORDERS):
        for j, (H, W) in enumerate(wb.SIZES):
            if not (border == "frame" and min(H, W) < 3):
                T = wb.FRAMES[1 + (i + j) % 3]
                cases.append((border, H, W, 3, T, wb.TAUS[(i + j) % 3], "none", "constant", wb.FORMS[(i + j) % 3], "const", wb.TIMES[k % 2], 0))
                k += 1
    for border in (wb.BORDERS[0][0], wb.BORDERS[2][0]):
        for i, n in enumerate(WALK):
            for pattern, wk in (("scatter", None), ("split", "sparse")):
                cases += [(border, 7, n, 3, 3, wb.TAUS[i % 3], pattern, wk, "lap", wb.LINKS[1 + i % 3], wb.TIMES[i % 2], 1),
                          (border, n, 6, 3, 4, wb.TAUS[(i + 1) % 3], pattern, wk, "gt", wb.LINKS[1 + (i + 1) % 3], wb.TIMES[(i + 1) % 2], 1)]
        for i, T in enumerate(FRAME_WALK):
            for pattern, wk in (("scatter", None), ("keyframes", "sparse"), ("hole", None)):
                cases.append((border, 7, 9, 3, T, wb.TAUS[i % 3], pattern, wk, "gt", wb.LINKS[1 + i % 3], wb.TIMES[i % 2], 1))
    lines = ["# WLS volume solve, float32: ERR, RES (tests/volume_wls_bounds.py) and iterations beside the reference iteration's",
             "# (volume_wls_np.pcg_f32, tol 1e-5) on the same input; one MI355X run of python tools/volume_wls_probe.py --lengths",
             "VWLEN border W H C T tau pattern weights form links time | ERR (x pcg_f32) RES (x pcg_f32) sweeps / pcg_f32 ERR RES iterations"]
    worst = {"err_ratio": (0, None), "res_ratio": (0, None), "err_zero": (0, None), "res_zero": (0, None), "sweeps_over": (-99, None)}
    for border, H, W, C, T, tau, pattern, wk, form, links, time, seed in cases:
        if pattern == "none":          # every state 0, a constant weight, constant links 2.5 in space and 0.4 in time
            p = wb.make_input(border, H, W, C, T, tau, "hole", wk, "none", time, seed)
            p["state"] = np.zeros_like(p["state"])
            p["sx"] = p["sy"] = np.full(p["data"].shape, 2.5, np.float32)
            p["smt"] = np.full(p["gt"].shape, 0.4, np.float32)
        else:
            p = wb.make_input(border, H, W, C, T, tau, pattern, wk, links, time, seed)
        p = wb.nan_unread(p)
        y = wb.Yardstick(p, form)
        out = wls_call(inst, p, form)
        sweeps = inst.info().sweeps
        err, res = y.measure(out)
        er, rr = err / y.err32 if y.err32 else float("inf"), res / y.res32 if y.res32 else float("inf")
        tag = f"{border} {W}x{H}x{C}x{T} tau {tau:g} {pattern} {wk} {form} {links} {time}"
        lines.append(f"VWLEN {border:11s} {W:3d} {H:3d} {C} {T:3d} {tau:4g} {pattern:9s} {str(wk):9s} {form:8s} {links:5s} {time:8s} | ERR {err:.2e} (x{er:.2f}) "
                     f"RES {res:.2e} (x{rr:.2f}) sweeps {sweeps:3d} / pcg_f32 {y.err32:.2e} {y.res32:.2e} {y.iters32:3d}")
        print(lines[-1], flush=True)
        if y.iters32 == 0:
            worst["err_zero"] = max(worst["err_zero"], (err, tag))
            worst["res_zero"] = max(worst["res_zero"], (res, tag))
        else:
            worst["err_ratio"] = max(worst["err_ratio"], (er, tag))
            worst["res_ratio"] = max(worst["res_ratio"], (rr, tag))
        worst["sweeps_over"] = max(worst["sweeps_over"], (sweeps - y.max_sweeps(), tag))
    for k, (v, tag) in worst.items():
        lines.append(f"VWLEN worst {k}: {v:.4g} ({tag})")
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def big_links(kind, data, loop):
    """(sx, sy, smt, contrast) of one timing case: float32 T x H x W (smt: T - 1 frames, loop: T), contrast = the largest over the smallest
    link; None, None, None, 1 for unit links"""
    from seamlesscloneoptimization_amd import seamless_clone as sc
    import volume_wls_bounds as wb
    T, H, W = data.shape[:3]
    tshape = ((T if loop else T - 1), H, W)
    if kind == "unit":
        return None, None, None, 1.0
    if kind == "two_decades":
        links = [wb.loguniform((T, H, W), 31), wb.loguniform((T, H, W), 32), wb.loguniform(tshape, 33)]
    elif kind == "wls_filter":          # wls_filter_video's: lam / (|forward difference of log-luminance|^alpha + eps), lam 1, alpha 1.2, eps 1e-4
        lum = np.log(np.maximum(np.asarray(data, np.float64).mean(3), 0.0) + 1e-6)
        links = [(1.0 / (d ** 1.2 + 1e-4)).astype(np.float32) for d in sc._video_abs_differences(lum, loop)]
    else:
        raise ValueError(kind)
    live = np.concatenate([links[0][:, :, :-1].ravel(), links[1][:, :-1].ravel(), links[2].ravel()])
    return links[0], links[1], links[2], float(live.max() / live.min())


def timing(capi, inst, path, calls, warmup):
    import volume_probe
    rng = np.random.default_rng(5)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "a") as f:
        for T, H, W, C in ((16, 512, 512, 3), (32, 1024, 1024, 1)):
            data = volume_probe.big_data(T, H, W, C, rng) + np.float32(2.5)          # (positive: a luminance)
            lap = np.zeros((T, H, W, C), np.float32)
            st = volume_probe.big_state("scatter", T, H, W, C)
            for kind in ("unit", "wls_filter", "two_decades"):
                for loop in (False, True):
                    sx, sy, smt, contrast = big_links(kind, data, loop)
                    ms, wall, its = [], [], []
                    for k in range(warmup + calls):
                        t0 = time.perf_counter()
                        inst.volume_wls(data, st, None, sx, sy, smt, lap=lap, tau=1.0, loop=loop, neumann=True, allow_not_converged=True)
                        t1 = time.perf_counter()
                        info = inst.info()
                        if k >= warmup:
                            ms.append(info.ms_solve)
                            wall.append(1e3 * (t1 - t0))
                            its.append(info.sweeps)
                    rec = dict(probe="volume_wls", size=[W, H, C, T], tau=1.0, links=kind, contrast=contrast, time="periodic" if loop else "free",
                               unknown=int((st == 0).sum()), iterations=its[-1], converged=int(info.converged), rel_residual=float(info.rel_residual),
                               ms_solve=float(np.median(ms)), ms_wall=float(np.median(wall)))
                    f.write(json.dumps(rec) + "\n")
                    f.flush()
                    print(json.dumps(rec), flush=True)


def kernels(capi, inst):
    import volume_probe
    rng = np.random.default_rng(6)
    T, H, W = 16, 512, 512
    data = volume_probe.big_data(T, H, W, 1, rng)
    sx, sy, smt, _ = big_links("two_decades", data, True)
    inst.volume_wls(data, volume_probe.big_state("scatter", T, H, W, 1), None, sx, sy, smt, lap=np.zeros_like(data), tau=1.0, loop=True, neumann=True,
                    allow_not_converged=True)
    print("volume_wls periodic", T, H, W, "iterations", inst.info().sweeps, flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lengths", action="store_true")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--lengths-out", default=os.path.join(ROOT, "profiles", "volume_wls_lengths.txt"))
    ap.add_argument("--time-out", default=os.path.join(ROOT, "profiles", "volume_wls_probe.json"))
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    from seamlesscloneoptimization_amd import capi
    inst = capi.Instance(0)
    try:
        if a.lengths:
            lengths(capi, inst, a.lengths_out)
        if a.time:
            timing(capi, inst, a.time_out, a.calls, a.warmup)
        if a.kernels:
            kernels(capi, inst)
    finally:
        inst.destroy()


if __name__ == "__main__":
    main()
