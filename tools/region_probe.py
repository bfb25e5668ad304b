#!/usr/bin/env python3
"""Measures the region solve (sc_hip_region*).

--walk     CPU only, numpy: the reference iteration's count (region_np.pcg_f32, tol 1e-5) over the GPU tests' own inputs with the
           preconditioner's w-bar at 1/4, 1/2, 1, 2 and 4 times the automatic value (sum of w + sum of the UNKNOWN - KNOWN links) /
           (UNKNOWN pixels): one line per input, then per factor the inputs on which it needs at least a quarter fewer iterations than
           the automatic value.  Written to --walk-out (default profiles/region_lambda_walk.txt).
--lengths  GPU: ERR, RES (tests/region_bounds.py) and the iteration count beside the reference iteration's over the GPU tests' own inputs
           (tests/region_bounds.py's matrix(): five borders x four sizes x four state patterns with 3 channels, links and weights rotating
           through none / constant / log-uniform and none / constant / sparse, both forms of the right-hand side, and every links x weights
           pair with 1 channel; NaN in every element that is not read), the same sizes with every state 0
           under constant links and a constant weight (the reference iteration takes no step: the floors), and a length walk along x and
           along y (Neumann and free left + top; scatter and split): one line per input, then the worst ratios and the worst values where
           the reference iteration took no step -- what RES_FACTOR / RES_FLOOR / ERR_FACTOR / ERR_FLOOR are set from.  Written to
           --lengths-out (default profiles/region_lengths.txt).
--time     GPU: iterations, stream time (sc_run_info.ms_solve) and wall time of host calls (medians of --calls after --warmup) at 1024^2 x 3 channels
           and 2048^2 x 1 channel, Neumann borders, unit links, zero guidance: an ellipse of unknowns, 1 in 30 known pixels scattered
           plus an excluded blob, a known frame plus an excluded blob, and the membrane fill of a hole 200 pixels across.  Beside each
           the only other route to the same answer: the soft constraint w = 1e4 at the pinned pixels through sc_hip_weighted (through
           sc_hip_wls with links of 1e-4 around the excluded pixels where there are any: it refuses a zero link) -- its iterations, time
           and its distance from the hard-constraint answer, max over the UNKNOWN pixels / max |answer|.  JSON lines appended to --time-out
           (default profiles/region_probe.json).

    python tools/region_probe.py --walk
    python tools/region_probe.py --lengths --time [--calls 5] [--warmup 1]
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
WALK = [2, 3, 4, 5, 8, 9, 24, 25, 31, 32, 33, 40, 41, 63, 64, 65]
FACTORS = [0.25, 0.5, 1.0, 2.0, 4.0]


def walk(path):
    import region_bounds as rb
    import region_np
    lines = ["# region solve: iterations of the reference iteration (region_np.pcg_f32, float32, tol 1e-5) with w-bar at a multiple of the",
             "# automatic value, over the GPU tests' inputs; python tools/region_probe.py --walk (CPU only)",
             "RWALK border W H C pattern weights links form | w-bar s-bar | iterations at x0.25 x0.5 x1 x2 x4"]
    better = {f: [] for f in FACTORS}
    worst = 0
    for border, H, W, C, pattern, wk, sk, form in rb.matrix():
        p = rb.make_input(border, H, W, C, pattern, wk, sk)
        args = rb.np_args(p, form)
        b = p["boundary"] if region_np.has_dirichlet(p["sides"], p["periodic"]) else None
        sbar, wbar, _, _ = region_np.precond_means(*args[:6])
        its = [region_np.pcg_f32(*args, b, precond_lambda=f * wbar)[1] for f in FACTORS]
        worst = max(worst, its[2])
        for f, n in zip(FACTORS, its):
            if f != 1.0 and its[2] > 0 and n <= 0.75 * its[2]:
                better[f].append(f"{border} {W}x{H} {pattern}")
        lines.append(f"RWALK {border:11s} {W:3d} {H:3d} {C} {pattern:8s} {str(wk):9s} {str(sk):10s} {form:8s} | {wbar:.3g} {sbar:.3g} | " + " ".join(f"{n:3d}" for n in its))
        print(lines[-1], flush=True)
    n = len(lines) - 3
    for f in FACTORS:
        if f != 1.0:
            lines.append(f"RWALK x{f:g}: at least a quarter fewer iterations than the automatic value on {len(better[f])} of {n} inputs" +
                         (": " + "; ".join(better[f]) if better[f] else ""))
    lines.append(f"RWALK the automatic value's worst count: {worst}")
    for l in lines[-5:]:
        print(l, flush=True)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def region_call(inst, p, form, **kw):
    import region_np
    b = p["boundary"] if region_np.has_dirichlet(p["sides"], p["periodic"]) else None
    g = dict(gx=p["gx"], gy=p["gy"]) if form == "guidance" else dict(lap=p["lap"])
    return inst.region(p["data"], p["state"], p["weight"], p["sx"], p["sy"], boundary=b, free_sides=p["sides"], periodic=p["periodic"], **g, **kw)


def lengths(capi, inst, path):
    import region_bounds as rb
    cases = [c + (0,) for c in rb.matrix()]
    cases += [(border, H, W, 3, "none", "constant", "constant", "lap", 0) for border, _, _ in rb.BORDERS for (H, W) in rb.SIZES
              if not (border == "frame" and min(H, W) < 3)]
    for border in (rb.BORDERS[0][0], rb.BORDERS[2][0]):
        for n in WALK:
            for pattern, wk, sk in (("scatter", None, "loguniform"), ("split", "sparse", None)):
                cases += [(border, 7, n, 3, pattern, wk, sk, "lap", 1), (border, n, 6, 3, pattern, wk, sk, "guidance", 1)]
    lines = ["# region solve, float32: ERR, RES (tests/region_bounds.py) and iterations beside the reference iteration's",
             "# (region_np.pcg_f32, tol 1e-5) on the same input; one MI355X run of python tools/region_probe.py --lengths",
             "RLEN border W H C pattern weights links form | ERR (x pcg_f32) RES (x pcg_f32) sweeps / pcg_f32 ERR RES iterations"]
    worst = {"err_ratio": (0, None), "res_ratio": (0, None), "err_zero": (0, None), "res_zero": (0, None), "sweeps_over": (-99, None)}
    for border, H, W, C, pattern, wk, sk, form, seed in cases:
        if pattern == "none":
            p = rb.make_input(border, H, W, C, "ellipse", wk, sk, seed)
            p["state"] = np.zeros_like(p["state"])
        else:
            p = rb.make_input(border, H, W, C, pattern, wk, sk, seed)
        p = rb.nan_unread(p)
        y = rb.Yardstick(p, form)
        out = region_call(inst, p, form)
        sweeps = inst.info().sweeps
        err, res = y.measure(out)
        er, rr = err / y.err32 if y.err32 else float("inf"), res / y.res32 if y.res32 else float("inf")
        tag = f"{border} {W}x{H}x{C} {pattern} {wk} {sk} {form}"
        lines.append(f"RLEN {border:11s} {W:3d} {H:3d} {C} {pattern:8s} {str(wk):9s} {str(sk):10s} {form:8s} | ERR {err:.2e} (x{er:.2f}) RES {res:.2e} (x{rr:.2f}) "
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
        lines.append(f"RLEN worst {k}: {v:.4g} ({tag})")
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def big_state(case, H, W, C):
    """float32 H x W x C of one timing case"""
    import region_bounds as rb
    rng = np.random.default_rng(77)
    y, x = np.mgrid[0:H, 0:W]
    blob = (y - 0.3 * H) ** 2 + (x - 0.65 * W) ** 2 <= (0.18 * min(H, W)) ** 2
    if case in ("ellipse", "scatter"):
        return rb.pattern_state(case, H, W, C, rng)
    st = np.zeros((H, W), np.float32)
    if case == "frame_blob":
        st[0], st[-1], st[:, 0], st[:, -1] = 1, 1, 1, 1
        st[blob] = 2
    elif case == "inpaint200":
        st[...] = 1
        st[(y - H / 2) ** 2 + (x - W / 2) ** 2 <= 100.0 ** 2] = 0
    else:
        raise ValueError(case)
    return np.ascontiguousarray(np.broadcast_to(st[:, :, None], (H, W, C)))


def timing(capi, inst, path, calls, warmup):
    rng = np.random.default_rng(5)
    med = lambda v: float(np.median(v))
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "a") as f:
        for H, W, C in ((1024, 1024, 3), (2048, 2048, 1)):
            yy, xx = np.mgrid[0:H, 0:W]
            smooth = (np.sin(xx / 37.0) + np.cos(yy / 53.0))[:, :, None] * np.ones((1, 1, C))
            data = (smooth + 0.05 * rng.standard_normal((H, W, C))).astype(np.float32)
            lap = np.zeros((H, W, C), np.float32)
            for case in ("ellipse", "scatter", "frame_blob", "inpaint200"):
                st = big_state(case, H, W, C)
                unk = st == 0
                ms, wall, its = [], [], []
                for k in range(warmup + calls):
                    t0 = time.perf_counter()
                    out = inst.region(data, st, lap=lap, neumann=True, allow_not_converged=True)
                    t1 = time.perf_counter()
                    info = inst.info()
                    if k >= warmup:
                        ms.append(info.ms_solve)
                        wall.append(1e3 * (t1 - t0))
                        its.append(info.sweeps)
                rec = dict(probe="region", size=[W, H, C], case=case, unknown=int(unk.sum()), iterations=its[-1], converged=int(info.converged),
                           rel_residual=float(info.rel_residual), ms_solve=med(ms), ms_wall=med(wall))
                # the soft route: w = 1e4 at the pinned pixels
                w = np.where(st == 1, np.float32(1e4), np.float32(0)).astype(np.float32)
                soft_ms, soft = [], None
                for k in range(warmup + calls):
                    if (st == 2).any():
                        out_x = (st == 2) | np.roll(st == 2, -1, 1)
                        out_y = (st == 2) | np.roll(st == 2, -1, 0)
                        sx, sy = (np.where(m, np.float32(1e-4), np.float32(1)).astype(np.float32) for m in (out_x, out_y))
                        soft = inst.wls(data, w, sx, sy, lap=lap, neumann=True, allow_not_converged=True)
                        rec["soft_call"] = "sc_hip_wls"
                    else:
                        soft = inst.weighted(data, w, lap=lap, neumann=True, allow_not_converged=True)
                        rec["soft_call"] = "sc_hip_weighted"
                    sinfo = inst.info()
                    if k >= warmup:
                        soft_ms.append(sinfo.ms_solve)
                scale = float(np.abs(out[unk]).max())
                rec.update(soft_iterations=int(sinfo.sweeps), soft_converged=int(sinfo.converged), soft_ms_solve=med(soft_ms),
                           soft_error=float(np.abs(soft.astype(np.float64) - out)[unk].max()) / scale)
                f.write(json.dumps(rec) + "\n")
                f.flush()
                print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--walk", action="store_true")
    ap.add_argument("--lengths", action="store_true")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--walk-out", default=os.path.join(ROOT, "profiles", "region_lambda_walk.txt"))
    ap.add_argument("--lengths-out", default=os.path.join(ROOT, "profiles", "region_lengths.txt"))
    ap.add_argument("--time-out", default=os.path.join(ROOT, "profiles", "region_probe.json"))
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    if a.walk:
        walk(a.walk_out)
    if a.lengths or a.time:
        from seamlesscloneoptimization_amd import capi
        inst = capi.Instance(0)
        try:
            if a.lengths:
                lengths(capi, inst, a.lengths_out)
            if a.time:
                timing(capi, inst, a.time_out, a.calls, a.warmup)
        finally:
            inst.destroy()


if __name__ == "__main__":
    main()
