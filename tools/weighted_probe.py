#!/usr/bin/env python3
"""Measures the weighted solve (sc_hip_weighted*) on the GPU.

--lengths  ERR, RES (tests/weighted_bounds.py) and the iteration count beside the reference iteration's (weighted_np.pcg_f32) over the
           GPU tests' own inputs (five borders x three sizes x three kinds of weights) and a length walk along x and along y
           (Neumann and free left + top, log-uniform and sparse weights): one line per input, then the worst ratios and, among the
           inputs where the reference iteration took no step, the worst values -- what RES_FACTOR / RES_FLOOR / ERR_FACTOR /
           ERR_FLOOR are set from.  Written to --lengths-out (default profiles/weighted_lengths.txt).
--time     device time of a bSync call on resident arrays at 1024^2 and 2048^2, C = 3, Neumann, log-uniform weights in [1e-2, 1]:
           calls of 4 and of 12 iterations (tol far below the float32 floor, so the budget ends them), their difference / 8 = the time
           per iteration; beside it one screened direct solve on the same arrays = the preconditioner step, and its share.  Median of
           --calls after --warmup.  Written as JSON lines to --time-out (default profiles/weighted_probe.json, appended).

    python tools/weighted_probe.py --lengths --time [--calls 9] [--warmup 2]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WALK = [2, 3, 4, 5, 8, 9, 24, 25, 31, 32, 33, 40, 41, 63, 64, 65]


def lengths(capi, inst, path):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import weighted_bounds as wb
    import weighted_np
    cases = [(name, s, p, H, W, wk, 0) for name, s, p in wb.BORDERS for (H, W) in wb.SIZES for wk in wb.WEIGHTS
             if not (name == "frame" and min(H, W) < 3)]
    for name, s, p in (wb.BORDERS[0], wb.BORDERS[2]):
        for n in WALK:
            for wk in ("loguniform", "sparse"):
                cases += [(name, s, p, 7, n, wk, 1), (name, s, p, n, 6, wk, 1)]
    lines = ["# weighted solve, float32: ERR, RES (tests/weighted_bounds.py) and iterations beside the reference iteration's",
             "# (weighted_np.pcg_f32, tol 1e-5) on the same input; one MI355X run of python tools/weighted_probe.py --lengths",
             "WLEN border W H weights | ERR (x pcg_f32) RES (x pcg_f32) sweeps / pcg_f32 ERR RES iterations"]
    worst = {"err_ratio": (0, None), "res_ratio": (0, None), "err_zero": (0, None), "res_zero": (0, None), "sweeps_over": (-99, None)}
    for name, s, p, H, W, wk, seed in cases:
        data, weight, lap, boundary = wb.make_input(H, W, 3, wk, seed)
        blk = weighted_np.unknowns(s, p, H, W)
        if not weighted_np.has_dirichlet(s, p) and (weight[blk].reshape(-1, 3).sum(0) == 0).any():
            weight[blk[0].start, blk[1].start] = 1.0          # (a walk input whose seed left a channel without weight)
        y = wb.Yardstick(s, p, weight, data, lap, boundary)
        b = boundary if weighted_np.has_dirichlet(s, p) else None
        out = inst.weighted(data, weight, lap=lap, boundary=b, free_sides=s, periodic=p)
        sweeps = inst.info().sweeps
        err, res = y.measure(out)
        er, rr = err / y.err32, res / y.res32
        tag = f"{name} {W}x{H} {wk}"
        lines.append(f"WLEN {name:11s} {W:3d} {H:3d} {wk:10s} | ERR {err:.2e} (x{er:.2f}) RES {res:.2e} (x{rr:.2f}) sweeps {sweeps:2d} / "
                     f"pcg_f32 {y.err32:.2e} {y.res32:.2e} {y.iters32:2d}")
        print(lines[-1], flush=True)
        if y.iters32 == 0:
            worst["err_zero"] = max(worst["err_zero"], (err, tag))
            worst["res_zero"] = max(worst["res_zero"], (res, tag))
        else:
            worst["err_ratio"] = max(worst["err_ratio"], (er, tag))
            worst["res_ratio"] = max(worst["res_ratio"], (rr, tag))
        worst["sweeps_over"] = max(worst["sweeps_over"], (sweeps - y.max_sweeps(), tag))
    for k, (v, tag) in worst.items():
        lines.append(f"WLEN worst {k}: {v:.4g} ({tag})")
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def timing(capi, inst, path, calls, warmup):
    recs = []
    for n in (1024, 2048):
        rng = np.random.default_rng(n)
        shape = (n, n, 3)
        data = rng.standard_normal(shape).astype(np.float32)
        lap = (0.1 * rng.standard_normal(shape)).astype(np.float32)
        weight = np.exp(rng.uniform(np.log(1e-2), 0.0, shape)).astype(np.float32)
        lay = capi.poisson_layout_of(data)
        dev = [inst.to_device(a) for a in (lap, data, weight)] + [inst.malloc(data.nbytes)]
        try:
            kind = capi.SC_POISSON_LAPLACIAN | capi.SC_POISSON_NEUMANN
            wj = capi.Instance.make_weighted_jobs(1)
            wj[0].lap, wj[0].data, wj[0].weight, wj[0].out = dev
            sj = capi.Instance.make_screened_jobs(1)
            sj[0].lap, sj[0].data, sj[0].out = dev[0], dev[1], dev[3]
            t = {4: [], 12: [], "direct": []}
            for i in range(warmup + calls):
                for iters in (4, 12):
                    inst.weighted_device(capi.WeightedParams(kind, 1e-30, iters, 0.0), lay, wj)
                    if i >= warmup:
                        t[iters].append(inst.info().ms_call)
                inst.screened_device(capi.ScreenedParams(kind, float(weight.mean())), lay, sj)
                if i >= warmup:
                    t["direct"].append(inst.info().ms_device_total)
            inst.weighted_device(capi.WeightedParams(kind, 0.0, 0, 0.0), lay, wj)
            full = inst.info()
            m4, m12, md = (float(np.median(t[k])) for k in (4, 12, "direct"))
            per = (m12 - m4) / 8.0
            recs.append({"probe": "weighted_time", "size": n, "channels": 3, "border": "neumann", "weights": "loguniform [1e-2, 1]",
                         "ms_call_4_iters": round(m4, 4), "ms_call_12_iters": round(m12, 4), "ms_per_iteration": round(per, 4),
                         "ms_direct_solve": round(md, 4), "preconditioner_share": round(md / per, 3),
                         "default_call": {"sweeps": full.sweeps, "rel_residual": full.rel_residual, "ms_call": round(full.ms_call, 4),
                                          "converged": full.converged}, "calls": calls})
            print(json.dumps(recs[-1]), flush=True)
        finally:
            for p in dev:
                inst.free(p)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "a") as f:
        for r in recs:
            f.write(json.dumps(r) + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lengths", action="store_true")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--lengths-out", default=os.path.join(ROOT, "profiles", "weighted_lengths.txt"))
    ap.add_argument("--time-out", default=os.path.join(ROOT, "profiles", "weighted_probe.json"))
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
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
