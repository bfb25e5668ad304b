#!/usr/bin/env python3
"""Measures the WLS solve (sc_hip_wls*) on the GPU.

--lengths  ERR, RES (tests/wls_bounds.py) and the iteration count beside the reference iteration's (wls_np.pcg_f32) over the GPU
           tests' own inputs (five borders x four sizes x three kinds of links x two kinds of data weights, NaN in the dead links) and
           a length walk along x and along y (Neumann and free left + top; log-uniform links with sparse weights, edge links with a
           constant weight): one line per input, then the worst ratios and, among the inputs where the reference iteration took no
           step, the worst values -- what RES_FACTOR / RES_FLOOR / ERR_FACTOR / ERR_FLOOR are set from.  Written to --lengths-out
           (default profiles/wls_lengths.txt).
--time     device time of bSync calls on resident arrays at 1024^2, C = 3, Neumann, data weights log-uniform in [1e-2, 1]
           (tools/weighted_probe.py's): per kind of links (log-uniform over two decades; edges: tests/wls_bounds.py's checkerboard) a
           default call's iterations and time, and calls of 4 and of 12 iterations (tol far below the float32 floor, so the budget ends
           them), their difference / 8 = the time per iteration; beside them the same three figures of sc_hip_weighted on the same
           data weights.  The two families' iterations differ in the operator launch alone (k_pcg_op with WlsCoef, five plane
           transfers, for WeightedCoef's three).  Median of --calls after --warmup.  Written as JSON lines to --time-out (default
           profiles/wls_probe.json, appended).
           Kernel times: the same leg under  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/wls_probe.py --time --calls 3

    python tools/wls_probe.py --lengths --time [--calls 9] [--warmup 2]
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
    import wls_bounds as lb
    import wls_np
    cases = [(name, s, p, H, W, sk, wk, 0) for name, s, p in lb.BORDERS for (H, W) in lb.SIZES for sk in lb.LINKS for wk in lb.WEIGHTS
             if not (name == "frame" and min(H, W) < 3)]
    for name, s, p in (lb.BORDERS[0], lb.BORDERS[2]):
        for n in WALK:
            for sk, wk in (("loguniform", "sparse"), ("edges", "constant")):
                cases += [(name, s, p, 7, n, sk, wk, 1), (name, s, p, n, 6, sk, wk, 1)]
    lines = ["# WLS solve, float32: ERR, RES (tests/wls_bounds.py) and iterations beside the reference iteration's",
             "# (wls_np.pcg_f32, tol 1e-5) on the same input; one MI355X run of python tools/wls_probe.py --lengths",
             "SLEN border W H links weights | ERR (x pcg_f32) RES (x pcg_f32) sweeps / pcg_f32 ERR RES iterations"]
    worst = {"err_ratio": (0, None), "res_ratio": (0, None), "err_zero": (0, None), "res_zero": (0, None), "sweeps_over": (-99, None)}
    for name, s, p, H, W, sk, wk, seed in cases:
        data, weight, sx, sy, lap, boundary = lb.make_input(H, W, 3, wk, sk, seed)
        blk = wls_np.unknowns(s, p, H, W)
        if not wls_np.has_dirichlet(s, p) and (weight[blk].reshape(-1, 3).sum(0) == 0).any():
            weight[blk[0].start, blk[1].start] = 1.0          # (a walk input whose seed left a channel without weight)
        sx, sy = lb.dead_to_nan(s, p, sx, sy)
        y = lb.Yardstick(s, p, weight, sx, sy, data, lap, boundary)
        b = boundary if wls_np.has_dirichlet(s, p) else None
        out = inst.wls(data, weight, sx, sy, lap=lap, boundary=b, free_sides=s, periodic=p)
        sweeps = inst.info().sweeps
        err, res = y.measure(out)
        er, rr = err / y.err32, res / y.res32
        tag = f"{name} {W}x{H} {sk} {wk}"
        lines.append(f"SLEN {name:11s} {W:3d} {H:3d} {sk:10s} {wk:8s} | ERR {err:.2e} (x{er:.2f}) RES {res:.2e} (x{rr:.2f}) sweeps {sweeps:3d} / "
                     f"pcg_f32 {y.err32:.2e} {y.res32:.2e} {y.iters32:3d}")
        print(lines[-1], flush=True)
        if y.iters32 == 0:
            worst["err_zero"] = max(worst["err_zero"], (err, tag))
            worst["res_zero"] = max(worst["res_zero"], (res, tag))
        else:
            worst["err_ratio"] = max(worst["err_ratio"], (er, tag))
            worst["res_ratio"] = max(worst["res_ratio"], (rr, tag))
        worst["sweeps_over"] = max(worst["sweeps_over"], (sweeps - y.max_sweeps(), tag))
    for k, (v, tag) in worst.items():
        lines.append(f"SLEN worst {k}: {v:.4g} ({tag})")
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def timing(capi, inst, path, calls, warmup):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import wls_bounds as lb
    n = 1024
    rng = np.random.default_rng(n)
    shape = (n, n, 3)
    data = rng.standard_normal(shape).astype(np.float32)
    lap = (0.1 * rng.standard_normal(shape)).astype(np.float32)
    weight = np.exp(rng.uniform(np.log(1e-2), 0.0, shape)).astype(np.float32)
    lay = capi.poisson_layout_of(data)
    kind = capi.SC_POISSON_LAPLACIAN | capi.SC_POISSON_NEUMANN
    base = [inst.to_device(a) for a in (lap, data, weight)] + [inst.malloc(data.nbytes)]
    recs = []
    try:
        wj = capi.Instance.make_weighted_jobs(1)
        wj[0].lap, wj[0].data, wj[0].weight, wj[0].out = base
        legs = [("weighted", None)] + [("wls " + sk, lb.links(sk, shape, 7)) for sk in ("loguniform", "edges")]
        for name, links in legs:
            dev = [] if links is None else [inst.to_device(a) for a in links]
            try:
                if links is None:
                    call = lambda tol, iters: inst.weighted_device(capi.WeightedParams(kind, tol, iters, 0.0), lay, wj)
                else:
                    sj = capi.Instance.make_wls_jobs(1)
                    sj[0].lap, sj[0].data, sj[0].weight, sj[0].out = base
                    sj[0].smooth_x, sj[0].smooth_y = dev
                    call = lambda tol, iters: inst.wls_device(capi.WlsParams(kind, tol, iters, 0.0, 0.0), lay, sj)
                t = {4: [], 12: [], 0: []}
                full = None
                for i in range(warmup + calls):
                    for iters in (4, 12, 0):
                        call(1e-30 if iters else 0.0, iters)
                        if i >= warmup:
                            t[iters].append(inst.info().ms_call)
                        if not iters:
                            full = inst.info()
                m4, m12, m0 = (float(np.median(t[k])) for k in (4, 12, 0))
                recs.append({"probe": "wls_time", "leg": name, "size": n, "channels": 3, "border": "neumann", "weights": "loguniform [1e-2, 1]",
                             "ms_call_4_iters": round(m4, 4), "ms_call_12_iters": round(m12, 4), "ms_per_iteration": round((m12 - m4) / 8.0, 4),
                             "default_call": {"sweeps": full.sweeps, "rel_residual": full.rel_residual, "ms_call": round(m0, 4),
                                              "converged": full.converged}, "calls": calls})
                print(json.dumps(recs[-1]), flush=True)
            finally:
                for p in dev:
                    inst.free(p)
    finally:
        for p in base:
            inst.free(p)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "a") as f:
        for r in recs:
            f.write(json.dumps(r) + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lengths", action="store_true")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--lengths-out", default=os.path.join(ROOT, "profiles", "wls_lengths.txt"))
    ap.add_argument("--time-out", default=os.path.join(ROOT, "profiles", "wls_probe.json"))
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
