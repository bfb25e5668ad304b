#!/usr/bin/env python3
"""Measures the screened Poisson solve (sc_hip_screened*) on the GPU.

--lengths  the Neumann float32 solve's ERR and RES (tests/direct_bounds.py) beside the float32 restatement's over the length walk of
           tests/test_gpu_screened.py (every convolution-length class along x and along y, the sizes of its restatement test), random
           guidance, data and lam in 1e-3, 0.1, 10: one line per input, then the worst ratios over the inputs with more than 3 pixels
           along both sides and the worst values at 2 or 3 pixels -- what RES_FACTOR / RES_FLOOR / ERR_FACTOR / ERR_FLOOR are set from.
           Written to --lengths-out (default profiles/screened_lengths.txt).
--time     device time box to box (sc_run_info.ms_device_total of a bSync call, arrays resident): the screened call and the unscreened
           SC_METHOD_FFT call of the same kind on the same instance and arrays, alternating, median of --calls after --warmup, and
           the p10-p90 spread of each: Neumann GUIDANCE 2048^2 C=3 and 4096^2 C=1, Dirichlet GUIDANCE 722^2 C=3 (planar).
           Written as JSON lines to --time-out (default profiles/screened_probe.txt, appended).
--root DIR measure the package of another checkout (built there): a checkout without the screened entry points times the unscreened
           calls only -- the parent's figures for the comparison.

    python tools/screened_probe.py --lengths --time [--calls 25] [--warmup 5] [--label TEXT]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIME_CASES = [("neumann", 2048, 2048, 3), ("neumann", 4096, 4096, 1), ("dirichlet", 722, 722, 3)]


def configure(capi, inst, method, flags=0):
    d = inst.default_opts()
    inst.set_solver(**{k: getattr(d, k) for k, _ in capi.SolverOpts._fields_})
    inst.set_solver(method=method, flags=flags)


def lengths(capi, inst, path):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import direct_np
    from direct_bounds import SCREENED
    import test_gpu_screened as T
    sizes = sorted(set(T.identity_sizes(True)) | set(T.EXACT_SIZES))
    configure(capi, inst, capi.SC_METHOD_FFT)
    lines = ["# screened Neumann solve, float32 transforms: ERR and RES (tests/direct_bounds.py) beside the float32 restatement's",
             "# (direct_np.solve_f32) on the same input; random guidance (sigma 20), random data; one MI355X run of",
             "# python tools/screened_probe.py --lengths",
             "SCRLEN W H C lam | f32 RES (x restatement) ERR (x restatement) / solve_f32 RES ERR"]
    worst = {"res_ratio": (0, None), "err_ratio": (0, None), "res_small": (0, None), "err_small": (0, None)}
    for W, H in sizes:
        for C, lam in ((1, 1e-3), (3, 0.1), (4, 10.0), (1, 10.0), (3, 1e-3)):
            if W * H > 300000 and C > 1 and lam != 0.1:
                continue
            d, gx, gy, _ = T.random_problem(H, W, C, W * 11 + H * 17 + C)
            lap = direct_np.divergence(gx, gy)
            y = SCREENED.yardstick("lrtb", "", lam, d, lap, None)
            out = inst.screened(d, gx=gx, gy=gy, lam=lam, neumann=True)
            err, res = y.measure(out)
            rr, er = res / y.res32, err / y.err32
            lines.append(f"SCRLEN {W:5d} {H:5d} {C} {lam:6g} | f32 RES {res:.2e} (x{rr:.1f}) ERR {err:.2e} (x{er:.1f}) / solve_f32 {y.res32:.2e} {y.err32:.2e}")
            print(lines[-1], flush=True)
            key = (W, H, C, lam)
            if min(W, H) > 3:
                if rr > worst["res_ratio"][0]: worst["res_ratio"] = (rr, key)
                if er > worst["err_ratio"][0]: worst["err_ratio"] = (er, key)
            else:
                if res > worst["res_small"][0]: worst["res_small"] = (res, key)
                if err > worst["err_small"][0]: worst["err_small"] = (err, key)
    lines.append("# worst over the inputs with more than 3 pixels along both sides: RES ratio %.2f %s, ERR ratio %.2f %s" %
                 (worst["res_ratio"] + worst["err_ratio"]))
    lines.append("# worst value with 2 or 3 pixels along a side: RES %.3g %s, ERR %.3g %s" % (worst["res_small"] + worst["err_small"]))
    print("\n".join(lines[-2:]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def timing(capi, inst, calls, warmup, label, path):
    have = hasattr(capi, "ScreenedParams")
    rows = []
    for bc, W, H, C in TIME_CASES:
        n = W * H * C
        rng = np.random.default_rng(W + H + C)
        host = np.concatenate([rng.normal(0, 20, 2 * n), rng.uniform(-50, 300, 2 * n), np.zeros(n)]).astype(np.float32)
        dev = inst.malloc(host.nbytes)
        try:
            inst._check(inst.L.sc_hip_memcpy_h2d(inst.h, dev, host.ctypes.data, host.nbytes))
            layout = capi.PoissonLayout(W, H, C, 1, W, W * H)
            kind = capi.SC_POISSON_GUIDANCE | (capi.SC_POISSON_NEUMANN if bc == "neumann" else 0)
            pj = capi.Instance.make_poisson_jobs(1)
            pj[0].gx, pj[0].gy, pj[0].boundary, pj[0].out = dev, dev + 4 * n, dev + 12 * n, dev + 16 * n
            if have:
                sj = capi.Instance.make_screened_jobs(1)
                sj[0].gx, sj[0].gy, sj[0].data, sj[0].boundary, sj[0].out = dev, dev + 4 * n, dev + 8 * n, dev + 12 * n, dev + 16 * n
            configure(capi, inst, capi.SC_METHOD_FFT)
            t, stages = {"unscreened": [], "screened": []}, {}
            for k in range(warmup + calls):
                inst.poisson_device(capi.PoissonParams(kind, 0.0), layout, pj)
                i = inst.info()
                if k >= warmup:
                    t["unscreened"].append(i.ms_device_total)
                    stages["unscreened"] = (i.ms_pre, i.ms_solve, i.ms_post)
                if have:
                    inst.screened_device(capi.ScreenedParams(kind, 0.5), layout, sj)
                    i = inst.info()
                    if k >= warmup:
                        t["screened"].append(i.ms_device_total)
                        stages["screened"] = (i.ms_pre, i.ms_solve, i.ms_post)
            spread = lambda v: float((np.percentile(v, 90) - np.percentile(v, 10)) / np.median(v))
            row = {"label": label, "boundary": bc, "W": W, "H": H, "C": C, "calls": calls, "unscreened_fft_ms": float(np.median(t["unscreened"])),
                   "unscreened_spread_p10_p90": spread(t["unscreened"]), "unscreened_stages_ms": stages["unscreened"]}
            if have:
                row.update(screened_ms=float(np.median(t["screened"])), screened_spread_p10_p90=spread(t["screened"]),
                           screened_stages_ms=stages["screened"], ratio_same_build=float(np.median(t["screened"]) / np.median(t["unscreened"])))
            rows.append(row)
            print(json.dumps(row), flush=True)
        finally:
            inst.free(dev)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "a") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lengths", action="store_true")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--label", default="this build")
    ap.add_argument("--calls", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--lengths-out", default=os.path.join(ROOT, "profiles", "screened_lengths.txt"))
    ap.add_argument("--time-out", default=os.path.join(ROOT, "profiles", "screened_probe.txt"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    from seamlesscloneoptimization_amd import capi
    inst = capi.Instance(0)
    try:
        if a.lengths:
            lengths(capi, inst, a.lengths_out)
        if a.time:
            timing(capi, inst, a.calls, a.warmup, a.label, a.time_out)
    finally:
        inst.destroy()


if __name__ == "__main__":
    main()
