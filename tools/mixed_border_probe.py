#!/usr/bin/env python3
"""Measures the Poisson solver's per-side free borders (SC_POISSON_FREE_*) on the GPU.

--lengths   the length walk of tests/direct_bounds.py (mixed_length_cases(): every length class of the transform of a Dirichlet end paired
            with a free end, along x and y, both orders of the ends, both kinds of the other axis; rough inputs, and the smooth
            low-mode reconstruction from 256 unknowns up): per case RES and ERR of the float32 transforms beside the float32
            restatement's (tests/direct_np.solve_f32) and of the double transforms in float32 ulps, then the summary the bounds of
            direct_bounds.MIXED are taken from -- the worst ratios over the inputs with more than 3 unknowns along the walked axis,
            the worst values at 1 to 3.  Written to --lengths-out (profiles/mixed_lengths.txt).
(default)   device time (sc_run_info.ms_device_total of a bSync call on device arrays) of one mixed solve -- left side free, the rest
            Dirichlet lines -- beside the SC_POISSON_NEUMANN solve of the same arrays on the same instance, 2048 x 2048 x 3 and
            300 x 200 x 3: median of --calls calls after --warmup, the two alternating.  Written to --out (profiles/mixed_probe.json).
(tools/mixed_probe.py is an older tool about batches of mixed ROI sizes.)

    python tools/mixed_border_probe.py [--lengths] [--lengths-out FILE] [--out FILE] [--calls 25] [--warmup 5]
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

from seamlesscloneoptimization_amd import capi  # noqa: E402
import direct_np  # noqa: E402
from direct_bounds import MIXED, mixed_length_cases as length_cases, rough_inputs, smooth_input  # noqa: E402

PREC = {"f32": 0, "f64": capi.SC_FLAG_FFT_FP64}


def configure(inst, prec):
    inst.set_solver(method=capi.SC_METHOD_FFT, flags=(inst.default_opts().flags & ~capi.SC_FLAG_FFT_FP64) | PREC[prec])


def lengths(inst, path):
    lines = ["n axis sides WxH input | f32 RES (x restatement) ERR (x restatement) | solve_f32 RES ERR | f64 RES, ERR in float32 ulps"]
    worst = {"res_ratio": (0.0, None), "err_ratio": (0.0, None), "res_small": (0.0, None), "err_small": (0.0, None),
             "f64_ulps": (0.0, None), "f64_res_reconstruction": (0.0, None), "err_smooth_ratio": (0.0, None)}

    def note(key, value, tag):
        if value > worst[key][0]:
            worst[key] = (value, tag)

    for n, axis, sides, W, H, precs in length_cases():
        inputs = rough_inputs(W, H, 3, seed=1000 * n + 10 * len(sides) + (axis == "y"))
        if n >= 256:
            inputs.append(smooth_input(W, H, 3, seed=n + len(sides)))
        for what, gx, gy, b in inputs:
            lap = direct_np.divergence(gx, gy)
            y = MIXED.yardstick(sides, "", 0.0, None, lap, b)
            tag = "n=%d %s %s %s" % (n, axis, sides, what)
            s = "n=%4d %s %-3s %4dx%-4d %-14s |" % (n, axis, sides, W, H, what)
            for prec in precs:
                configure(inst, prec)
                err, res = y.measure(inst.poisson(b, gx=gx, gy=gy, free_sides=sides))
                if prec == "f32":
                    rr, er = res / max(y.res32, 1e-300), err / max(y.err32, 1e-300)
                    s += " f32 RES %.2e (x%.1f) ERR %.2e (x%.1f) | solve_f32 %.2e %.2e |" % (res, rr, err, er, y.res32, y.err32)
                    if what == "smooth":
                        note("err_smooth_ratio", er, tag)
                    elif n > 3:
                        note("res_ratio", rr, tag)
                        note("err_ratio", er, tag)
                    else:
                        note("res_small", res, tag)
                        note("err_small", err, tag)
                else:
                    ulps = err * y.R / float(np.spacing(np.float32(y.R)))
                    s += " f64 RES %.2e ERR %.2f ulp" % (res, ulps)
                    note("f64_ulps", ulps, tag)
                    if what == "reconstruction":
                        note("f64_res_reconstruction", res, tag)
            lines.append(s)
            print(s, flush=True)
    lines.append("")
    for key, (value, tag) in worst.items():
        lines.append("WORST %-24s %.3e   at %s" % (key, value, tag))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def timing(inst, path, calls, warmup):
    rows = []
    for W, H in ((2048, 2048), (300, 200)):
        C = 3
        rng = np.random.default_rng(W + H)
        arrays = [rng.normal(0, 20, (H, W, C)).astype(np.float32) for _ in range(2)] + [rng.uniform(-50, 300, (H, W, C)).astype(np.float32)]
        nbytes = arrays[0].nbytes
        slot = (nbytes + 255) // 256 * 256
        d = inst.malloc(4 * slot)
        try:
            for k, a in enumerate(arrays):
                inst._check(inst.L.sc_hip_memcpy_h2d(inst.h, d + k * slot, a.ctypes.data, nbytes))
            layout = capi.poisson_layout_of(arrays[0])
            configure(inst, "f32")
            times = {"mixed_left_free": [], "neumann": []}
            kinds = {"mixed_left_free": capi.SC_POISSON_GUIDANCE | capi.SC_POISSON_FREE_LEFT, "neumann": capi.SC_POISSON_GUIDANCE | capi.SC_POISSON_NEUMANN}
            for it in range(warmup + calls):
                for name, kind in kinds.items():
                    jobs = capi.Instance.make_poisson_jobs(1)
                    jobs[0].gx, jobs[0].gy, jobs[0].boundary, jobs[0].out = d, d + slot, d + 2 * slot, d + 3 * slot
                    inst.poisson_device(capi.PoissonParams(kind, 0.0), layout, jobs, sync=True)
                    if it >= warmup:
                        times[name].append(inst.info().ms_device_total)
            row = {"W": W, "H": H, "C": C, "calls": calls, "warmup": warmup}
            for name, t in times.items():
                row[name + "_ms_median"] = float(np.median(t))
                row[name + "_ms_min"] = float(np.min(t))
            row["mixed_over_neumann"] = row["mixed_left_free_ms_median"] / row["neumann_ms_median"]
            rows.append(row)
            print(json.dumps(row), flush=True)
        finally:
            inst.free(d)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump({"what": "device ms of one float32 solve, left side free vs SC_POISSON_NEUMANN, same arrays and instance", "rows": rows}, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lengths", action="store_true")
    ap.add_argument("--lengths-out", default=os.path.join(ROOT, "profiles", "mixed_lengths.txt"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mixed_probe.json"))
    ap.add_argument("--calls", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    inst = capi.Instance(0)
    try:
        if a.lengths:
            lengths(inst, a.lengths_out)
        else:
            timing(inst, a.out, a.calls, a.warmup)
    finally:
        inst.destroy()


if __name__ == "__main__":
    main()
