#!/usr/bin/env python3
"""Measures the Neumann option of the Poisson solver (SC_POISSON_NEUMANN) on the GPU and writes profiles/neumann_probe.json:

accuracy  max |out - want| / R per size, for the float32 and the double transforms, on the two problems the tests use
          (reconstruction from forward differences; random guidance, sigma = 20, random boundary); want = tests/direct_np.py on the
          same float32 inputs, R = max |want|.  The float32 figures set the bound of tests/test_gpu_neumann.py (4 x the worst,
          rounded up to one digit).
time      device time (sc_run_info.ms_device_total of a bSync call on device arrays) of the Neumann call and of the Dirichlet
          SC_METHOD_FFT call on the same instance and arrays, C = 3, planar and HWC: median of `--calls` calls after `--warmup`, the
          two alternating so that clock drift hits both; sizes whose n and n - 2 take the same convolution length.

    python tools/neumann_probe.py [--out profiles/neumann_probe.json] [--calls 25] [--skip-accuracy] [--skip-time]
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

SIZES = [(2, 2), (2, 41), (41, 2), (37, 29), (300, 200), (723, 722), (1280, 721), (4000, 143), (2050, 1030), (8192, 64)]      # (W, H)
TIME_SIZES = [(300, 200), (512, 512), (1024, 1024), (2048, 2048), (4096, 4096)]
NEU = capi.SC_POISSON_NEUMANN


def configure(inst, method, flags=0):
    d = inst.default_opts()
    inst.set_solver(**{k: getattr(d, k) for k, _ in capi.SolverOpts._fields_})
    inst.set_solver(method=method, flags=flags)


def accuracy(inst):
    """per size the worst figure over C = 1 .. 4 (the images and fields of tests/test_gpu_neumann.py, seed for seed)"""
    rows = []
    for W, H in SIZES:
        row = {"W": W, "H": H, "C": "1..4"}
        for C in (1, 2, 3, 4):
            rng = np.random.default_rng(W * 7 + H * 13 + C)
            img = rng.uniform(-50, 300, (H, W, C)).astype(np.float32)
            gx, gy = direct_np.forward_differences(img)
            b = rng.uniform(-100, 400, (H, W, C)).astype(np.float32)
            rx = rng.normal(0, 20, (H, W, C)).astype(np.float32)
            ry = rng.normal(0, 20, (H, W, C)).astype(np.float32)
            problems = {"reconstruction": (gx, gy, img, direct_np.solve_free(direct_np.divergence(gx, gy), img)),
                        "random": (rx, ry, b, direct_np.solve_free(direct_np.divergence(rx, ry), b))}
            for prec, flags in (("float32", 0), ("double", capi.SC_FLAG_FFT_FP64)):
                if prec == "double" and max(W, H) > 4096:
                    continue
                configure(inst, capi.SC_METHOD_FFT, flags)
                for name, (ax, ay, bb, want) in problems.items():
                    out = inst.poisson(bb, gx=ax, gy=ay, neumann=True).astype(np.float64)
                    R = float(np.abs(want).max())
                    for key, v in ((f"{name}_{prec}_rel_err", float(np.abs(out - want).max()) / R),
                                   (f"{name}_{prec}_mean_rel_err", float(np.abs(out.mean(axis=(0, 1)) - direct_np.mean_of(bb)).max()) / R)):
                        row[key] = max(row.get(key, 0.0), v)
                        if key.endswith("float32_rel_err"):
                            row.setdefault(key + "_by_C", []).append(v)
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def timing(inst, calls, warmup):
    rows = []
    for W, H in TIME_SIZES:
        C = 3
        rng = np.random.default_rng(W + H)
        n = W * H * C
        host = np.concatenate([rng.normal(0, 20, 2 * n), rng.uniform(-50, 300, n), np.zeros(n)]).astype(np.float32)
        d = inst.malloc(host.nbytes)
        try:
            inst._check(inst.L.sc_hip_memcpy_h2d(inst.h, d, host.ctypes.data, host.nbytes))
            for layout_name, layout in (("planar", capi.PoissonLayout(W, H, C, 1, W, W * H)), ("hwc", capi.PoissonLayout(W, H, C, C, C * W, 1))):
                jobs = capi.Instance.make_poisson_jobs(1)
                jobs[0].gx, jobs[0].gy, jobs[0].boundary, jobs[0].out = d, d + 4 * n, d + 8 * n, d + 12 * n
                configure(inst, capi.SC_METHOD_FFT)
                t = {"dirichlet": [], "neumann": []}
                stages = {}
                for k in range(warmup + calls):
                    for name, kind in (("dirichlet", capi.SC_POISSON_GUIDANCE), ("neumann", capi.SC_POISSON_GUIDANCE | NEU)):
                        inst.poisson_device(capi.PoissonParams(kind, 0.0), layout, jobs)
                        i = inst.info()
                        if k >= warmup:
                            t[name].append(i.ms_device_total)
                            stages[name] = (i.ms_pre, i.ms_solve, i.ms_post)
                md, mn = float(np.median(t["dirichlet"])), float(np.median(t["neumann"]))
                spread = lambda v: float((np.percentile(v, 90) - np.percentile(v, 10)) / np.median(v))
                row = {"W": W, "H": H, "C": C, "layout": layout_name, "calls": calls, "dirichlet_fft_ms": md, "neumann_ms": mn,
                       "ratio": mn / md, "dirichlet_spread_p10_p90": spread(t["dirichlet"]), "neumann_spread_p10_p90": spread(t["neumann"]),
                       "dirichlet_stages_ms": stages["dirichlet"], "neumann_stages_ms": stages["neumann"]}
                rows.append(row)
                print(json.dumps(row), flush=True)
        finally:
            inst.free(d)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "neumann_probe.json"))
    ap.add_argument("--calls", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--skip-accuracy", action="store_true")
    ap.add_argument("--skip-time", action="store_true")
    a = ap.parse_args()
    inst = capi.Instance(0)
    res = {"what": "tools/neumann_probe.py: SC_POISSON_NEUMANN on one MI355X; rel_err = max |out - want| / max |want| against tests/direct_np.py"}
    try:
        if not a.skip_accuracy:
            res["accuracy"] = accuracy(inst)
            res["worst_float32_rel_err"] = max(v for r in res["accuracy"] for k, v in r.items() if k.endswith("float32_rel_err"))
            res["float32_test_bound"] = "4 x worst_float32_rel_err, rounded up to one digit (tests/test_gpu_neumann.py)"
            res["worst_double_rel_err"] = max(v for r in res["accuracy"] for k, v in r.items() if k.endswith("double_rel_err"))
        if not a.skip_time:
            res["time"] = timing(inst, a.calls, a.warmup)
    finally:
        inst.destroy()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
