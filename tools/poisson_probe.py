"""Device time of the Poisson solver on float32 images (sc_hip_poisson_device) at 1024^2 and 2048^2, C = 1 and 3, planar (CHW) and
interleaved (HWC) layouts: per solve (median, p95) under SC_METHOD_AUTO, MULTIGRID and FFT, and per solve in batches of 16, with the
split into pre-process / solve / output launch.

    python tools/poisson_probe.py [--reps R] [--out F]              timings (bSync stage marks: each adds a few us of bubble)
    python tools/poisson_probe.py --trace [--reps R]                the same calls without stage marks, for
        rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/poisson_probe.py --trace
    python tools/poisson_probe.py --fold DIR/.../run_kernel_trace.csv [--out F]
                                                                     adds the pre-process and output launches' achieved bytes/s
                                                                     (20 B per element in, 8 B out; 8 B per element for the
                                                                     output launch) to F
"""
from __future__ import annotations

import argparse
import csv
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from seamlesscloneoptimization_amd import capi  # noqa: E402

SIZES = (1024, 2048)
CHANNELS = (1, 3)
LAYOUTS = ("chw", "hwc")
TOL = lambda n: 4e-7 * 300.0 * n      # noqa: E731  seamless_clone.poisson_tol of these images: a stop the float32 cycles reach
METHODS = (("auto", capi.SC_METHOD_AUTO, 0), ("mg", capi.SC_METHOD_MULTIGRID, 0), ("fft", capi.SC_METHOD_FFT, 0))


def configs():
    for n in SIZES:
        for c in CHANNELS:
            for lay in LAYOUTS:
                if c == 1 and lay == "hwc":
                    continue            # one channel: the two layouts are the same
                yield n, c, lay


def layout_of(n, c, lay):
    if lay == "chw":
        return capi.PoissonLayout(n, n, c, 1, n, n * n)
    return capi.PoissonLayout(n, n, c, c, c * n, 1)


def setup(inst, n, c, members):
    """Device arrays of `members` problems (gx, gy, boundary, out each), one block: the jobs.  Every problem reconstructs a white-noise
    image in [-50, 300] from its forward differences (boundary = the image), the hardest case for the float32 floor."""
    rng = np.random.default_rng(n + c)
    span = n * n * c
    img = rng.uniform(-50, 300, (n, n, c)).astype(np.float32)
    gx = np.zeros_like(img); gy = np.zeros_like(img)
    gx[:, :-1] = img[:, 1:] - img[:, :-1]
    gy[:-1] = img[1:] - img[:-1]
    one = np.concatenate([a.reshape(-1) for a in (gx, gy, img, img)])
    host = np.tile(one, members)                             # gx | gy | boundary | out per member (interleaved HWC order)
    d = inst.malloc(host.nbytes)
    inst._check(inst.L.sc_hip_memcpy_h2d(inst.h, d, host.ctypes.data, host.nbytes))
    jobs = capi.Instance.make_poisson_jobs(members)
    for k, j in enumerate(jobs):
        base = d + 4 * span * 4 * k
        j.gx, j.gy, j.boundary, j.out = base, base + 4 * span, base + 8 * span, base + 12 * span
    return d, jobs


def run(reps, timed):
    rows = []
    inst = capi.Instance(0)
    try:
        for n, c, lay in configs():
            l = layout_of(n, c, lay)
            for members in (1, 16):
                d, jobs = setup(inst, n, c, members)
                try:
                    for name, method, flags in METHODS:
                        if members > 1 and name == "fft":
                            continue
                        inst.set_solver(method=method, flags=flags)
                        p = capi.PoissonParams(capi.SC_POISSON_GUIDANCE, TOL(n))
                        inst.poisson_device(p, l, jobs, sync=timed, allow_job_errors=True)     # warm: per-size state, tables
                        inst.sync()
                        t, pre, post, cyc = [], [], [], []
                        for _ in range(reps):
                            rc = inst.poisson_device(p, l, jobs, sync=timed, allow_job_errors=True)
                            if rc not in (capi.SC_OK, capi.SC_ERR_NOT_CONVERGED):
                                raise capi.SeamlessCloneError(rc, "poisson_device")
                            i = inst.info()
                            t.append(i.ms_call / members); pre.append(i.ms_pre); post.append(i.ms_post); cyc.append(i.sweeps)
                        inst.sync()
                        if timed:
                            rows.append(dict(size=n, channels=c, layout=lay, batch=members, method=name, ran=inst.info().method,
                                             ms_per_solve_median=float(np.median(t)), ms_per_solve_p95=float(np.percentile(t, 95)),
                                             ms_pre_median=float(np.median(pre)), ms_out_median=float(np.median(post)),
                                             cycles=int(np.median(cyc)), tol=TOL(n), reps=reps))
                            print(json.dumps(rows[-1]), flush=True)
                finally:
                    inst.free(d)
    finally:
        inst.destroy()
    return rows


def fold(trace_csv):
    """Per launch kind and layout: median duration and achieved bytes/s of the single-problem launches (grid z = 1)."""
    out = []
    rows = list(csv.DictReader(open(trace_csv)))
    for kernel, bpe in (("k_poisson_pre<", 20), ("k_poisson_out<", 8)):
        for inter in ("true", "false"):
            for n in SIZES:
                for c in CHANNELS:
                    w = n + 3 & ~3 if kernel.startswith("k_poisson_pre") else n
                    gx = (w * c + 255) // 256 * 256      # Grid_Size_X counts work-items
                    sel = [r for r in rows if kernel in r["Kernel_Name"] and re.search(r"<%s" % inter, r["Kernel_Name"]) and
                           int(r.get("Grid_Size_X", 0)) in (gx, gx // 256) and int(r.get("Grid_Size_Z", 1)) == 1 and
                           int(r.get("Grid_Size_Y", 0)) == (n + 15) // 16]
                    if not sel:
                        continue
                    dur = np.median([int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in sel]) * 1e-9
                    b = bpe * n * n * c
                    out.append(dict(kernel=kernel.rstrip("<"), interleaved=inter == "true", size=n, channels=c, launches=len(sel),
                                    us_median=dur * 1e6, bytes=b, tb_per_s=b / dur / 1e12))
                    print(json.dumps(out[-1]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--fold", default=None)
    a = ap.parse_args()
    if a.fold is not None:
        res = fold(a.fold)
        if a.out:
            doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
            doc["launches"] = res
            json.dump(doc, open(a.out, "w"), indent=1)
        return
    rows = run(a.reps if not a.trace else min(a.reps, 10), timed=not a.trace)
    if a.out and not a.trace:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump({"source": capi.source_fingerprint(), "solves": rows}, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
