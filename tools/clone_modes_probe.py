"""The cost of the clone modes (NORMAL / MIXED / MONOCHROME, sc_hip_set_clone_mode) on one GPU, modes alternating inside one run.

    python tools/clone_modes_probe.py [--roi 2048] [--reps 32] [--steps 20] [--out FILE.json]

Prints, for each mode:
  * single: the device time of one ROI x ROI clone (sc_hip_run_device, synchronous, SC_FLAG_NO_STAGE_MARKS, library defaults),
    median and p95 over --reps runs, after warm-up, and the multigrid cycle counts those runs took;
  * group: Mpix/s of bench.py's default step -- 32 device-resident clones of ROI x ROI per step, 2 streams x groups of 16, the
    multigrid solver, destinations restored in the step -- over --steps steps, after warm-up;
  * field_retry: how many single clones, and how many clones of the group steps, were repeated on float fields because the 16-bit
    fixed-point field saturated (sc_run_info.field_retry; SC_FLAG_FLOAT_FIELD in seamlessclone_hip.h).
A mixed gradient field is not conservative, so its solutions may leave the fixed-point range more often than NORMAL's.
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

from bench import BatchSynth  # noqa: E402  (bench.py's image generator: the same statistics as the headline step)
from seamlesscloneoptimization_amd import capi  # noqa: E402

MODES = {"normal": capi.SC_NORMAL_CLONE, "mixed": capi.SC_MIXED_CLONE, "monochrome": capi.SC_MONOCHROME_TRANSFER}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--roi", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=32, help="single clones per mode (at least 24)")
    ap.add_argument("--steps", type=int, default=20, help="group steps per mode")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 24:
        ap.error("--reps must be at least 24")
    syn = BatchSynth(a.roi, 7)
    res = {m: {"single_ms": [], "single_cycles": [], "single_retries": 0, "group_s": 0.0, "group_steps": 0, "group_retried_clones": 0} for m in MODES}

    # ---- one clone at a time: one instance per mode, the same images, modes interleaved run by run
    dst, patch, mask, cx, cy = syn.image(0)
    insts = {}
    for m, v in MODES.items():
        i = capi.Instance(0)
        i.set_solver(flags=capi.SC_FLAG_NO_STAGE_MARKS)
        i.set_clone_mode(v)
        insts[m] = i
    dev = {}
    ref = insts["normal"]
    d_face, d_mask, d_b0 = ref.to_device(patch), ref.to_device(mask), ref.to_device(dst)
    d_body = ref.malloc(dst.nbytes)
    try:
        for rep in range(-3, a.reps):          # 3 warm-up rounds
            for m, i in insts.items():
                ref.copy_d2d_async(d_body, d_b0, dst.nbytes)
                ref.sync()
                i.run_device(d_face, patch.shape[:2], d_body, dst.shape[:2], d_mask, mask.shape[:2], cx, cy, sync=True)
                info = i.info()
                if rep >= 0:
                    res[m]["single_ms"].append(float(info.ms_device_total))
                    res[m]["single_cycles"].append(int(info.sweeps))
                    res[m]["single_retries"] += int(info.field_retry)
        for m, i in insts.items():             # the modes really differ
            ref.copy_d2d_async(d_body, d_b0, dst.nbytes)
            ref.sync()
            i.run_device(d_face, patch.shape[:2], d_body, dst.shape[:2], d_mask, mask.shape[:2], cx, cy, sync=True)
            dev[m] = ref.from_device(d_body, dst.shape)
    finally:
        for p in (d_face, d_mask, d_b0, d_body):
            ref.free(p)
        for i in insts.values():
            i.destroy()
    distinct = {f"{x}_vs_{y}": int((dev[x] != dev[y]).sum()) for x in MODES for y in MODES if x < y}

    # ---- bench.py's default step, one pool per mode, modes interleaved step by step
    pools = {m: capi.Pool(0, streams=2, group=16, clone_mode=v, method=capi.SC_METHOD_MULTIGRID) for m, v in MODES.items()}
    owner = pools["normal"].instances[0]
    bufs = []
    jobs = capi.Pool.make_jobs(a.batch)
    try:
        for k, j in enumerate(jobs):
            d, p, mk, x, y = syn.image(k)
            f, b0, b, mm = owner.to_device(p), owner.to_device(d), owner.malloc(d.nbytes), owner.to_device(mk)
            bufs += [f, b0, b, mm]
            j.face, j.face_cols, j.face_rows, j.face_step = f, p.shape[1], p.shape[0], 3 * p.shape[1]
            j.body, j.body_cols, j.body_rows, j.body_step = b, d.shape[1], d.shape[0], 3 * d.shape[1]
            j.mask, j.mask_cols, j.mask_rows, j.mask_step = mm, mk.shape[1], mk.shape[0], mk.shape[1]
            j.centerX, j.centerY, j.body_restore = x, y, b0
        owner.sync()
        for step in range(-3, a.steps):
            for m, pool in pools.items():
                t0 = time.perf_counter()
                pool.run(jobs, device_resident=True)
                dt = time.perf_counter() - t0
                if step >= 0:
                    res[m]["group_s"] += dt
                    res[m]["group_steps"] += 1
                    res[m]["group_retried_clones"] += sum(i.info().group_members for i in pool.instances if i.info().field_retry)
    finally:
        for p in bufs:
            owner.free(p)
        for pool in pools.values():
            pool.close()

    pix = float(a.roi * a.roi)
    out = {"roi": a.roi, "single_reps": a.reps, "group_steps": a.steps, "batch": a.batch, "streams": 2, "group": 16,
           "differing_bytes_between_modes": distinct, "modes": {}}
    for m, r in res.items():
        s = np.asarray(r["single_ms"])
        out["modes"][m] = {
            "single_ms_median": round(float(np.median(s)), 4), "single_ms_p95": round(float(np.percentile(s, 95)), 4),
            "single_cycles": sorted(set(r["single_cycles"])), "single_field_retry": r["single_retries"], "single_clones": len(s),
            "group_Mpix_per_s": round(pix * a.batch * r["group_steps"] / r["group_s"] / 1e6, 1),
            "group_ms_per_step": round(r["group_s"] / r["group_steps"] * 1e3, 3),
            "group_field_retry_clones": r["group_retried_clones"], "group_clones": a.batch * r["group_steps"]}
    n = out["modes"]["normal"]
    for m in ("mixed", "monochrome"):
        out["modes"][m]["single_vs_normal"] = round(out["modes"][m]["single_ms_median"] / n["single_ms_median"], 4)
        out["modes"][m]["group_vs_normal"] = round(out["modes"][m]["group_Mpix_per_s"] / n["group_Mpix_per_s"], 4)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
