"""Throughput of batched whole-image edits: 32 device-resident frames of one size, one at a time against grouped.

    python tools/edit_batch_probe.py [--frames 32] [--reps 12] [--sizes 512x512,1920x1080,2048x2048] [--out FILE.json]

For each size and op (OpenCV's default parameters, an ellipse mask over half the image, frames tiled from bench.py's synthetic
destinations and shifted per frame so that they differ), after two warm-up passes:
  * solo: one instance, sc_hip_edit_device(bSync = false) for every frame, then one stream synchronise;
  * pool: a pool of two streams, groups of 16 (sc_hip_pool_edit, device-resident: each chunk one sc_hip_edit_device_batch);
each pass timed with the host clock around work that ends in a synchronise.  Reported: frames per second (median and p95 of the pass
times), the pool's speed-up, and for textureFlattening the hysteresis launches and mailbox reads of the last call (solo: one frame;
pool: one group).
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

from bench import BatchSynth  # noqa: E402
from seamlesscloneoptimization_amd import capi  # noqa: E402

OPS = {"color": capi.SC_EDIT_COLOR_CHANGE, "illumination": capi.SC_EDIT_ILLUMINATION_CHANGE, "texture": capi.SC_EDIT_TEXTURE_FLATTENING}


def _frames(W, H, n):
    syn = BatchSynth(max(W, H), 7)
    dst = syn.image(0)[0]
    reps_y, reps_x = -(-(H + n) // dst.shape[0]), -(-(W + n) // dst.shape[1])
    big = np.tile(dst, (reps_y, reps_x, 1))
    frames = [np.ascontiguousarray(big[k:k + H, 2 * k % n:2 * k % n + W]) for k in range(n)]
    yy, xx = np.mgrid[0:H, 0:W]
    mask = np.zeros((H, W), np.uint8)
    mask[((xx - W / 2) / (W / 2.8)) ** 2 + ((yy - H / 2) / (H / 2.8)) ** 2 <= 1] = 255
    return frames, mask


def _fps(times, n):
    t = np.asarray(times, float)
    # p95 of the frame rate = the rate of the pass at the 95th percentile of the pass time
    return {"median": round(n / float(np.median(t)), 1), "p95": round(n / float(np.percentile(t, 95)), 1),
            "median_ms": round(1e3 * float(np.median(t)), 3)}


def probe_size(W, H, n, reps):
    frames, mask = _frames(W, H, n)
    pool = capi.Pool(0, streams=2, group=16)
    solo = capi.Instance(0)
    inst = pool.instances[0]
    ptrs = []
    out = {}
    try:
        d_mask = inst.to_device(mask)
        ptrs.append(d_mask)
        d_src = [inst.to_device(f) for f in frames]
        d_dst = [inst.malloc(f.nbytes) for f in frames]
        ptrs += d_src + d_dst
        for name, op in OPS.items():
            p = inst.edit_params(op)
            jobs = capi.Instance.make_edit_jobs(n)
            for j, s, d in zip(jobs, d_src, d_dst):
                j.src, j.cols, j.rows, j.src_step = s, W, H, 3 * W
                j.mask, j.mask_step = d_mask, W
                j.dst, j.dst_step = d, 3 * W
            t_solo, t_pool = [], []
            for rep in range(-2, reps):                  # the two kinds alternate: drift in the machine hits both alike
                t0 = time.perf_counter()
                for s, d in zip(d_src, d_dst):
                    solo.edit_device(p, s, (H, W), d_mask, d, sync=False, allow_not_converged=True)
                solo.sync()
                t1 = time.perf_counter()
                pool.edit(p, jobs, device_resident=True)
                t2 = time.perf_counter()
                if rep >= 0:
                    t_solo.append(t1 - t0)
                    t_pool.append(t2 - t1)
            r = {"solo_fps": _fps(t_solo, n), "pool_fps": _fps(t_pool, n)}
            r["speedup"] = round(r["pool_fps"]["median"] / r["solo_fps"]["median"], 2)
            r["group_members"] = max(i.info().group_members for i in pool.instances)
            if op == capi.SC_EDIT_TEXTURE_FLATTENING:
                r["solo_hyst"] = list(solo.edit_counts())
                r["pool_hyst"] = list(pool.instances[0].edit_counts())
            out[name] = r
    finally:
        for q in ptrs:
            inst.free(q)
        solo.destroy()
        pool.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--sizes", default="512x512,1920x1080,2048x2048")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"frames": a.frames, "reps": a.reps, "sizes": {}}
    for s in a.sizes.split(","):
        W, H = (int(v) for v in s.split("x"))
        res["sizes"][s] = probe_size(W, H, a.frames, a.reps)
        for name, r in res["sizes"][s].items():
            extra = ""
            if "solo_hyst" in r:
                extra = " | hysteresis solo %d launches %d reads, group %d launches %d reads" % (*r["solo_hyst"], *r["pool_hyst"])
            print("%-10s %-12s solo %7.1f fps (p95 %7.1f) | pool 2 x 16 %7.1f fps (p95 %7.1f) | x%.2f | group %d%s" % (
                s, name, r["solo_fps"]["median"], r["solo_fps"]["p95"], r["pool_fps"]["median"], r["pool_fps"]["p95"], r["speedup"],
                r["group_members"], extra), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
