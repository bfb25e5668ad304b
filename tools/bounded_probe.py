#!/usr/bin/env python3
"""Measures the bounded solve (sc_hip_bounded*).

--lengths  GPU: RANGE, ERR, RES_FREE, SIGN (tests/bounded_bounds.py) and the rounds beside the float64 reference's and beside
           bounded_np.pdas_f32's over the GPU tests' own inputs (tests/bounded_bounds.py's matrix(), NaN in every element that is not
           read) and a length walk along x and along y (Neumann and free left + top; scatter; both bounds and arrays): one line per
           input, then the worst ratios to the yardstick and the worst values where the yardstick's quantity is 0 -- what the FACTOR /
           FLOOR constants of tests/bounded_bounds.py are set from.  Written to --lengths-out (default profiles/bounded_lengths.txt).
--time     GPU: rounds, inner iterations, stream time (sc_run_info.ms_solve) and wall time of host calls (medians of --calls after
           --warmup) at 1024^2 x 3 channels and 2048^2 x 1 channel beside the unconstrained sc_hip_region call on the same input: the
           Poisson clone of a patch that overshoots [0, 1] by a quarter of the range, interpolation from 1 in 30 scattered samples
           kept between the samples' quartiles, and at 512^2 x 1 the smooth obstacle problem (constant load, zero frame, one upper
           bound).  JSON lines appended to --time-out (default profiles/bounded_probe.json).

    python tools/bounded_probe.py --lengths --time [--calls 5] [--warmup 1]
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
WALK = [3, 4, 5, 8, 9, 24, 25, 31, 32, 33, 40, 41, 63, 64, 65]


def bounded_call(inst, p, form, **kw):
    import region_np
    g = dict(gx=p["gx"], gy=p["gy"]) if form == "guidance" else dict(lap=p["lap"])
    b = p["boundary"] if region_np.has_dirichlet(p["sides"], p["periodic"]) else None
    return inst.bounded(p["data"], p["state"], p["lower"], p["upper"], p["weight"], p["sx"], p["sy"], boundary=b, free_sides=p["sides"],
                        periodic=p["periodic"], **g, **kw)


def lengths(capi, inst, path):
    import bounded_bounds as bb
    cases = list(bb.matrix())
    for border in ("neumann", "free_lt"):
        for n in WALK:
            for k, (H, W) in enumerate(((n, 9), (9, n))):
                cases.append((border, H, W, 3, "scatter", (None, "sparse")[n % 2], (None, "loguniform")[(n // 2) % 2], ("lap", "guidance")[k],
                              ("both", "arrays")[(n + k) % 2]))
    lines = ["# bounded solve on the GPU against tests/bounded_np.py; python tools/bounded_probe.py --lengths",
             "BLEN input | rounds lib ref f32 | sweeps | RANGE | ERR lib f32 | RES_FREE lib f32 | SIGN lib f32 | converged"]
    ratio = {"ERR": (0.0, ""), "RES_FREE": (0.0, ""), "SIGN": (0.0, "")}
    floor = {"ERR": (0.0, ""), "RES_FREE": (0.0, ""), "SIGN": (0.0, "")}
    worst_rounds = (0.0, "")
    for case in cases:
        p, y = bb.case_input(case)
        out = bounded_call(inst, p, case[7])
        info = inst.info()
        changed, active, iters = inst.bounded_trace()
        rng, err, res, sign = y.measure(out)
        tag = bb.case_id(case)
        lines.append(f"BLEN {tag} | {len(iters)} {y.rounds} {y.rounds32} | {info.sweeps} ({sum(y.iters32)}) | {rng:.3g} | {err:.3g} {y.err32:.3g} | "
                     f"{res:.3g} {y.res32:.3g} | {sign:.3g} {y.sign32:.3g} | {info.converged}")
        print(lines[-1], flush=True)
        for name, v, ref in (("ERR", err, y.err32), ("RES_FREE", res, y.res32), ("SIGN", sign, y.sign32)):
            if ref > 0 and sum(y.iters32) > 0:
                ratio[name] = max(ratio[name], (v / ref, tag))
            else:
                floor[name] = max(floor[name], (v, tag))
        worst_rounds = max(worst_rounds, (len(iters) / (2.0 * y.rounds + 2), tag))
    for name in ratio:
        lines.append(f"BLEN worst {name} ratio {ratio[name][0]:.3g} ({ratio[name][1]}); worst value without a yardstick {floor[name][0]:.3g} ({floor[name][1]})")
    lines.append(f"BLEN worst rounds / (2 x reference + 2): {worst_rounds[0]:.3g} ({worst_rounds[1]})")
    print("\n".join(lines[-4:]))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def _image(H, W, C, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    return (0.5 + 0.25 * np.sin(xx / 37.0 + seed)[:, :, None] + 0.2 * np.cos(yy / 53.0)[:, :, None] * np.linspace(1.0, 0.4, C) +
            0.02 * rng.standard_normal((H, W, C))).astype(np.float32)


def big_input(case, H, W, C):
    """(data, state, gx, gy, lap, lower, upper) of one timing case, Neumann borders, unit links"""
    from seamlesscloneoptimization_amd import seamless_clone
    yy, xx = np.mgrid[0:H, 0:W]
    if case == "clone":          # a bright patch into a dark scene: the unconstrained clone overshoots 1 by about a quarter
        mask = ((yy - H / 2) / (0.3 * H)) ** 2 + ((xx - W / 2) / (0.3 * W)) ** 2 <= 1.0
        dst = np.clip(_image(H, W, C, 1) + 0.25, 0, 1).astype(np.float32)
        bump = np.exp(-(((yy - H / 2) / (0.12 * H)) ** 2 + ((xx - W / 2) / (0.12 * W)) ** 2))[:, :, None]
        src = (0.3 * _image(H, W, C, 2) + 0.45 * bump).astype(np.float32)
        gx, gy = seamless_clone._forward_differences(src)
        return dst, np.where(mask, 0, 1).astype(np.uint8), gx, gy, None, 0.0, 1.0
    if case == "scatter":
        rng = np.random.default_rng(7)
        vals = _image(H, W, C, 3)
        known = rng.random((H, W)) < 1 / 30
        q25, q75 = np.quantile(vals[known], (0.25, 0.75))
        return vals, known.astype(np.uint8), None, None, None, float(q25), float(q75)
    # the obstacle problem: -lap u = 1 scaled so that the free membrane rises to about 1, zero frame, u <= 0.5
    data = np.zeros((H, W, C), np.float32)
    lap = np.full((H, W, C), -1.0 / (0.0737 * H * W), np.float32)
    return data, np.zeros((H, W), np.uint8), None, None, lap, None, 0.5


def timing(capi, inst, path, calls, warmup):
    for case, H, W, C, borders in (("clone", 1024, 1024, 3, dict(neumann=True)), ("clone", 2048, 2048, 1, dict(neumann=True)),
                                   ("scatter", 1024, 1024, 3, dict(neumann=True)), ("scatter", 2048, 2048, 1, dict(neumann=True)),
                                   ("obstacle", 512, 512, 1, dict())):
        data, state, gx, gy, lap, lo, hi = big_input(case, H, W, C)
        kw = dict(gx=gx, gy=gy, lap=lap, boundary=None if borders else data, max_iters=2000, **borders)
        rec = dict(case=case, W=W, H=H, C=C, lower=lo, upper=hi)
        for name, call in (("region", lambda: inst.region(data, state, **kw)),
                           ("bounded", lambda: inst.bounded(data, state, lo, hi, max_rounds=200, **kw))):
            ms, wall = [], []
            for k in range(warmup + calls):
                t = time.perf_counter()
                out = call()
                if k >= warmup:
                    wall.append((time.perf_counter() - t) * 1e3)
                    ms.append(inst.info().ms_solve)
            info = inst.info()
            solved = out[np.broadcast_to(state[:, :, None] == 0, out.shape)]
            rec[name] = dict(sweeps=info.sweeps, converged=info.converged, ms_solve=float(np.median(ms)), ms_wall=float(np.median(wall)),
                             min=float(solved.min()), max=float(solved.max()))
            if name == "bounded":
                changed, active, iters = inst.bounded_trace()
                rec[name].update(rounds=len(iters), active=int(active[-1]), changed=[int(c) for c in changed], iters=[int(i) for i in iters])
        print(json.dumps(rec), flush=True)
        with open(path, "a") as f:
            f.write(json.dumps(rec) + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lengths", action="store_true")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--lengths-out", default=os.path.join(ROOT, "profiles", "bounded_lengths.txt"))
    ap.add_argument("--time-out", default=os.path.join(ROOT, "profiles", "bounded_probe.json"))
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
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
