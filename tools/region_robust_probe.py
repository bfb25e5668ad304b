#!/usr/bin/env python3
"""Measures the robust region solve (sc_hip_region_robust*).

--lengths  GPU: ERR, RES and ENERGY (tests/region_robust_bounds.py) beside the reference rounds' figures over the GPU tests' own inputs
           (tests/region_robust_bounds.py's matrix(); NaN in every element that is not read) and a length walk along x and along y
           (Neumann and free left + top; patterns, weights, links, couplings, exponents and eps rotating): one line per input, then the
           worst ratios, the worst values where the reference's figure is 0 and the worst ENERGY -- what ERR_FACTOR / ERR_FLOOR /
           RES_FACTOR / RES_FLOOR / ENERGY_REL are set from.  Written to --lengths-out (default profiles/region_robust_lengths.txt).
--time     GPU: two problems at 1024^2 x 3 on resident arrays, 4 fixed rounds (round_tol -1), tol and max_iters the defaults:
           tv_inpaint (zero guidance, a hole 200 pixels across, every other pixel KNOWN, isotropic p = 1, eps 1e-2) and masked
           integration (the gradients of a smooth image with 5 % gross outliers on an ellipse, 1 pixel in 30 KNOWN, the rest of the
           rectangle OUTSIDE, p = 1, eps 1e-3).  Per problem: rounds, inner iterations per round, stream time (sc_run_info.ms_call) as the
           median of --calls calls with the spread, the wall time; beside it sc_hip_robust on the same arrays with every state 0 (a weight
           of 1e-3 in place of the states), alternating call by call in one process, and the ratio of the two medians: the cost of
           carrying states.  JSON lines appended to --time-out (default profiles/region_robust_probe.json).  Under rocprofv3
           --kernel-trace --stats with --calls 1 --warmup 0 the same leg gives the three launches' times beside k_robust_setup's.

    python tools/region_robust_probe.py --lengths --time [--calls 9] [--warmup 1]
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
WALK = [2, 3, 5, 8, 9, 31, 33, 65, 257]


def lengths(capi, inst, path):
    import region_robust_bounds as rb
    cases = [c + (0,) for c in rb.matrix()]
    for border in (rb.BORDERS[0][0], rb.BORDERS[2][0]):
        for i, n in enumerate(WALK):
            cases += [(border, 7, n, 3, rb.PATTERNS[i % 5], rb.WEIGHTS[i % 3], rb.LINKS[i % 2], rb.COUPLINGS[i % 4], rb.EXPONENTS[i % 4], rb.EPS[i % 2], 1),
                      (border, n, 6, 1 + 2 * (i % 2), rb.PATTERNS[(i + 2) % 5], rb.WEIGHTS[(i + 1) % 3], rb.LINKS[(i + 1) % 2], rb.COUPLINGS[(i + 1) % 4],
                       rb.EXPONENTS[(i + 1) % 4], rb.EPS[(i + 1) % 2], 1)]
    lines = ["# robust region solve, float32, %d rounds behind the quadratic one: ERR, RES, ENERGY (tests/region_robust_bounds.py) beside the" % rb.ROUNDS,
             "# reference rounds' (region_robust_np.irls_f32, tol 1e-5) on the same input; one MI355X run of python tools/region_robust_probe.py --lengths",
             "RRLEN border W H C pattern weights links coupling (p, q) eps | ERR (x irls_f32) RES (x irls_f32) ENERGY sweeps rounds' iterations / irls_f32 ERR RES iterations"]
    worst = {"err_ratio": (0, None), "res_ratio": (0, None), "err_zero": (0, None), "res_zero": (0, None), "energy": (0, None), "trace_rise": (-1, None)}
    for border, H, W, C, pattern, wk, links, cpl, exps, epsf, seed in cases:
        clean = rb.make_input(border, H, W, C, pattern, wk, links, seed)
        pen = rb.penalties(clean, exps, epsf)
        y = rb.Yardstick(clean, pen, cpl)
        p = rb.nan_unread(clean)
        prev = inst.region_robust(**rb.call_args(p, pen, cpl, max_rounds=rb.ROUNDS - 1, round_tol=-1.0, allow_not_converged=True))
        out = inst.region_robust(**rb.call_args(p, pen, cpl, max_rounds=rb.ROUNDS, round_tol=-1.0, allow_not_converged=True))
        sweeps = inst.info().sweeps
        energy, iters = inst.robust_trace()
        err, res = y.measure(prev, out)
        want = float(y.energy(out).sum())
        en = abs(float(energy[-1]) - want) / want
        rise = max((float(energy[k + 1]) - float(energy[k])) / float(energy[k]) for k in range(len(energy) - 1))
        er, rr = err / y.err32 if y.err32 else float("inf"), res / y.res32 if y.res32 else float("inf")
        tag = f"{border} {W}x{H}x{C} {pattern} {wk} {links} coupling {cpl} {exps} eps {epsf:g}"
        lines.append(f"RRLEN {border:11s} {W:3d} {H:3d} {C} {pattern:8s} {str(wk):9s} {str(links):10s} {cpl} {str(exps):11s} {epsf:5g} | "
                     f"ERR {err:.2e} (x{er:.2f}) RES {res:.2e} (x{rr:.2f}) ENERGY {en:.2e} sweeps {sweeps:3d} {list(map(int, iters))} / irls_f32 "
                     f"{y.err32:.2e} {y.res32:.2e} {y.iters32}")
        print(lines[-1], flush=True)
        assert sweeps == int(iters.sum()), (sweeps, iters)
        if y.err32 == 0:
            worst["err_zero"] = max(worst["err_zero"], (err, tag))
        else:
            worst["err_ratio"] = max(worst["err_ratio"], (er, tag))
        if y.res32 == 0:
            worst["res_zero"] = max(worst["res_zero"], (res, tag))
        else:
            worst["res_ratio"] = max(worst["res_ratio"], (rr, tag))
        worst["energy"] = max(worst["energy"], (en, tag))
        worst["trace_rise"] = max(worst["trace_rise"], (rise, tag))
    for k, (v, tag) in worst.items():
        lines.append(f"RRLEN worst {k}: {v:.4g} ({tag})")
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def problems(n, C):
    """the two timed problems at n x n x C: name -> (host arrays by job field, RobustParams' penalties, coupling)"""
    rng = np.random.default_rng(11)
    y, x = np.mgrid[0:n, 0:n].astype(np.float32)
    img = np.stack([0.5 + 0.3 * np.sin(x / 37.0) * np.cos(y / 29.0) + 0.2 * ((x > n / 2.0) ^ (y > n / 3.0)) - 0.05 * c for c in range(C)], 2).astype(np.float32)
    zero = np.zeros_like(img)
    hole = (x - n / 2.0) ** 2 + (y - n / 2.0) ** 2 <= 100.0 ** 2
    st_hole = np.repeat(np.where(hole, 0, 1).astype(np.float32)[:, :, None], C, 2)
    gx, gy = np.roll(img, -1, 1) - img, np.roll(img, -1, 0) - img
    for g in (gx, gy):
        bad = rng.random(g.shape) < 0.05
        g[bad] += np.where(rng.random(g.shape) < 0.5, 1.0, -1.0).astype(np.float32)[bad]
    ell = ((x - n / 2.0) / (0.45 * n)) ** 2 + ((y - n / 2.0) / (0.4 * n)) ** 2 <= 1.0
    st_ell = np.where(ell, np.where(rng.random((n, n)) < 1 / 30, 1, 0), 2).astype(np.float32)
    st_ell = np.repeat(st_ell[:, :, None], C, 2)
    anchor = np.full(img.shape, 1e-3, np.float32)
    return {"tv_inpaint": (dict(gx=zero, gy=zero, data=img, state=st_hole), (1.0, 1e-2, 2.0, 1e-2), 1, dict(hole_pixels=int(hole.sum()))),
            "integrate_masked": (dict(gx=gx, gy=gy, data=img, state=st_ell), (1.0, 1e-3, 2.0, 1e-3), 0,
                                 dict(ellipse_pixels=int(ell.sum()), known=int((st_ell[:, :, 0] == 1).sum()))), "_anchor": anchor}


def timing(capi, inst, path, calls, warmup):
    n, C, rounds = 1024, 3, 4
    prob = problems(n, C)
    anchor = prob.pop("_anchor")
    G = capi.SC_POISSON_GUIDANCE | capi.SC_POISSON_NEUMANN
    os.makedirs(os.path.dirname(path), exist_ok=True)
    for name, (host, (p, eg, q, ed), cpl, facts) in prob.items():
        lay = capi.poisson_layout_of(host["data"])
        dev = {k: inst.to_device(v) for k, v in host.items()}
        dev["weight"] = inst.to_device(anchor)
        dev["out"] = inst.malloc(host["data"].nbytes)
        try:
            jr = capi.Instance.make_region_robust_jobs(1)
            for k in ("gx", "gy", "data", "state", "out"):
                setattr(jr[0], k, dev[k])
            jp = capi.Instance.make_robust_jobs(1)
            for k in ("gx", "gy", "data", "weight", "out"):
                setattr(jp[0], k, dev[k])
            prm = capi.RobustParams(G | capi.robust_coupling_bits(bool(cpl & 1), bool(cpl & 2)), p, eg, q, ed, rounds, -1.0, 0.0, 0)
            ms, wall, ms0, its, its0 = [], [], [], None, None
            for i in range(warmup + calls):          # alternating: the region call, then the plain robust call on the same arrays
                t0 = time.perf_counter()
                inst.region_robust_device(prm, lay, jr)
                t1 = time.perf_counter()
                a = inst.info().ms_call
                its = [int(v) for v in inst.robust_trace()[1]]
                inst.robust_device(prm, lay, jp)
                b = inst.info().ms_call
                its0 = [int(v) for v in inst.robust_trace()[1]]
                if i >= warmup:
                    ms.append(float(a)); wall.append(1e3 * (t1 - t0)); ms0.append(float(b))
            rec = dict(probe="region_robust_time", problem=name, size=[n, n, C], border="neumann", coupling=cpl, exponents=[p, q], eps=[eg, ed],
                       rounds=rounds, calls=calls, **facts, inner_iterations=its, sweeps=int(sum(its)), ms_call=ms, ms_wall=wall,
                       ms_call_median=float(np.median(ms)), ms_call_spread=float(max(ms) - min(ms)), ms_wall_median=float(np.median(wall)),
                       robust_all_unknown=dict(weight=1e-3, inner_iterations=its0, sweeps=int(sum(its0)), ms_call=ms0,
                                               ms_call_median=float(np.median(ms0)), ms_call_spread=float(max(ms0) - min(ms0))),
                       ratio_per_call=float(np.median(ms) / np.median(ms0)),
                       ratio_per_iteration=float((np.median(ms) / max(sum(its), 1)) / (np.median(ms0) / max(sum(its0), 1))))
            print(json.dumps(rec), flush=True)
            with open(path, "a") as f:
                f.write(json.dumps(rec) + "\n")
        finally:
            for ptr in dev.values():
                inst.free(ptr)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lengths", action="store_true")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--lengths-out", default=os.path.join(ROOT, "profiles", "region_robust_lengths.txt"))
    ap.add_argument("--time-out", default=os.path.join(ROOT, "profiles", "region_robust_probe.json"))
    ap.add_argument("--calls", type=int, default=9)
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
