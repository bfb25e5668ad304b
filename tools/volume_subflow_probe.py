#!/usr/bin/env python3
"""Measures the sub-pixel flow volume solve (sc_hip_volume_subflow*).

--lengths   GPU: ERR, RES (tests/volume_subflow_bounds.py) and the iteration count beside the reference iteration's over the GPU tests'
            own inputs (tests/volume_subflow_bounds.py's matrix(); NaN in every element that is not read), the same borders and sizes
            with every state 0 under a constant weight, constant links and a flow of zeros (the reference iteration takes no step: the
            floors), and a length walk along x, along y and along the frames with the eight flows rotating: one line per input, then
            the worst ratios and the worst values where the reference iteration took no step -- what RES_FACTOR / RES_FLOOR /
            ERR_FACTOR / ERR_FLOOR are set from.  The references are computed first, on --jobs processes, before the GPU is opened.
            Written to --lengths-out (default profiles/volume_subflow_lengths.txt).
--time      GPU: iterations, stream time (sc_run_info.ms_solve) and wall time of host calls (medians of --calls after --warmup) at
            512^2 x 3 channels x 16 frames and 1024^2 x 1 channel x 32 frames, Neumann borders, zero guidance, tau = 1, 1 in 30 known
            pixels scattered around an excluded tube, a pan of (2.25, -0.75) per frame: sc_hip_volume_wls (no flow) beside
            sc_hip_volume_flow on the rounded pan and sc_hip_volume_subflow on the pan itself.  JSON lines appended to --time-out
            (default profiles/volume_subflow_probe.json).
--kernels   GPU: the pan at 512^2 x 3 x 16 frames through sc_hip_volume_flow (rounded) and through sc_hip_volume_subflow, once each, for
            a kernel trace taken around this process (k_volume_flow_op beside k_subflow_rho + k_subflow_op per application, and the
            launches of the transpose's build).

    python tools/volume_subflow_probe.py --lengths --time [--calls 3] [--warmup 1]
"""
from __future__ import annotations

import argparse
import json
import multiprocessing
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
WALK = [2, 3, 4, 5, 8, 9, 31, 32, 33, 64, 65]
FRAME_WALK = [3, 4, 7, 8, 9, 16, 17, 33, 64]
SIZES = ((16, 512, 512, 3), (32, 1024, 1024, 1))


def length_cases():
    import volume_subflow_bounds as fb
    cases = [c + (0,) for c in fb.matrix()]
    k = 0
    for i, (border, _, _) in enumerate(fb.BORDERS):
        for j, (H, W) in enumerate(fb.SIZES):
            if not (border == "frame" and min(H, W) < 3):
                T = fb.FRAMES[1 + (i + j) % 3]
                cases.append((border, H, W, 3, T, fb.TAUS[(i + j) % 3], "none", "constant", fb.FORMS[(i + j) % 3], "const", fb.TIMES[k % 2], "zero", 0))
                k += 1
    flows = fb.FLOWS
    for border in (fb.BORDERS[0][0], fb.BORDERS[2][0]):
        for i, n in enumerate(WALK):
            for pattern, wk in (("scatter", None), ("split", "sparse")):
                fl = (flows[i % 8], flows[(i + 3) % 8])
                tau = [fb.TAUS[(i + d) % 3] if fb.TAUS[(i + d) % 3] != 10.0 or fl[d] in fb.STRONG_TAU_FLOWS else 1.0 for d in (0, 1)]
                cases += [(border, 7, n, 3, 3, tau[0], pattern, wk, "lap", fb.LINKS[1 + i % 3], fb.TIMES[i % 2], fl[0], 1),
                          (border, n, 6, 3, 4, tau[1], pattern, wk, "gt", fb.LINKS[1 + (i + 1) % 3], fb.TIMES[(i + 1) % 2], fl[1], 1)]
        for i, T in enumerate(FRAME_WALK):
            for j, (pattern, wk) in enumerate((("scatter", None), ("keyframes", "sparse"), ("hole", None))):
                fl = flows[(i + 2 * j) % 8]
                wk = "sparse" if fl == "collapse" and wk is None else wk          # (the matrix's rule: a frame's links onto one point need a weight)
                tau = fb.TAUS[i % 3] if fb.TAUS[i % 3] != 10.0 or fl in fb.STRONG_TAU_FLOWS else 1.0
                cases.append((border, 7, 9, 3, T, tau, pattern, wk, "gt", fb.LINKS[1 + i % 3], fb.TIMES[i % 2], fl, 1))
    return cases


def length_input(case):
    import volume_subflow_bounds as fb
    border, H, W, C, T, tau, pattern, wk, form, links, time_, flow, seed = case
    small = dict(amount=2) if flow in ("whole", "random") and min(H, W) < 7 else {}
    if pattern == "none":          # every state 0, a constant weight, constant links 2.5 in space and 0.4 in time, a flow of zeros
        p = fb.make_input(border, H, W, C, T, tau, "hole", wk, "none", time_, "edge", seed)
        p["state"] = np.zeros_like(p["state"])
        p["sx"] = p["sy"] = np.full(p["data"].shape, 2.5, np.float32)
        p["smt"] = np.full(p["gt"].shape, 0.4, np.float32)
        p["flow"] = np.where(p["flow"] == 0, p["flow"], np.float32(0))          # (edge's -0.0 stay)
        p["links"] = fb.links_of(p)
    else:
        p = fb.make_input(border, H, W, C, T, tau, pattern, wk, links, time_, flow, seed, **small)
    return fb.nan_unread(p)


def length_reference(case):
    import volume_subflow_bounds as fb
    return fb.Yardstick(length_input(case), case[8])


def flow_call(inst, p, form, **kw):
    import volume_subflow_bounds as fb
    import volume_subflow_np as vf
    b = p["boundary"] if vf.has_dirichlet(p["sides"], p["periodic"]) else None
    return inst.volume_subflow(p["data"], p["state"], weight=p["weight"], boundary=b, tau=p["tau"], free_sides=p["sides"], periodic=p["periodic"],
                            **fb.call_args(p, form), **kw)


def lengths(path, jobs):
    cases = length_cases()
    with multiprocessing.Pool(jobs) as pool:          # (before the GPU is opened: the workers never see it)
        refs = pool.map(length_reference, cases, chunksize=1)
    from seamlesscloneoptimization_amd import capi
    inst = capi.Instance(0)
    lines = ["# sub-pixel flow volume solve, float32: ERR, RES (tests/volume_subflow_bounds.py) and iterations beside the reference iteration's",
             "# (volume_subflow_np.pcg_f32, tol 1e-5) on the same input; one MI355X run of python tools/volume_subflow_probe.py --lengths",
             "VSLEN border W H C T tau pattern weights form links time flow | ERR (x pcg_f32) RES (x pcg_f32) sweeps / pcg_f32 ERR RES iterations"]
    worst = {"err_ratio": (0, None), "res_ratio": (0, None), "err_zero": (0, None), "res_zero": (0, None), "sweeps_over": (-999, None)}
    try:
        for case, y in zip(cases, refs):
            border, H, W, C, T, tau, pattern, wk, form, links, time_, flow, seed = case
            out = flow_call(inst, length_input(case), form, allow_not_converged=True)
            sweeps = inst.info().sweeps
            err, res = y.measure(out)
            er, rr = err / y.err32 if y.err32 else float("inf"), res / y.res32 if y.res32 else float("inf")
            tag = f"{border} {W}x{H}x{C}x{T} tau {tau:g} {pattern} {wk} {form} {links} {time_} {flow}"
            lines.append(f"VSLEN {border:11s} {W:3d} {H:3d} {C} {T:3d} {tau:4g} {pattern:9s} {str(wk):9s} {form:8s} {links:5s} {time_:8s} {flow:8s} | "
                         f"ERR {err:.2e} (x{er:.2f}) RES {res:.2e} (x{rr:.2f}) sweeps {sweeps:3d} / pcg_f32 {y.err32:.2e} {y.res32:.2e} {y.iters32:3d}")
            print(lines[-1], flush=True)
            if y.rel32 > 1e-5 or y.max_sweeps() > 400:
                lines.append(f"VSLEN   (left out of the worst values: the reference iteration is beyond the call's budget, rel {y.rel32:.2e})")
                continue
            if y.iters32 == 0:
                worst["err_zero"] = max(worst["err_zero"], (err, tag))
                worst["res_zero"] = max(worst["res_zero"], (res, tag))
            else:
                worst["err_ratio"] = max(worst["err_ratio"], (er, tag))
                worst["res_ratio"] = max(worst["res_ratio"], (rr, tag))
            worst["sweeps_over"] = max(worst["sweeps_over"], (sweeps - y.max_sweeps(), tag))
    finally:
        inst.destroy()
    for k, (v, tag) in worst.items():
        lines.append(f"VSLEN worst {k}: {v:.4g} ({tag})")
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


PAN = (2.25, -0.75)


def big_input(T, H, W, C, rng):
    import volume_probe
    return volume_probe.big_data(T, H, W, C, rng), volume_probe.big_state("scatter", T, H, W, C)


def big_runs(inst, data, st, lap):
    T, H, W = data.shape[:3]
    pan = np.ascontiguousarray(np.broadcast_to(np.float32(PAN), (T - 1, H, W, 2)))
    return (("sc_hip_volume_wls", "none", lambda: inst.volume_wls(data, st, lap=lap, tau=1.0, neumann=True, allow_not_converged=True)),
            ("sc_hip_volume_flow", "pan rounded", lambda: inst.volume_flow(data, st, pan, lap=lap, tau=1.0, neumann=True, allow_not_converged=True)),
            ("sc_hip_volume_subflow", "pan", lambda: inst.volume_subflow(data, st, pan, lap=lap, tau=1.0, neumann=True, allow_not_converged=True)))


def timing(inst, path, calls, warmup):
    rng = np.random.default_rng(5)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "a") as f:
        for T, H, W, C in SIZES:
            data, st = big_input(T, H, W, C, rng)
            lap = np.zeros((T, H, W, C), np.float32)
            for call, kind, run in big_runs(inst, data, st, lap):
                ms, wall, its = [], [], []
                for k in range(warmup + calls):
                    t0 = time.perf_counter()
                    run()
                    t1 = time.perf_counter()
                    info = inst.info()
                    if k >= warmup:
                        ms.append(info.ms_solve)
                        wall.append(1e3 * (t1 - t0))
                        its.append(info.sweeps)
                rec = dict(probe="volume_subflow", call=call, size=[W, H, C, T], tau=1.0, flow=kind, pan=list(PAN), unknown=int((st == 0).sum()),
                           iterations=its[-1], converged=int(info.converged), rel_residual=float(info.rel_residual), ms_solve=float(np.median(ms)),
                           ms_per_iteration=float(np.median(ms)) / max(its[-1], 1), ms_wall=float(np.median(wall)))
                f.write(json.dumps(rec) + "\n")
                f.flush()
                print(json.dumps(rec), flush=True)


def kernels(inst):
    rng = np.random.default_rng(5)
    T, H, W, C = SIZES[0]
    data, st = big_input(T, H, W, C, rng)
    lap = np.zeros((T, H, W, C), np.float32)
    for call, kind, run in big_runs(inst, data, st, lap)[1:]:
        run()
        print(call, kind, "iterations", inst.info().sweeps, flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lengths", action="store_true")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--jobs", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--lengths-out", default=os.path.join(ROOT, "profiles", "volume_subflow_lengths.txt"))
    ap.add_argument("--time-out", default=os.path.join(ROOT, "profiles", "volume_subflow_probe.json"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    if args.lengths:
        lengths(args.lengths_out, args.jobs)
    if args.time or args.kernels:
        from seamlesscloneoptimization_amd import capi
        inst = capi.Instance(0)
        try:
            if args.time:
                timing(inst, args.time_out, args.calls, args.warmup)
            if args.kernels:
                kernels(inst)
        finally:
            inst.destroy()


if __name__ == "__main__":
    main()
