#!/usr/bin/env python3
"""Measures the flow volume solve (sc_hip_volume_flow*).

--lengths   GPU: ERR, RES (tests/volume_flow_bounds.py) and the iteration count beside the reference iteration's over the GPU tests' own
            inputs (tests/volume_flow_bounds.py's matrix(); NaN in every element that is not read), the same borders and sizes with
            every state 0 under a constant weight, constant links and a flow of zeros (the reference iteration takes no step: the
            floors), and a length walk along x, along y and along the frames with the seven flows rotating: one line per input, then
            the worst ratios and the worst values where the reference iteration took no step -- what RES_FACTOR / RES_FLOOR /
            ERR_FACTOR / ERR_FLOOR are set from.  The references are computed first, on --jobs processes, before the GPU is opened.
            Written to --lengths-out (default profiles/volume_flow_lengths.txt).
--time      GPU: iterations, stream time (sc_run_info.ms_solve) and wall time of host calls (medians of --calls after --warmup) at
            512^2 x 3 channels x 16 frames and 1024^2 x 1 channel x 32 frames, Neumann borders, zero guidance, tau = 1, 1 in 30 known
            pixels scattered around an excluded tube: sc_hip_volume_wls (flow=None) beside sc_hip_volume_flow with a flow of zeros, a
            pan of (2, 1) per frame, and that pan with an occluded band (NaN) an eighth of the width across.  JSON lines appended to
            --time-out (default profiles/volume_flow_probe.json).
--existing  GPU: ms_solve of the four calls whose templated code the flow forms share -- sc_hip_volume, _volume_wls, _volume_robust
            (two rounds), _volume_coupled (space-time, two rounds) -- at the two sizes above, --calls after --warmup each; --tree DIR
            runs another checkout's library (tools/ab_trees.sh build <rev> makes one in _ab_old) for a same-machine A/B.  One line per
            call and size, appended to --existing-out (default profiles/volume_flow_ab.txt).
--kernels   GPU: the pan case at 512^2 x 1 x 16 frames through sc_hip_volume_wls and through sc_hip_volume_flow, once each, for a
            kernel trace taken around this process (k_volume_op beside k_volume_flow_op per launch).

    python tools/volume_flow_probe.py --lengths --time [--calls 3] [--warmup 1]
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
    import volume_flow_bounds as fb
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
                fl = (flows[i % 7], flows[(i + 3) % 7])
                tau = [fb.TAUS[(i + d) % 3] if fb.TAUS[(i + d) % 3] != 10.0 or fl[d] in fb.STRONG_TAU_FLOWS else 1.0 for d in (0, 1)]
                cases += [(border, 7, n, 3, 3, tau[0], pattern, wk, "lap", fb.LINKS[1 + i % 3], fb.TIMES[i % 2], fl[0], 1),
                          (border, n, 6, 3, 4, tau[1], pattern, wk, "gt", fb.LINKS[1 + (i + 1) % 3], fb.TIMES[(i + 1) % 2], fl[1], 1)]
        for i, T in enumerate(FRAME_WALK):
            for j, (pattern, wk) in enumerate((("scatter", None), ("keyframes", "sparse"), ("hole", None))):
                fl = flows[(i + 2 * j) % 7]
                wk = "sparse" if fl == "collapse" and wk is None else wk          # (the matrix's rule: one link per frame needs a weight)
                tau = fb.TAUS[i % 3] if fb.TAUS[i % 3] != 10.0 or fl in fb.STRONG_TAU_FLOWS else 1.0
                cases.append((border, 7, 9, 3, T, tau, pattern, wk, "gt", fb.LINKS[1 + i % 3], fb.TIMES[i % 2], fl, 1))
    return cases


def length_input(case):
    import volume_flow_bounds as fb
    border, H, W, C, T, tau, pattern, wk, form, links, time_, flow, seed = case
    small = dict(amount=2) if flow in ("split", "random") and min(H, W) < 7 else {}
    if pattern == "none":          # every state 0, a constant weight, constant links 2.5 in space and 0.4 in time, a flow of zeros
        p = fb.make_input(border, H, W, C, T, tau, "hole", wk, "none", time_, "far", seed)
        p["state"] = np.zeros_like(p["state"])
        p["sx"] = p["sy"] = np.full(p["data"].shape, 2.5, np.float32)
        p["smt"] = np.full(p["gt"].shape, 0.4, np.float32)
        p["flow"] = np.where(p["flow"] == 0, p["flow"], np.float32(0))          # (far's -0.0 stay)
        p["links"] = fb.links_of(p)
    else:
        p = fb.make_input(border, H, W, C, T, tau, pattern, wk, links, time_, flow, seed, **small)
    return fb.nan_unread(p)


def length_reference(case):
    import volume_flow_bounds as fb
    return fb.Yardstick(length_input(case), case[8])


def flow_call(inst, p, form, **kw):
    import volume_flow_bounds as fb
    import volume_flow_np as vf
    b = p["boundary"] if vf.has_dirichlet(p["sides"], p["periodic"]) else None
    return inst.volume_flow(p["data"], p["state"], weight=p["weight"], boundary=b, tau=p["tau"], free_sides=p["sides"], periodic=p["periodic"],
                            **fb.call_args(p, form), **kw)


def lengths(path, jobs):
    cases = length_cases()
    with multiprocessing.Pool(jobs) as pool:          # (before the GPU is opened: the workers never see it)
        refs = pool.map(length_reference, cases, chunksize=1)
    from seamlesscloneoptimization_amd import capi
    inst = capi.Instance(0)
    lines = ["# flow volume solve, float32: ERR, RES (tests/volume_flow_bounds.py) and iterations beside the reference iteration's",
             "# (volume_flow_np.pcg_f32, tol 1e-5) on the same input; one MI355X run of python tools/volume_flow_probe.py --lengths",
             "VFLEN border W H C T tau pattern weights form links time flow | ERR (x pcg_f32) RES (x pcg_f32) sweeps / pcg_f32 ERR RES iterations"]
    worst = {"err_ratio": (0, None), "res_ratio": (0, None), "err_zero": (0, None), "res_zero": (0, None), "sweeps_over": (-999, None)}
    try:
        for case, y in zip(cases, refs):
            border, H, W, C, T, tau, pattern, wk, form, links, time_, flow, seed = case
            out = flow_call(inst, length_input(case), form, allow_not_converged=True)
            sweeps = inst.info().sweeps
            err, res = y.measure(out)
            er, rr = err / y.err32 if y.err32 else float("inf"), res / y.res32 if y.res32 else float("inf")
            tag = f"{border} {W}x{H}x{C}x{T} tau {tau:g} {pattern} {wk} {form} {links} {time_} {flow}"
            lines.append(f"VFLEN {border:11s} {W:3d} {H:3d} {C} {T:3d} {tau:4g} {pattern:9s} {str(wk):9s} {form:8s} {links:5s} {time_:8s} {flow:8s} | "
                         f"ERR {err:.2e} (x{er:.2f}) RES {res:.2e} (x{rr:.2f}) sweeps {sweeps:3d} / pcg_f32 {y.err32:.2e} {y.res32:.2e} {y.iters32:3d}")
            print(lines[-1], flush=True)
            if y.rel32 > 1e-5 or y.max_sweeps() > 400:
                lines.append(f"VFLEN   (left out of the worst values: the reference iteration is beyond the call's budget, rel {y.rel32:.2e})")
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
        lines.append(f"VFLEN worst {k}: {v:.4g} ({tag})")
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def big_flow(kind, T, H, W):
    """None, or float32 (T - 1) x H x W x 2 of one timing case"""
    if kind == "none":
        return None
    f = np.zeros((T - 1, H, W, 2), np.float32)
    if kind in ("pan", "pan_occluded"):
        f[..., 0], f[..., 1] = 2, 1
    if kind == "pan_occluded":          # a band an eighth of the width across, moving with the pan
        for t in range(T - 1):
            f[t, :, (W // 3 + 2 * t):(W // 3 + 2 * t + W // 8)] = np.nan
    return f


def big_input(T, H, W, C, rng):
    import volume_probe
    return volume_probe.big_data(T, H, W, C, rng), volume_probe.big_state("scatter", T, H, W, C)


def timing(inst, path, calls, warmup):
    rng = np.random.default_rng(5)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "a") as f:
        for T, H, W, C in SIZES:
            data, st = big_input(T, H, W, C, rng)
            lap = np.zeros((T, H, W, C), np.float32)
            for kind in ("none", "zero", "pan", "pan_occluded"):
                flow = big_flow(kind, T, H, W)
                ms, wall, its = [], [], []
                for k in range(warmup + calls):
                    t0 = time.perf_counter()
                    inst.volume_flow(data, st, flow, lap=lap, tau=1.0, neumann=True, allow_not_converged=True)
                    t1 = time.perf_counter()
                    info = inst.info()
                    if k >= warmup:
                        ms.append(info.ms_solve)
                        wall.append(1e3 * (t1 - t0))
                        its.append(info.sweeps)
                rec = dict(probe="volume_flow", call="sc_hip_volume_wls" if flow is None else "sc_hip_volume_flow", size=[W, H, C, T], tau=1.0, flow=kind,
                           unknown=int((st == 0).sum()), iterations=its[-1], converged=int(info.converged), rel_residual=float(info.rel_residual),
                           ms_solve=float(np.median(ms)), ms_per_iteration=float(np.median(ms)) / max(its[-1], 1), ms_wall=float(np.median(wall)))
                f.write(json.dumps(rec) + "\n")
                f.flush()
                print(json.dumps(rec), flush=True)


def existing(capi, inst, path, calls, warmup, label):
    rng = np.random.default_rng(5)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "a") as f:
        for T, H, W, C in SIZES:
            data, st = big_input(T, H, W, C, rng)
            lap = np.zeros((T, H, W, C), np.float32)
            zero = np.zeros((T, H, W, C), np.float32)
            w = np.full((T, H, W, C), 0.3, np.float32)
            runs = (("sc_hip_volume", lambda: inst.volume(data, st, lap=lap, tau=1.0, neumann=True, allow_not_converged=True)),
                    ("sc_hip_volume_wls", lambda: inst.volume_wls(data, st, lap=lap, tau=1.0, loop=True, neumann=True, allow_not_converged=True)),
                    ("sc_hip_volume_robust", lambda: inst.volume_robust(zero, zero, data, st, w, tau=1.0, neumann=True, max_rounds=2, round_tol=-1.0,
                                                                        allow_not_converged=True)),
                    ("sc_hip_volume_coupled", lambda: inst.volume_coupled(capi.volume_coupling(spacetime=True), zero, zero, data, st, w, tau=1.0, neumann=True,
                                                                          p_time=1.0, max_rounds=2, round_tol=-1.0, allow_not_converged=True)))
            for name, run in runs:
                ms = []
                for k in range(warmup + calls):
                    run()
                    if k >= warmup:
                        ms.append(inst.info().ms_solve)
                line = f"VFAB {label:8s} {name:22s} {W}x{H}x{C}x{T} sweeps {inst.info().sweeps:3d} ms_solve " + " ".join(f"{v:.2f}" for v in ms)
                f.write(line + "\n")
                f.flush()
                print(line, flush=True)


def kernels(inst):
    rng = np.random.default_rng(6)
    T, H, W = 16, 512, 512
    data, st = big_input(T, H, W, 1, rng)
    for kind in ("none", "pan"):
        inst.volume_flow(data, st, big_flow(kind, T, H, W), lap=np.zeros_like(data), tau=1.0, neumann=True, allow_not_converged=True)
        print("volume_flow", kind, T, H, W, "iterations", inst.info().sweeps, flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lengths", action="store_true")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--existing", action="store_true")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--tree", default=ROOT, help="the checkout whose library runs (--existing)")
    ap.add_argument("--label", default="this")
    ap.add_argument("--lengths-out", default=os.path.join(ROOT, "profiles", "volume_flow_lengths.txt"))
    ap.add_argument("--time-out", default=os.path.join(ROOT, "profiles", "volume_flow_probe.json"))
    ap.add_argument("--existing-out", default=os.path.join(ROOT, "profiles", "volume_flow_ab.txt"))
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--jobs", type=int, default=12)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    if a.lengths:
        lengths(a.lengths_out, a.jobs)
    if not (a.time or a.existing or a.kernels):
        return
    from seamlesscloneoptimization_amd import capi
    inst = capi.Instance(0)
    try:
        if a.time:
            timing(inst, a.time_out, a.calls, a.warmup)
        if a.existing:
            existing(capi, inst, a.existing_out, a.calls, a.warmup, a.label)
        if a.kernels:
            kernels(inst)
    finally:
        inst.destroy()


if __name__ == "__main__":
    main()
