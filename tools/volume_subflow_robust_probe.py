#!/usr/bin/env python3
"""Measures the robust sub-pixel flow volume solve (sc_hip_volume_subflow_robust*).

--references FILE  no GPU: the CPU side of --lengths -- every input's float64 rounds and reference rounds (volume_subflow_robust_np), on
           --jobs processes -- pickled to FILE, so that the GPU run only runs the library.  An input of the walk whose reference
           rounds do not stop by their rule is run under the bounds file's substitution rule (eps 1e-2, tau at most 1, under
           collapse 0.1) and marked `sub` on its line.
--lengths  GPU: ERR, RES and ENERGY (tests/volume_subflow_robust_bounds.py) beside the reference rounds' figures over the GPU tests'
           own inputs (its matrix(); NaN in every element that is not read) and a length walk along x, along y and along the frames
           (Neumann and free left + top; scatter, split, keyframes and hole; link forms, kinds of time, exponents, eps and the eight
           flows rotating): one line per input, then per flow and overall the worst ratios, the worst values where the reference's
           figure is 0, the worst ENERGY and the worst rise of the trace's energy from one round to the next -- what ERR_FACTOR /
           ERR_FLOOR / RES_FACTOR / RES_FLOOR / ENERGY_REL are set from.  With --references-in FILE the references are read, else
           computed first.  Written to --lengths-out (default profiles/volume_subflow_robust_lengths.txt).
--time     GPU: tv_denoise_video's problem (lam 8, tau 1, p = p_time = 1, q = 2, eps 1e-2 of the range, the library's default rounds)
           on a noisy texture that pans by (2.25, -0.75) pixels per frame, at 512^2 x 3 channels x 16 frames and 1024^2 x 1 channel x 32
           frames (--small: 128^2 x 3 x 8 alone): sc_hip_volume_subflow_robust along the pan, sc_hip_volume_flow_robust along the
           rounded pan and sc_hip_volume_robust, alternated in one process -- rounds, inner iterations per round, stream time
           (sc_run_info.ms_solve) as the median of --calls host calls after --warmup with their spread, wall time and the rms error
           against the clean video.  JSON lines appended to --time-out (default profiles/volume_subflow_robust_probe.json).
--subflow  GPU: sc_hip_volume_subflow (the quadratic call, whose operator class the robust one stands on) on the README's pan input --
           tools/volume_subflow_probe.py --time's at 512^2 x 3 x 16 under the pan of (2.25, -0.75) -- `--calls` times after --warmup:
           ms_solve of every call and the iteration count, one JSON line labelled --label.  Run it from this tree and from the parent's (--root DIR:
           another checkout's built package), alternating, to see whether the two builds differ by more than a build's own spread.
--kernels  GPU: the --time problem at 512^2 x 3 x 16 through sc_hip_volume_subflow_robust and through sc_hip_volume_flow_robust on the
           rounded pan, once each with two reweighting rounds, for a kernel trace around the process: rocprofv3 --kernel-trace
           --output-format csv -d DIR -- python tools/volume_subflow_robust_probe.py --kernels
--fold CSV no GPU: a rocprofv3 kernel-trace CSV folded per kernel -- launches, median and mean duration, total -- to stdout

    python tools/volume_subflow_robust_probe.py --references refs.pkl
    python tools/volume_subflow_robust_probe.py --lengths --references-in refs.pkl --time [--calls 3] [--warmup 1]
"""
from __future__ import annotations

import argparse
import json
import os
import pickle
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WALK = [2, 3, 5, 8, 9, 31, 33, 65]
FRAME_WALK = [3, 4, 7, 9, 16, 33]
PAN = (2.25, -0.75)


def _paths(root):
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(ROOT, "tests"))


def length_cases():
    import volume_subflow_robust_bounds as sb
    cases = [c + (0,) for c in sb.matrix()]
    walk = []
    nf = len(sb.FLOWS)
    for border in (sb.BORDERS[0][0], sb.BORDERS[2][0]):
        for i, n in enumerate(WALK):
            pattern, wk = (("scatter", None), ("split", "sparse"))[i % 2]
            walk += [(border, 7, n, 3, 3, sb.TAUS[i % 3], pattern, wk, sb.LINKS[i % 4], sb.TIMES[i % 2], bool(i % 2), sb.EXPONENTS[i % 4], sb.EPS[i % 2],
                      sb.FLOWS[i % nf], 1),
                     (border, n, 6, 1, 4, sb.TAUS[(i + 1) % 3], pattern, wk, sb.LINKS[(i + 1) % 4], sb.TIMES[(i + 1) % 2], not i % 2,
                      sb.EXPONENTS[(i + 1) % 4], sb.EPS[(i + 1) % 2], sb.FLOWS[(i + 3) % nf], 1)]
        for i, T in enumerate(FRAME_WALK):
            pattern, wk = (("scatter", None), ("keyframes", "sparse"), ("hole", None))[i % 3]
            walk.append((border, 7, 9, 1, T, sb.TAUS[i % 3], pattern, wk, sb.LINKS[(i + 2) % 4], sb.TIMES[i % 2], bool(i % 2), sb.EXPONENTS[(i + 2) % 4],
                         sb.EPS[i % 2], sb.FLOWS[(i + 5) % nf], 1))
    return cases + walk


def reference(case):
    """(the case as it ran, whether the substitution rule altered it, the clean input, its penalties, its Yardstick): the CPU side, run
    in a worker"""
    import volume_subflow_robust_bounds as sb
    sb.ERR_FACTOR = sb.RES_FACTOR = sb.ERR_FLOOR = sb.RES_FLOOR = 0.0          # (the probe measures; it does not judge)

    def build(c):
        border, H, W, C, T, tau, pattern, wk, links, tm, gt, exps, epsf, flow, seed = c
        clean = sb.make_input(border, H, W, C, T, tau, pattern, wk, links, tm, gt, flow, seed)
        pen = sb.penalties(clean, exps, epsf)
        return clean, pen, sb.Yardstick(clean, pen)

    clean, pen, y = build(case)
    stops = lambda y: max(y.rels32) <= 1e-5 and max(y.iters32) <= sb.MAX_ITERS
    sub = False
    if not stops(y):
        case, sub = sb.substitute(case[:14]) + case[14:], True
        clean, pen, y = build(case)
    return case, sub, stops(y), clean, pen, y


def references(jobs):
    import multiprocessing
    with multiprocessing.Pool(jobs) as pool:
        return pool.map(reference, length_cases(), chunksize=1)


def lengths(path, refs):
    import volume_subflow_robust_bounds as sb
    from seamlesscloneoptimization_amd import capi
    inst = capi.Instance(0)
    lines = ["# robust sub-pixel flow volume solve, float32, %d rounds behind the quadratic one: ERR, RES, ENERGY (tests/volume_subflow_robust_bounds.py)" % sb.ROUNDS,
             "# beside the reference rounds' (volume_subflow_robust_np.irls_f32, tol 1e-5) on the same input; one MI355X run of",
             "# python tools/volume_subflow_robust_probe.py --lengths.  sub: the input runs under the bounds file's substitution rule",
             "VSRLEN border W H C T tau pattern weights links time gt (p, r, q) eps flow | ERR (x irls_f32) RES (x irls_f32) ENERGY sweeps rounds' iterations / irls_f32 ERR RES iterations"]
    new = lambda: {"err_ratio": (0, None), "res_ratio": (0, None), "err_zero": (0, None), "res_zero": (0, None), "energy": (0, None), "trace_rise": (-1, None)}
    worst, per_flow = new(), {}
    try:
        for (border, H, W, C, T, tau, pattern, wk, links, tm, gt, exps, epsf, flow, seed), sub, stops, clean, pen, y in refs:
            tag = f"{border} {W}x{H}x{C}x{T} tau {tau:g} {pattern} {wk} {links} {tm} gt {int(gt)} {exps} eps {epsf:g} {flow}"
            if not stops:
                lines.append(f"VSRLEN left out: the reference rounds do not stop under the rule either ({tag}: {y.iters32}, rel {max(y.rels32):.1e})")
                print(lines[-1], flush=True)
                continue
            p = sb.nan_unread(clean)
            prev = inst.volume_subflow_robust(**sb.call_args(p, pen, max_rounds=sb.ROUNDS - 1, round_tol=-1.0, allow_not_converged=True))
            out = inst.volume_subflow_robust(**sb.call_args(p, pen, max_rounds=sb.ROUNDS, round_tol=-1.0, allow_not_converged=True))
            sweeps = inst.info().sweeps
            energy, iters = inst.robust_trace()
            err, res = y.measure(prev, out)
            want = float(y.energy(out).sum())
            en = abs(float(energy[-1]) - want) / want
            rise = max((float(energy[k + 1]) - float(energy[k])) / float(energy[k]) for k in range(len(energy) - 1))
            er, rr = err / y.err32 if y.err32 else float("inf"), res / y.res32 if y.res32 else float("inf")
            lines.append(f"VSRLEN {border:11s} {W:3d} {H:3d} {C} {T:3d} {tau:4g} {pattern:9s} {str(wk):9s} {links:5s} {tm:8s} {int(gt)} {str(exps):16s} {epsf:5g} {flow:8s} "
                         f"{'sub' if sub else '   '} | ERR {err:.2e} (x{er:.2f}) RES {res:.2e} (x{rr:.2f}) ENERGY {en:.2e} rise {rise:.1e} sweeps {sweeps:3d} "
                         f"{list(map(int, iters))} / irls_f32 {y.err32:.2e} {y.res32:.2e} {y.iters32} rel {max(y.rels32):.1e}")
            print(lines[-1], flush=True)
            assert sweeps == int(iters.sum()), (sweeps, iters)
            for w in (worst, per_flow.setdefault(flow, new())):
                if y.err32 == 0:
                    w["err_zero"] = max(w["err_zero"], (err, tag))
                else:
                    w["err_ratio"] = max(w["err_ratio"], (er, tag))
                if y.res32 == 0:
                    w["res_zero"] = max(w["res_zero"], (res, tag))
                else:
                    w["res_ratio"] = max(w["res_ratio"], (rr, tag))
                w["energy"] = max(w["energy"], (en, tag))
                w["trace_rise"] = max(w["trace_rise"], (rise, tag))
    finally:
        inst.destroy()
        for flow, w in per_flow.items():
            lines.append(f"VSRLEN flow {flow:8s}: ERR x{w['err_ratio'][0]:.2f} RES x{w['res_ratio'][0]:.2f} ENERGY {w['energy'][0]:.2e} rise {w['trace_rise'][0]:.1e} "
                         f"ERR where irls_f32's is 0 {w['err_zero'][0]:.2e} RES where irls_f32's is 0 {w['res_zero'][0]:.2e}")
            print(lines[-1], flush=True)
        for k, (v, tag) in worst.items():
            lines.append(f"VSRLEN worst {k}: {v:.4g} ({tag})")
            print(lines[-1], flush=True)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


def panning_video(T, H, W, C, pan, rng, sigma=0.05):
    """(clean, noisy) float32 T x H x W x C: a texture of smooth waves and soft steps that moves by the real-valued pan = (dx, dy)
    pixels per frame (evaluated at the moved coordinates; the waves wrap), noise of sigma"""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)

    def base(xx, yy):
        return (0.5 + 0.3 * np.sin(2 * np.pi * 3 * xx / W) * np.cos(2 * np.pi * 2 * yy / H)
                + 0.1 * np.tanh(4 * np.sin(2 * np.pi * 8 * xx / W)) * np.tanh(4 * np.sin(2 * np.pi * 6 * yy / H)))
    clean = np.stack([base(x - t * pan[0], y - t * pan[1]) for t in range(T)])
    clean = np.ascontiguousarray(clean[..., None] * (1.0 - 0.2 * np.arange(C)), np.float32)
    return clean, (clean + sigma * rng.standard_normal(clean.shape)).astype(np.float32)


def _denoise(T, H, W, C):
    clean, frames = panning_video(T, H, W, C, PAN, np.random.default_rng(7))
    eps = 1e-2 * float(frames.max() - frames.min())
    flow = np.broadcast_to(np.float32(PAN), (T - 1, H, W, 2)).copy()
    args = dict(tau=1.0, neumann=True, p_grad=1.0, eps_grad=eps, p_time=1.0, eps_time=eps, p_data=2.0, eps_data=eps, allow_not_converged=True)
    return clean, frames, flow, np.zeros_like(frames), np.zeros(frames.shape, np.float32), np.full(frames.shape, 8.0, np.float32), args


def timing(path, calls, warmup, small):
    from seamlesscloneoptimization_amd import capi
    inst = capi.Instance(0)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    try:
        with open(path, "a") as f:
            for T, H, W, C in (((8, 128, 128, 3),) if small else ((16, 512, 512, 3), (32, 1024, 1024, 1))):
                clean, frames, flow, zero, state, weight, args = _denoise(T, H, W, C)
                runs = {"subpixel": lambda: inst.volume_subflow_robust(zero, zero, frames, state, flow, weight, **args),
                        "rounded": lambda: inst.volume_flow_robust(zero, zero, frames, state, flow, weight, **args),
                        "straight": lambda: inst.volume_robust(zero, zero, frames, state, weight, **args)}
                rec = {name: dict(ms=[], wall=[]) for name in runs}
                for k in range(warmup + calls):
                    for name, run in runs.items():          # alternated: all three see the same state of the device
                        t0 = time.perf_counter()
                        out = run()
                        t1 = time.perf_counter()
                        info = inst.info()
                        _, iters = inst.robust_trace()
                        if k >= warmup:
                            r = rec[name]
                            r["ms"].append(float(info.ms_solve))
                            r["wall"].append(1e3 * (t1 - t0))
                            r["iterations"] = list(map(int, iters))
                            r["converged"] = int(info.converged)
                            r["rms_error"] = float(np.sqrt(np.mean((out.astype(np.float64) - clean) ** 2)))
                for name, r in rec.items():
                    line = dict(probe="volume_subflow_robust", call="tv_denoise_video", links=name, pan=list(PAN), size=[W, H, C, T], lam=8.0, tau=1.0,
                                exponents=[1, 1, 2], rounds=len(r["iterations"]) - 1, iterations=r["iterations"], total_iterations=int(sum(r["iterations"])),
                                converged=r["converged"], rms_error=r["rms_error"], rms_noise=float(np.sqrt(np.mean((frames.astype(np.float64) - clean) ** 2))),
                                ms_solve=r["ms"], ms_wall=r["wall"], ms_solve_median=float(np.median(r["ms"])), ms_solve_spread=float(max(r["ms"]) - min(r["ms"])))
                    f.write(json.dumps(line) + "\n")
                    f.flush()
                    print(json.dumps(line), flush=True)
    finally:
        inst.destroy()


def subflow(path, calls, warmup, label, small):
    """the quadratic sub-pixel call on tools/volume_subflow_probe.py --time's input at 512^2 x 3 x 16 (the README's figures)"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import volume_subflow_probe as vp
    from seamlesscloneoptimization_amd import capi
    inst = capi.Instance(0)
    T, H, W, C = (8, 128, 128, 3) if small else vp.SIZES[0]
    try:
        data, st = vp.big_input(T, H, W, C, np.random.default_rng(5))
        run = vp.big_runs(inst, data, st, np.zeros((T, H, W, C), np.float32))[2][2]
        ms, its = [], None
        for k in range(warmup + calls):
            run()
            if k >= warmup:
                ms.append(float(inst.info().ms_solve))
                its = int(inst.info().sweeps)
        line = dict(probe="volume_subflow_robust", call="sc_hip_volume_subflow", label=label, library=os.path.relpath(os.path.dirname(capi.__file__), ROOT), pan=list(vp.PAN),
                    size=[W, H, C, T], tau=1.0, iterations=its, ms_solve=ms, ms_solve_median=float(np.median(ms)), ms_solve_spread=float(max(ms) - min(ms)))
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "a") as f:
            f.write(json.dumps(line) + "\n")
        print(json.dumps(line), flush=True)
    finally:
        inst.destroy()


def kernels(small):
    from seamlesscloneoptimization_amd import capi
    inst = capi.Instance(0)
    T, H, W, C = (8, 128, 128, 3) if small else (16, 512, 512, 3)
    try:
        _, frames, flow, zero, state, weight, args = _denoise(T, H, W, C)
        args = dict(args, max_rounds=2, round_tol=-1.0)
        inst.volume_flow_robust(zero, zero, frames, state, flow, weight, **args)
        print("rounded: iterations", list(map(int, inst.robust_trace()[1])), flush=True)
        inst.volume_subflow_robust(zero, zero, frames, state, flow, weight, **args)
        print("subpixel: iterations", list(map(int, inst.robust_trace()[1])), flush=True)
    finally:
        inst.destroy()


def fold(path):
    import csv
    import re
    per = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = re.sub(r"\(.*", "", row["Kernel_Name"].replace("(anonymous namespace)::", "")).replace("void ", "").replace("sc::", "")
            per.setdefault(name, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    for name, d in sorted(per.items(), key=lambda kv: -sum(kv[1])):
        print(f"{name[:68]:68s} n={len(d):4d} median {np.median(d):8.1f} us  mean {np.mean(d):8.1f}  total {sum(d) / 1e3:7.2f} ms")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--references", metavar="FILE")
    ap.add_argument("--references-in", metavar="FILE")
    ap.add_argument("--lengths", action="store_true")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--subflow", action="store_true")
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--fold", metavar="CSV")
    ap.add_argument("--root", default=ROOT, help="the checkout whose built package is measured (--subflow)")
    ap.add_argument("--label", default="this tree")
    ap.add_argument("--lengths-out", default=os.path.join(ROOT, "profiles", "volume_subflow_robust_lengths.txt"))
    ap.add_argument("--time-out", default=os.path.join(ROOT, "profiles", "volume_subflow_robust_probe.json"))
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--jobs", type=int, default=8)
    a = ap.parse_args()
    _paths(a.root)
    if a.references:
        with open(a.references, "wb") as f:
            pickle.dump(references(a.jobs), f)
    if a.lengths:
        if a.references_in:
            with open(a.references_in, "rb") as f:
                refs = pickle.load(f)
        else:
            refs = references(a.jobs)
        lengths(a.lengths_out, refs)
    if a.time:
        timing(a.time_out, a.calls, a.warmup, a.small)
    if a.subflow:
        subflow(a.time_out, a.calls, a.warmup, a.label, a.small)
    if a.kernels:
        kernels(a.small)
    if a.fold:
        fold(a.fold)


if __name__ == "__main__":
    main()
