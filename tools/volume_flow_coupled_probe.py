#!/usr/bin/env python3
"""Measures the coupled flow volume solve (sc_hip_volume_flow_coupled*).  Every GPU step runs in a fresh child process of its own,
under its own time limit; the steps run in the order below and the probe stops at the first one that fails.

--lengths  GPU: ERR, RES and ENERGY (tests/volume_flow_coupled_bounds.py) beside the reference rounds' figures over the GPU tests' own
           inputs (its matrix(); NaN in every element that is not read) and a length walk along x, along y and along the frames
           (Neumann and free left + top; scatter, split, keyframes and hole; link forms, kinds of time, exponents, eps, flows and
           couplings rotating, the bounds file's substitution rule applied): one line per input, then the worst ratios, the worst
           values where the reference's figure is 0 and the worst ENERGY -- what ERR_FACTOR / ERR_FLOOR / RES_FACTOR / RES_FLOOR /
           ENERGY_REL are set from.  The references are computed first, on --jobs processes, before the device is opened.  Written to
           --lengths-out (default profiles/volume_flow_coupled_lengths.txt).
--time     GPU: tv_denoise_video_along_flow(isotropic=True)'s problem (lam 8, tau 1, p = p_time = 1, q = 2, eps 1e-2 of the range, the
           library's default rounds) on a noisy texture that pans by (2, 1) pixels per frame, at 512^2 x 3 channels x 16 frames and
           1024^2 x 1 channel x 32 frames (--small: 128^2 x 3 x 8 alone): the call, the straight coupled call and the anisotropic flow
           call on the same input in the same process, alternated -- rounds, inner iterations per round, stream time
           (sc_run_info.ms_solve), wall time and the rms error against the clean video of every one of --calls host calls after
           --warmup.  JSON lines appended to --time-out (default profiles/volume_flow_coupled_probe.json).
--passthrough  GPU: at 512^2 x 3 x 16 the call with coupling 0 beside sc_hip_volume_flow_robust on the same input, alternated, --calls
           times after --warmup: the medians and each call's own run-to-run spread.  JSON lines appended to --time-out.
--kernels  GPU: that problem at 512^2 x 1 channel x 16 frames through the straight coupled call and through the call with the flow,
           once each with two reweighting rounds, for a kernel trace around that one process: rocprofv3 --kernel-trace -d DIR --
           python tools/volume_flow_coupled_probe.py --child kernels
--fold CSV no GPU: a rocprofv3 kernel-trace CSV folded per kernel -- launches, median and mean duration, total -- to stdout

    python tools/volume_flow_coupled_probe.py --lengths --time --passthrough [--calls 3] [--warmup 1]
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
WALK = [2, 3, 5, 8, 9, 31, 33, 65]
FRAME_WALK = [3, 4, 7, 9, 16, 33]
LIMITS = dict(lengths=1100, time=600, passthrough=300, kernels=300)          # seconds a child may take


def _coupled(case, i):
    """a flow robust matrix tuple with coupling i mod 5 behind it, by the bounds file's rule (CHANNELS: 3 channels; TIME: its exponents)"""
    import volume_flow_coupled_bounds as fb
    import volume_flow_coupled_np as vfc
    border, H, W, C, T, tau, pattern, wk, links, tm, gt, exps, epsf, flow = case
    coupling = fb.COUPLINGS[i % len(fb.COUPLINGS)]
    if coupling & vfc.CHANNELS:
        C = 3
    if coupling & vfc.TIME:
        exps = fb.TIME_EXPONENTS[i % len(fb.TIME_EXPONENTS)]
    return fb.substitute((border, H, W, C, T, tau, pattern, wk, links, tm, gt, exps, epsf, flow, coupling))


def length_cases():
    import volume_flow_coupled_bounds as fb
    import volume_robust_bounds as rb
    cases = [c + (0,) for c in fb.matrix()]
    walk = []
    for border in (fb.BORDERS[0][0], fb.BORDERS[2][0]):
        for i, n in enumerate(WALK):
            pattern, wk = (("scatter", None), ("split", "sparse"))[i % 2]
            walk += [(border, 7, n, 3, 3, rb.TAUS[i % 3], pattern, wk, rb.LINKS[i % 4], rb.TIMES[i % 2], bool(i % 2), rb.EXPONENTS[i % 4], rb.EPS[i % 2],
                      fb.FLOWS[i % 7]),
                     (border, n, 6, 1, 4, rb.TAUS[(i + 1) % 3], pattern, wk, rb.LINKS[(i + 1) % 4], rb.TIMES[(i + 1) % 2], not i % 2,
                      rb.EXPONENTS[(i + 1) % 4], rb.EPS[(i + 1) % 2], fb.FLOWS[(i + 3) % 7])]
        for i, T in enumerate(FRAME_WALK):
            pattern, wk = (("scatter", None), ("keyframes", "sparse"), ("hole", None))[i % 3]
            walk.append((border, 7, 9, 1, T, rb.TAUS[i % 3], pattern, wk, rb.LINKS[(i + 2) % 4], rb.TIMES[i % 2], bool(i % 2), rb.EXPONENTS[(i + 2) % 4],
                         rb.EPS[i % 2], fb.FLOWS[(i + 5) % 7]))
    return cases + [_coupled(c, i) + (1,) for i, c in enumerate(walk)]


def reference(case):
    """(the clean input, its penalties, its Yardstick) of one case: the CPU side, run in a worker"""
    import volume_flow_coupled_bounds as fb
    fb.ERR_FACTOR = fb.RES_FACTOR = fb.ERR_FLOOR = fb.RES_FLOOR = 0.0          # (the probe measures; it does not judge)
    border, H, W, C, T, tau, pattern, wk, links, tm, gt, exps, epsf, flow, coupling, seed = case
    clean = fb.make_input(border, H, W, C, T, tau, pattern, wk, links, tm, gt, flow, seed)
    pen = fb.penalties(clean, exps, epsf)
    return clean, pen, fb.Yardstick(clean, pen, coupling)


def lengths(path, jobs):
    import multiprocessing
    import volume_flow_coupled_bounds as fb
    import volume_flow_coupled_np as vfc
    cases = length_cases()
    with multiprocessing.Pool(jobs) as pool:
        refs = pool.map(reference, cases, chunksize=1)
    from seamlesscloneoptimization_amd import capi
    inst = capi.Instance(0)
    lines = ["# coupled flow volume solve, float32, %d rounds behind the quadratic one: ERR, RES, ENERGY (tests/volume_flow_coupled_bounds.py) beside the" % fb.ROUNDS,
             "# reference rounds' (volume_flow_coupled_np.irls_f32, tol 1e-5) on the same input; one MI355X run of python tools/volume_flow_coupled_probe.py --lengths",
             "VFCLEN border W H C T tau pattern weights links time gt (p, r, q) eps flow coupling | ERR (x irls_f32) RES (x irls_f32) ENERGY sweeps rounds' iterations / irls_f32 ERR RES iterations"]
    worst = {"err_ratio": (0, None), "res_ratio": (0, None), "err_zero": (0, None), "res_zero": (0, None), "energy": (0, None), "trace_rise": (-1, None),
             "reference_rel": (0, None), "reference_iterations": (0, None)}
    try:
        for (border, H, W, C, T, tau, pattern, wk, links, tm, gt, exps, epsf, flow, coupling, seed), (clean, pen, y) in zip(cases, refs):
            p = fb.nan_unread(clean)
            prev = inst.volume_flow_coupled(**fb.call_args(p, pen, coupling, max_rounds=fb.ROUNDS - 1, round_tol=-1.0, allow_not_converged=True))
            out = inst.volume_flow_coupled(**fb.call_args(p, pen, coupling, max_rounds=fb.ROUNDS, round_tol=-1.0, allow_not_converged=True))
            sweeps = inst.info().sweeps
            energy, iters = inst.robust_trace()
            err, res = y.measure(prev, out)
            want = float(y.energy(out).sum())
            en = abs(float(energy[-1]) - want) / want
            rise = max((float(energy[k + 1]) - float(energy[k])) / float(energy[k]) for k in range(len(energy) - 1))
            er, rr = err / y.err32 if y.err32 else float("inf"), res / y.res32 if y.res32 else float("inf")
            name = vfc.NAMES[coupling]
            tag = f"{border} {W}x{H}x{C}x{T} tau {tau:g} {pattern} {wk} {links} {tm} gt {int(gt)} {exps} eps {epsf:g} {flow} {name}"
            lines.append(f"VFCLEN {border:11s} {W:3d} {H:3d} {C} {T:3d} {tau:4g} {pattern:9s} {str(wk):9s} {links:5s} {tm:8s} {int(gt)} {str(exps):16s} {epsf:5g} {flow:8s} "
                         f"{name:18s} | ERR {err:.2e} (x{er:.2f}) RES {res:.2e} (x{rr:.2f}) ENERGY {en:.2e} sweeps {sweeps:3d} {list(map(int, iters))} / irls_f32 "
                         f"{y.err32:.2e} {y.res32:.2e} {y.iters32} rel {max(y.rels32):.1e}")
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
            worst["reference_rel"] = max(worst["reference_rel"], (max(y.rels32), tag))
            worst["reference_iterations"] = max(worst["reference_iterations"], (max(y.iters32), tag))
    finally:
        inst.destroy()
        for k, (v, tag) in worst.items():
            lines.append(f"VFCLEN worst {k}: {v:.4g} ({tag})")
            print(lines[-1], flush=True)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


def panning_video(T, H, W, C, pan, rng):
    """(clean, noisy) float32 T x H x W x C: tools/volume_flow_robust_probe.py's texture of smooth waves and steps that moves by pan =
    (dx, dy) pixels per frame (it wraps), noise of sigma 0.05"""
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    base = 0.5 + 0.3 * np.sin(x / 37.0) * np.cos(y / 29.0) + 0.2 * ((x % 64 > 32) ^ (y % 48 > 24))
    clean = np.stack([np.roll(base, (t * pan[1], t * pan[0]), (0, 1)) for t in range(T)])
    clean = np.ascontiguousarray(clean[..., None] * (1.0 - 0.2 * np.arange(C, dtype=np.float32)), np.float32)
    return clean, (clean + 0.05 * rng.standard_normal(clean.shape)).astype(np.float32)


def _problem(T, H, W, C, pan, rng):
    clean, frames = panning_video(T, H, W, C, pan, rng)
    eps = 1e-2 * float(frames.max() - frames.min())
    flow = np.broadcast_to(np.float32(pan), (T - 1, H, W, 2)).copy()
    arrays = (np.zeros_like(frames), np.zeros_like(frames), frames, np.zeros(frames.shape, np.float32))
    args = dict(weight=np.full(frames.shape, 8.0, np.float32), tau=1.0, neumann=True, p_grad=1.0, eps_grad=eps, p_time=1.0, eps_time=eps, p_data=2.0,
                eps_data=eps, allow_not_converged=True)
    return clean, frames, flow, arrays, args


def _alternate(inst, runs, calls, warmup, clean):
    rec = {name: dict(ms=[], wall=[]) for name in runs}
    for k in range(warmup + calls):
        for name, run in runs.items():          # alternated: all see the same state of the device
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
    return rec


def _report(f, rec, frames, clean, **fields):
    for name, r in rec.items():
        line = dict(probe="volume_flow_coupled", links=name, lam=8.0, tau=1.0, exponents=[1, 1, 2], rounds=len(r["iterations"]) - 1,
                    iterations=r["iterations"], total_iterations=int(sum(r["iterations"])), converged=r["converged"], rms_error=r["rms_error"],
                    rms_noise=float(np.sqrt(np.mean((frames.astype(np.float64) - clean) ** 2))), ms_solve=r["ms"], ms_wall=r["wall"],
                    ms_solve_median=float(np.median(r["ms"])), ms_solve_spread=float(max(r["ms"]) - min(r["ms"])), **fields)
        f.write(json.dumps(line) + "\n")
        f.flush()
        print(json.dumps(line), flush=True)


def timing(path, calls, warmup, small):
    from seamlesscloneoptimization_amd import capi
    inst = capi.Instance(0)
    rng = np.random.default_rng(7)
    pan = (2, 1)
    S = capi.SC_VOLUME_COUPLE_SPACE
    os.makedirs(os.path.dirname(path), exist_ok=True)
    try:
        with open(path, "a") as f:
            for T, H, W, C in (((8, 128, 128, 3),) if small else ((16, 512, 512, 3), (32, 1024, 1024, 1))):
                clean, frames, flow, arrays, args = _problem(T, H, W, C, pan, rng)
                runs = {"isotropic along the flow": lambda: inst.volume_flow_coupled(S, *arrays, flow, **args),
                        "isotropic straight": lambda: inst.volume_coupled(S, *arrays, **args),
                        "anisotropic along the flow": lambda: inst.volume_flow_robust(*arrays, flow, **args)}
                _report(f, _alternate(inst, runs, calls, warmup, clean), frames, clean, call="tv_denoise_video_along_flow", pan=list(pan), size=[W, H, C, T])
    finally:
        inst.destroy()


def passthrough(path, calls, warmup):
    from seamlesscloneoptimization_amd import capi
    inst = capi.Instance(0)
    pan, (T, H, W, C) = (2, 1), (16, 512, 512, 3)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    try:
        clean, frames, flow, arrays, args = _problem(T, H, W, C, pan, np.random.default_rng(7))
        runs = {"sc_hip_volume_flow_robust": lambda: inst.volume_flow_robust(*arrays, flow, **args),
                "sc_hip_volume_flow_coupled, coupling 0": lambda: inst.volume_flow_coupled(0, *arrays, flow, **args)}
        with open(path, "a") as f:
            _report(f, _alternate(inst, runs, calls, warmup, clean), frames, clean, call="pass-through", pan=list(pan), size=[W, H, C, T])
    finally:
        inst.destroy()


def kernels():
    from seamlesscloneoptimization_amd import capi
    inst = capi.Instance(0)
    S = capi.SC_VOLUME_COUPLE_SPACE
    try:
        _, _, flow, arrays, args = _problem(16, 512, 512, 1, (2, 1), np.random.default_rng(7))
        args = dict(args, max_rounds=2, round_tol=-1.0)
        inst.volume_coupled(S, *arrays, **args)
        print("straight: iterations", list(map(int, inst.robust_trace()[1])), flush=True)
        inst.volume_flow_coupled(S, *arrays, flow, **args)
        print("flow: iterations", list(map(int, inst.robust_trace()[1])), flush=True)
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
    for step in LIMITS:
        ap.add_argument("--" + step, action="store_true")
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--fold", metavar="CSV")
    ap.add_argument("--child", metavar="STEP", help="run STEP in this process (what the probe starts for every GPU step)")
    ap.add_argument("--lengths-out", default=os.path.join(ROOT, "profiles", "volume_flow_coupled_lengths.txt"))
    ap.add_argument("--time-out", default=os.path.join(ROOT, "profiles", "volume_flow_coupled_probe.json"))
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--jobs", type=int, default=8)
    a = ap.parse_args()
    if a.child:
        {"lengths": lambda: lengths(a.lengths_out, a.jobs), "time": lambda: timing(a.time_out, a.calls, a.warmup, a.small),
         "passthrough": lambda: passthrough(a.time_out, a.calls, a.warmup), "kernels": kernels}[a.child]()
        return 0
    if a.fold:
        fold(a.fold)
    passed = [arg for arg in sys.argv[1:] if arg not in ["--" + s for s in LIMITS]]
    for step, limit in LIMITS.items():
        if not getattr(a, step):
            continue
        try:          # a fresh process per GPU step, under the step's own time limit; the first failure ends the probe
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", step] + passed, timeout=limit).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc:
            print(f"volume_flow_coupled_probe: --{step} ended with {rc}; nothing more runs", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
