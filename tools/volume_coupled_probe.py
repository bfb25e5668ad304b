#!/usr/bin/env python3
"""Measures the coupled volume solve (sc_hip_volume_coupled*).

--lengths  GPU: ERR, RES and ENERGY (tests/volume_coupled_bounds.py) beside the reference rounds' figures over the GPU tests' own inputs
           (tests/volume_coupled_bounds.py's matrix(); NaN in every element that is not read) and a length walk along x, along y and
           along the frames (Neumann and free left + top; scatter, split, keyframes and hole; the five couplings, link forms, kinds of
           time, exponents and eps rotating): one line per input, then the worst ratios, the worst values where the reference's figure
           is 0 and the worst ENERGY -- what ERR_FACTOR / RES_FACTOR / ENERGY_REL are held against.  Written to --lengths-out (default
           profiles/volume_coupled_lengths.txt).
--time     GPU: tv_denoise_video's problem (lam 8, tau 1, p = p_time = 1, q = 2, eps 1e-2 of the range, the library's default rounds)
           at 512^2 x 3 channels x 16 frames and 1024^2 x 1 channel x 32 frames on tools/volume_robust_probe.py's video, under no
           coupling (sc_hip_volume_robust itself), SPACE, SPACE | TIME and SPACE | CHANNELS in one run: rounds, inner iterations per
           round, stream time (sc_run_info.ms_solve) and wall time of every one of --calls host calls after --warmup, and the floats
           of the rho planes.  JSON lines appended to --time-out (default profiles/volume_coupled_probe.json).  --small: 128^2 x 3 x 8
           only (a kernel trace around it stays short).

    python tools/volume_coupled_probe.py --lengths --time [--calls 3] [--warmup 1]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
WALK = [2, 3, 5, 8, 9, 31, 33, 65]
FRAME_WALK = [3, 4, 7, 9, 16, 33]


def lengths(capi, inst, path):
    import volume_coupled_bounds as cb
    import volume_coupled_np as vc
    cpl = lambda i: cb.COUPLINGS[i % 5]
    exps = lambda c, i: cb.TIME_EXPONENTS[i % 3] if c & vc.TIME else cb.EXPONENTS[i % 4]
    cases = [c + (0,) for c in cb.matrix()]
    for border in (cb.BORDERS[0][0], cb.BORDERS[2][0]):
        for i, n in enumerate(WALK):
            pattern, wk = (("scatter", None), ("split", "sparse"))[i % 2]
            a, b = cpl(i), cpl(i + 2)
            cases += [(border, 7, n, 3, 3, cb.TAUS[i % 3], pattern, wk, cb.LINKS[i % 4], cb.TIMES[i % 2], bool(i % 2), exps(a, i), cb.EPS[i % 2], a, 1),
                      (border, n, 6, 3 if b & vc.CHANNELS else 1, 4, cb.TAUS[(i + 1) % 3], pattern, wk, cb.LINKS[(i + 1) % 4], cb.TIMES[(i + 1) % 2], not i % 2,
                       exps(b, i + 1), cb.EPS[(i + 1) % 2], b, 1)]
        for i, T in enumerate(FRAME_WALK):
            pattern, wk = (("scatter", None), ("keyframes", "sparse"), ("hole", None))[i % 3]
            c = cpl(i + 1)
            cases.append((border, 7, 9, 3 if c & vc.CHANNELS else 1, T, cb.TAUS[i % 3], pattern, wk, cb.LINKS[(i + 2) % 4], cb.TIMES[i % 2], bool(i % 2),
                          exps(c, i + 2), cb.EPS[i % 2], c, 1))
    lines = ["# coupled volume solve, float32, %d rounds behind the quadratic one: ERR, RES, ENERGY (tests/volume_coupled_bounds.py) beside the" % cb.ROUNDS,
             "# reference rounds' (volume_coupled_np.irls_f32, tol 1e-5) on the same input; one MI355X run of python tools/volume_coupled_probe.py --lengths",
             "VCLEN border W H C T tau pattern weights links time gt (p, r, q) eps coupling | ERR (x irls_f32) RES (x irls_f32) ENERGY code sweeps rounds' iterations / irls_f32 ERR RES iterations"]
    worst = {"err_ratio": (0, None), "res_ratio": (0, None), "err_zero": (0, None), "res_zero": (0, None), "energy": (0, None), "trace_rise": (-1, None)}
    for border, H, W, C, T, tau, pattern, wk, links, tm, gt, ex, epsf, coupling, seed in cases:
        clean = cb.make_input(border, H, W, C, T, tau, pattern, wk, links, tm, gt, seed)
        pen = cb.penalties(clean, ex, epsf)
        y = cb.Yardstick(clean, pen, coupling)
        p = cb.nan_unread(clean)
        prev = inst.volume_coupled(**cb.call_args(p, pen, coupling, max_rounds=cb.ROUNDS - 1, round_tol=-1.0, allow_not_converged=True))
        out = inst.volume_coupled(**cb.call_args(p, pen, coupling, max_rounds=cb.ROUNDS, round_tol=-1.0, allow_not_converged=True))
        info = inst.info()
        sweeps = info.sweeps
        energy, iters = inst.robust_trace()
        err, res = y.measure(prev, out)
        want = float(y.energy(out).sum())
        en = abs(float(energy[-1]) - want) / want
        rise = max((float(energy[k + 1]) - float(energy[k])) / float(energy[k]) for k in range(len(energy) - 1))
        er, rr = err / y.err32 if y.err32 else float("inf"), res / y.res32 if y.res32 else float("inf")
        code = "ok" if max(map(int, iters)) < 400 else "inner-budget"
        tag = f"{border} {W}x{H}x{C}x{T} tau {tau:g} {pattern} {wk} {links} {tm} gt {int(gt)} {ex} eps {epsf:g} {vc.NAMES[coupling]}"
        lines.append(f"VCLEN {border:11s} {W:3d} {H:3d} {C} {T:3d} {tau:4g} {pattern:9s} {str(wk):9s} {links:5s} {tm:8s} {int(gt)} {str(ex):16s} {epsf:5g} "
                     f"{vc.NAMES[coupling]:18s} | ERR {err:.2e} (x{er:.2f}) RES {res:.2e} (x{rr:.2f}) ENERGY {en:.2e} {code} sweeps {sweeps:3d} "
                     f"{list(map(int, iters))} / irls_f32 {y.err32:.2e} {y.res32:.2e} {y.iters32}")
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
        lines.append(f"VCLEN worst {k}: {v:.4g} ({tag})")
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def rho_floats(T, H, W, C, coupling):
    """the floats of the rho planes of one volume under reflecting borders with p = p_time = 1 (every component stored)"""
    S, TT, J = 1, 2, 4
    frame = (W * H + 63) // 64 * 64
    comps = 1 if coupling & TT else 2 if coupling & S else 3
    return 0 if not coupling else comps * T * frame * (1 if coupling & J else C)


def timing(capi, inst, path, calls, warmup, small):
    from volume_robust_probe import noisy_video
    rng = np.random.default_rng(7)
    S, TT, J = capi.SC_VOLUME_COUPLE_SPACE, capi.SC_VOLUME_COUPLE_TIME, capi.SC_VOLUME_COUPLE_CHANNELS
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "a") as f:
        for T, H, W, C in (((8, 128, 128, 3),) if small else ((16, 512, 512, 3), (32, 1024, 1024, 1))):
            frames = noisy_video(T, H, W, C, rng)
            eps = 1e-2 * float(frames.max() - frames.min())
            zero = np.zeros_like(frames)
            state = np.zeros(frames.shape, np.float32)
            weight = np.full(frames.shape, 8.0, np.float32)
            args = dict(tau=1.0, neumann=True, p_grad=1.0, eps_grad=eps, p_time=1.0, eps_time=eps, p_data=2.0, eps_data=eps, allow_not_converged=True)
            for name, coupling in (("none", 0), ("space", S), ("spacetime", S | TT), ("space+channels", S | J)):
                ms, wall, its = [], [], []
                for k in range(warmup + calls):
                    t0 = time.perf_counter()
                    if coupling:
                        inst.volume_coupled(coupling, zero, zero, frames, state, weight, **args)
                    else:
                        inst.volume_robust(zero, zero, frames, state, weight, **args)
                    t1 = time.perf_counter()
                    info = inst.info()
                    _, iters = inst.robust_trace()
                    if k >= warmup:
                        ms.append(float(info.ms_solve))
                        wall.append(1e3 * (t1 - t0))
                        its.append(list(map(int, iters)))
                rec = dict(probe="volume_coupled", call="tv_denoise_video", coupling=name, size=[W, H, C, T], lam=8.0, tau=1.0, exponents=[1, 1, 2],
                           rounds=len(its[-1]) - 1, iterations=its[-1], total_iterations=int(sum(its[-1])), converged=int(info.converged), ms_solve=ms,
                           ms_wall=wall, ms_solve_median=float(np.median(ms)), ms_solve_spread=float(max(ms) - min(ms)),
                           rho_megabytes=4e-6 * rho_floats(T, H, W, C, coupling))
                f.write(json.dumps(rec) + "\n")
                f.flush()
                print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lengths", action="store_true")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--lengths-out", default=os.path.join(ROOT, "profiles", "volume_coupled_lengths.txt"))
    ap.add_argument("--time-out", default=os.path.join(ROOT, "profiles", "volume_coupled_probe.json"))
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    from seamlesscloneoptimization_amd import capi
    inst = capi.Instance(0)
    try:
        if a.lengths:
            lengths(capi, inst, a.lengths_out)
        if a.time:
            timing(capi, inst, a.time_out, a.calls, a.warmup, a.small)
    finally:
        inst.destroy()


if __name__ == "__main__":
    main()
