#!/usr/bin/env python3
"""Measures the robust volume solve (sc_hip_volume_robust*).

--lengths  GPU: ERR, RES and ENERGY (tests/volume_robust_bounds.py) beside the reference rounds' figures over the GPU tests' own inputs
           (tests/volume_robust_bounds.py's matrix(); NaN in every element that is not read) and a length walk along x, along y and
           along the frames (Neumann and free left + top; scatter, split, keyframes and hole; link forms, kinds of time, exponents and
           eps rotating): one line per input, then the worst ratios, the worst values where the reference's figure is 0 and the worst
           ENERGY -- what ERR_FACTOR / ERR_FLOOR / RES_FACTOR / RES_FLOOR / ENERGY_REL are set from.  Written to --lengths-out (default
           profiles/volume_robust_lengths.txt).
--time     GPU: tv_denoise_video's problem (lam 8, tau 1, p = p_time = 1, q = 2, eps 1e-2 of the range, the library's default rounds)
           at 512^2 x 3 channels x 16 frames and 1024^2 x 1 channel x 32 frames on a noisy smooth-plus-steps video: rounds, inner
           iterations per round, stream time (sc_run_info.ms_solve) and wall time of every one of --calls host calls after --warmup.
           JSON lines appended to --time-out (default profiles/volume_robust_probe.json).

    python tools/volume_robust_probe.py --lengths --time [--calls 3] [--warmup 1]
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
WALK = [2, 3, 5, 8, 9, 31, 33, 65]
FRAME_WALK = [3, 4, 7, 9, 16, 33]


def lengths(capi, inst, path):
    import volume_robust_bounds as rb
    cases = [c + (0,) for c in rb.matrix()]
    for border in (rb.BORDERS[0][0], rb.BORDERS[2][0]):
        for i, n in enumerate(WALK):
            pattern, wk = (("scatter", None), ("split", "sparse"))[i % 2]
            cases += [(border, 7, n, 3, 3, rb.TAUS[i % 3], pattern, wk, rb.LINKS[i % 4], rb.TIMES[i % 2], bool(i % 2), rb.EXPONENTS[i % 4], rb.EPS[i % 2], 1),
                      (border, n, 6, 1, 4, rb.TAUS[(i + 1) % 3], pattern, wk, rb.LINKS[(i + 1) % 4], rb.TIMES[(i + 1) % 2], not i % 2,
                       rb.EXPONENTS[(i + 1) % 4], rb.EPS[(i + 1) % 2], 1)]
        for i, T in enumerate(FRAME_WALK):
            pattern, wk = (("scatter", None), ("keyframes", "sparse"), ("hole", None))[i % 3]
            cases.append((border, 7, 9, 1, T, rb.TAUS[i % 3], pattern, wk, rb.LINKS[(i + 2) % 4], rb.TIMES[i % 2], bool(i % 2), rb.EXPONENTS[(i + 2) % 4],
                          rb.EPS[i % 2], 1))
    lines = ["# robust volume solve, float32, %d rounds behind the quadratic one: ERR, RES, ENERGY (tests/volume_robust_bounds.py) beside the" % rb.ROUNDS,
             "# reference rounds' (volume_robust_np.irls_f32, tol 1e-5) on the same input; one MI355X run of python tools/volume_robust_probe.py --lengths",
             "VRLEN border W H C T tau pattern weights links time gt (p, r, q) eps | ERR (x irls_f32) RES (x irls_f32) ENERGY sweeps rounds' iterations / irls_f32 ERR RES iterations"]
    worst = {"err_ratio": (0, None), "res_ratio": (0, None), "err_zero": (0, None), "res_zero": (0, None), "energy": (0, None), "trace_rise": (-1, None)}
    for border, H, W, C, T, tau, pattern, wk, links, tm, gt, exps, epsf, seed in cases:
        clean = rb.make_input(border, H, W, C, T, tau, pattern, wk, links, tm, gt, seed)
        pen = rb.penalties(clean, exps, epsf)
        y = rb.Yardstick(clean, pen)
        p = rb.nan_unread(clean)
        prev = inst.volume_robust(**rb.call_args(p, pen, max_rounds=rb.ROUNDS - 1, round_tol=-1.0, allow_not_converged=True))
        out = inst.volume_robust(**rb.call_args(p, pen, max_rounds=rb.ROUNDS, round_tol=-1.0, allow_not_converged=True))
        sweeps = inst.info().sweeps
        energy, iters = inst.robust_trace()
        err, res = y.measure(prev, out)
        want = float(y.energy(out).sum())
        en = abs(float(energy[-1]) - want) / want
        rise = max((float(energy[k + 1]) - float(energy[k])) / float(energy[k]) for k in range(len(energy) - 1))
        er, rr = err / y.err32 if y.err32 else float("inf"), res / y.res32 if y.res32 else float("inf")
        tag = f"{border} {W}x{H}x{C}x{T} tau {tau:g} {pattern} {wk} {links} {tm} gt {int(gt)} {exps} eps {epsf:g}"
        lines.append(f"VRLEN {border:11s} {W:3d} {H:3d} {C} {T:3d} {tau:4g} {pattern:9s} {str(wk):9s} {links:5s} {tm:8s} {int(gt)} {str(exps):16s} {epsf:5g} | "
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
        lines.append(f"VRLEN worst {k}: {v:.4g} ({tag})")
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def noisy_video(T, H, W, C, rng):
    """smooth plus steps that move a pixel per frame, brightness drifting with t, noise of sigma 0.05; float32 T x H x W x C"""
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    out = np.empty((T, H, W, C), np.float32)
    for t in range(T):
        f = 0.5 + 0.3 * np.sin((x + t) / 37.0) * np.cos(y / 29.0) + 0.2 * ((x + t > W / 2.0) ^ (y > H / 3.0)) + 0.01 * t
        for c in range(C):
            out[t, :, :, c] = f * (1.0 - 0.2 * c) + 0.05 * rng.standard_normal((H, W)).astype(np.float32)
    return out


def timing(capi, inst, path, calls, warmup):
    rng = np.random.default_rng(7)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "a") as f:
        for T, H, W, C in ((16, 512, 512, 3), (32, 1024, 1024, 1)):
            frames = noisy_video(T, H, W, C, rng)
            eps = 1e-2 * float(frames.max() - frames.min())
            zero = np.zeros_like(frames)
            state = np.zeros(frames.shape, np.float32)
            weight = np.full(frames.shape, 8.0, np.float32)
            ms, wall, rounds, its = [], [], [], []
            for k in range(warmup + calls):
                t0 = time.perf_counter()
                inst.volume_robust(zero, zero, frames, state, weight, tau=1.0, neumann=True, p_grad=1.0, eps_grad=eps, p_time=1.0, eps_time=eps,
                                   p_data=2.0, eps_data=eps, allow_not_converged=True)
                t1 = time.perf_counter()
                info = inst.info()
                _, iters = inst.robust_trace()
                if k >= warmup:
                    ms.append(float(info.ms_solve))
                    wall.append(1e3 * (t1 - t0))
                    rounds.append(len(iters) - 1)
                    its.append(list(map(int, iters)))
            rec = dict(probe="volume_robust", call="tv_denoise_video", size=[W, H, C, T], lam=8.0, tau=1.0, exponents=[1, 1, 2], rounds=rounds[-1],
                       iterations=its[-1], total_iterations=int(sum(its[-1])), converged=int(info.converged), ms_solve=ms, ms_wall=wall,
                       ms_solve_median=float(np.median(ms)), ms_solve_spread=float(max(ms) - min(ms)))
            f.write(json.dumps(rec) + "\n")
            f.flush()
            print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lengths", action="store_true")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--lengths-out", default=os.path.join(ROOT, "profiles", "volume_robust_lengths.txt"))
    ap.add_argument("--time-out", default=os.path.join(ROOT, "profiles", "volume_robust_probe.json"))
    ap.add_argument("--calls", type=int, default=3)
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
