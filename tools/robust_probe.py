#!/usr/bin/env python3
"""Measures the robust solve (sc_hip_robust*) on the GPU.

--lengths  ERR, RES and ENERGY (tests/robust_bounds.py) beside the restatement's rounds (robust_np.irls_f32) over the GPU tests' own
           accuracy cases (robust_bounds.accuracy_cases: NaN in every dead link) and a length walk along x and along y (Neumann and free
           left + top; p = 1, q = 2, eps 1e-3, sparse weights, no base links -- and p = 1.5, q = 2, eps 1e-2, dense weights, base
           links): 8 fixed rounds, one line per input, then the worst ratios, the worst values among the inputs where the
           restatement's figure is 0, the worst relative energy difference and the worst rise of the energy over a round -- what
           ERR_FACTOR / ERR_FLOOR / RES_FACTOR / RES_FLOOR / ENERGY_REL are set from.  Written to --lengths-out (default
           profiles/robust_lengths.txt).
--time     at 1024^2, C = 3, Neumann, on resident arrays (the smooth-plus-steps image of the tests with noise and the lattice of outliers,
           data weights log-uniform in [1e-2, 1], p = 1, q = 2, eps = 1e-3 of the range): the device time of a call of 8 and of 4 fixed
           rounds (their difference / 4: a late round), of the quadratic call (p = q = 2) and of sc_hip_wls on the same arrays with
           links of 1 (the difference: the final energy evaluation and its wait); the inner iterations of every round, warm; and the
           same 8 rounds driven from the host through sc_hip_wls_device -- download u, links and weights in numpy, upload, a cold solve
           -- with its inner iterations, its device time and its wall time beside the robust call's wall time.  Median of --calls after
           --warmup (the host-driven loop: once).  Written as JSON lines to --time-out (default profiles/robust_probe.json, appended).
           Kernel times (k_robust_setup beside k_wls_setup): the same leg under
               rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/robust_probe.py --time --calls 1 --warmup 0 --no-host-loop

--coupling iso | joint | both | all    the coupled gradient terms (SC_ROBUST_ISOTROPIC, SC_ROBUST_JOINT_CHANNELS) instead:
           --lengths  the same figures against tests/robust_coupled_np.py over tests/robust_coupled_bounds.py's cases (accuracy_cases,
                      and large_cases: RES and ENERGY only) and the length walk with the chosen couplings in turn, to
                      profiles/robust_coupled_lengths.txt -- what robust_coupled_bounds' constants are set from.
           --time     tv_denoise's problem (zero guidance, weight 2, p = 1, q = 2, eps = 1e-2) at 1024^2, C = 3, Neumann, on resident
                      arrays, 8 fixed rounds: the call's device time, the rounds' inner iterations and the final energy of the
                      anisotropic form and of every chosen coupling, to profiles/robust_coupled_probe.json.  Kernel times
                      (k_robust_rho and k_robust_setup_rho beside k_robust_setup): the same leg under rocprofv3 as above, with
                      --base-links for the launches' base-link forms.

    python tools/robust_probe.py --lengths --time [--calls 5] [--warmup 1] [--coupling all]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WALK = [2, 3, 4, 5, 8, 9, 24, 25, 31, 32, 33, 40, 41, 63, 64, 65]


def run_rounds(inst, sides, periodic, p, q, eps, a, rounds, **kw):
    import wls_np
    b = a["boundary"] if wls_np.has_dirichlet(sides, periodic) else None
    return inst.robust(a["gx"], a["gy"], a["data"], a["weight"], a["cx"], a["cy"], boundary=b, free_sides=sides, periodic=periodic, p_grad=p,
                       eps_grad=eps, p_data=q, eps_data=eps, max_rounds=rounds, round_tol=-1.0, **kw)


def lengths(capi, inst, path):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import robust_bounds as rb
    borders = {b[0]: b[1:] for b in rb.BORDERS}
    cases = [c + (0,) for c in rb.accuracy_cases()]
    for name in ("neumann", "free_lt"):
        for n in WALK:
            for pq, epsf, links, wk in (((1.0, 2.0), 1e-3, False, "sparse"), ((1.5, 2.0), 1e-2, True, "dense")):
                cases += [(name, (7, n), pq, epsf, links, wk, 3, 1), (name, (n, 6), pq, epsf, links, wk, 3, 1)]
    lines = ["# robust solve, float32, 8 fixed rounds: ERR, RES, ENERGY (tests/robust_bounds.py) beside the restatement's rounds",
             "# (robust_np.irls_f32, inner tol 1e-5) on the same input; one MI355X run of python tools/robust_probe.py --lengths",
             "RLEN border W H C p q eps links weights | ERR (x irls_f32) RES (x irls_f32) ENERGY rel rise sweeps / irls_f32 ERR RES iterations"]
    worst = {k: (0.0, None) for k in ("err_ratio", "res_ratio", "err_zero", "res_zero", "energy_rel")}
    worst["energy_rise"] = (-1.0, None)          # (the largest relative change of the energy over a round: negative when it fell in all)
    for name, (H, W), (p, q), epsf, links, wk, C, seed in cases:
        sides, periodic = borders[name]
        a = rb.with_dead_nan(sides, periodic, rb.make_input(H, W, C, wk, links, seed))
        eps = epsf * a["range"]
        y = rb.Yardstick(sides, periodic, p, q, eps, eps, a)
        prev = run_rounds(inst, sides, periodic, p, q, eps, a, rb.ROUNDS - 1)
        out = run_rounds(inst, sides, periodic, p, q, eps, a, rb.ROUNDS)
        sweeps = inst.info().sweeps
        energy, iters = inst.robust_trace()
        err, res = y.measure(prev, out)
        want_e = float(y.energy(out).sum())
        erel = abs(float(energy[-1]) - want_e) / want_e
        rise = float(np.max(np.diff(energy) / energy[:-1]))
        tag = f"{name} {W}x{H} p={p} q={q} eps={epsf} links={int(links)} {wk}"
        er = err / y.err32 if y.err32 > 0 else float("nan")
        rr = res / y.res32 if y.res32 > 0 else float("nan")
        lines.append(f"RLEN {name:11s} {W:3d} {H:3d} {C} {p} {q} {epsf:g} {int(links)} {wk:6s} | ERR {err:.2e} (x{er:.2f}) RES {res:.2e} (x{rr:.2f}) "
                     f"ENERGY {erel:.2e} rise {rise:+.1e} sweeps {sweeps:3d} / irls_f32 {y.err32:.2e} {y.res32:.2e} {sum(y.iters32):3d}")
        print(lines[-1], flush=True)
        for key, ratio, value, ref in (("err", er, err, y.err32), ("res", rr, res, y.res32)):
            if ref > 0:
                worst[key + "_ratio"] = max(worst[key + "_ratio"], (ratio, tag))
            else:
                worst[key + "_zero"] = max(worst[key + "_zero"], (value, tag))
        worst["energy_rel"] = max(worst["energy_rel"], (erel, tag))
        worst["energy_rise"] = max(worst["energy_rise"], (rise, tag))
    # the batch test's members (robust_bounds.batch_problems): one joint call, the refused member left out
    sides, periodic, probs, eps, refused = rb.batch_problems()
    H, W = probs[0]["data"].shape[:2]
    names = ("gx", "gy", "data", "weight", "smooth_x", "smooth_y", "out")
    dev = []
    try:
        jobs = capi.Instance.make_robust_jobs(len(probs))
        for k, a in enumerate(probs):
            ptrs = [inst.to_device(v) for v in (a["gx"], a["gy"], a["data"], a["weight"], a["cx"], a["cy"], np.zeros((H, W, 3), np.float32))]
            dev += ptrs
            for nm, ptr in zip(names, ptrs):
                setattr(jobs[k], nm, ptr)
        prm = capi.RobustParams(capi.SC_POISSON_GUIDANCE | capi.SC_POISSON_NEUMANN, 1.0, eps, 2.0, eps, rb.ROUNDS, -1.0, 0.0, 0)
        inst.robust_device(prm, capi.poisson_layout_of(probs[0]["data"]), jobs, allow_job_errors=True)
        outs = [inst.from_device(jobs[k].out, (H, W, 3), np.float32) for k in range(len(probs))]
    finally:
        for ptr in dev:
            inst.free(ptr)
    for k, a in enumerate(probs):
        if k == refused:
            continue
        y = rb.Yardstick(sides, periodic, 1.0, 2.0, eps, eps, a)
        solo = run_rounds(inst, sides, periodic, 1.0, 2.0, eps, a, rb.ROUNDS)
        for tag, u in ((f"batch member {k}", outs[k]), (f"batch member {k} solo", solo)):
            err = float(np.abs(u.astype(np.float64) - y.want).max()) / a["range"]
            lines.append(f"RLEN {tag}: ERR {err:.2e} (x{err / y.err32:.2f}) / irls_f32 {y.err32:.2e}")
            print(lines[-1], flush=True)
            worst["err_ratio"] = max(worst["err_ratio"], (err / y.err32, tag))
    for k, (v, tag) in worst.items():
        lines.append(f"RLEN worst {k}: {v:.4g} ({tag})")
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def coupled_lengths(capi, inst, path, couplings):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import robust_bounds as rb
    import robust_coupled_bounds as cb
    import robust_coupled_np as rc
    borders = {b[0]: b[1:] for b in cb.BORDERS}
    cases = [c + (0, True) for c in cb.accuracy_cases() if c[7] in couplings] + [c + (0, False) for c in cb.large_cases() if c[7] in couplings]
    i = 0
    for name in ("neumann", "free_lt"):
        for n in WALK:
            for pq, epsf, links, wk in (((1.0, 2.0), 1e-3, False, "sparse"), ((1.5, 2.0), 1e-2, True, "dense")):
                for size in ((7, n), (n, 6)):
                    cases.append((name, size, pq, epsf, links, wk, 3, couplings[i % len(couplings)], 1, True))
                    i += 1
    lines = ["# robust solve, coupled gradient terms, float32, 8 fixed rounds: ERR, RES, ENERGY (tests/robust_coupled_bounds.py) beside the",
             "# restatement's rounds (robust_coupled_np.irls_f32, inner tol 1e-5) on the same input; one MI355X run of",
             "# python tools/robust_probe.py --lengths --coupling " + ("all" if len(couplings) == 3 else rc.NAMES[couplings[0]]),
             "CLEN coupling border W H C p q eps links weights | ERR (x irls_f32) RES (x irls_f32) ENERGY rel rise sweeps / irls_f32 ERR RES iterations"]
    worst = {k: (0.0, None) for k in ("err_ratio", "res_ratio", "err_zero", "res_zero", "energy_rel")}
    worst["energy_rise"] = (-1.0, None)
    for name, (H, W), (p, q), epsf, links, wk, C, cpl, seed, exact in cases:
        sides, periodic = borders[name]
        a = rb.with_dead_nan(sides, periodic, rb.make_input(H, W, C, wk, links, seed))
        eps = epsf * a["range"]
        y = cb.Yardstick(sides, periodic, p, q, eps, eps, a, cpl, exact=exact)
        kw = dict(isotropic=bool(cpl & rc.ISO), joint_channels=bool(cpl & rc.JOINT))
        prev = run_rounds(inst, sides, periodic, p, q, eps, a, cb.ROUNDS - 1, **kw)
        out = run_rounds(inst, sides, periodic, p, q, eps, a, cb.ROUNDS, **kw)
        sweeps = inst.info().sweeps
        energy, iters = inst.robust_trace()
        err, res = y.measure(prev, out)
        want_e = float(y.energy(out).sum())
        erel = abs(float(energy[-1]) - want_e) / want_e
        rise = float(np.max(np.diff(energy) / energy[:-1]))
        tag = f"{rc.NAMES[cpl]} {name} {W}x{H}x{C} p={p} q={q} eps={epsf} links={int(links)} {wk}"
        er = err / y.err32 if y.err32 > 0 else float("nan")
        rr = res / y.res32 if y.res32 > 0 else float("nan")
        lines.append(f"CLEN {rc.NAMES[cpl]:9s} {name:11s} {W:3d} {H:3d} {C} {p} {q} {epsf:g} {int(links)} {wk:6s} | ERR {err:.2e} (x{er:.2f}) RES {res:.2e} "
                     f"(x{rr:.2f}) ENERGY {erel:.2e} rise {rise:+.1e} sweeps {sweeps:3d} / irls_f32 {y.err32:.2e} {y.res32:.2e} {sum(y.iters32):3d}")
        print(lines[-1], flush=True)
        for key, ratio, value, ref in (("err", er, err, y.err32), ("res", rr, res, y.res32)):
            if ref > 0:
                worst[key + "_ratio"] = max(worst[key + "_ratio"], (ratio, tag))
            elif exact or key == "res":
                worst[key + "_zero"] = max(worst[key + "_zero"], (value, tag))
        worst["energy_rel"] = max(worst["energy_rel"], (erel, tag))
        worst["energy_rise"] = max(worst["energy_rise"], (rise, tag))
    for k, (v, tag) in worst.items():
        lines.append(f"CLEN worst {k}: {v:.4g} ({tag})")
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def coupled_timing(capi, inst, path, calls, warmup, couplings, base_links):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import robust_bounds as rb
    import robust_coupled_np as rc
    n, rounds = 1024, 8
    img = (rb.clean_image(n, n, 3) + 0.1 * np.random.default_rng(5).standard_normal((n, n, 3))).astype(np.float32)
    zero = np.zeros_like(img)
    lay = capi.poisson_layout_of(img)
    G = capi.SC_POISSON_GUIDANCE | capi.SC_POISSON_NEUMANN
    host = {"gx": zero, "gy": zero, "data": img, "weight": np.full(img.shape, 2.0, np.float32)}
    if base_links:
        rng = np.random.default_rng(7)
        host["smooth_x"], host["smooth_y"] = (np.exp(rng.uniform(np.log(0.25), 0.0, img.shape)).astype(np.float32) for _ in range(2))
    dev = {k: inst.to_device(v) for k, v in host.items()}
    dev["out"] = inst.malloc(img.nbytes)
    try:
        jobs = capi.Instance.make_robust_jobs(1)
        for k, ptr in dev.items():
            setattr(jobs[0], k, ptr)
        for cpl in [0] + list(couplings):
            prm = capi.RobustParams(G | capi.robust_coupling_bits(bool(cpl & rc.ISO), bool(cpl & rc.JOINT)), 1.0, 1e-2, 2.0, 1e-2, rounds, -1.0, 0.0, 0)
            ms = []
            for i in range(warmup + calls):
                inst.robust_device(prm, lay, jobs)
                if i >= warmup:
                    ms.append(inst.info().ms_call)
            energy, iters = inst.robust_trace()
            rec = {"probe": "robust_coupled_time", "form": rc.NAMES[cpl], "size": n, "channels": 3, "border": "neumann", "base_links": bool(base_links),
                   "problem": "tv_denoise: zero guidance, weight 2, p = 1, q = 2, eps = 1e-2", "rounds": rounds, "calls": calls,
                   "ms_call": round(float(np.median(ms)), 4), "inner_iterations": [int(v) for v in iters], "sweeps": int(inst.info().sweeps),
                   "energy_first_last": [float(energy[0]), float(energy[-1])]}
            print(json.dumps(rec), flush=True)
            os.makedirs(os.path.dirname(path), exist_ok=True)
            with open(path, "a") as f:
                f.write(json.dumps(rec) + "\n")
    finally:
        for p in dev.values():
            inst.free(p)


def timing(capi, inst, path, calls, warmup, host_loop):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import robust_bounds as rb
    import robust_np
    import wls_np
    n, rounds = 1024, 8
    a = rb.make_input(n, n, 3, "dense", False, 5)
    eps = 1e-3 * a["range"]
    ones = np.ones_like(a["data"])
    lay = capi.poisson_layout_of(a["data"])
    G = capi.SC_POISSON_GUIDANCE | capi.SC_POISSON_NEUMANN
    dev = {k: inst.to_device(v) for k, v in (("gx", a["gx"]), ("gy", a["gy"]), ("data", a["data"]), ("weight", a["weight"]), ("sx", ones), ("sy", ones),
                                             ("lap", ones))}
    dev["out"] = inst.malloc(a["data"].nbytes)
    rec = {"probe": "robust_time", "size": n, "channels": 3, "border": "neumann", "p": 1.0, "q": 2.0, "eps": "1e-3 of the range", "rounds": rounds,
           "calls": calls}
    try:
        rj = capi.Instance.make_robust_jobs(1)
        rj[0].gx, rj[0].gy, rj[0].data, rj[0].weight, rj[0].out = (dev[k] for k in ("gx", "gy", "data", "weight", "out"))
        wj = capi.Instance.make_wls_jobs(1)
        wj[0].gx, wj[0].gy, wj[0].data, wj[0].weight, wj[0].smooth_x, wj[0].smooth_y, wj[0].out = (dev[k] for k in ("gx", "gy", "data", "weight", "sx", "sy", "out"))
        robust = lambda p, r: inst.robust_device(capi.RobustParams(G, p, eps, 2.0, eps, r, -1.0, 0.0, 0), lay, rj)
        legs = {"robust_8_rounds": lambda: robust(1.0, 8), "robust_4_rounds": lambda: robust(1.0, 4), "robust_quadratic": lambda: robust(2.0, 0),
                "wls_unit_links": lambda: inst.wls_device(capi.WlsParams(G, 0.0, 0, 0.0, 0.0), lay, wj)}
        ms = {k: [] for k in legs}
        wall = []
        for i in range(warmup + calls):
            for k, call in legs.items():
                t0 = time.perf_counter()
                call()
                t1 = time.perf_counter()
                if i >= warmup:
                    ms[k].append(inst.info().ms_call)
                    if k == "robust_8_rounds":
                        wall.append((t1 - t0) * 1e3)
                if k == "robust_8_rounds":
                    energy, iters = inst.robust_trace()
                    sweeps = inst.info().sweeps
        med = {k: float(np.median(v)) for k, v in ms.items()}
        rec.update({"ms_call_" + k: round(v, 4) for k, v in med.items()})
        rec["ms_per_late_round"] = round((med["robust_8_rounds"] - med["robust_4_rounds"]) / 4.0, 4)
        rec["ms_final_energy_and_wait"] = round(med["robust_quadratic"] - med["wls_unit_links"], 4)
        rec["ms_wall_robust_8_rounds"] = round(float(np.median(wall)), 3)
        rec["inner_iterations_warm"] = [int(v) for v in iters]
        rec["sweeps"] = int(sweeps)
        rec["energy"] = [float(v) for v in energy]
        robust(1.0, 8)          # (the legs' last call was another one: the 8 rounds' iterate once more)
        u_dev = inst.from_device(dev["out"], a["data"].shape, np.float32)
        if host_loop:
            # the same rounds from the host: u down, links and weights in numpy, links, weights and div(s g) up, a cold sc_hip_wls_device
            hj = capi.Instance.make_wls_jobs(1)
            hj[0].lap, hj[0].data, hj[0].weight, hj[0].smooth_x, hj[0].smooth_y, hj[0].out = (dev[k] for k in ("lap", "data", "weight", "sx", "sy", "out"))
            L = capi.SC_POISSON_LAPLACIAN | capi.SC_POISSON_NEUMANN
            cold, dev_ms, np_ms, copy_ms = [], 0.0, 0.0, 0.0
            sx, sy, w2 = ones, ones, a["weight"]
            t_all = time.perf_counter()
            for k in range(rounds + 1):
                t0 = time.perf_counter()
                if k:
                    u = inst.from_device(dev["out"], a["data"].shape, np.float32)
                    t1 = time.perf_counter()
                    sx, sy, w2 = robust_np.reweigh("lrtb", "", 1.0, 2.0, eps, eps, a["weight"], None, None, a["gx"], a["gy"], a["data"], u)
                else:
                    t1 = t0
                lap = wls_np.divergence("lrtb", "", sx, sy, a["gx"], a["gy"])
                t2 = time.perf_counter()
                for name, arr in (("sx", sx), ("sy", sy), ("weight", w2), ("lap", lap)):
                    arr = np.ascontiguousarray(np.nan_to_num(arr, nan=1.0))
                    inst._check(inst.L.sc_hip_memcpy_h2d(inst.h, dev[name], arr.ctypes.data, arr.nbytes))
                t3 = time.perf_counter()
                inst.wls_device(capi.WlsParams(L, 0.0, 0, 0.0, 0.0), lay, hj)
                cold.append(int(inst.info().sweeps))
                dev_ms += inst.info().ms_call
                np_ms += (t2 - t1) * 1e3
                copy_ms += (t1 - t0 + t3 - t2) * 1e3
            rec["host_loop"] = {"inner_iterations_cold": cold, "ms_device_solves": round(dev_ms, 3), "ms_numpy_links": round(np_ms, 3),
                                "ms_copies": round(copy_ms, 3), "ms_wall": round((time.perf_counter() - t_all) * 1e3, 3)}
            u_host = inst.from_device(dev["out"], a["data"].shape, np.float32)
            # two inexact runs of the same rounds: how far apart they end, and what the energy says of either
            diff = np.abs(u_host.astype(np.float64) - u_dev)
            fixed = (a["weight"], None, None, a["gx"], a["gy"], a["data"])
            rec["host_loop"]["difference_to_the_device_loop"] = {"max": float(diff.max()), "p999": float(np.quantile(diff, 0.999)),
                                                                 "median": float(np.median(diff)), "range": a["range"]}
            rec["host_loop"]["energy"] = float(robust_np.energy("lrtb", "", 1.0, 2.0, eps, eps, *fixed, u_host).sum())
            rec["energy_of_the_written_iterate"] = float(robust_np.energy("lrtb", "", 1.0, 2.0, eps, eps, *fixed, u_dev).sum())
        print(json.dumps(rec), flush=True)
    finally:
        for p in dev.values():
            inst.free(p)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "a") as f:
        f.write(json.dumps(rec) + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lengths", action="store_true")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--lengths-out", default=os.path.join(ROOT, "profiles", "robust_lengths.txt"))
    ap.add_argument("--time-out", default=os.path.join(ROOT, "profiles", "robust_probe.json"))
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-host-loop", action="store_true")
    ap.add_argument("--coupling", choices=["iso", "joint", "both", "all"], help="measure the coupled gradient terms instead")
    ap.add_argument("--base-links", action="store_true", help="--coupling --time: the jobs carry base links")
    a = ap.parse_args()
    if a.coupling:
        couplings = {"iso": [1], "joint": [2], "both": [3], "all": [1, 2, 3]}[a.coupling]
        if a.lengths_out == ap.get_default("lengths_out"):
            a.lengths_out = os.path.join(ROOT, "profiles", "robust_coupled_lengths.txt")
        if a.time_out == ap.get_default("time_out"):
            a.time_out = os.path.join(ROOT, "profiles", "robust_coupled_probe.json")
    sys.path.insert(0, ROOT)
    from seamlesscloneoptimization_amd import capi
    inst = capi.Instance(0)
    try:
        if a.coupling:
            if a.lengths:
                coupled_lengths(capi, inst, a.lengths_out, couplings)
            if a.time:
                coupled_timing(capi, inst, a.time_out, a.calls, a.warmup, couplings, a.base_links)
        else:
            if a.lengths:
                lengths(capi, inst, a.lengths_out)
            if a.time:
                timing(capi, inst, a.time_out, a.calls, a.warmup, not a.no_host_loop)
    finally:
        inst.destroy()


if __name__ == "__main__":
    main()
