#!/usr/bin/env python3
"""Measures the robust volume, coupled volume, robust region and bounded calls at the tilings of tests/round_tilings_bounds.py (GPU).

Walks the matrices of tests/test_gpu_round_tilings.py (NaN in every element that is not read) and prints, per case and round k = 1, 2,
3, ERR and RES of a call of k rounds (round_tol = -1) beside the float32 restatement's of that round with their ratios, per case the
ENERGY of the last round's trace entry against the restatement's energy of the written iterate; per capped region run D beside the
float32 restatement's; per bounded case the rounds, ERR, RES_FREE, SIGN and the trace's counts beside the reference's.  Then a WORST
line per family: the worst ratios -- what the families' own factors are held against at these shapes.  Written to --out (default
profiles/round_tilings.txt).

    python tools/round_tilings_probe.py [--families volume,region,capped,bounded] [--out FILE]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


class Worst:
    def __init__(self):
        self.w = {}

    def take(self, name, value, tag):
        if name not in self.w or value > self.w[name][0]:
            self.w[name] = (value, tag)

    def lines(self, family, factors):
        return [f"WORST {family} {name}: {v:.4g} ({tag}){factors.get(name, '')}" for name, (v, tag) in self.w.items()]


def rounds_of(emit, family, tag, y, run, quadratic, trace, limit, worst):
    prev = quadratic()
    for k in range(1, len(y.fig32)):
        out = run(k)
        err, res = y.measure(prev, out, k)
        e32, r32 = y.fig32[k]
        emit(f"ROUND {family} {tag} k={k}: ERR {err:.3e} (x{err / e32:.2f} of {e32:.3e}) RES {res:.3e} (x{res / r32:.2f} of {r32:.3e})")
        worst.take("ERR ratio", err / e32, f"{tag} k={k}")
        worst.take("RES ratio", res / r32, f"{tag} k={k}")
        prev = out
    energy, iters = trace()
    want = float(np.sum(y.energy(out)))
    rel = abs(float(energy[-1]) - want) / want
    emit(f"ENERGY {family} {tag}: {rel:.3e} (x{rel / limit:.2f} of the bound {limit:.1e}) inner iterations {list(map(int, iters))} / {y.iters32}")
    worst.take("ENERGY", rel, tag)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--families", default="volume,region,capped,bounded")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "round_tilings.txt"))
    a = ap.parse_args()
    families = a.families.split(",")
    from seamlesscloneoptimization_amd import capi
    import bounded_bounds as bb
    import region_np
    import region_robust_bounds as gr
    import region_robust_np as rr
    import round_tilings_bounds as tb
    import volume_coupled_bounds as cb
    import volume_robust_bounds as rb
    import volume_robust_np as vr

    lines = ["# robust volume, coupled volume, robust region and bounded calls at the tilings of tests/round_tilings_bounds.py, float32, %d rounds behind" % tb.ROUNDS,
             "# the quadratic one, round by round beside the float32 restatement on the same input; one MI355X run of python tools/round_tilings_probe.py"]

    def emit(line):
        lines.append(line)
        print(line, flush=True)

    fixed = dict(round_tol=-1.0)
    inst = capi.Instance(0)
    try:
        if "volume" in families:
            worst = {"robust volume": Worst(), "coupled volume": Worst()}
            for i, case in enumerate(tb.volume_matrix()):
                clean, pen, cpl, y = tb.volume_case(i)
                p = rb.nan_unread(clean)
                run = (lambda k: inst.volume_coupled(**cb.call_args(p, pen, cpl, max_rounds=k, **fixed))) if cpl else \
                      (lambda k: inst.volume_robust(**rb.call_args(p, pen, max_rounds=k, **fixed)))
                quadratic = lambda: inst.volume_wls(p["data"], p["state"], p["weight"], p["sx"], p["sy"], p["smt"], p["gx"], p["gy"], p["gt"],
                                                    boundary=vr._boundary(p), tau=p["tau"], loop=p["tper"], free_sides=p["sides"], periodic=p["periodic"])
                family = "coupled volume" if cpl else "robust volume"
                rounds_of(emit, family, tb.volume_id(case), y, run, quadratic, inst.robust_trace, cb.ENERGY_REL if cpl else rb.ENERGY_REL, worst[family])
            emit("\n".join(worst["robust volume"].lines("robust volume", {"ERR ratio": f" of {rb.ERR_FACTOR:g}", "RES ratio": f" of {rb.RES_FACTOR:g}", "ENERGY": f" of {rb.ENERGY_REL:g}"})))
            emit("\n".join(worst["coupled volume"].lines("coupled volume", {"ERR ratio": f" of {cb.ERR_FACTOR:g}", "RES ratio": f" of {cb.RES_FACTOR:g}", "ENERGY": f" of {cb.ENERGY_REL:g}"})))
        if "region" in families:
            worst = Worst()
            for i, case in enumerate(tb.region_matrix()):
                clean, pen, cpl, y = tb.region_case(i)
                p = gr.nan_unread(clean)
                run = lambda k: inst.region_robust(**gr.call_args(p, pen, cpl, max_rounds=k, **fixed))
                quadratic = lambda: inst.region(p["data"], p["state"], p["weight"], p["sx"], p["sy"], gx=p["gx"], gy=p["gy"], boundary=rr._boundary(p),
                                                free_sides=p["sides"], periodic=p["periodic"])
                rounds_of(emit, "robust region", tb.region_id(case), y, run, quadratic, inst.robust_trace, gr.ENERGY_REL, worst)
            emit("\n".join(worst.lines("robust region", {"ERR ratio": f" of {gr.ERR_FACTOR:g}", "RES ratio": f" of {gr.RES_FACTOR:g}", "ENERGY": f" of {gr.ENERGY_REL:g}"})))
        if "capped" in families:
            worst = Worst()
            for i in tb.CAPPED:
                shape, border, pattern, cpl, exps, epsf = tb.region_matrix()[i]
                clean = tb.region_input(shape, border, pattern)
                pen = gr.penalties(clean, exps, epsf)
                p = gr.nan_unread(clean)
                u0 = inst.region(p["data"], p["state"], p["weight"], p["sx"], p["sy"], gx=p["gx"], gy=p["gy"], boundary=rr._boundary(p), free_sides=p["sides"],
                                 periodic=p["periodic"], max_iters=tb.CAP, allow_not_converged=True)
                out = inst.region_robust(**gr.call_args(p, pen, cpl, max_rounds=1, max_iters=tb.CAP, allow_not_converged=True, **fixed))
                u64, bound = tb.capped_bound(clean, pen, cpl, u0)
                d, d32 = tb.distance(clean, out, u64), bound / tb.STEP_FACTOR
                emit(f"CAPPED {tb.region_id(tb.region_matrix()[i])}: D {d:.3e} (x{d / d32:.2f} of {d32:.3e})")
                worst.take("D ratio", d / d32, tb.region_id(tb.region_matrix()[i]))
            emit("\n".join(worst.lines("capped region round", {"D ratio": f" of {tb.STEP_FACTOR:g}"})))
        if "bounded" in families:
            worst = Worst()
            for case in tb.bounded_matrix():
                p, y = bb.case_input(case)
                b = p["boundary"] if region_np.has_dirichlet(p["sides"], p["periodic"]) else None
                guidance = dict(gx=p["gx"], gy=p["gy"]) if case[7] == "guidance" else dict(lap=p["lap"])
                out = inst.bounded(p["data"], p["state"], p["lower"], p["upper"], p["weight"], p["sx"], p["sy"], boundary=b, free_sides=p["sides"],
                                   periodic=p["periodic"], **guidance)
                changed, active, iters = inst.bounded_trace()
                rng, err, res, sign = y.measure(out)
                outside, near = tb.violated(p, y)
                tag = bb.case_id(case)
                emit(f"BOUNDED {tag}: rounds {len(iters)} (reference {y.rounds}, pdas_f32 {y.rounds32}) RANGE {rng:.3g} ERR {err:.3e} (x{err / y.err32:.2f} of "
                     f"{y.err32:.3e}) RES_FREE {res:.3e} (x{res / y.res32:.2f} of {y.res32:.3e}) SIGN {sign:.3g} ({y.sign32:.3g}) active {list(map(int, active))} "
                     f"changed {list(map(int, changed))}; the unconstrained reference violates {outside} ({near} within the ERR bound of a bound), the "
                     f"reference's set {int((y.set != 0).sum())} of {int(y.unk.sum())} unknowns")
                worst.take("ERR ratio", err / y.err32, tag)
                worst.take("RES_FREE ratio", res / y.res32, tag)
                worst.take("SIGN", sign, tag)
                worst.take("RANGE", rng, tag)
                worst.take("rounds over the reference's", len(iters) - y.rounds, tag)
            emit("\n".join(worst.lines("bounded", {"ERR ratio": f" of {bb.ERR_FACTOR:g}", "RES_FREE ratio": f" of {bb.RES_FACTOR:g}"})))
    finally:
        inst.destroy()
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
