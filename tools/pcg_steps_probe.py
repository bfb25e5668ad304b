#!/usr/bin/env python3
"""Measures single iterates and whole solves of the conjugate-gradient families on the GPU at the tilings of tests/pcg_steps_bounds.py
(its cases(): weighted, WLS, region, volume and WLS volume under free and periodic time, each at every shape it can take).

Per input, first the facts of sc_hip_pcg_plan the shape is there for, then
  STEP   k = 1, 2, 3: a call with max_iters = k, its sweeps, and D = max |u - u64_k| / max |u64_k| against iterate k of the family's
         float64 iteration, beside the same D of its pcg_f32 and the ratio of the two;
  SOLVE  the default call's ERR, RES (the family's own *_bounds.py Yardstick, the exact solve sparse or by float64 conjugate gradients
         above the dense limits) and sweeps beside pcg_f32's -- every shape but 1025 x 1025;
then the worst ratios and where: what STEP_FACTOR / STEP_FLOOR of tests/pcg_steps_bounds.py are set from, and whether the families'
ERR / RES factors hold at these shapes with half to spare.  Written to --out (default profiles/pcg_steps.txt).

    python tools/pcg_steps_probe.py [--families weighted,wls,...] [--shapes three_groups,...] [--no-solve]
"""
from __future__ import annotations

import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--families", default="")
    ap.add_argument("--shapes", default="")
    ap.add_argument("--no-solve", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pcg_steps.txt"))
    args = ap.parse_args()
    from seamlesscloneoptimization_amd import capi
    import pcg_steps_bounds as sb

    bounds = {"weighted": sb.wb, "wls": sb.lb, "region": sb.rb, "volume": sb.vb}
    cases = [c for c in sb.cases() if (not args.families or c[0] in args.families.split(",")) and (not args.shapes or c[1] in args.shapes.split(","))]
    lines = ["# Conjugate-gradient families at the tilings of tests/pcg_steps_bounds.py: single iterates against the float64 iteration, whole",
             "# solves against the exact solve; one MI355X run of python tools/pcg_steps_probe.py",
             "PLAN family shape border W H C T | cg bands rows eparts egroups stride | the shape's facts",
             "STEP family shape border k | sweeps D (x pcg_f32) / pcg_f32 D",
             "SOLVE family shape border | ERR (x pcg_f32) RES (x pcg_f32) sweeps / pcg_f32 ERR RES iterations"]
    worst = {"step_ratio": (0.0, None), "step_zero": (0.0, None), "step_d": (0.0, None)}
    solve_worst = {}
    bad = []
    inst = capi.Instance(0)
    try:
        for family, shape, border in cases:
            t0 = time.time()
            c = sb.case(family, shape, border)
            tag = f"{family} {shape} {border}"
            H, W = c.size
            plan = capi.pcg_plan(W, H, c.kind(), c.T)
            facts = sb.regime(shape, plan)
            lines.append(f"PLAN {tag} {W} {H} {c.C} {c.T} | {plan['cg']} {plan['bands']} {plan['rows']} {plan['eparts']} {plan['egroups']} {plan['stride']} | "
                         + ", ".join(f"{name}: {'yes' if ok else 'NO'}" for name, ok in facts))
            ref, ran = sb.steps(family, shape, border)
            if ran <= max(sb.STEPS) + sb.POLL:
                bad.append(f"{tag}: pcg_f32 converged in {ran} iterations")
            for k in sb.STEPS:
                out = c.call(inst, max_iters=k, allow_not_converged=True)
                sweeps = inst.info().sweeps
                u64, d32 = ref[k]
                d = c.distance(out, u64)
                lines.append(f"STEP {tag} {k} | {sweeps} {d:.3e} ({d / d32 if d32 else float('inf'):.2f}) / {d32:.3e}")
                if sweeps != k:
                    bad.append(f"{tag}: max_iters {k} ran {sweeps} sweeps")
                if d32 > 0:
                    worst["step_ratio"] = max(worst["step_ratio"], (d / d32, f"{tag} k={k}"), key=lambda v: v[0])
                else:
                    worst["step_zero"] = max(worst["step_zero"], (d, f"{tag} k={k}"), key=lambda v: v[0])
                worst["step_d"] = max(worst["step_d"], (d, f"{tag} k={k}"), key=lambda v: v[0])
            if not args.no_solve and shape != "capped_segments":
                y = c.yardstick()
                out = c.call(inst)
                info = inst.info()
                err, res = y.measure(out)
                er, rr = (err / y.err32 if y.err32 else float("inf")), (res / y.res32 if y.res32 else float("inf"))
                lines.append(f"SOLVE {tag} | {err:.3e} ({er:.2f}) {res:.3e} ({rr:.2f}) {info.sweeps} / {y.err32:.3e} {y.res32:.3e} {y.iters32}")
                b = bounds.get(family, sb.vwb)
                w = solve_worst.setdefault(family.split("_free")[0].split("_periodic")[0], {"err": (0.0, None), "res": (0.0, None), "b": b})
                w["err"] = max(w["err"], (er, tag), key=lambda v: v[0])
                w["res"] = max(w["res"], (rr, tag), key=lambda v: v[0])
                if info.sweeps > y.max_sweeps() or not info.converged:
                    bad.append(f"{tag}: {info.sweeps} sweeps (pcg_f32 {y.iters32}), converged {info.converged}")
            print(lines[-1], f"[{time.time() - t0:.1f} s]", flush=True)
    finally:
        inst.destroy()
    lines.append("# worst")
    lines.append(f"WORST step ratio {worst['step_ratio'][0]:.2f} ({worst['step_ratio'][1]})")
    lines.append(f"WORST step D {worst['step_d'][0]:.3e} ({worst['step_d'][1]})")
    lines.append(f"WORST step D where pcg_f32's is 0: {worst['step_zero'][0]:.3e} ({worst['step_zero'][1]})")
    for fam, w in solve_worst.items():
        b = w["b"]
        lines.append(f"WORST solve {fam}: ERR ratio {w['err'][0]:.2f} of {b.ERR_FACTOR:g} ({w['err'][1]}), RES ratio {w['res'][0]:.2f} of {b.RES_FACTOR:g} ({w['res'][1]})")
    lines += [f"BAD {b}" for b in bad]
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[lines.index("# worst"):]))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
