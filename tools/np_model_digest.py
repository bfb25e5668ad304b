#!/usr/bin/env python3
"""The record of the tests' numpy yardsticks, host only: for a fixed list of inputs, one line per group of cases (a shape or a walked
length, with its inputs, border combinations and lambdas),

    <group> n=<cases> <SHA-256> err32=<float.hex> res32=<float.hex> max|u|=<of the float64 references> [rel=<...>]

The SHA-256 runs over every case's float32 yardstick solve (its bytes) followed by that case's err32 and res32 as float.hex(); the
err32 and res32 printed are the group's largest.  err32 and res32 are what the GPU tests' float32 bounds are factors of (tests/direct_bounds.py, and the PCG yardsticks of
tests/weighted_bounds.py, wls_bounds.py, robust_bounds.py, whose preconditioner is the direct float32 solve).  Two trees hold the GPU
tests to the same bounds exactly when their outputs are equal line for line (the rel column apart).

    python tools/np_model_digest.py [--root DIR] [--against OTHER_ROOT] > profiles/np_models.txt

--root: the checkout whose tests/ is read (default: this one).  --against: rel = the group's largest max |u - u'| / max |u'| against the float64
reference of another checkout, computed by a child process case by case.  Nothing of the package is imported.

The cases: the two length walks of direct_bounds (strips capped at 512 unknowns), the shapes of tests/test_gpu_neumann*.py,
test_gpu_screened.py, test_gpu_mixed.py, test_gpu_periodic.py and of tests/test_screened_host.py and test_neumann_lengths_host.py
(columns first), the preconditioner call of weighted_np, and one weighted, WLS and robust yardstick per border of BORDERS."""
import argparse
import dataclasses
import hashlib
import os
import subprocess
import sys
import zlib

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--against")
ap.add_argument("--wants", action="store_true", help="write the float64 references' bytes to stdout instead (what --against reads)")
ARGS = ap.parse_args()
sys.path.insert(0, os.path.join(os.path.abspath(ARGS.root), "tests"))

import direct_bounds as db  # noqa: E402
import direct_np as dn  # noqa: E402

# family -> the Bounds whose conventions its yardstick follows
FAMILIES = {"neumann": db.NEUMANN, "screened": db.SCREENED, "mixed": db.MIXED, "periodic": db.PERIODIC,
            "neumann-columns": dataclasses.replace(db.NEUMANN, order=dn.COLUMNS_FIRST),      # test_neumann_lengths_host.py's table
            "frame": db.MIXED}                                                               # test_screened_host.py's Dirichlet sizes


def direct(family, sides, periodic, lam, data, lap, boundary):
    """(float32 yardstick solve, err32, res32, float64 reference)"""
    y = FAMILIES[family].yardstick(sides, periodic, lam, data, lap, boundary)
    return y.u32, y.err32, y.res32, y.want


# ---- the cases
BORDERS = [("lrtb", ""), ("", ""), ("t", "x")]
STRIP = 512


def inputs(name, kind, W, H, C, periodic):
    """(data, lap, boundary), float32: the reconstruction of a white-noise or a smooth image from its forward differences (data and
    boundary the image), or a random guidance field (sigma 20) with random data and boundary"""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    if kind == "random":
        gx, gy = (rng.normal(0, 20, (H, W, C)).astype(np.float32) for _ in range(2))
        return rng.uniform(-50, 300, (H, W, C)).astype(np.float32), dn.divergence(gx, gy, periodic), rng.uniform(-100, 400, (H, W, C)).astype(np.float32)
    img = dn.smooth_image(H, W, C, int(rng.integers(1 << 30))) if kind == "smooth" else rng.uniform(-50, 300, (H, W, C)).astype(np.float32)
    return img, dn.divergence(*dn.forward_differences(img, periodic), periodic), img


def capped(cases, strip64, lines):
    """a length walk with both strips replaced by one of STRIP unknowns (`lines`: the walked axis's pixels less its unknowns)"""
    out = [c for c in cases if c[0] < strip64]
    for c in cases:
        if c[0] == strip64:
            W, H = c[-3], c[-2]
            out.append((STRIP,) + c[1:-3] + ((STRIP + lines, H) if W > H else (W, STRIP + lines)) + c[-1:])
    return out


def direct_cases():
    """{group: [(name, family, sides, periodic, lam, kind, W, H, C)]}, name the seed of the case's inputs"""
    out = {}

    def add(group, family, sides, periodic, lam, kinds, W, H, C):
        for kind in kinds:
            case = ("%s %s/%s lam=%g %s %dx%dx%d" % (family, sides or "-", periodic or "-", lam, kind, W, H, C), family, sides, periodic, lam, kind, W, H, C)
            if case not in out.setdefault(family + " " + group, []):
                out[family + " " + group].append(case)

    rough = ("reconstruction", "random")
    for W, H in [(2, 2), (2, 41), (41, 2), (37, 29), (300, 200), (723, 722), (1280, 721), (4000, 143), (2050, 1030), (8192, 64)]:      # test_gpu_neumann.py
        add("%dx%d" % (W, H), "neumann", "lrtb", "", 0.0, rough, W, H, 3 if W * H <= 60000 else 1)
    for n in [2, 3, 4, 5, 24, 25, 32, 33, 40, 41, 129, 300, STRIP]:                     # test_gpu_neumann_lengths.py: the walk, the cuts, the mean parts
        add("walk n=%d" % n, "neumann", "lrtb", "", 0.0, rough + (("smooth",) if n >= 256 else ()), n, 9, 2)
        add("walk n=%d" % n, "neumann", "lrtb", "", 0.0, rough + (("smooth",) if n >= 256 else ()), 9, n, 2)
    for W, H in [(1024, 1024), (1025, 1024), (1024, 513), (513, 1024), (3000, 400), (400, 3000), (9, 255), (9, 257), (9, 513)]:
        add("%dx%d" % (W, H), "neumann", "lrtb", "", 0.0, ("reconstruction",), W, H, 1)
    for W, H in [(8192, 9), (9, 8192), (8192, 64), (4097, 9), (5121, 9), (2050, 1030), (300, 200), (3, 9), (2, 2)]:      # test_neumann_lengths_host.py
        add("%dx%d" % (W, H), "neumann-columns", "lrtb", "", 0.0, ("reconstruction", "smooth") if max(W, H) >= 256 else ("reconstruction",), W, H, 1)
    for W, H in [(2, 2), (3, 3), (2, 41), (41, 3), (37, 29), (300, 200), (723, 722), (1280, 721), (4000, 143), (1030, 1026)]:           # test_gpu_screened.py
        for lam in (1e-3, 0.1, 10.0):
            add("%dx%d" % (W, H), "screened", "lrtb", "", lam, ("random",), W, H, 3 if W * H <= 60000 else 1)
    for n in [2, 3, 4, 5, 8, 9, 24, 25, 31, 32, 33, 40, 41, 96, 97, 128, 129, 160, 161, 251]:
        add("walk n=%d" % n, "screened", "lrtb", "", 1e-3, ("random",), n, 7, 2)
        add("walk n=%d" % n, "screened", "lrtb", "", 0.1, ("random",), 7, n, 2)
    for lam in (1e-3, 0.1, 10.0, 1e4):                                                  # test_screened_host.py
        for H, W, C in [(2, 2, 1), (2, 5, 2), (3, 3, 1), (7, 2, 1), (37, 29, 3), (64, 50, 4), (9, 130, 1)]:
            add("host %dx%dx%d" % (W, H, C), "screened", "lrtb", "", lam, ("random",), W, H, C)
        for H, W, C in [(3, 3, 1), (3, 17, 2), (19, 3, 1), (37, 29, 3), (64, 50, 4), (9, 130, 1)]:
            add("host %dx%dx%d" % (W, H, C), "frame", "", "", lam, ("random",), W, H, C)
    for n, axis, sides, W, H, _ in capped(db.mixed_length_cases(), db.MIXED_STRIP64, 1):
        add("walk n=%d" % n, "mixed", sides, "", 0.0, rough + (("smooth",) if n >= 256 else ()), W, H, 2)
    for sides in dn.MIXED_SIDES:                                                        # test_gpu_mixed.py
        for lam in (0.0, 1e-3, 0.5):
            add("%s 37x29" % sides, "mixed", sides, "", lam, rough, 37, 29, 3)
    for n, axis, sides, periodic, W, H, _ in capped(db.periodic_length_cases(), db.PERIODIC_STRIP64, 0):
        add("walk n=%d" % n, "periodic", sides, periodic, 0.0, rough + (("smooth",) if n >= 256 else ()), W, H, 2)
    for sides, periodic in dn.COMBOS:                                                   # test_gpu_periodic.py
        for lam in (0.0, 0.25, 0.5):
            add("%s/%s 37x29" % (sides or "-", periodic), "periodic", sides, periodic, lam, rough, 37, 29, 3)
    return out


class Line:
    """one output line: the digest and the worst figures of the cases added to it"""

    def __init__(self, group):
        self.group, self.n, self.sha, self.err32, self.res32, self.R, self.rel = group, 0, hashlib.sha256(), 0.0, 0.0, 0.0, None

    def add(self, u32, err32, res32, want, other=None):
        self.n += 1
        self.sha.update(np.ascontiguousarray(u32, np.float32).tobytes() + (float(err32).hex() + float(res32).hex()).encode())
        self.err32, self.res32, self.R = max(self.err32, float(err32)), max(self.res32, float(res32)), max(self.R, float(np.abs(want).max()))
        if other is not None:
            self.rel = max(self.rel or 0.0, float(np.abs(want - other).max()) / float(np.abs(other).max()))
        return self

    def print(self):
        print("%s n=%d %s err32=%s res32=%s max|u|=%.17g%s" % (self.group, self.n, self.sha.hexdigest(), self.err32.hex(), self.res32.hex(), self.R,
                                                               "" if self.rel is None else " rel=%.3g" % self.rel), flush=True)


def main():
    child = None
    if ARGS.against:
        child = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--root", ARGS.against, "--wants"], stdout=subprocess.PIPE)
    worst = 0.0
    for group, cases in direct_cases().items():
        out = Line(group)
        for name, family, sides, periodic, lam, kind, W, H, C in cases:
            data, lap, boundary = inputs(name, kind, W, H, C, periodic)
            u32, err32, res32, want = direct(family, sides, periodic, lam, data if lam else None, lap, boundary)
            if ARGS.wants:
                sys.stdout.buffer.write(np.ascontiguousarray(want, np.float64).tobytes())
                continue
            out.add(u32, err32, res32, want, np.frombuffer(child.stdout.read(want.size * 8), np.float64).reshape(want.shape) if child else None)
        if not ARGS.wants:
            out.print()
            worst = max(worst, out.rel or 0.0)
    if child:
        assert child.stdout.read() == b"" and child.wait() == 0
        print("# worst rel %.3g" % worst)
    if ARGS.wants:
        return
    # the preconditioner of the PCG yardsticks, and one yardstick of each PCG family per border
    import robust_bounds as rb
    import weighted_bounds as wb
    import weighted_np
    import wls_bounds as lb
    import wls_np
    H, W, C = 5, 16, 3
    for sides, periodic in BORDERS:
        tag = "%s/%s %dx%dx%d" % (sides or "-", periodic or "-", W, H, C)
        blk = dn.unknowns(sides, periodic, H, W)
        r = np.random.default_rng(zlib.crc32(tag.encode())).normal(0, 1, (H, W, C)).astype(np.float32)[blk]
        z = [weighted_np._precond(sides, periodic, np.float32(lam), r, (H, W, C)) for lam in (0.0, 0.3)]
        print("precond %s lam=0,0.3 %s" % (tag, hashlib.sha256(np.ascontiguousarray(z).tobytes()).hexdigest()), flush=True)
        data, weight, sx, sy, lap, boundary = lb.make_input(H, W, C, "loguniform" if "loguniform" in wb.WEIGHTS else wb.WEIGHTS[0], "loguniform")
        b = boundary if weighted_np.has_dirichlet(sides, periodic) else None
        y = wb.Yardstick(sides, periodic, weight, data, lap, boundary)
        Line("weighted " + tag).add(weighted_np.pcg_f32(sides, periodic, weight, data, lap, b)[0], y.err32, y.res32, y.want).print()
        y = lb.Yardstick(sides, periodic, weight, sx, sy, data, lap, boundary)
        Line("wls " + tag).add(wls_np.pcg_f32(sides, periodic, weight, sx, sy, data, lap, b, max_iters=lb.MAX_ITERS)[0], y.err32, y.res32, y.want).print()
        a = rb.with_dead_nan(sides, periodic, rb.make_input(H, W, C, "dense", True))
        eps = rb.EPS[0] * a["range"]
        y = rb.Yardstick(sides, periodic, *rb.PQ[0], eps, eps, a)
        Line("robust " + tag).add(y.u32[-1], y.err32, y.res32, y.want).print()


main()
