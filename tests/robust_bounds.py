"""The quantities the robust GPU tests hold the library to, their bounds and their inputs (tests/test_gpu_robust.py), after the pattern
of tests/wls_bounds.py with the reweighting rounds of tests/robust_np.py around the WLS solve.  Every run is ROUNDS = 8 fixed rounds
(round_tol = -1) behind the quadratic one:

    ERR     max |u - irls_exact| / R        u the last iterate, irls_exact the float64 rounds with exact inner solves, R the data's range
    RES     max |L u - rhs| / max |rhs|     of the last round's system: L and rhs from the iterate before the last (the library's own,
                                            read from a run of ROUNDS - 1 rounds, whose bytes are that iterate's)
    ENERGY  |sc_hip_robust_trace's last energy - robust_np.energy of the written iterate| / that energy

Bounds:  ERR and RES <= max(FACTOR x the same quantity for robust_np.irls_f32 on the same input, FLOOR); ENERGY <= ENERGY_REL.  irls_f32
is the same rounds with the same inner iteration, start and stop rule; the inner solves stop at tol = 1e-5 and the rounds carry what
they leave on (a relative perturbation of 1e-5 on every inner solve moves the tenth iterate by 2e-5 to 3e-4 of the range at these
sizes), so ERR is of that order in both, not the WLS call's 1e-7.  The constants come from one MI355X run of tools/robust_probe.py
--lengths over these cases and a length walk (DESIGN.md section 4 holds the table, profiles/robust_lengths.txt the record): each factor
is twice the worst ratio to the restatement, rounded up to one digit; each floor twice the worst value among the inputs where the
restatement's figure is 0 (none occurred: the floors are 0); ENERGY_REL twice the worst relative difference, rounded up to one digit."""
import numpy as np

import robust_np
import weighted_bounds as wb
import wls_bounds as lb
import wls_np

ROUNDS = 8
ERR_FACTOR, ERR_FLOOR = 20.0, 0.0              # measured: worst ratio 7.25 (neumann 6 x 9, p = 1, q = 2, eps 1e-3, sparse weights); no input where irls_f32's ERR is 0
RES_FACTOR, RES_FLOOR = 3.0, 0.0               # measured: worst ratio 1.29 (neumann 2 x 7, p = 1.5, q = 2, eps 1e-2, base links); no input where irls_f32's RES is 0
ENERGY_REL = 2e-7                              # measured: worst 6.27e-8 (neumann 6 x 4, p = 1.5, q = 2, eps 1e-2, base links)

BORDERS = wb.BORDERS
SIZES = lb.SIZES                               # rows x columns: 33 x 47, 16 x 5, 2 x 7 and 300 x 9 pixels
PQ = [(1.0, 2.0), (1.0, 1.0), (1.5, 2.0)]
EPS = [1e-2, 1e-3]                             # times the data's range
WEIGHTS = ["dense", "sparse"]


def clean_image(H, W, C=1):
    """smooth plus steps: 0.5 + 0.3 sin(x / 7) cos(y / 5) + 0.2 [(x > W / 2) xor (y > H / 3)], the channels 1, 0.8, 0.6, .. times it"""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    img = 0.5 + 0.3 * np.sin(x / 7.0) * np.cos(y / 5.0) + 0.2 * ((x > W / 2.0) ^ (y > H / 3.0))
    return img[:, :, None] * (1.0 - 0.2 * np.arange(C))[None, None, :]


def forward_differences(img):
    """(gx, gy), wrapped: the last column / row holds the difference across the seam"""
    return np.roll(img, -1, 1) - img, np.roll(img, -1, 0) - img


def corrupt(gx, gy):
    """gross outliers on a lattice that gives no pixel two corrupted links: gx += +-0.75 where x mod 7 = 3 and y mod 5 = 2,
    gy -= +-0.6 where x mod 7 = 0 and y mod 5 = 4, the sign (-1)^(x + y)"""
    H, W = gx.shape[:2]
    y, x = np.mgrid[0:H, 0:W]
    sign = np.where((x + y) % 2 == 0, 1.0, -1.0)
    gx = gx + (0.75 * sign * ((x % 7 == 3) & (y % 5 == 2)))[:, :, None]
    gy = gy - (0.6 * sign * ((x % 7 == 0) & (y % 5 == 4)))[:, :, None]
    return gx, gy


def dead_to_nan(sides, periodic, ax, ay):
    """copies of two per-link arrays (gx, gy or the base links) with NaN in every element that is not live under these borders"""
    return lb.dead_to_nan(sides, periodic, np.asarray(ax, np.float32), np.asarray(ay, np.float32))


def _sparse_weight(H, W, C, seed):
    """1 on a seeded 10 % of the pixels, 0 elsewhere; the seed moves on until every channel has a pixel set strictly inside the image
    (an unknown under every border) -- or anywhere, where the image has no inside"""
    for s in range(seed, seed + 1000):
        w = wb.weights("sparse", (H, W, C), s)
        inner = w[1:-1, 1:-1] if min(H, W) >= 3 else w
        if (inner.reshape(-1, C).sum(0) > 0).all():
            return w
    raise AssertionError("no seed sets a pixel in every channel")


def make_input(H, W, C, wkind, base_links, seed=0):
    """One problem, float32 H x W x C: dict(gx, gy, data, weight, cx, cy, boundary, range).  The guidance is the clean image's wrapped
    forward differences plus noise of sigma 0.02 and the lattice of outliers; data the clean image plus noise of sigma 0.05; boundary the
    clean image; weight log-uniform in [1e-2, 1] ("dense") or 1 on 10 % of the pixels ("sparse"); cx, cy log-uniform in [0.25, 1], or None."""
    rng = np.random.default_rng(3000 + seed + 11 * H + W)
    img = clean_image(H, W, C)
    gx, gy = forward_differences(img)
    gx, gy = corrupt(gx + 0.02 * rng.standard_normal(img.shape), gy + 0.02 * rng.standard_normal(img.shape))
    data = (img + 0.05 * rng.standard_normal(img.shape)).astype(np.float32)
    weight = wb.weights("loguniform", img.shape, 200 + seed + H) if wkind == "dense" else _sparse_weight(H, W, C, 300 + seed + H)
    cx = cy = None
    if base_links:
        cx, cy = (np.exp(rng.uniform(np.log(0.25), 0.0, img.shape)).astype(np.float32) for _ in range(2))
    return dict(gx=gx.astype(np.float32), gy=gy.astype(np.float32), data=data, weight=weight, cx=cx, cy=cy, boundary=img.astype(np.float32),
                range=float(data.max() - data.min()))


def with_dead_nan(sides, periodic, a):
    """the problem with NaN in every dead element of gx, gy and the base links"""
    a = dict(a)
    a["gx"], a["gy"] = dead_to_nan(sides, periodic, a["gx"], a["gy"])
    if a["cx"] is not None:
        a["cx"], a["cy"] = dead_to_nan(sides, periodic, a["cx"], a["cy"])
    return a


def accuracy_cases():
    """[(border, (H, W), (p, q), eps factor, base links?, weight kind, C)]: every border at every size, the options taking turns so
    that each occurs at every size and under every border (300 x 9: one channel, the exact rounds' dense solves are the cost), then the
    full product of the options at 16 x 5 under free left + top, three channels"""
    cases, i = [], 0
    for b, _, _ in BORDERS:
        for (H, W) in SIZES:
            cases.append((b, (H, W), PQ[i % 3], EPS[(i // 3) % 2], bool((i // 2) % 2), WEIGHTS[i % 2], 1 if W >= 256 else 3))
            i += 1
    for pq in PQ:
        for eps in EPS:
            for links in (False, True):
                for wk in WEIGHTS:
                    cases.append(("free_lt", (5, 16), pq, eps, links, wk, 3))
    return [c for c in dict.fromkeys(cases) if not (c[0] == "frame" and min(c[1]) < 3)]


class Yardstick:
    """One input's references: the exact rounds' last iterate and energies, and irls_f32's (ERR, RES, inner iterations) on it"""

    def __init__(self, sides, periodic, p, q, eps_g, eps_d, a, rounds=ROUNDS):
        self.border = (sides, periodic)
        self.pen = (p, q, eps_g, eps_d)
        self.a = a
        self.fixed = (a["weight"], a["cx"], a["cy"], a["gx"], a["gy"], a["data"])
        self.exact = robust_np.irls_exact(sides, periodic, p, q, eps_g, eps_d, *self.fixed, a["boundary"], rounds)
        self.want = self.exact[-1]
        self.u32, self.iters32 = robust_np.irls_f32(sides, periodic, p, q, eps_g, eps_d, *self.fixed, a["boundary"], rounds)
        self.err32, self.res32 = self.measure(self.u32[-2], self.u32[-1])

    def energy(self, u):
        return robust_np.energy(*self.border, *self.pen, *self.fixed, u)

    def measure(self, prev, out):
        """(ERR, RES) of the last iterate `out`, `prev` the iterate before it"""
        err = float(np.abs(np.asarray(out, np.float64).reshape(self.want.shape) - self.want).max()) / self.a["range"]
        res = robust_np.round_residual(*self.border, *self.pen, *self.fixed, np.asarray(prev).reshape(self.want.shape), np.asarray(out).reshape(self.want.shape))
        return err, res

    def check(self, prev, out):
        """[(quantity, measured, bound)] that fail, and the measured (ERR, RES)"""
        err, res = self.measure(prev, out)
        eb, rb = max(ERR_FACTOR * self.err32, ERR_FLOOR), max(RES_FACTOR * self.res32, RES_FLOOR)
        bad = ([("ERR", err, eb)] if not err <= eb else []) + ([("RES", res, rb)] if not res <= rb else [])
        return bad, err, res


_yard = {}


def yardstick(case):
    """(Yardstick, the problem with NaN in its dead links, sides, periodic, eps) of one accuracy case, computed once"""
    if case not in _yard:
        border, (H, W), (p, q), epsf, links, wk, C = case
        sides, periodic = {b[0]: b[1:] for b in BORDERS}[border]
        a = with_dead_nan(sides, periodic, make_input(H, W, C, wk, links))
        eps = epsf * a["range"]
        _yard[case] = (Yardstick(sides, periodic, p, q, eps, eps, a), a, sides, periodic, eps)
    return _yard[case]


def robust_problem(H, W, border):
    """The outlier test's problem under "frame", "free_l" or "periodic_x" (periodic x, free top and bottom): (sides, periodic, the
    problem, the true image); one channel, exact wrapped forward differences with the lattice of outliers, w = 0.01 towards the true
    image wherever the border leaves the constant free (all of it is an unknown then), 0 under a Dirichlet line"""
    sides, periodic = {"frame": ("", ""), "free_l": ("l", ""), "periodic_x": ("tb", "x")}[border]
    img = clean_image(H, W, 1)
    gx, gy = corrupt(*forward_differences(img))
    w = 0.0 if wls_np.has_dirichlet(sides, periodic) else 0.01
    a = dict(gx=gx.astype(np.float32), gy=gy.astype(np.float32), data=img.astype(np.float32), weight=np.full(img.shape, w, np.float32), cx=None,
             cy=None, boundary=img.astype(np.float32), range=float(img.max() - img.min()))
    return sides, periodic, with_dead_nan(sides, periodic, a), img


def batch_problems():
    """The batch test's members: (sides, periodic, [problems], eps, the index of the member whose weight holds a NaN at an unknown) --
    four Neumann problems of 17 x 23 x 3 with base links, dense and sparse weights in turn"""
    sides, periodic = "lrtb", ""
    probs = [with_dead_nan(sides, periodic, make_input(23, 17, 3, "sparse" if k % 2 else "dense", True, seed=10 + k)) for k in range(4)]
    refused = 2
    probs[refused]["weight"] = probs[refused]["weight"].copy()
    probs[refused]["weight"][5, 7, 1] = np.nan
    return sides, periodic, probs, 1e-3 * probs[0]["range"], refused
