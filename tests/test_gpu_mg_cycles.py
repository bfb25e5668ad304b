"""Every multigrid cycle on the device against its numpy restatement, at every tile seam (the walk: tests/mg_cycle_cases.py; the bounds and
where they come from: tests/mg_cycle_bounds.py; regimes and sharpness without a GPU: tests/test_mg_cycles_host.py).

A converged solve forgets a defect of the smoother, the prolongation or the restriction -- the cycle's residual is exact --, so every
route here runs a fixed budget: max_sweeps = n, update_tol = 1e-30, tol = 0 answers SC_ERR_NOT_CONVERGED and leaves iterate n.

  (a) field hooks (field_load, field_solve, field_store; one plane of noise): the float32 forms, fused and sweeps_per_launch = 1
  (b) a clone that keeps its field (SC_FLAG_KEEP_FIELD | SC_FLAG_EXACT_TABLES): with SC_FLAG_FLOAT_L1 the float32 cycle on the float16
      right-hand side and initial field; without it also float16 level 1 on the composed schedule
  (c) the same clone without SC_FLAG_KEEP_FIELD: the default fast path -- besides (b)'s formats the 16-bit field between the first launches
      (from n = 2 on; sc_hip_fused_schedule says what ran) -- judged by its output bytes.  Under update_tol = 1e-30 the bytes the judged launch
      leaves are refused, the cycle runs again in the form that keeps its field, and the post-process writes the bytes.
SC_FLAG_EXACT_TABLES takes the float-table correction away, and with it the band and node tags of the level-0 launches (other
instantiations of k_cycle0).  So (d) runs (c) on the DEFAULT tables, two and three cycles on one channel of every shape, against the twin
plus oracle/lowmode_np.correction: at n = 2 (update_tol = 1e-30) the launch before the judged one leaves the correction's cell shares, the
judged launch writes bytes with node values and is refused, the field form leaves cell shares again and the post-process adds the
correction of iterate 2; at n = 3 under the default update_tol the stop rule accepts the third cycle and the bytes are the judged
launch's own: iterate 3 plus the correction of iterate 2 -- the default clone as every caller runs it.

SC_MG_CYCLES_RECORD=<file> writes the worst figures per route and class to that file (profiles/mg_cycles.txt is one such run)."""
import os
import time

import numpy as np
import pytest

import decided_np
import mg_cycle_bounds as mb
import mg_cycle_cases as cases

pytestmark = pytest.mark.gpu

RECORD = {}


def note(route, name, n, d_gpu, d_u32, e_fmt, seconds):
    key = (route, cases.SHAPES[name][0])
    r = RECORD.setdefault(key, dict(ratio=0.0, d_gpu=0.0, d_u32=0.0, e_fmt=0.0, share=0.0, seconds=0.0, at=""))
    ratio = d_gpu / d_u32 if d_u32 > 0 else 0.0
    share = d_gpu / (mb.STEP_FACTOR * d_u32 + e_fmt) if max(d_u32, e_fmt) > 0 else 0.0
    if share >= r["share"]:
        r.update(ratio=ratio, d_gpu=d_gpu, d_u32=d_u32, e_fmt=e_fmt, share=share, at="%s n=%d" % (name, n))
    r["seconds"] = max(r["seconds"], seconds)


@pytest.fixture(scope="module")
def inst():
    from seamlesscloneoptimization_amd import capi
    i = capi.Instance(0)
    yield i
    i.destroy()
    record = os.environ.get("SC_MG_CYCLES_RECORD")
    if record:
        os.makedirs(os.path.dirname(os.path.abspath(record)), exist_ok=True)
        with open(record, "w") as f:
            f.write("# route class: worst share of the bound (D(gpu) / (%g D(u32) + E_fmt)) at shape and budget; D(gpu) D(u32) ratio E_fmt; slowest test [s]\n" % mb.STEP_FACTOR)
            for (route, cls), r in sorted(RECORD.items()):
                f.write("%-22s %-13s share %.3f at %-22s D(gpu) %.3e D(u32) %.3e ratio %.2f E_fmt %.3e  %.2f s\n"
                        % (route, cls, r["share"], r["at"], r["d_gpu"], r["d_u32"], r["ratio"], r["e_fmt"], r["seconds"]))


def fixed_budget(inst, n, flags=0, **kw):
    from seamlesscloneoptimization_amd import capi
    d = inst.default_opts()
    opts = {f[0]: getattr(d, f[0]) for f in d._fields_}
    opts.update(method=capi.SC_METHOD_MULTIGRID, max_sweeps=n, update_tol=1e-30, tol=0.0, flags=d.flags | flags, **kw)
    inst.set_solver(**opts)


# ---------------------------------------------------------------------------------------------------------------- (a) field hooks
@pytest.mark.parametrize("name", cases.NAMES)
def test_field_hooks_follow_the_cycle(inst, name):
    t0 = time.time()
    U, F = cases.noise_fields(name)
    for n in (1, 2, 3):
        for fused in (True, False):
            fixed_budget(inst, n, sweeps_per_launch=0 if fused else 1)
            inst.field_load(U, F)
            inst.field_solve(allow_not_converged=True)
            got = inst.field_store()
            assert got.shape == U.shape and inst.info().sweeps == n
            d_gpu, d_u32 = mb.distance(got[0], name, "fields", 0, n, "u64", fused), mb.yardstick(name, "fields", 0, n, fused)
            cap = mb.interior_max(got[0] - mb.solve(name, "fields", 0, n, "spec", fused))
            print("%s n=%d %s: D(gpu) %.3g D(u32) %.3g ratio %.2f; against the default spec %.3g" % (name, n, "fused" if fused else "unfused", d_gpu, d_u32, d_gpu / d_u32, cap))
            note("a_fused" if fused else "a_unfused", name, n, d_gpu, d_u32, 0.0, time.time() - t0)
            assert np.array_equal(got[0, 0], U[0, 0]) and np.array_equal(got[0, :, -1], U[0, :, -1])          # the ring stays
            assert d_gpu <= mb.STEP_FACTOR * d_u32, (name, n, fused, d_gpu, d_u32)
            if n in mb.ABS_CAP:
                assert cap < mb.ABS_CAP[n], (name, n, fused, cap)


# ---------------------------------------------------------------------------------------------------------------- (b), (c) clones
def run_clone(inst, name, n, flags):
    from seamlesscloneoptimization_amd import capi
    dst, patch, mask, cx, cy = cases.clone_inputs(name)[:5]
    fixed_budget(inst, n, flags | capi.SC_FLAG_EXACT_TABLES)
    body = dst.copy()
    rc = inst.run(patch, body, mask, cx, cy, allow_not_converged=True)
    info = inst.info()
    assert rc == capi.SC_ERR_NOT_CONVERGED and info.method == capi.SC_METHOD_MULTIGRID
    assert (info.W, info.H, info.sweeps, info.field_retry) == (*cases.shape(name), n, 0), (info.W, info.H, info.sweeps, info.field_retry)
    return body, info


@pytest.mark.parametrize("name", cases.NAMES)
def test_clone_kept_field_follows_the_cycle(inst, name):
    from seamlesscloneoptimization_amd import capi
    t0 = time.time()
    B = cases.clone_inputs(name)[5]
    for n in cases.budgets(name):
        for float_l1 in (True, False):
            run_clone(inst, name, n, capi.SC_FLAG_KEEP_FIELD | (capi.SC_FLAG_FLOAT_L1 if float_l1 else 0))
            got = inst.field_store()
            assert got.shape == B.shape
            for c in cases.channels(name, n):
                d_u32 = mb.yardstick(name, "clone", c, n)
                if float_l1:
                    d_gpu, e_fmt, bound = mb.distance(got[c], name, "clone", c, n, "u64"), 0.0, mb.float_bound(name, "clone", c, n)
                else:
                    d_gpu, e_fmt, bound = mb.distance(got[c], name, "clone", c, n, "u64_half"), mb.e_fmt(name, c, n, False), mb.format_bound(name, c, n, False)
                print("%s n=%d channel %d %s: D(gpu) %.3g D(u32) %.3g ratio %.2f E_fmt %.3g bound %.3g" % (name, n, c, "float level 1" if float_l1 else "float16 level 1",
                                                                                                          d_gpu, d_u32, d_gpu / d_u32, e_fmt, bound))
                note("b_float_l1" if float_l1 else "b_float16_l1", name, n, d_gpu, d_u32, e_fmt, time.time() - t0)
                assert np.array_equal(got[c, 0], B[c, 0]) and np.array_equal(got[c, :, 0], B[c, :, 0])
                assert d_gpu <= bound, (name, n, c, float_l1, d_gpu, bound)


@pytest.mark.parametrize("name", cases.NAMES)
def test_clone_bytes_follow_the_fast_cycle(inst, name):
    from seamlesscloneoptimization_amd import capi
    t0 = time.time()
    W, H = cases.shape(name)
    dst = cases.clone_inputs(name)[0]
    ltx, lty = cases.clone_inputs(name)[7]
    composed = bool(capi.cycle0_plan(W, H, 2)["composes"])
    for n in cases.budgets(name):
        body, info = run_clone(inst, name, n, 0)
        # what ran: the schedule of these facts, every judged launch refused (the bytes, then the field form)
        q16 = composed and n > 1
        rows, sweeps, launches, code = capi.fused_schedule([1], budget=n, q16=int(q16), composed=int(composed), early_kind=0)
        assert (sweeps, launches, code) == (info.sweeps, info.sweep_launches, capi.SC_ERR_NOT_CONVERGED)
        assert any(r["q16_out"] for r in rows) == q16 and any(r["q16_in"] for r in rows) == q16
        assert rows[0]["u_half"] == 1 and any(r["out_bytes"] for r in rows) == (n > 1)          # (one cycle: the first is the judged one, in its field form)
        # nothing outside the ROI's interior changes
        frame = np.ones(dst.shape[:2], bool)
        frame[lty + 1:lty + H - 1, ltx + 1:ltx + W - 1] = False
        assert np.array_equal(body[frame], dst[frame])
        for c in cases.channels(name, n):
            kind = "u64_fast" if q16 else "u64_half"          # (nothing composed: the twin without formats)
            u = mb.solve(name, "clone", c, n, kind)[1:-1, 1:-1]
            d_gpu = float(decided_np.crossed_bound(u, body[lty + 1:lty + H - 1, ltx + 1:ltx + W - 1, c]).max())
            d_u32, e_fmt, bound = mb.yardstick(name, "clone", c, n), mb.e_fmt(name, c, n, q16), mb.format_bound(name, c, n, q16)
            print("%s n=%d channel %d: bytes imply |u - spec| >= %.3g; D(u32) %.3g E_fmt %.3g bound %.3g" % (name, n, c, d_gpu, d_u32, e_fmt, bound))
            note("c_bytes", name, n, d_gpu, d_u32, e_fmt, time.time() - t0)
            assert d_gpu <= bound, (name, n, c, d_gpu, bound)


# ---------------------------------------------------------------------------------------------------------------- (d) default tables
@pytest.mark.parametrize("name", cases.NAMES)
def test_clone_bytes_on_the_default_tables(inst, name):
    from seamlesscloneoptimization_amd import capi
    t0 = time.time()
    W, H = cases.shape(name)
    dst, patch, mask, cx, cy = cases.clone_inputs(name)[:5]
    ltx, lty = cases.clone_inputs(name)[7]
    composed = bool(capi.cycle0_plan(W, H, 2)["composes"])
    kind = "u64_fast" if composed else "u64_half"
    for n in (2, 3):
        c = cases.channels(name, n)[0]
        if n == 2:
            fixed_budget(inst, n)
        else:           # the default stop rule on a budget of three
            d = inst.default_opts()
            inst.set_solver(**dict({f[0]: getattr(d, f[0]) for f in d._fields_}, method=capi.SC_METHOD_MULTIGRID, max_sweeps=n))
        body = dst.copy()
        rc = inst.run(patch, body, mask, cx, cy, allow_not_converged=True)
        info = inst.info()
        assert (info.W, info.H, info.sweeps, info.field_retry, info.method) == (W, H, n, 0, capi.SC_METHOD_MULTIGRID)
        accepted = rc == 0
        assert rc in (0, capi.SC_ERR_NOT_CONVERGED) and (n == 3 or not accepted)
        # what ran: every kind of early correction that adds one gives the same launches
        rows, sweeps, launches, code = capi.fused_schedule([0 if accepted else 1], budget=n, q16=int(composed), composed=int(composed), early_kind=1)
        assert (sweeps, launches, code) == (info.sweeps, info.sweep_launches, rc)
        assert any(r["bands"] for r in rows) and any(r["lm"] and r["out_bytes"] for r in rows) and any(r["q16_out"] for r in rows) == composed
        # accepted: the judged launch's bytes carry the correction of the iterate before; refused: the post-process adds the last iterate's
        corr, allow = mb.table_correction(name, c, n - 1 if accepted else n, kind)
        u = mb.solve(name, "clone", c, n, kind)[1:-1, 1:-1] + corr
        d_gpu = float(decided_np.crossed_bound(u, body[lty + 1:lty + H - 1, ltx + 1:ltx + W - 1, c]).max())
        d_u32, e_fmt, bound = mb.yardstick(name, "clone", c, n), mb.e_fmt(name, c, n, composed), mb.format_bound(name, c, n, composed) + allow
        print("%s n=%d channel %d %s: bytes imply |u - spec| >= %.3g; D(u32) %.3g E_fmt %.3g correction %.3g (allowance %.3g) bound %.3g"
              % (name, n, c, "accepted" if accepted else "refused", d_gpu, d_u32, e_fmt, float(np.abs(corr).max()), allow, bound))
        note("d_tables_accepted" if accepted else "d_tables_refused", name, n, d_gpu, d_u32, e_fmt + allow, time.time() - t0)
        assert d_gpu <= bound, (name, n, c, accepted, d_gpu, bound)
