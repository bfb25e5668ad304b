"""The schedule of a fused multigrid solve's level-0 launches (csrc/sc_multigrid.cpp: fused_next, which mg_solve_fused asks for every
launch) against a recording of the loop it replaced.  No GPU: sc_hip_fused_schedule walks the schedule and launches nothing.

tests/golden/fused_schedule.json is that recording: mg_solve_fused as it stood when the schedule was still written out inside it, its
launchers replaced by notes and the read-back behind each judged launch by the verdict wanted, run over the product of "inputs"
(see its "about").  Every run must give its recorded launches row for row, and sc_run_info's sweeps, sweep_launches and the code."""
import base64
import functools
import itertools
import json
import lzma
import os

import numpy as np
import pytest

from seamlesscloneoptimization_amd import capi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fused_schedule.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        g = json.load(f)
    g["index"] = np.frombuffer(lzma.decompress(base64.b64decode(g["index_lzma_b64"])), dtype="<u2")
    return g


@functools.lru_cache(maxsize=None)
def instantiated(form):
    return capi.cycle0_form(**dict(form)) != -1


def facts_of(x, t):
    """The facts the driver hands the schedule for input x of the recording (q16, composed and out_wanted as the recorded driver computed
    them: transcript t), and the initial field's format, which the recording ties to the 16-bit field's eligibility."""
    return dict(pre=x["pre"], post=x["post"], budget=x["budget"], tol=x["tol"], out_wanted=t[2], q16=t[0], u_half=x["q16_eligible"], composed=t[1],
                separate_restrict=x["legacy_separate_restrict"], early_kind=x["early_kind"], bytes_form=x["bytes_form"], small=x["small"])


def recorded_view(rows, facts):
    """The schedule's rows as the recording saw them: what a stubbed launcher and the stubs around it can note."""
    out, nodes = [], 0
    for r in rows:
        launched = not (r["out_bytes"] and not facts["bytes_form"])
        out.append([r["sweeps"], r["prolong"], r["final_cycle"], r["out_bytes"], r["u_half"], r["q16_in"], r["q16_out"], r["composed"], r["bands"],
                    int(r["lm"] and nodes in (1, 2)),                   # lm.CN is set where a node correction was computed
                    r["nodes"] if r["nodes"] in (1, 2) else 0,
                    int(r["judged"] and launched),                      # nothing to read back behind a form that does not exist
                    r["coarse_first"],
                    int(r["sat"] and facts["q16"]),                     # the word exists in a 16-bit solve only
                    r["bands_asked"], r["early_asked"],
                    int(r["lm"] and nodes == 2),                        # the main stream waits for the second one's correction
                    (r["cycle"] + 1) & 1 if r["prolong"] else -1])      # this cycle's half of the maxima
        if r["nodes"]:
            nodes = r["nodes"]
    return out


def test_every_recorded_run_gives_its_transcript(golden):
    names = [n for n, _ in golden["inputs"]]
    domain = [v for _, v in golden["inputs"]]
    index, transcripts, rows = golden["index"], golden["transcripts"], golden["rows"]
    assert len(index) == np.prod([len(v) for v in domain]) == 516096 and len(names) == 13 and names[-1] == "verdicts"
    assert int(index.max()) == len(transcripts) - 1
    seen = {}
    for i, values in enumerate(itertools.product(*domain)):
        x = dict(zip(names, values))
        t = transcripts[index[i]]
        facts = facts_of(x, t)
        key = (tuple(facts.values()), tuple(x["verdicts"]))
        if key in seen:                 # the same facts and verdicts: the recording must have given the same transcript
            assert seen[key] == index[i], (x, facts)
            continue
        seen[key] = index[i]
        got, sweeps, launches, code = capi.fused_schedule(x["verdicts"], **facts)
        assert (sweeps, launches, code) == tuple(t[3:6]), (x, facts)
        assert recorded_view(got, facts) == [rows[k] for k in t[6]], (x, facts)
        for r in got:                   # every launch names an instantiated form (the 16-bit field needs float16 fields around it)
            form = dict(sweeps=r["sweeps"], prolong=r["prolong"], final_cycle=r["final_cycle"], out_bytes=r["out_bytes"], u_half=r["u_half"],
                        q16_in=r["q16_in"], q16_out=r["q16_out"], composed=r["composed"], bands=int(r["bands"] != 0))
            halves = [(1, 1)] if facts["q16"] else [(0, 0), (1, 0)] + ([(1, 1)] if facts["composed"] and not facts["tol"] else [])
            if not (r["out_bytes"] and not facts["bytes_form"]):
                assert any(instantiated(tuple(sorted(dict(form, f_half=fh, l1_half=lh).items()))) for fh, lh in halves), (x, r)
    assert len(seen) > 20000


def test_default_solve_judges_its_third_cycle():
    rows, sweeps, launches, code = capi.fused_schedule()
    assert [r["kind"] for r in rows] == [1, 2, 3, 4] and (sweeps, launches, code) == (3, 4, 0)
    assert [r["judged"] for r in rows] == [0, 0, 0, 1] and rows[3]["cycle"] == 2
    rows, sweeps, launches, code = capi.fused_schedule([1, 1, 0])      # the bytes refused, the field form refused, the fourth cycle accepted
    assert [r["kind"] for r in rows] == [1, 2, 3, 4, 5, 6, 5] and (sweeps, launches, code) == (4, 6, 0)
    assert [r["coarse_first"] for r in rows] == [0, 1, 1, 1, 0, 0, 1]


def test_timing_twins_are_steps_of_the_default_schedule():
    """sc_hip_time_cycle0_form's four launches (tests/test_cycle0_forms_host.py: descriptor(), the fast path's twins) are the default
    schedule's steps with `timing` set and the fast path's formats around them."""
    rows = capi.fused_schedule()[0]
    fast = dict(timing=1, f_half=1, l1_half=1)
    twins = {0: dict(fast, sweeps=4, prolong=1, composed=1, q16_in=1, q16_out=1),
             1: dict(fast, sweeps=4, prolong=1, composed=1, q16_in=1, bands=1),
             2: dict(fast, sweeps=2, prolong=1, composed=1, final_cycle=1, out_bytes=1),
             3: dict(fast, sweeps=2, u_half=1, q16_out=1)}
    step_of_form = {0: 1, 1: 2, 2: 3, 3: 0}
    for form, want in twins.items():
        r = rows[step_of_form[form]]
        got = dict(fast, **{k: r[k] for k in ("sweeps", "prolong", "final_cycle", "out_bytes", "u_half", "q16_in", "q16_out", "composed")}, bands=int(r["bands"] != 0))
        assert {k: v for k, v in got.items() if v} == want, form
        assert capi.cycle0_form(**got) != -1
