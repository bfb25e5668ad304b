"""The level-0 launcher's one form outside its table (csrc/sc_cycle0.hip): the judged bytes form of a same-size group that writes the
members' interleaved bytes itself, C0_OUT3 = 4096.  No GPU: sc_hip_cycle0_form looks a form up and launches nothing.

It exists for exactly one set of facts -- what the fast path's judged cycle says, plus out_interleaved -- and with out_interleaved
left out every fact set of the recording in tests/golden/cycle0_forms.json answers what it answered before (the same rule as
tests/test_cycle0_forms_host.py, whose descriptor() and two_answers() are used here)."""
import itertools
import json

from seamlesscloneoptimization_amd import capi

import test_cycle0_forms_host as forms

C0_OUT3 = 4096
JUDGED = dict(sweeps=2, prolong=1, composed=1, final_cycle=1, out_bytes=1, f_half=1, l1_half=1)      # TAG 186: the fast path's judged bytes form


def test_the_new_form_is_found_from_exactly_its_facts():
    assert capi.cycle0_form(**JUDGED) == (2, 1, 186)
    assert capi.cycle0_form(out_interleaved=1, **JUDGED) == (2, 1, 186 | C0_OUT3)
    # every other fact set with out_interleaved has no form: one fact flipped or changed at a time, and nothing but the bit
    for k in capi.CYCLE0_FACTS:
        if k == "bands":        # a final cycle takes the pointer or not: the same form (the table's rule)
            assert capi.cycle0_form(out_interleaved=1, bands=1, **JUDGED) == (2, 1, 186 | C0_OUT3)
            continue
        for v in ((1, 3, 4) if k == "sweeps" else (1 - JUDGED.get(k, 0),)):
            assert capi.cycle0_form(out_interleaved=1, **dict(JUDGED, **{k: v})) == -1, (k, v)
    assert capi.cycle0_form(out_interleaved=1) == -1


def test_the_table_does_not_hold_it():
    table = capi.cycle0_forms()
    assert len(table) == 65 and all(not TAG & C0_OUT3 for _, _, TAG in table)


def test_every_recorded_fact_set_answers_as_before_without_the_bit():
    with open(forms.GOLDEN) as f:
        g = json.load(f)
    n = 0
    for name, t in g.items():
        launched = {tuple(row[:-1]): tuple(row[-1]) for row in t["launches"]}
        for x in itertools.product(*[range(k) for k in t["domain"]]):
            r = dict(zip(t["fields"], x))
            facts = forms.descriptor(name, r)
            if facts is None or forms.two_answers(name, r) is not None:
                continue        # (the rows one descriptor cannot say both ways: tests/test_cycle0_forms_host.py)
            want = launched.get(x, -1)
            assert capi.cycle0_form(out_interleaved=0, **facts) == want, (name, r)
            # ... and with the bit every one of them but the new form's own facts launches nothing
            got3 = capi.cycle0_form(out_interleaved=1, **facts)
            is_judged = all(facts.get(k, 0) == JUDGED.get(k, 0) for k in capi.CYCLE0_FACTS if k != "bands")
            assert got3 == ((2, 1, 186 | C0_OUT3) if is_judged else -1), (name, r, got3)
            n += 1
    assert n > 2000      # (the recording's rows less those named by two_answers and the twin launcher's non-launches)
