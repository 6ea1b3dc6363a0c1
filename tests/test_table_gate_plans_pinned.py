"""CPU: the launch plans of the masked and the table gates (qcx_mc_gate_plan, qcx_diagonal_plan, qcx_permutation_plan,
qcx_multi_gate_plan; include/qcx_plan.h) are those of commit 14ef617, the one before their argument checks, the runs of a mask
and the tile geometry were stated once.  tests/table_gate_plan_cases.py enumerates the calls and spells each answer as a line;
tests/golden/table_gate_plan_digests.json holds what that commit's own build answered: one SHA-256 per entry point and knob set,
the case counts and a sample of lines.  The coverage the enumeration claims is asserted on the lines themselves."""
import json
import os
import re

import pytest

import table_gate_plan_cases as tgc

GOLDEN = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "table_gate_plan_digests.json")))


@pytest.fixture(scope="module")
def answers(qc):
    """(entry, knob set) -> its lines, computed once; the knobs are put back after each computation"""
    cache = {}

    def get(entry, name):
        if (entry, name) not in cache:
            old = {k: qc.lib().qcx_tune_get(k.encode()) for k in tgc.KNOBS}
            qc.tune(**{k: tgc.KNOB_SETS[entry][name].get(k, v) for k, v in old.items()})
            try:
                cache[entry, name] = tgc.answer_lines(qc, entry)
            finally:
                qc.tune(**old)
        return cache[entry, name]
    return get


def test_the_fixture_is_the_enumerations():
    assert set(GOLDEN["digests"]) == set(tgc.ENTRIES) and GOLDEN["commit"] == "14ef617"
    for e in tgc.ENTRIES:
        assert set(GOLDEN["digests"][e]) == set(tgc.KNOB_SETS[e]) and "default" in tgc.KNOB_SETS[e]
        assert GOLDEN["cases"][e] == len(tgc.cases(e))
        assert {s["knobs"] for s in GOLDEN["sample"] if s["entry"] == e} == set(tgc.KNOB_SETS[e])
    # every knob the planners read is moved by a set of its entry point
    moved = {e: {k for s in tgc.KNOB_SETS[e].values() for k in s} for e in tgc.ENTRIES}
    assert moved["mc"] == {"ph_lines", "ph_nt", "u2_nt", "u2_variant", "ph_streams_log2", "u2_streams_log2"}
    assert moved["diagonal"] == {"diag_lds", "diag_grid_cap"}
    assert moved["permutation"] == {"perm_tile_log2", "perm_grid_cap", "perm_store_all", "perm_nt"}
    assert moved["multi"] == {"multi_grid_cap", "multi_store_all", "multi_nt"}


def test_the_enumeration_reaches_what_it_claims():
    """on the arguments alone: the exhaustive part, the widths and the special qubits of the seeded part"""
    for e in ("mc", "multi"):
        cs = tgc.cases(e)
        for n in range(1, 7):
            ks = (1, 2) if e == "mc" else (1, 2, 3, 4, 5)
            want = sum(_perms(n, k) * 3 ** (n - k) for k in ks if k <= n)
            assert sum(1 for c in cs if c[0] == n and c[-1] != tgc.NULL) >= want, (e, n)
    for e in tgc.ENTRIES:
        ns = {c[0] for c in tgc.cases(e)}
        assert {0, 41, 9, 10, 12, 13, 14, 30, 33, 34, 40} <= ns, e
    for e, at in (("mc", 1), ("permutation", 1), ("multi", 1)):
        for n in (33, 34, 40):
            masks = [c[at] for c in tgc.cases(e) if c[0] == n]
            for q in (31, 32, n - 1):
                assert any((m >> q) & 1 for m in masks), (e, n, q)
    for n in (33, 34, 40):
        for q in (31, 32, n - 1):
            assert any(c[0] == n and c[3] == 1 and c[4] == q for c in tgc.cases("mc")), (n, q)
            assert any(c[0] == n and c[-1] not in (tgc.NULL, tgc.NO_TARGETS) and q in c[3] for c in tgc.cases("multi")), (n, q)
            assert any(c[0] == n and c[3] <= q < c[3] + c[4] for c in tgc.cases("permutation")), (n, q)
            assert any(c[0] == n and c[1] <= q < c[1] + c[2] for c in tgc.cases("diagonal")), (n, q)


def _perms(n, k):
    out = 1
    for j in range(k):
        out *= n - j
    return out


@pytest.mark.parametrize("entry,name", [(e, s) for e in tgc.ENTRIES for s in tgc.KNOB_SETS[e]])
def test_plans_are_the_parents(answers, entry, name):
    """every line of one entry point under one knob set: digest and sample lines"""
    lines = answers(entry, name)
    have = set(lines)
    for s in GOLDEN["sample"]:
        if s["entry"] == entry and s["knobs"] == name:
            assert s["line"] in have, s["line"]
    assert tgc.digest(lines) == GOLDEN["digests"][entry][name]


def test_the_lines_cover_the_planners(answers):
    """every form, every kernel name the planners can spell, every refusal status of every entry point; 10^5 lines or more"""
    total = 0
    for e in tgc.ENTRIES:
        forms, kernels, refused = set(), set(), set()
        for name in tgc.KNOB_SETS[e]:
            lines = answers(e, name)
            total += len(lines)
            for ln in lines:
                tail = ln.split(" | ", 1)[1]
                if tail.startswith("refused "):
                    refused.add(int(re.match(r"refused (\d+)", tail).group(1)))
                else:
                    forms.add(int(re.search(r" form=(\d+) ", tail).group(1)))
                    kernels.add(tail[tail.index(" kernel=") + 8:])
        assert forms == tgc.FORMS[e], e
        assert kernels == tgc.KERNELS[e], e
        assert refused == tgc.REFUSALS[e], e
    assert total >= 10 ** 5


def test_refusal_lines_do_not_depend_on_call_order(qc):
    """a refusal that writes no text leaves the previous one standing: its line carries none, whatever was refused before it"""
    c = tgc.Caller(qc, "permutation")
    quiet, loud = (12, 0, 0, 13, 0), (12, 1, 3, 4, 1)
    a = [c.line(quiet), c.line(loud), c.line(quiet), c.line(quiet)]
    assert a[0] == a[2] == a[3] == "permutation 12 0 0 13 0 | refused 6"
    assert a[1] == "permutation 12 1 3 4 1 | refused 2: permutation_gate: ctrl_values 0x3 has bits outside ctrl_mask 0x1"
