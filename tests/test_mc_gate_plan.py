"""CPU: qcx_mc_gate_plan (include/qcx_plan.h), the launch rule of qcx_mc_one_qubit_gate / qcx_mc_two_qubit_gate on its own -- the
library launches from this very function.  The plan's work numbering is emulated in numpy (mc_gate_ref.visited) and must visit
exactly the definition's index set, each index once; its launch geometry is audited at widths no test allocates.  No GPU needed."""
import numpy as np
import pytest

import mc_gate_ref as mc

BAD_ARGUMENTS, BAD_QUBIT = 2, 6
LAUNCH_BOUND = 64          # __launch_bounds__ of every K17 kernel


def squeezed_of(pl):
    s = 0
    for k in range(pl.nruns):
        assert pl.run_len[k] >= 1 and (k == 0 or pl.run_pos[k] > pl.run_pos[k - 1] + pl.run_len[k - 1]), "ascending, merged runs"
        s |= ((1 << pl.run_len[k]) - 1) << pl.run_pos[k]
    return s


def check_numbering(qc, n, targets, mask, values):
    st, pl = qc.mc_gate_plan(n, mask, values, targets)
    assert st == 0, (n, targets, mask, values)
    what = (n, targets, hex(mask), hex(values), pl.kernel)
    idx = np.arange(1 << n, dtype=np.uint64)
    want = idx[(idx & np.uint64(mask)) == np.uint64(values)]
    i, hit, got = mc.visited(pl, targets)
    assert np.array_equal(got, want), what                        # (sorted and equal to a set without repeats: each index once)
    sq = squeezed_of(pl)
    assert int(pl.count) == 1 << (n - bin(sq).count("1")), what
    assert pl.or_const == values & sq and not pl.low_mask & sq and pl.low_mask == mask & ~sq and pl.low_values == values & ~sq, what
    tsq = sum(1 << q for q in targets if sq >> q & 1)
    assert not np.any(i & np.uint64(tsq)), "a work item is the base of its pair / quad"
    lo, hi = min(targets), max(targets)
    p = np.arange(int(pl.count), dtype=np.uint64)
    runs = [(int(pl.run_pos[k]), int(pl.run_len[k])) for k in range(pl.nruns)]
    shuffled = [q for q in targets if not sq >> q & 1]
    if shuffled:
        # the partner of a shuffled target: the lane `shfl` away, inside the same wave, one target bit away in the index
        assert pl.form in (qc._lib.MC_LINE_SHFL, qc._lib.MC_LINES2) and int(pl.count) % 64 == 0 and pl.low_mask < 8, what
        masks = [1 << lo] if len(targets) == 1 else ([pl.shfl_lo, pl.shfl_hi] if len(shuffled) == 2 else [pl.shfl_lo])
        for q, m in zip(sorted(shuffled), masks):
            assert 0 < m < 64 and np.array_equal(mc.deposit(p ^ np.uint64(m), runs) | np.uint64(pl.or_const), i ^ np.uint64(1 << q)), what
        assert pl.ns == (len(shuffled) if len(targets) == 2 else 0), what
    if pl.low_mask:
        assert pl.store_all == (1 if pl.low_mask & 3 else 0), what
    # the lane's predicate and a shuffled target's bit come from the lane number alone (the kernels form them once)
    lane_bits = pl.low_mask | sum(1 << q for q in shuffled)
    if int(pl.count) >= 64:
        assert np.array_equal(i & np.uint64(lane_bits), np.tile(i[:64] & np.uint64(lane_bits), int(pl.count) // 64)), what
    assert not pl.nt or not sq & 7, "nontemporal accesses only where a wave covers whole lines"
    return pl


@pytest.mark.parametrize("n", [4, 5, 6, 7])
def test_numbering_small_registers_every_form(qc, n):
    """3. every (mask, values, targets) at n = 4 .. 7"""
    for t, m, v in mc.forms1(n) + mc.forms2(n):
        pl = check_numbering(qc, n, t, m, v)
        assert pl.form == (qc._lib.MC_PAIR if len(t) == 1 else qc._lib.MC_QUAD), "below n = 9: the pair or quad form"


@pytest.mark.parametrize("n", [9, 10, 13])
def test_numbering_seeded_draws(qc, n):
    """3. 300 stratified draws each at n = 9, 10 and 13; every form must turn up"""
    seen = set()
    for t, m, v in mc.draws(n, 300, 9000 + n):
        pl = check_numbering(qc, n, t, m, v)
        seen.add((pl.form, pl.ns))
    L = qc._lib
    assert seen >= {(L.MC_PAIR, 0), (L.MC_LINE_PAIR, 0), (L.MC_LINE_SHFL, 0), (L.MC_QUAD, 0), (L.MC_LINES2, 0), (L.MC_LINES2, 1), (L.MC_LINES2, 2)}, seen


def test_numbering_under_the_knobs(qc):
    """ph_lines = 0: the pair / quad form for everything; the numbering holds under every knob the plan reads"""
    keys = ("ph_lines", "ph_nt", "u2_variant", "u2_nt")
    defaults = {k: qc.lib().qcx_tune_get(k.encode()) for k in keys}
    try:
        for knobs in (dict(ph_lines=0), dict(ph_nt=0), dict(u2_variant=1), dict(u2_nt=0)):
            qc.tune(**defaults); qc.tune(**knobs)
            for t, m, v in mc.draws(10, 60, 77):
                pl = check_numbering(qc, 10, t, m, v)
                if "ph_lines" in knobs or ("u2_variant" in knobs and len(t) == 2):
                    assert pl.form in (qc._lib.MC_PAIR, qc._lib.MC_QUAD) and pl.low_mask == 0
                if ("ph_nt" in knobs and len(t) == 1) or ("u2_nt" in knobs and len(t) == 2):
                    assert pl.nt == 0                             # (K12's knob for one target, K13's for two)
                elif "ph_nt" in knobs or "u2_nt" in knobs:
                    assert pl.nt == (0 if squeezed_of(pl) & 7 else 1), "the other knob does not reach this gate"
    finally:
        qc.tune(**defaults)


def wide_cases(n):
    top = [b for b in (31, 32) if b < n] or [n - 2]            # bits 31 and 32 where the register has them
    tsets = [(n - 1,), (top[0],), (0,), (3,), (n - 1, 0), (top[-1], top[-1] - 2), (n - 1, n - 2), (2, 1), (5, n - 1), (top[-1], 7)]
    for t in tsets:
        free = [q for q in range(n) if q not in t]
        hi_first = sorted(free, key=lambda q: -q)
        for k in (0, 1, 16, n - len(t)):
            for cs in {tuple(hi_first[:k]), tuple(free[:k]), tuple((hi_first[:(k + 1) // 2] + free[:k // 2]))}:
                if len(set(cs)) != k:
                    continue
                mask = sum(1 << c for c in cs)
                for vals in {mask, 0, mask & 0x5555555555555555}:
                    yield t, mask, vals


@pytest.mark.parametrize("n", [30, 31, 32, 33, 34])
def test_geometry_at_widths_nobody_allocates(qc, n):
    """4. targets and controls at bits 31, 32 and n - 1; k = 0, 1, 16 and every other qubit"""
    L = qc._lib
    cases = 0
    for t, mask, vals in wide_cases(n):
        st, pl = qc.mc_gate_plan(n, mask, vals, t)
        what = (n, t, hex(mask), hex(vals), pl.kernel)
        assert st == 0, what
        cases += 1
        assert 1 <= pl.grid <= 2 ** 31 - 1 and pl.block == 64 <= LAUNCH_BOUND and pl.items_per_thread == 1, what
        assert pl.grid * pl.block < 2 ** 32, "HIP's limit on the threads of a launch"
        capped = pl.grid == (2 ** 32 - 1) // 64                   # (the kernels stride: a capped grid loops)
        assert capped or pl.grid * pl.block * pl.items_per_thread >= pl.count, what
        assert capped or (pl.grid - 1) * pl.block < pl.count, "no idle workgroup"
        if pl.form == L.MC_LINE_SHFL or (pl.form == L.MC_LINES2 and pl.ns):
            assert pl.count % 64 == 0, what
        sq = squeezed_of(pl)
        high, low = mask & ~7, mask & 7
        lines = pl.form in (L.MC_LINE_PAIR, L.MC_LINE_SHFL, L.MC_LINES2)
        in_regs = [q for q in t if sq >> q & 1]
        if lines:
            assert sq == high | sum(1 << q for q in in_regs) and (pl.low_mask, pl.low_values) == (low, vals & 7), what
            assert pl.count == 2 ** (n - len(in_regs) - bin(high).count("1")), what
            assert min(t) < 3 or low, "a line form only with a target or a control inside a line"
        else:
            assert sq == mask | sum(1 << q for q in t) and pl.low_mask == 0 and pl.count == 2 ** (n - len(t) - bin(mask).count("1")), what
            assert (min(t) >= 3 and not low) or pl.count < 64, "the pair / quad form: nothing inside a line, or fewer than 64 work items"
        assert pl.or_const == vals & sq, what
        # the ends of the numbering in 64-bit arithmetic: work item 0 and the last one
        runs = [(int(pl.run_pos[k]), int(pl.run_len[k])) for k in range(pl.nruns)]
        ends = mc.deposit(np.array([0, pl.count - 1], dtype=np.uint64), runs) | np.uint64(pl.or_const)
        assert int(ends[0]) == vals & sq and int(ends[1]) == ((2 ** n - 1) & ~sq) | (vals & sq), what
        assert (pl.glog, pl.slog) == (0, 0) or (pl.grid == 1 << pl.glog and pl.grid * 64 == pl.count and pl.slog <= pl.glog), what
    assert cases > 100


def test_the_work_count_of_2_to_the_32(qc):
    """n = 33, one target in registers, no control: 2^32 pairs on a capped grid; target and control at bit 32"""
    st, pl = qc.mc_gate_plan(33, 0, 0, (32,))
    assert st == 0 and pl.count == 2 ** 32 and pl.grid == (2 ** 32 - 1) // 64 and (pl.glog, pl.slog) == (0, 0)
    st, pl = qc.mc_gate_plan(33, 1 << 32, 0, (3,))
    assert st == 0 and pl.count == 2 ** 31 and pl.or_const == 0 and (pl.run_pos[0], pl.run_len[0], pl.run_pos[1], pl.run_len[1]) == (3, 1, 32, 1)


def test_refusals(qc):
    """5. the refusals of include/qcx.h by return code, in their order"""
    lib = qc.lib()
    plan = qc.mc_gate_plan
    pl = qc._lib.McPlan()
    assert lib.qcx_mc_gate_plan(10, 0, 0, 1, 0, 0, None) == BAD_ARGUMENTS
    assert lib.qcx_mc_gate_plan(10, 0, 0, 3, 0, 1, qc._lib.C.byref(pl)) == BAD_ARGUMENTS
    assert lib.qcx_mc_gate_plan(10, 0, 0, 0, 0, 1, qc._lib.C.byref(pl)) == BAD_ARGUMENTS
    assert plan(0, 0, 0, (0,))[0] == BAD_ARGUMENTS
    assert plan(10, 0b0110, 0b1000, (0,))[0] == BAD_ARGUMENTS and "ctrl_values" in lib.qcx_last_error().decode()
    assert plan(10, 0b0110, 0b0111, (5,))[0] == BAD_ARGUMENTS
    assert plan(10, 1 << 10, 1 << 11, (10,))[0] == BAD_ARGUMENTS, "values outside the mask come before the qubits"
    assert plan(10, 0, 0, (10,))[0] == BAD_QUBIT
    assert plan(10, 0, 0, (3, 10))[0] == BAD_QUBIT
    assert plan(10, 0, 0, (3, 3))[0] == BAD_QUBIT
    assert plan(10, 1 << 10, 0, (3,))[0] == BAD_QUBIT
    assert plan(10, 1 << 63, 0, (3,))[0] == BAD_QUBIT
    assert plan(10, 1 << 3, 1 << 3, (3,))[0] == BAD_QUBIT
    assert plan(10, 1 << 4, 0, (3, 4))[0] == BAD_QUBIT
    assert plan(1, 0, 0, (0,))[0] == 0 and plan(2, 0, 0, (1, 0))[0] == 0 and plan(10, 0x3F6, 0x124, (3, 0))[0] == 0
