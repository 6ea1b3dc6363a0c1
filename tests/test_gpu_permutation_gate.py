"""GPU: a permutation of a qubit range's basis states from a table, under any controls (qcx_permutation_gate, K19).  Every state
must be, bit for bit, what tests/permutation_ref.py defines on whatever the register held: every range and control placement
of small registers, the edges of the tile rule (the whole-wave threshold of the mc plan, one partial tile, exactly one tile,
several tiles, tiles that share lines, squeezed controls below and above the range, predicates on the element and on the
tile), the existing kernels it generalises (new against old), the observers behind it, every lazy form the library keeps a
state in, registers that hold Inf, NaN and -0, the identity table, and every refusal in its order."""
import ctypes as C

import numpy as np
import pytest

import permutation_ref as pr
import sequence_replay as sr
import tolerance_twin as tt
from bitwise import bits, same, same_with_nans

pytestmark = pytest.mark.gpu

BAD_ARGUMENTS, BAD_QUBIT, UNSUPPORTED = 2, 6, 7
SEED = 77
_STATES = {}


def filled(ob, n, seed=SEED):
    """what reg.fill_random(seed) leaves on n qubits, computed once and never changed"""
    if (n, seed) not in _STATES:
        a = ob.fill_random(n, seed)
        a.setflags(write=False)
        _STATES[(n, seed)] = a
    return _STATES[(n, seed)]


def masks_of(controls):
    """{qubit: value} -> (mask, values)"""
    return sum(1 << c for c in controls), sum(1 << c for c, v in controls.items() if v)


def run(qc, reg, first, num, perm, controls):
    cm, cv = masks_of(controls)
    qc.permutation_gate(first, num, perm, reg, controls=cm, values=cv)
    return cm, cv


def moving_table(rs, num):
    """a random table that is not the identity (num >= 1)"""
    while True:
        perm = rs.permutation(1 << num)
        if not np.array_equal(perm, np.arange(1 << num)):
            return perm


def check(qc, ob, reg, n, first, num, perm, controls, what=""):
    """fill_random, the call, a read-back against the definition; the stats against the plan and the table"""
    a = filled(ob, n)
    reg.fill_random(SEED)
    cm, cv = run(qc, reg, first, num, perm, controls)
    got = reg.read()
    same(got, pr.apply(a, n, first, num, perm, cm, cv), f"{what} n={n} first={first} num={num} controls={controls}")
    st, pl = qc.permutation_plan(n, cm, cv, first, num)
    assert st == 0 and reg.permutation_stats() == (pl.form, int(np.count_nonzero(np.asarray(perm) != np.arange(1 << num))))
    return got


# ---- small registers: every range, every single control, pairs of mixed polarity -----------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])
def test_small_registers_every_range_and_control(qc, ob, n):
    rs = np.random.RandomState(100 + n)
    with qc.Register(n, 0) as reg:
        for first in range(n + 1):
            for num in range(min(n, 5, n - first) + 1):
                free = [c for c in range(n) if not first <= c < first + num]
                sets = [{}] + [{c: v} for c in free for v in (1, 0)]
                sets += [{a: 1, b: 0} for a in free for b in free if a != b]
                for controls in sets:
                    for _ in range(3):
                        check(qc, ob, reg, n, first, num, rs.permutation(1 << num), controls)


# ---- the edges where the kernel can go wrong ---------------------------------------------------------------------------------------

EDGES = {
    9: [(0, 9), (3, 6)],                        # the whole-wave threshold of the mc plan
    11: [(0, 11), (5, 6)],                      # one partial tile
    12: [(0, 12)],                              # exactly one tile
    13: [(0, 12), (1, 12), (4, 9), (10, 3)],    # the first register with several tiles; (1, 12): tiles that share lines
    14: [(2, 12), (0, 1), (13, 1), (5, 4)],     # several tiles
}


def edge_controls(n, first, num):
    sets = [{}, {0: 1}, {2: 1}, {3: 1}, {n - 1: 1}, {first - 1: 1, n - 1: 0}]
    if (n, first, num) == (14, 5, 4):
        sets += [{4: 1}, {3: 0, 4: 1}]                                       # a control between bit 3 and first
    out = []
    for s in sets:
        if all(0 <= c < n and not first <= c < first + num for c in s) and s not in out:
            out.append(s)
    return out


@pytest.mark.parametrize("n,first,num", [(n, f, k) for n, shapes in EDGES.items() for f, k in shapes])
def test_edges_of_the_tile_rule(qc, ob, n, first, num):
    rs = np.random.RandomState(1000 * n + 10 * first + num)
    with qc.Register(n, 0) as reg:
        for controls in edge_controls(n, first, num):
            perm = moving_table(rs, num)
            got = check(qc, ob, reg, n, first, num, perm, controls)
            assert not np.array_equal(bits(got), bits(filled(ob, n)))
            # the table's inverse under the same controls restores the bits
            run(qc, reg, first, num, pr.inverse(perm, num), controls)
            same(reg.read(), filled(ob, n), f"inverse n={n} first={first} num={num} controls={controls}")


@pytest.mark.parametrize("knobs", [dict(perm_grid_cap=3), dict(perm_grid_cap=0), dict(perm_store_all=0), dict(perm_nt=1), dict(perm_nt=1, perm_store_all=0),
                                   dict(perm_tile_log2=8), dict(perm_tile_log2=10, perm_grid_cap=5), dict(perm_tile_log2=0)],
                         ids=["cap3", "nocap", "no-store_all", "nt", "nt-no-store_all", "tile8", "tile10-cap5", "tile0"])
def test_knobs_change_no_bit(qc, ob, knobs):
    """a grid that does not divide the units (a workgroup walks several tiles), one tile each, the two store policies, and
    tiles of other sizes than the default's"""
    keep = {k: qc.lib().qcx_tune_get(k.encode()) for k in knobs}
    rs = np.random.RandomState(4)
    try:
        qc.tune(**knobs)
        with qc.Register(14, 0) as reg:
            for first, num, controls in [(2, 9, {}), (3, 9, {0: 1}), (4, 3, {1: 0, 13: 1}), (1, 12, {0: 1}), (0, 2, {2: 0}), (5, 4, {3: 0, 4: 1})]:
                check(qc, ob, reg, 14, first, num, rs.permutation(1 << num), controls, str(knobs))
    finally:
        qc.tune(**keep)


def test_more_than_one_tile_per_workgroup(qc, ob):
    """n = 24 has many more tiles than the 2048 workgroups of the default cap; the range at the top, a squeezed control in mid-register"""
    n = 24
    rs = np.random.RandomState(5)
    st, pl = qc.permutation_plan(n, 0, 0, 20, 4)
    assert st == 0 and pl.units >= 2 * pl.grid and pl.grid == 2048
    with qc.Register(n, 0) as reg:
        check(qc, ob, reg, n, 20, 4, rs.permutation(16), {})
        check(qc, ob, reg, n, 7, 5, rs.permutation(32), {15: 0, 1: 1})


# ---- new against old ------------------------------------------------------------------------------------------------------------

def test_against_the_mc_gates(qc, ob):
    n = 13
    Xm = np.array([[0, 1], [1, 0]], dtype=complex)
    SWAP = np.eye(4, dtype=complex)[[0, 2, 1, 3]]
    with qc.Register(n, 0) as reg, qc.Register(n, 0) as twin:
        def both(new, old, what):
            reg.fill_random(SEED); twin.fill_random(SEED)
            new(reg); old(twin)
            got = reg.read()
            assert np.array_equal(bits(got), bits(twin.read())), what
            assert not np.array_equal(bits(got), bits(filled(ob, n))), what
        for q, controls in [(0, {}), (12, {}), (5, {}), (1, {7: 1}), (9, {0: 1}), (3, {12: 0}), (6, {2: 1, 11: 1}), (0, {1: 1, 2: 0}), (12, {3: 1, 4: 1, 5: 0})]:
            cm, cv = masks_of(controls)                                      # X, CNOT, Toffoli and beyond
            both(lambda r: qc.permutation_gate(q, 1, [1, 0], r, controls=cm, values=cv), lambda r: qc.mc_one_qubit_gate(cm, q, Xm, r, values=cv), ("X", q, controls))
        for q, controls in [(0, {}), (11, {}), (2, {}), (4, {9: 1}), (7, {0: 1}), (0, {12: 0}), (10, {1: 1, 6: 0})]:
            cm, cv = masks_of(controls)                                      # SWAP, Fredkin
            both(lambda r: qc.permutation_gate(q, 2, [0, 2, 1, 3], r, controls=cm, values=cv),
                 lambda r: qc.mc_two_qubit_gate(cm, q, q + 1, SWAP, r, values=cv), ("SWAP", q, controls))


@pytest.mark.parametrize("Cn,a,M", [(15, 7, 4), (21, 2, 5)])
def test_against_c_amodc_gate(qc, ob, Cn, a, M):
    n = 13
    with qc.Register(n - M, M) as reg, qc.Register(n - M, M) as twin:
        for ctl in (M, 8, n - 1):
            reg.fill_random(SEED); twin.fill_random(SEED)
            qc.permutation_gate(0, M, qc.modmul_table(a, Cn, M), reg, controls=[ctl])
            qc.c_amodc_gate(Cn, a, ctl, twin)
            got = reg.read()
            assert np.array_equal(bits(got), bits(twin.read())), (Cn, a, M, ctl)
            assert not np.array_equal(bits(got), bits(filled(ob, n)))


# ---- observers behind it -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("controls", [{}, {11: 1}], ids=["plain", "controlled"])
def test_observers_after_a_table(qc, ob, controls):
    n, first, num = 13, 4, 6
    perm = np.random.RandomState(6).permutation(1 << num)
    cm, cv = masks_of(controls)
    with qc.Register(n, 0) as reg:
        reg.fill_random(SEED)
        before = reg.marginal(first, num)
        norm = reg.norm2()
        qc.permutation_gate(first, num, perm, reg, controls=cm, values=cv)
        after = reg.marginal(first, num)
        if not controls:
            want = np.empty_like(before)
            want[perm] = before                                              # outcome k's probability is now perm[k]'s: the same
            same(after, want, "the marginal, permuted")                      # amplitudes, summed by the same tree over the other bits
        # under a control the outcomes mix; either way the observers of the definition's state are the library's own of a
        # register that was WRITTEN that state
        with qc.Register(n, 0) as twin:
            twin.write(pr.apply(filled(ob, n), n, first, num, perm, cm, cv))
            same(after, twin.marginal(first, num), "the marginal")
            assert reg.norm2() == twin.norm2()
        # norm2 sums the same 2^n squares in another order: two pairwise sums of n levels over terms that are themselves a
        # square and a sum (n + 2 roundings each, relative 2^-53 apiece) differ by no more than this
        assert abs(reg.norm2() - norm) <= 2 * (n + 2) * 2.0 ** -53 * norm


# ---- every lazy form -----------------------------------------------------------------------------------------------------------------

LAZY = (4, 6)                                   # the range of every lazy-form test, on n = 13


def lazy_table(seed):
    return np.random.RandomState(seed).permutation(1 << LAZY[1])


def queue_some_gates(qc, ob, reg, want, n):
    for q in (0, 3, n - 1):
        qc.hadamard_gate(q, reg)
        ob.hadamard(want, n, q)
    qc.c_phase_shift_gate(3, n - 1, 0.7, reg)
    ob.cphase(want, n, 3, n - 1, 0.7)


def test_queued_gates_are_flushed_first(qc, ob):
    n = 13
    first, num = LAZY
    with qc.Register(n, 0) as reg:
        reg.set_fusion(1)
        reg.fill_random(8)
        want = ob.fill_random(n, 8)
        queue_some_gates(qc, ob, reg, want, n)
        s0 = reg.fusion_stats()
        reg.flush()
        flush_counts = tt.stats_delta(reg.fusion_stats(), s0)
        assert flush_counts != (0, 0)
        for k, controls in enumerate(({}, {12: 1}, {0: 0})):
            perm = lazy_table(20 + k)
            reg.fill_random(8)
            want = ob.fill_random(n, 8)
            queue_some_gates(qc, ob, reg, want, n)
            before = reg.fusion_stats()
            cm, cv = run(qc, reg, first, num, perm, controls)
            assert tt.stats_delta(reg.fusion_stats(), before) == flush_counts, "the flush's passes, and nothing counted for the table"
            want = pr.apply(want, n, first, num, perm, cm, cv)
            qc.hadamard_gate(1, reg); ob.hadamard(want, n, 1)                # queued behind it
            same(reg.read(), want)


def test_behind_mode_2_work_against_a_twin(qc, ob, tmp_path):
    """tolerance_twin's method: the state S a twin register reads back after the same mode-2 work is the reference; the table
    is exact in mode 2, and the zero pass the tolerance flush owes runs first (the definition turns every -0 of S into +0)"""
    shape = (13, 0, 1, 1)
    n = 13
    first, num = LAZY
    prefix = tt.prefix_ops("iqft", shape)
    twin = tt.run_twin(qc, shape, prefix, tmp_path)
    S = twin[0]
    tt.check_twin(twin, tt.oracle_state(ob, "iqft", shape)[0], prefix, shape)
    for k, controls in enumerate(({}, {12: 1})):
        perm = lazy_table(30 + k)
        with qc.Register(n, 0) as reg:
            before = reg.fusion_stats()
            tt.run_prefix(qc, reg, prefix, tmp_path, {})
            cm, cv = run(qc, reg, first, num, perm, controls)
            assert tt.stats_delta(reg.fusion_stats(), before) == twin[1][:2], "the queued mode-2 work ran, nothing else is counted"
            got = reg.read()
            same(got, pr.apply(S, n, first, num, perm, cm, cv), f"mode 2, controls={controls}")
            assert tt.negative_zeros(got) == 0


def test_behind_a_pending_basis_state(qc):
    n = 13
    first, num = LAZY
    with qc.Register(n, 0) as reg:
        for k, controls in enumerate(({}, {0: 1}, {0: 0}, {12: 0})):
            perm = lazy_table(40 + k)
            perm[[0, int(np.flatnonzero(perm == 5)[0])]] = 5, perm[0]        # perm[0] = 5: the basis state moves
            qc.reset_register(reg)                                           # pending basis state |1>
            assert reg.expectation((0, 0)) == 1.0 and reg.expectation_stats() == (2, 0), "the basis state is still pending"
            cm, cv = run(qc, reg, first, num, perm, controls)
            e = np.zeros(2 << n); e[2 * 1] = 1.0
            got = reg.read()
            same(got, pr.apply(e, n, first, num, perm, cm, cv))
            fires = (1 & cm) == cv
            assert got[2 * ((1 | (5 << first)) if fires else 1)] == 1.0      # |1> lands on 1 | perm[0] << first where it fires


def test_behind_a_compact_circuit_result(qc):
    """the compact chain exists from n = 16 on (L = 11, M = 5): the one lazy form that n = 13 does not have"""
    L, M, Cn, a = 11, 5, 21, 2
    n = L + M
    first, num = LAZY
    for k, controls in enumerate(({}, {15: 1}, {2: 0})):
        perm = lazy_table(50 + k)
        with qc.Register(L, M) as flushed:
            qc.reset_register(flushed); qc.quantum_computation(Cn, a, flushed)
            flushed.flush()
            state = flushed.read()
        with qc.Register(L, M) as reg:
            c0 = sr.compact_chains(qc, reg)
            qc.reset_register(reg); qc.quantum_computation(Cn, a, reg)
            cm, cv = run(qc, reg, first, num, perm, controls)
            assert sr.compact_chains(qc, reg) - c0 == 1, "the circuit ran as a compact chain"
            got = reg.read()
        same(got, pr.apply(state, n, first, num, perm, cm, cv))
        assert not np.array_equal(bits(got), bits(state))


def test_after_the_pointer_was_handed_out_and_on_a_callers_stream(qc, ob):
    n = 13
    first, num = LAZY
    ctx = {}
    with qc.Register(n, 0) as reg:
        reg.fill_random(SEED)
        want = np.array(filled(ob, n))
        same(sr.read_through_pointer(reg, 0, 1 << n, ctx), want, "through the pointer")
        for k, controls in enumerate(({}, {1: 1}, {12: 0, 3: 1})):
            perm = lazy_table(60 + k)
            qc.hadamard_gate(2, reg); ob.hadamard(want, n, 2)
            cm, cv = run(qc, reg, first, num, perm, controls)
            want = pr.apply(want, n, first, num, perm, cm, cv)
            same(sr.read_through_pointer(reg, 0, 1 << n, ctx), want, f"through the pointer, after table {k}")
        sr.set_stream(reg, 1, ctx)
        for k, controls in enumerate(({}, {0: 1}, {11: 1}, {})):
            perm = lazy_table(70 + k)
            table = perm.copy()
            cm, cv = run(qc, reg, first, num, table, controls)
            table[:] = 0                                                     # the caller may reuse the table at once
            want = pr.apply(want, n, first, num, perm, cm, cv)
            if k == 1:
                sr.set_stream(reg, 0, ctx)                                   # back on its own stream, in mid-sequence
        same(reg.read(), want, "on a caller's stream")


# ---- registers that hold Inf, NaN and -0; the identity table -----------------------------------------------------------------------

def test_nonfinite_registers_take_the_strict_pass(qc, ob):
    n = 13
    rs = np.random.RandomState(84)
    a = ob.random_state(n, 21)
    a[2 * 700] = np.inf
    a[2 * 5] = -0.0
    a[2 * 4100 + 1] = -0.0
    b = a.copy()
    b[2 * 3000 + 1] = np.nan
    b[2 * 8191] = -np.inf
    for state in (a, b):
        for first, num, controls in ((4, 6, {}), (0, 12, {12: 1}), (1, 12, {0: 0}), (9, 3, {2: 1, 12: 0}), (12, 1, {3: 1}), (5, 0, {})):
            perm = rs.permutation(1 << num)
            cm, cv = masks_of(controls)
            for table in (perm, np.arange(1 << num)):                        # the identity table still rewrites every amplitude
                with qc.Register(n, 0) as reg:
                    reg.write(state)
                    qc.permutation_gate(first, num, table, reg, controls=cm, values=cv)
                    w = pr.apply(state, n, first, num, table, cm, cv)
                    got = reg.read()
                    same_with_nans(got, w, f"first={first} num={num} controls={controls}")
                    assert np.isnan(got).sum() == np.isnan(w).sum() >= 1     # the Inf poisoned its other component
                    assert tt.negative_zeros(got[~np.isnan(got)]) == 0
                    qc.hadamard_gate(2, reg)                                 # the flag is kept: still the strict gate, the oracle's products
                    ob.hadamard(w, n, 2)
                    same_with_nans(reg.read(), w)


def test_negative_zeros_do_not_survive_on_finite_registers(qc, ob):
    n = 13
    rs = np.random.RandomState(12)
    a = ob.random_state(n, 22)
    a[rs.randint(0, a.size, a.size // 2)] = -0.0
    for first, num, controls in ((4, 6, {}), (4, 6, {12: 1}), (0, 12, {}), (2, 3, {0: 1}), (7, 0, {})):
        perm = rs.permutation(1 << num)
        cm, cv = masks_of(controls)
        with qc.Register(n, 0) as reg:
            reg.write(a)
            qc.permutation_gate(first, num, perm, reg, controls=cm, values=cv)
            got = reg.read()
            same(got, pr.apply(a, n, first, num, perm, cm, cv), f"first={first} num={num} controls={controls}")
            assert tt.negative_zeros(got) == 0


def test_identity_table_on_a_finite_register(qc, ob):
    n = 13
    with qc.Register(n, 0) as reg:
        for first, num, controls in ((4, 6, {}), (0, 12, {12: 1}), (13, 0, {}), (0, 0, {0: 1})):
            reg.set_fusion(1)
            reg.fill_random(8)
            want = ob.fill_random(n, 8)
            queue_some_gates(qc, ob, reg, want, n)
            before = reg.fusion_stats()
            cm, cv = run(qc, reg, first, num, np.arange(1 << num), controls)
            assert tt.stats_delta(reg.fusion_stats(), before) != (0, 0), "the call still flushes the queue"
            st, pl = qc.permutation_plan(n, cm, cv, first, num)
            assert reg.permutation_stats() == (pl.form, 0)
            same(reg.read(), want)
            reg.set_fusion(0)


def test_stats_follow_the_plan_and_the_table(qc):
    n = 14
    with qc.Register(n, 0) as reg:
        reg.fill_random(1)
        for first, num, controls, perm in ((1, 12, {}, qc.modadd_table(1, 12)), (1, 12, {0: 1}, qc.modadd_table(1, 12)), (0, 5, {9: 1}, qc.modmul_table(2, 21, 5)),
                                           (3, 2, {}, [0, 2, 1, 3]), (2, 11, {13: 0}, qc.qubit_permutation_table(range(11)[::-1]))):
            cm, cv = run(qc, reg, first, num, perm, controls)
            st, pl = qc.permutation_plan(n, cm, cv, first, num)
            moved = int(np.count_nonzero(np.asarray(perm) != np.arange(1 << num)))
            assert st == 0 and reg.permutation_stats() == (pl.form, moved)
        assert qc.permutation_plan(n, 0, 0, 1, 12)[1].form == qc.PERM_SHARED and qc.permutation_plan(n, 0, 0, 0, 5)[1].form == qc.PERM_LINES
        assert reg.permutation_stats()[1] == 2048 - 64                       # the bit reversal of 11 bits fixes its 2^6 palindromes


def test_a_modular_adder_returns_after_its_period(qc, ob):
    """k -> k + c mod 61 on six qubits, 61 times: every state of the range is back where it was, bit for bit"""
    n = 13
    table = qc.modadd_table(17, 6, modulus=61)
    with qc.Register(n, 0) as reg:
        reg.fill_random(SEED)
        for _ in range(60):
            qc.permutation_gate(3, 6, table, reg)
        assert not np.array_equal(bits(reg.read()), bits(filled(ob, n)))
        qc.permutation_gate(3, 6, table, reg)
        same(reg.read(), filled(ob, n))


# ---- arguments -----------------------------------------------------------------------------------------------------------------------

def test_refusals_in_the_documented_order(qc):
    lib = qc.lib()
    ident = np.arange(1 << 13, dtype=np.uint32)
    p = ident.ctypes.data_as(C.c_void_p)
    call = lambda cm, cv, first, num, table, h: lib.qcx_permutation_gate(cm, cv, first, num, table, h)
    with qc.Register(14, 0) as reg:
        reg.fill_random(1)
        before = bits(reg.read())
        h = reg._h
        # 1. NULL, before everything
        assert call(0, 0, 0, 1, p, None) == BAD_ARGUMENTS and call(0, 0, 0, 1, None, h) == BAD_ARGUMENTS
        assert call(1, 3, 20, 1, None, h) == BAD_ARGUMENTS
        # 2. values outside the mask, with mc_gate's message, before the range
        assert call(0x10, 0x30, 20, 1, p, h) == BAD_ARGUMENTS
        assert b"permutation_gate: ctrl_values 0x30 has bits outside ctrl_mask 0x10" in lib.qcx_last_error()
        # 3. the range, before the mask's bits and the width
        for first, num in ((0, 15), (14, 1), (15, 0), (5, 10), (0xFFFFFFFF, 1), (1, 0xFFFFFFFF)):
            assert call(1 << 20, 0, first, num, p, h) == BAD_QUBIT, (first, num)
        # 4. a mask bit at or above n, or inside the range, before the width
        for cm, first, num in ((1 << 14, 0, 1), (1 << 63, 0, 1), (1 << 3, 3, 1), (1 << 8, 2, 7), (1 << 5, 1, 13)):
            assert call(cm, 0, first, num, p, h) == BAD_QUBIT, (cm, first, num)
        # 5. wider than a tile, before the entries
        bad = ident.copy(); bad[0] = 1
        assert call(0, 0, 0, 13, bad.ctypes.data_as(C.c_void_p), h) == BAD_ARGUMENTS
        assert b"12" in lib.qcx_last_error() and b"entry" not in lib.qcx_last_error()
        # 6. the entries: out of range, repeated; the first offender is named with its value
        for num, k, v, other in ((12, 17, 4096, None), (12, 4095, 0xFFFFFFFF, None), (3, 5, 8, None), (12, 3000, 7, 7), (1, 1, 0, 0), (0, 0, 1, None)):
            t = ident[:1 << num].copy()
            t[k] = v
            if num == 12 and other is None:
                t[k + 1:] = 5000                                             # later offenders are not the ones named
            assert call(0, 0, 1, num, t.ctypes.data_as(C.c_void_p), h) == BAD_ARGUMENTS, (num, k, v)
            msg = lib.qcx_last_error().decode()
            assert f"entry {k} is {v}," in msg, msg
            if other is not None:
                assert f"entry {other} already has" in msg, msg
        with pytest.raises(ValueError):
            qc.permutation_gate(0, 3, np.arange(4), reg)
        with pytest.raises(ValueError):
            qc.permutation_gate(0, 2, [0.0, 1.0, 2.0, 3.0], reg)
        with pytest.raises(ValueError):
            qc.permutation_gate(0, 2, [0, 1, 2, -1], reg)
        with pytest.raises(qc.QcxError) as e:
            qc.permutation_gate(0, 2, [0, 1, 1, 3], reg)
        assert e.value.status == BAD_ARGUMENTS
        with pytest.raises(qc.QcxError) as e:
            qc.permutation_gate(0, 2, [0, 1, 3, 2], reg, controls=[1])
        assert e.value.status == BAD_QUBIT
        assert np.array_equal(bits(reg.read()), before)
        assert reg.permutation_stats() == (0, 0), "a refused call leaves no stats"
        assert call(0, 0, 1, 12, p, h) == 0 and np.array_equal(bits(reg.read()), before)
    with qc.Register(13, 0, shards=4, devices=qc.spread_devices(4)) as sh:  # 7. virtual shards on one GPU, after the entries
        sh.fill_random(3)
        before = bits(sh.read())
        swap = np.array([0, 2, 1, 3], dtype=np.uint32)
        assert call(0, 0, 2, 2, swap.ctypes.data_as(C.c_void_p), sh._h) == UNSUPPORTED
        swap[3] = 2
        assert call(0, 0, 2, 2, swap.ctypes.data_as(C.c_void_p), sh._h) == BAD_ARGUMENTS
        assert call(0, 0, 12, 2, swap.ctypes.data_as(C.c_void_p), sh._h) == BAD_QUBIT
        assert np.array_equal(bits(sh.read()), before)
