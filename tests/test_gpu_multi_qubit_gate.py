"""GPU: a dense matrix on 1 .. 5 target qubits under any controls (qcx_mc_multi_qubit_gate, K20).  Every state must be, bit for
bit, what tests/multi_qubit_ref.py defines on whatever the register held: every form of small registers, the edges of the tile
rule (the whole-wave threshold, one partial tile, exactly one tile, several tiles, targets inside a line, at the top and spread,
squeezed controls below, between and above the targets, so many of them that fewer than 12 unsqueezed bits remain, a control at
bit 0, every control that exists), the existing kernels it generalises (new against old on twin registers), every lazy form
the library keeps a state in, registers that hold Inf, NaN and -0, the observers behind it, every refusal in its order, and a
fused QFT block against the gate_batch of its gates."""
import ctypes as C
import itertools

import numpy as np
import pytest

import marginal_ref
import multi_qubit_ref as mq
import pauli_ref
import sequence_replay as sr
import tolerance_twin as tt
from bitwise import bits, random_unitary, same, same_with_nans

pytestmark = pytest.mark.gpu

BAD_ARGUMENTS, BAD_QUBIT, UNSUPPORTED = 2, 6, 7
SEED = 91
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


def check(qc, ob, reg, n, targets, U, controls, what=""):
    """fill_random, the call, a read-back against the definition; the stats against the plan"""
    a = filled(ob, n)
    reg.fill_random(SEED)
    cm, cv = masks_of(controls)
    qc.multi_qubit_gate(targets, U, reg, controls=cm, values=cv)
    got = reg.read()
    same(got, mq.apply(a, n, targets, U, cm, cv), f"{what} n={n} targets={targets} controls={controls}")
    st, pl = qc.multi_gate_plan(n, cm, cv, targets)
    assert st == 0 and reg.multi_qubit_stats() == (pl.form, len(targets)) and pl.form == qc.PERM_LINES
    return got


def matrices(k, seed):
    """a random unitary, one with exact zeros (of either sign), and a permutation matrix"""
    d = 1 << k
    Z = random_unitary(seed + 1, d).copy()
    Z[0, :d // 2] = 0.0; Z[d - 1, 1] = -0.0; Z[1, d - 1] = complex(0.0, -0.0)
    P = np.zeros((d, d)); P[np.random.RandomState(seed).permutation(d), np.arange(d)] = 1.0
    return [random_unitary(seed, d), Z, P]


def control_sets(n, targets):
    free = [c for c in range(n) if c not in targets]
    sets = [{}] + [{c: v} for c in free for v in (1, 0)]
    sets += [{a: 1, b: 0} for a in free for b in free if a != b]
    return sets


# ---- every form of small registers -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [3, 4, 5])
def test_three_targets_every_ordered_triple_and_control(qc, ob, n):
    with qc.Register(n, 0) as reg:
        for j, t in enumerate(itertools.permutations(range(n), 3)):
            Us = matrices(3, 10 * n + j)
            for i, controls in enumerate(control_sets(n, t)):
                check(qc, ob, reg, n, t, Us[(i + j) % 3] if i else Us[0], controls)


@pytest.mark.parametrize("k,n", [(4, 4), (4, 5), (4, 6), (5, 5), (5, 6), (5, 7)])
def test_four_and_five_targets_every_set_and_control(qc, ob, k, n):
    rs = np.random.RandomState(100 * k + n)
    with qc.Register(n, 0) as reg:
        for j, t in enumerate(itertools.combinations(range(n), k)):
            Us = matrices(k, 7 * n + j)
            for order in (t, tuple(int(q) for q in rs.permutation(t))):
                for i, controls in enumerate(control_sets(n, t)):
                    check(qc, ob, reg, n, order, Us[(i + j) % 3] if i else Us[0], controls)


# ---- the edges where the kernel can go wrong ---------------------------------------------------------------------------------------

def edge_targets(n):
    out = [(0, 1, 2), (0, 1, 2, 3, 4), (n - 3, n - 2, n - 1), (1, 6, n - 1), (n - 1, 3, 5), (3, 4, 5, 6), (7, 4, 8, 3, 6)]
    if n >= 13:
        out += [(2, 5, 8, 11, n - 1), (n - 1, n - 2, n - 3, n - 4, n - 5), (9, 11, 10)]
    return [t for t in out if max(t) < n]


def edge_controls(n, t):
    free = [c for c in range(n) if c not in t]
    above3 = [c for c in free if c >= 3]
    sets = [{}, {free[0]: 1}, {free[0]: 0, free[-1]: 1}]
    if above3:
        lo, hi = min(t), max(t)
        below = [c for c in above3 if c < lo][:1]
        between = [c for c in above3 if lo < c < hi][:1]
        above = [c for c in above3 if c > hi][:1]
        sets.append({c: (j + 1) % 2 for j, c in enumerate(below + between + above)})     # squeezed controls below, between, above
        sets.append({c: j % 2 for j, c in enumerate(above3[:max(1, n - len(t) - 5)])})   # fewer than 12 unsqueezed bits remain
    if 0 in free:
        sets.append({0: 1})                                                              # a control at bit 0, inside the tile
        sets.append({0: 0, above3[-1]: 1} if above3 else {0: 0})
    sets.append({c: (c * 7 // 3) % 2 for c in free})                                     # every control that exists
    out = []
    for s in sets:
        if s not in out:
            out.append(s)
    return out


@pytest.mark.parametrize("n", [9, 11, 12, 13, 14])
def test_edges_of_the_tile_rule(qc, ob, n):
    """n = 9: the whole-wave threshold; 11: one partial tile; 12: exactly one tile; 13, 14: several tiles"""
    with qc.Register(n, 0) as reg:
        for j, t in enumerate(edge_targets(n)):
            U = random_unitary(1000 * n + j, 1 << len(t))
            for controls in edge_controls(n, t):
                got = check(qc, ob, reg, n, t, U, controls)
                assert not np.array_equal(bits(got), bits(filled(ob, n)))
    st, pl = qc.multi_gate_plan(n, 0, 0, (0, 1, 2))
    assert st == 0 and pl.units == 1 << max(0, n - 12) and pl.T == min(n, 12)


@pytest.mark.parametrize("knobs", [dict(multi_grid_cap=3), dict(multi_grid_cap=0), dict(multi_store_all=0), dict(multi_nt=1), dict(multi_nt=1, multi_store_all=0)],
                         ids=["cap3", "nocap", "no-store_all", "nt", "nt-no-store_all"])
def test_knobs_change_no_bit(qc, ob, knobs):
    """a grid that does not divide the units (a workgroup walks several tiles), one tile each, and the two store policies"""
    keep = {k: qc.lib().qcx_tune_get(k.encode()) for k in knobs}
    try:
        qc.tune(**knobs)
        with qc.Register(14, 0) as reg:
            for j, (t, controls) in enumerate([((2, 9, 13), {}), ((3, 4, 5, 6), {0: 1}), ((4, 0, 8, 2, 11), {1: 0, 13: 1}), ((0, 1, 2), {}), ((12, 5, 7, 1), {2: 0})]):
                check(qc, ob, reg, 14, t, random_unitary(40 + j, 1 << len(t)), controls, str(knobs))
    finally:
        qc.tune(**keep)


def test_more_than_one_tile_per_workgroup(qc, ob):
    """n = 18 under a cap of 7 workgroups: 64 tiles, nine or ten to a workgroup (the default cap of 2048 is met from n = 24 on)"""
    n = 18
    keep = qc.lib().qcx_tune_get(b"multi_grid_cap")
    try:
        qc.tune(multi_grid_cap=7)
        st, pl = qc.multi_gate_plan(n, 0, 0, (3, 14, 16, 17))
        assert st == 0 and pl.units == 64 and pl.grid == 7
        with qc.Register(n, 0) as reg:
            check(qc, ob, reg, n, (3, 14, 16, 17), random_unitary(5, 16), {})
            check(qc, ob, reg, n, (17, 2, 9), random_unitary(6, 8), {15: 0, 1: 1})
    finally:
        qc.tune(multi_grid_cap=keep)


# ---- new against old on twin registers -----------------------------------------------------------------------------------------------

def both(qc, ob, reg, twin, n, new, old, what):
    reg.fill_random(SEED); twin.fill_random(SEED)
    new(reg); old(twin)
    got = reg.read()
    assert np.array_equal(bits(got), bits(twin.read())), what
    assert not np.array_equal(bits(got), bits(filled(ob, n))), what


def test_generic_knob_against_the_mc_gates(qc, ob):
    n = 13
    keep = qc.lib().qcx_tune_get(b"multi_generic")
    with qc.Register(n, 0) as reg, qc.Register(n, 0) as twin:
        try:
            qc.tune(multi_generic=1)
            for j, (q, controls) in enumerate([(0, {}), (12, {}), (5, {}), (1, {7: 1}), (9, {0: 1}), (3, {12: 0}), (6, {2: 1, 11: 1}), (0, {1: 1, 2: 0}), (12, {3: 1, 4: 1, 5: 0})]):
                cm, cv = masks_of(controls)
                U = random_unitary(200 + j, 2)
                both(qc, ob, reg, twin, n, lambda r: qc.multi_qubit_gate((q,), U, r, controls=cm, values=cv), lambda r: qc.mc_one_qubit_gate(cm, q, U, r, values=cv), (q, controls))
            for j, (q0, q1, controls) in enumerate([(0, 1, {}), (12, 11, {}), (2, 9, {}), (9, 2, {4: 1}), (7, 0, {1: 1}), (0, 5, {12: 0}), (10, 3, {1: 1, 6: 0}), (1, 2, {0: 0, 8: 1})]):
                cm, cv = masks_of(controls)
                U = random_unitary(300 + j, 4)
                both(qc, ob, reg, twin, n, lambda r: qc.multi_qubit_gate((q0, q1), U, r, controls=cm, values=cv),
                     lambda r: qc.mc_two_qubit_gate(cm, q0, q1, U, r, values=cv), (q0, q1, controls))
        finally:
            qc.tune(multi_generic=keep)
        # without the knob one and two targets ARE the mc calls
        U = random_unitary(1, 4)
        both(qc, ob, reg, twin, n, lambda r: qc.multi_qubit_gate((4, 2), U, r, controls=[9]), lambda r: qc.mc_two_qubit_gate([9], 4, 2, U, r), "k = 2, no knob")
        assert reg.multi_qubit_stats() == (qc.PERM_LINES, 2)


def test_embedded_two_qubit_gates_and_permutations_against_their_calls(qc, ob):
    n = 13
    with qc.Register(n, 0) as reg, qc.Register(n, 0) as twin:
        for j, (t0, t1, t2) in enumerate([(0, 1, 2), (5, 3, 12), (12, 0, 6), (7, 8, 1), (2, 11, 4)]):
            U4 = random_unitary(500 + j, 4)
            both(qc, ob, reg, twin, n, lambda r: qc.multi_qubit_gate((t0, t1, t2), np.kron(np.eye(2), U4), r), lambda r: qc.two_qubit_gate(t0, t1, U4, r), ("kron", t0, t1, t2))
            cU = np.eye(8, dtype=complex); cU[4:, 4:] = U4
            both(qc, ob, reg, twin, n, lambda r: qc.multi_qubit_gate((t0, t1, t2), cU, r), lambda r: qc.mc_two_qubit_gate([t2], t0, t1, U4, r), ("controlled", t0, t1, t2))
        rs = np.random.RandomState(3)
        for first, controls in [(0, {}), (9, {}), (4, {12: 1}), (2, {0: 0}), (6, {1: 1, 11: 0})]:
            perm = rs.permutation(16)
            P = np.zeros((16, 16)); P[perm, np.arange(16)] = 1.0
            cm, cv = masks_of(controls)
            both(qc, ob, reg, twin, n, lambda r: qc.multi_qubit_gate(range(first, first + 4), P, r, controls=cm, values=cv),
                 lambda r: qc.permutation_gate(first, 4, perm, r, controls=cm, values=cv), ("permutation", first, controls))


# ---- every lazy form -----------------------------------------------------------------------------------------------------------------

LAZY = (9, 2, 5, 4)                             # the targets of every lazy-form test, on n = 13


def queue_some_gates(qc, ob, reg, want, n):
    for q in (0, 3, n - 1):
        qc.hadamard_gate(q, reg)
        ob.hadamard(want, n, q)
    qc.c_phase_shift_gate(3, n - 1, 0.7, reg)
    ob.cphase(want, n, 3, n - 1, 0.7)


def test_queued_gates_are_flushed_first(qc, ob):
    n = 13
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
            U = random_unitary(20 + k, 16)
            reg.fill_random(8)
            want = ob.fill_random(n, 8)
            queue_some_gates(qc, ob, reg, want, n)
            before = reg.fusion_stats()
            cm, cv = masks_of(controls)
            qc.multi_qubit_gate(LAZY, U, reg, controls=cm, values=cv)
            assert tt.stats_delta(reg.fusion_stats(), before) == flush_counts, "the flush's passes, and nothing counted for the gate"
            want = mq.apply(want, n, LAZY, U, cm, cv)
            qc.hadamard_gate(1, reg); ob.hadamard(want, n, 1)                # queued behind it
            same(reg.read(), want)


def test_behind_mode_2_work_against_a_twin(qc, ob, tmp_path):
    """tolerance_twin's method: the state S a twin register reads back after the same mode-2 work is the reference; the gate is
    exact in mode 2, and the zero pass the tolerance flush owes runs first"""
    shape = (13, 0, 1, 1)
    n = 13
    prefix = tt.prefix_ops("iqft", shape)
    twin = tt.run_twin(qc, shape, prefix, tmp_path)
    S = twin[0]
    tt.check_twin(twin, tt.oracle_state(ob, "iqft", shape)[0], prefix, shape)
    for k, controls in enumerate(({}, {12: 1})):
        U = random_unitary(30 + k, 16)
        cm, cv = masks_of(controls)
        with qc.Register(n, 0) as reg:
            before = reg.fusion_stats()
            tt.run_prefix(qc, reg, prefix, tmp_path, {})
            qc.multi_qubit_gate(LAZY, U, reg, controls=cm, values=cv)
            assert tt.stats_delta(reg.fusion_stats(), before) == twin[1][:2], "the queued mode-2 work ran, nothing else is counted"
            got = reg.read()
            same(got, mq.apply(S, n, LAZY, U, cm, cv), f"mode 2, controls={controls}")      # (its identity rows turn every -0 of S into +0)
            assert tt.negative_zeros(got) == 0


def test_behind_a_pending_basis_state(qc):
    n = 13
    with qc.Register(n, 0) as reg:
        for k, controls in enumerate(({}, {0: 1}, {0: 0}, {12: 0})):
            U = random_unitary(40 + k, 16)
            qc.reset_register(reg)                                           # pending basis state |1>
            assert reg.expectation((0, 0)) == 1.0 and reg.expectation_stats() == (2, 0), "the basis state is still pending"
            cm, cv = masks_of(controls)
            qc.multi_qubit_gate(LAZY, U, reg, controls=cm, values=cv)
            e = np.zeros(2 << n); e[2 * 1] = 1.0
            got = reg.read()
            w = mq.apply(e, n, LAZY, U, cm, cv)
            same(got, w)
            assert (np.count_nonzero(got) > 1) == ((1 & cm) == cv)           # |1> spreads over its group where it fires


def test_behind_a_compact_circuit_result(qc):
    """the compact chain exists from n = 16 on (L = 11, M = 5)"""
    L, M, Cn, a = 11, 5, 21, 2
    n = L + M
    for k, controls in enumerate(({}, {15: 1}, {1: 0})):
        U = random_unitary(50 + k, 16)
        cm, cv = masks_of(controls)
        with qc.Register(L, M) as flushed:
            qc.reset_register(flushed); qc.quantum_computation(Cn, a, flushed)
            flushed.flush()
            state = flushed.read()
        with qc.Register(L, M) as reg:
            c0 = sr.compact_chains(qc, reg)
            qc.reset_register(reg); qc.quantum_computation(Cn, a, reg)
            qc.multi_qubit_gate(LAZY, U, reg, controls=cm, values=cv)
            assert sr.compact_chains(qc, reg) - c0 == 1, "the circuit ran as a compact chain"
            got = reg.read()
        same(got, mq.apply(state, n, LAZY, U, cm, cv))
        assert not np.array_equal(bits(got), bits(state))


def test_the_matrix_may_be_reused_at_once_and_calls_follow_each_other(qc, ob):
    n = 13
    with qc.Register(n, 0) as reg:
        reg.fill_random(SEED)
        want = np.array(filled(ob, n))
        for k, (t, controls) in enumerate([(LAZY, {}), ((0, 1, 2), {5: 1}), ((12, 3, 7, 1, 10), {0: 1}), ((6, 5, 4), {}), ((11, 2, 8, 9), {3: 0, 1: 1})]):
            U = random_unitary(60 + k, 1 << len(t))
            u = np.ascontiguousarray(U.reshape(-1)).view(np.float64).copy()
            cm, cv = masks_of(controls)
            qc.multi_qubit_gate(t, u, reg, controls=cm, values=cv)
            u[:] = 0.0                                                       # the caller may reuse the matrix at once
            want = mq.apply(want, n, t, U, cm, cv)
        same(reg.read(), want)


# ---- registers that hold Inf, NaN and -0 -------------------------------------------------------------------------------------------

def test_nonfinite_registers_take_the_strict_pass(qc, ob):
    n = 13
    a = ob.random_state(n, 21)
    a[2 * 700] = np.inf
    a[2 * 5] = -0.0
    a[2 * 4100 + 1] = -0.0
    b = a.copy()
    b[2 * 3000 + 1] = np.nan
    b[2 * 8191] = -np.inf
    for state in (a, b):
        for j, (t, controls) in enumerate((((4, 9, 6), {}), ((0, 1, 2, 3, 4), {12: 1}), ((12, 2, 7, 5), {0: 0}), ((9, 3, 1), {2: 1, 12: 0}), ((12,), {3: 1}), ((5, 8), {4: 0}),
                                           ((2, 5, 8, 11, 12), {})) ):
            U = random_unitary(80 + j, 1 << len(t))
            cm, cv = masks_of(controls)
            with qc.Register(n, 0) as reg:
                reg.write(state)
                qc.multi_qubit_gate(t, U, reg, controls=cm, values=cv)
                w = mq.apply(state, n, t, U, cm, cv)
                got = reg.read()
                same_with_nans(got, w, f"targets={t} controls={controls}")
                assert not np.all(np.isfinite(got)) and np.isnan(got).sum() == np.isnan(w).sum()      # (an identity row's 0 * Inf is a NaN; a dense row's Inf stays Inf)
                qc.hadamard_gate(2, reg)                                     # the flag is kept: still the strict gate, the oracle's products
                ob.hadamard(w, n, 2)
                same_with_nans(reg.read(), w)


def test_negative_zeros_on_finite_registers(qc, ob):
    """the canonical-zeros pass runs first, so the amplitudes that do not fire come back with +0 for every -0"""
    n = 13
    rs = np.random.RandomState(12)
    a = ob.random_state(n, 22)
    a[rs.randint(0, a.size, a.size // 2)] = -0.0
    for j, (t, controls) in enumerate((((4, 9, 6), {}), ((4, 9, 6), {12: 1}), ((0, 1, 2, 3, 4), {}), ((2, 3, 12, 5), {0: 1}))):
        U = matrices(len(t), 90 + j)[j % 3]
        cm, cv = masks_of(controls)
        with qc.Register(n, 0) as reg:
            reg.write(a)
            qc.multi_qubit_gate(t, U, reg, controls=cm, values=cv)
            got = reg.read()
            same(got, mq.apply(a, n, t, U, cm, cv), f"targets={t} controls={controls}")


# ---- observers behind it -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("controls", [{}, {11: 1}], ids=["plain", "controlled"])
def test_observers_after_a_gate(qc, ob, controls):
    n, t = 13, (4, 9, 6, 2)
    U = random_unitary(6, 16)
    cm, cv = masks_of(controls)
    with qc.Register(n, 0) as reg:
        reg.fill_random(SEED)
        qc.multi_qubit_gate(t, U, reg, controls=cm, values=cv)
        state = mq.apply(filled(ob, n), n, t, U, cm, cv)
        same(reg.marginal(4, 6), marginal_ref.marginal_ref(state, n, 4, 6), "the marginal")
        for spec in ("IIZIXIYII", {4: "X", 9: "Z"}, (0b1001010000, 0b0001000100)):
            x, z = pauli_ref.pauli_masks(spec, n)
            same(reg.expectation((x, z)), pauli_ref.pauli_ref(state, n, x, z), str(spec))


# ---- arguments -----------------------------------------------------------------------------------------------------------------------

def test_refusals_in_the_documented_order(qc):
    lib = qc.lib()
    U = np.ascontiguousarray(random_unitary(1, 32).reshape(-1)).view(np.float64).copy()
    p = U.ctypes.data_as(C.c_void_p)
    arr = lambda *t: C.cast((C.c_uint * max(len(t), 1))(*t), C.c_void_p)
    call = lambda cm, cv, k, t, u, h: lib.qcx_mc_multi_qubit_gate(cm, cv, k, t, u, h)
    with qc.Register(14, 0) as reg:
        reg.fill_random(1)
        before = bits(reg.read())
        h = reg._h
        # 1. NULL, before everything
        assert call(0, 0, 3, arr(0, 1, 2), p, None) == BAD_ARGUMENTS and call(0, 0, 3, arr(0, 1, 2), None, h) == BAD_ARGUMENTS
        assert call(1, 3, 9, None, p, h) == BAD_ARGUMENTS
        # 2. the number of targets, before the matrix
        bad = U.copy(); bad[0] = np.nan
        for k in (0, 6, 0xFFFFFFFF):
            assert call(0x10, 0x30, k, arr(20, 20, 20, 20, 20, 20), bad.ctypes.data_as(C.c_void_p), h) == BAD_ARGUMENTS
            assert b"1 to 5" in lib.qcx_last_error()
        # 3. the matrix, before the masks: the component is named
        for k, j, v in ((3, 0, np.nan), (3, 127, 1.5), (5, 2047, -np.inf), (1, 7, -1.0000000000000002)):
            bad = U.copy(); bad[j] = v
            assert call(0x10, 0x30, k, arr(20, 20, 20, 20, 20), bad.ctypes.data_as(C.c_void_p), h) == BAD_ARGUMENTS
            assert f"matrix component {j} is".encode() in lib.qcx_last_error(), lib.qcx_last_error()
        # 4. values outside the mask, before the qubits
        assert call(0x10, 0x30, 3, arr(20, 20, 1), p, h) == BAD_ARGUMENTS
        assert b"ctrl_values 0x30 has bits outside ctrl_mask 0x10" in lib.qcx_last_error()
        # 5. the qubits
        for t in ((14, 0, 1), (0, 1, 0xFFFFFFFF), (3, 4, 3), (1, 1), (5, 6, 7, 8, 5)):
            assert call(0, 0, len(t), arr(*t), p, h) == BAD_QUBIT, t
        for cm, t in ((1 << 14, (0, 1, 2)), (1 << 63, (0, 1, 2)), (1 << 3, (2, 3, 4)), (1 << 9, (13, 9, 1, 0))):
            assert call(cm, 0, len(t), arr(*t), p, h) == BAD_QUBIT, (cm, t)
        with pytest.raises(ValueError):
            qc.multi_qubit_gate((0, 1, 2), np.eye(4), reg)
        with pytest.raises(ValueError):
            qc.multi_qubit_gate((0, 1, 2, 3, 4, 5), np.eye(64), reg)
        with pytest.raises(qc.QcxError) as e:
            qc.multi_qubit_gate((0, 1, 2), 2 * np.eye(8), reg)
        assert e.value.status == BAD_ARGUMENTS
        with pytest.raises(qc.QcxError) as e:
            qc.multi_qubit_gate((0, 1, 2), np.eye(8), reg, controls=[1])
        assert e.value.status == BAD_QUBIT
        assert np.array_equal(bits(reg.read()), before)
        assert reg.multi_qubit_stats() == (0, 0), "a refused call leaves no stats"
        assert call(0, 0, 5, arr(0, 5, 13, 2, 7), p, h) == 0 and not np.array_equal(bits(reg.read()), before)
        assert reg.multi_qubit_stats() == (0, 5)
    with qc.Register(13, 0, shards=4, devices=qc.spread_devices(4)) as sh:  # 6. virtual shards on one GPU, after the qubits
        sh.fill_random(3)
        before = bits(sh.read())
        assert call(0, 0, 3, arr(2, 3, 4), p, sh._h) == UNSUPPORTED
        assert call(0, 0, 2, arr(2, 3), p, sh._h) == UNSUPPORTED
        assert call(0, 0, 3, arr(2, 3, 13), p, sh._h) == BAD_QUBIT
        bad = U.copy(); bad[5] = 7.0
        assert call(0, 0, 3, arr(2, 3, 4), bad.ctypes.data_as(C.c_void_p), sh._h) == BAD_ARGUMENTS
        assert np.array_equal(bits(sh.read()), before)


# ---- a fused block against the batch of its gates ------------------------------------------------------------------------------------

def qft_gates(qubits):
    """the QFT on `qubits` (first = most significant) as H and controlled phases, in gate_batch's form; no final swaps"""
    H = np.array([[1, 1], [1, -1]], dtype=complex) / np.sqrt(2.0)
    gates = []
    for i, q in enumerate(qubits):
        gates.append((H, q))
        for j, c in enumerate(qubits[i + 1:], start=2):
            gates.append((np.diag([1.0, np.exp(2j * np.pi / (1 << j))]), q, c))
    return gates


def test_fused_qft_block_against_the_gate_batch(qc, ob):
    """The same operator with different roundings.  Per component, to first order in 2^-53, with max|amp| <= 1 for every
    magnitude (test_multi_qubit_ref.py derives the terms): the block's one call rounds a row of 16 columns, 16 * 4 * 2^-53; its
    matrix carries the roundings of G = 10 numpy products, each a row of 16 columns, G * 16 * 4 * 2^-53; the batch applies G
    one-qubit gates (under a control or not), each a row of 2 columns, G * 2 * 4 * 2^-53."""
    n, t = 13, (3, 9, 12, 6)
    gates = qft_gates(list(t))
    assert len(gates) == 10
    F = qc.fused_matrix(gates, t)
    F = np.clip(F.real, -1, 1) + 1j * np.clip(F.imag, -1, 1)
    dft = np.exp(2j * np.pi * np.outer(np.arange(16), np.arange(16)) / 16) / 4
    rev = [int(f"{c:04b}"[::-1], 2) for c in range(16)]
    assert np.allclose(F[rev] if np.allclose(F[rev], dft) else F[:, rev], dft, atol=1e-14), "the block is the DFT up to the bit reversal"
    bound = (16 * 4 + len(gates) * 16 * 4 + len(gates) * 2 * 4) * 2.0 ** -53
    with qc.Register(n, 0) as reg, qc.Register(n, 0) as twin:
        reg.fill_random(SEED); twin.fill_random(SEED)
        qc.multi_qubit_gate(t, F, reg)
        qc.gate_batch(gates, twin)
        got, want = reg.read(), twin.read()
        same(got, mq.apply(filled(ob, n), n, t, F), "the block by its definition")
        err = float(np.max(np.abs(got - want)))
        print(f"fused QFT block against gate_batch: max component difference {err:.3e}, bound {bound:.3e}")
        assert 0.0 < err <= bound
