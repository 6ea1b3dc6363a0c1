"""GPU: a list of one- and two-qubit gates in as few passes as locality allows (qcx_gate_batch, K12b / K13b).  The state
afterwards must be, bit for bit, what the loop of tests/one_qubit_ref.apply / tests/two_qubit_ref.apply over the list leaves --
in all four variants of the kernel, on the partial tile of a small register, on tiles that are not the 12 lowest index bits, with
targets and controls on lane, wave, hot and base bits, across passes closed by the budget and by a fifth hot bit, and behind
every lazy form the library keeps a state in.  The passes a call ran are the plan's every time."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

import one_qubit_ref
import two_qubit_ref
from bitwise import bits, minus_zero_state, random_unitary, same, same_with_nans
from register_model import RegisterModel

pytestmark = pytest.mark.gpu


# ---- gates as gate_batch takes them: (U, targets) or (U, targets, control) ----------------------------------------------------

def parts(g):
    t = g[1]
    return g[0], ((t,) if isinstance(t, int) else tuple(t)), (g[2] if len(g) == 3 else None)


def ref_loop(a, n, gates):
    for g in gates:
        U, t, c = parts(g)
        a = one_qubit_ref.apply(a, n, t[0], U, control=c) if len(t) == 1 else two_qubit_ref.apply(a, n, t[0], t[1], U, control=c)
    return a


def call_loop(qc, reg, gates):
    """the four existing calls, gate by gate"""
    for g in gates:
        U, t, c = parts(g)
        if len(t) == 1:
            qc.one_qubit_gate(t[0], U, reg) if c is None else qc.c_one_qubit_gate(c, t[0], U, reg)
        else:
            qc.two_qubit_gate(t[0], t[1], U, reg) if c is None else qc.c_two_qubit_gate(c, t[0], t[1], U, reg)


def run_batch(qc, reg, gates):
    """the call, and what it ran against the plan"""
    qc.gate_batch(gates, reg)
    _, hots = qc.gate_batch_plan(gates, reg.num_qubits)
    assert reg.gate_batch_stats() == (len(hots), sum(1 for g in gates if min(parts(g)[1]) < 8))
    return hots


def state(n, seed):
    rs = np.random.RandomState(seed)
    a = rs.standard_normal(2 << n)
    return a / np.linalg.norm(a)


def check_lists(qc, n, a, lists, chained=True):
    """every list on ONE register that starts as `a`, a read-back after every call, each compared with the loop of the definition
    on what the register held before it; chained=False: the start state is written again before every list"""
    hots = []
    with qc.Register(n, 0) as reg:
        reg.write(a)
        have = a
        for k, gates in enumerate(lists):
            if k and not chained:
                reg.write(a)
                have = a
            hots += run_batch(qc, reg, gates)
            want = ref_loop(have, n, gates)
            have = reg.read()
            same(have, want, f"n = {n}, list {k}")
            assert not np.any((have == 0) & np.signbit(have)), (n, k)
    return hots


def pool1(qc):
    G = qc.GATES
    return [random_unitary(1, 2), G["X"], G["H"], random_unitary(2, 2), G["T"], G["Y"], qc.rz(0.37), G["S"], qc.phase(-1.1)]


def pool2(qc):
    G2 = qc.GATES2
    return [random_unitary(3, 4), G2["CNOT"], G2["SWAP"], qc.controlled(random_unitary(4, 2)), random_unitary(5, 4), G2["ISWAP"], G2["CZ"],
            qc.controlled(qc.GATES["H"])]


def random_gates(qc, rs, n, count, targets=None):
    """any of the four forms, targets from `targets` (default: every qubit), controls anywhere"""
    p1, p2 = pool1(qc), pool2(qc)
    targets = list(range(n)) if targets is None else list(targets)
    out = []
    for k in range(count):
        two = len(targets) >= 2 and rs.randint(0, 2) == 1
        t = tuple(int(q) for q in rs.choice(targets, 2 if two else 1, replace=False))
        rest = [q for q in range(n) if q not in t]
        U = p2[k % len(p2)] if two else p1[k % len(p1)]
        if rest and rs.randint(0, 2) == 1:
            out.append((U, t, int(rs.choice(rest))))
        else:
            out.append((U, t))
    return out


# ---- small registers: one partial tile ---------------------------------------------------------------------------------------

def test_one_qubit(qc):
    lists = [[(U, 0) for U in pool1(qc)[k:k + 3]] for k in (0, 3, 6)] + [[(qc.GATES["H"], (0,))]]
    assert check_lists(qc, 1, state(1, 1), lists) == [0] * 4


@pytest.mark.parametrize("n", [2, 3])
def test_every_placement_in_lists_of_3(qc, n):
    p1, p2 = pool1(qc), pool2(qc)
    gates = []
    for k, t in enumerate(itertools.permutations(range(n), 1)):
        gates.append((p1[k % len(p1)], t))
    for k, (q, c) in enumerate(itertools.permutations(range(n), 2)):
        gates.append((p1[(k + 2) % len(p1)], q, c))
    for k, t in enumerate(itertools.permutations(range(n), 2)):
        gates.append((p2[k % len(p2)], t))
    for k, (q0, q1, c) in enumerate(itertools.permutations(range(n), 3)):
        gates.append((p2[(k + 3) % len(p2)], (q0, q1), c))
    assert len(gates) == {2: 6, 3: 21}[n]
    lists = [gates[k:k + 3] for k in range(0, len(gates), 3)]
    check_lists(qc, n, state(n, 7 * n), lists)
    check_lists(qc, n, state(n, 8 * n), [gates[::-1]])


@pytest.mark.parametrize("n", [5, 11])
def test_partial_tile_random_lists_of_12(qc, n):
    rs = np.random.RandomState(n)
    lists = [random_gates(qc, rs, n, 12) for _ in range(3)]
    if n == 11:
        lists.append(random_gates(qc, rs, n, 12, targets=(8, 9, 10)))           # the variant without LDS
    hots = check_lists(qc, n, state(n, 3 * n), lists, chained=False)
    assert hots == [((1 << n) - 1) >> 8 << 8] * len(hots)


def test_minus_zero_state(qc, ob):
    n = 5
    rs = np.random.RandomState(55)
    a = minus_zero_state(ob, n, 4)
    assert np.any((a == 0) & np.signbit(a))
    # a controlled gate first: the amplitudes it does not touch must come out as +0 all the same
    gates = [(qc.GATES["X"], 1, 4)] + random_gates(qc, rs, n, 11)
    check_lists(qc, n, a, [gates])


# ---- one tile ---------------------------------------------------------------------------------------------------------------

def test_one_full_tile(qc):
    n = 12
    p1, p2 = pool1(qc), pool2(qc)
    gates = [
        (p1[0], 2), (p1[1], 7), (p1[2], 10),                        # a lane bit, a wave bit, a hot bit
        (p2[0], (1, 6)), (p2[1], (3, 9)), (p2[4], (8, 11)),         # lanes + wave; one low, one hot; both hot
        (p2[0], (9, 4)), (p2[3], (11, 8)), (p2[4], (7, 6)), (p2[1], (10, 9)),      # qubit0 > qubit1
        (p1[3], 10, 3), (p1[4], 10, 6), (p1[5], 10, 9),             # a hot target under a lane, a wave and a hot control
        (p1[6], 2, 5), (p1[7], 2, 7), (p1[0], 2, 11),               # a lane target
        (p1[3], 6, 0), (p1[8], 7, 8),                               # a wave target
        (p2[0], (1, 6), 10), (p2[4], (8, 11), 9), (p2[5], (8, 11), 4), (p2[0], (3, 9), 7), (p2[2], (3, 9), 11), (p2[4], (9, 10), 6),
        (p2[4], (0, 1), 2), (p2[0], (5, 7), 6),
    ]
    a = state(n, 12)
    hots = check_lists(qc, n, a, [gates, gates[::-1]])
    assert hots == [0xF00] * len(hots) and len(hots) >= 4           # only the budget splits
    hot_only = [g for g in gates if min(parts(g)[1]) >= 8]
    assert len(hot_only) >= 8
    assert check_lists(qc, n, a, [hot_only], chained=False) == [0xF00]                    # the variant without LDS
    # every pair of hot targets, both orders: the register swaps to j's bits 0 and 1 and back
    pairs = [(p2[(q0 + q1) % 2 * 4], (q0, q1)) for q0, q1 in itertools.permutations(range(8, 12), 2)]
    for c in (None, 3, 8, 9, 10, 11):
        with_c = [g if c is None or c in g[1] else g + (c,) for g in pairs]
        check_lists(qc, n, a, [with_c], chained=False)


# ---- tiles that are not the low 12 bits -------------------------------------------------------------------------------------

def hot_of(qubits):
    return sum(1 << q for q in qubits)


@pytest.mark.parametrize("hot", [(9, 10, 11, 12), (8, 10, 11, 12)], ids=["9-12", "8,10-12"])
def test_two_tiles_one_bit_outside(qc, hot):
    n = 13
    outside = [q for q in range(8, 13) if q not in hot][0]          # a base bit: qubit 8 or 9
    p1, p2 = pool1(qc), pool2(qc)
    gates = [
        (p2[0], (hot[0], hot[1])), (p2[4], (hot[3], hot[2])),       # all four hot bits
        (p1[0], hot[0], outside), (p1[3], 3, outside), (p2[0], (5, hot[2]), outside), (p2[4], (hot[1], hot[3]), outside),
        (p1[1], hot[3]), (p1[2], 6, hot[1]), (p2[1], (hot[0], 0)), (p2[3], (7, 2), hot[3]), (p1[4], hot[2], 4),
        (p2[0], (hot[0], hot[3]), hot[1]), (p1[5], hot[1], hot[2]),
    ]
    assert check_lists(qc, n, state(n, 13), [gates, gates[::-1]]) == [hot_of(hot)] * 2
    hot_only = [g for g in gates if min(parts(g)[1]) >= 8]
    assert check_lists(qc, n, state(n, 14), [hot_only]) == [hot_of(hot)]


def test_scattered_hot_set_a_fifth_hot_bit_and_a_budget_split(qc):
    n = 16
    hot = (8, 11, 13, 15)
    H = hot_of(hot)
    outside = (9, 10, 12, 14)
    rs = np.random.RandomState(16)
    p1, p2 = pool1(qc), pool2(qc)
    a = state(n, 16)
    run1 = [(p2[0], (15, 8)), (p2[4], (11, 13))] + random_gates(qc, rs, n, 5, targets=list(range(8)) + list(hot))
    run1 += [(p1[0], 13, 9), (p2[0], (2, 15), 14), (p1[3], 5, 12), (p2[4], (8, 13), 10)]      # controls on every base bit
    assert sum(1 if len(parts(g)[1]) == 1 else 4 for g in run1) <= qc.gate_batch_width()
    assert check_lists(qc, n, a, [run1], chained=False) == [H]
    # a fifth hot bit arrives mid-list
    run2 = run1[:6] + [(p1[1], 9), (p2[0], (12, 9)), (p1[2], 4, 15)] + random_gates(qc, rs, n, 4, targets=(0, 5, 9, 12))
    hots = check_lists(qc, n, a, [run2], chained=False)
    assert len(hots) == 2 and hots[0] == H and hots[1] & 0x1200 == 0x1200
    # the budget closes a pass: eleven two-target gates inside one tile
    run3 = [(p2[k % len(p2)], (hot[k % 4], (3 * k) % 8) if k % 3 else (hot[k % 4], hot[(k + 1) % 4])) for k in range(11)]
    assert qc.gate_batch_width() == 40
    hots = check_lists(qc, n, a, [run3], chained=False)
    assert len(hots) == 2 and hots[0] == H                          # ten of them are the 40 units


# ---- more units than workgroups -----------------------------------------------------------------------------------------------

def ry(theta):
    c, s = math.cos(theta / 2), math.sin(theta / 2)
    return np.array([[c, -s], [s, c]], dtype=complex)


def ansatz_layer(qc, n):
    """ry on every qubit, then CNOT(q, q + 1) along the chain"""
    return [(ry(0.1 + 0.07 * q), q) for q in range(n)] + [(qc.GATES2["CNOT"], (q, q + 1)) for q in range(n - 1)]


def test_ansatz_layer_with_more_than_one_unit_per_workgroup(qc):
    """the grid is capped at 2048 workgroups (prot_grid_cap): n = 25 has 2^13 tiles, so a workgroup walks four units"""
    n = 25
    gates = ansatz_layer(qc, n)
    with qc.Register(n, 0) as reg, qc.Register(n, 0) as twin:
        reg.fill_random(5); twin.fill_random(5)
        hots = run_batch(qc, reg, gates)
        assert len(hots) <= len(gates) // 4 and (1 << (n - 12)) > 2048
        call_loop(qc, twin, gates)
        got, want = bits(reg.read()), bits(twin.read())
    assert np.array_equal(got, want)


def test_grid_caps_that_do_not_divide_the_units(qc):
    """prot_grid_cap = 1 and 3 at n = 14: one workgroup walks all four units, and three share them unevenly"""
    n = 14
    a = state(n, 19)
    rs = np.random.RandomState(14)
    lists = [random_gates(qc, rs, n, 9, targets=list(range(8)) + [8, 10, 11, 13]), random_gates(qc, rs, n, 9, targets=(9, 10, 12, 13))]
    try:
        for cap in (1, 3):
            qc.tune(prot_grid_cap=cap)
            check_lists(qc, n, a, lists, chained=False)
    finally:
        qc.tune(prot_grid_cap=2048)


# ---- lazy forms and modes, against a twin register that runs the loop of the four calls ----------------------------------------

def list_14(qc):
    p1, p2 = pool1(qc), pool2(qc)
    return [(p1[0], 13), (p2[0], (12, 1)), (p1[2], 0, 9), (p2[1], (4, 13), 8), (p1[3], 10), (p2[4], (9, 11)), (p1[4], 6, 13), (p2[3], (3, 2))]


def test_pending_basis_state(qc):
    L, M = 10, 4
    gates = list_14(qc)
    with qc.Register(L, M) as reg, qc.Register(L, M) as twin:
        qc.reset_register(reg); qc.reset_register(twin)             # pending basis state |1>
        assert reg.expectation((0, 0)) == 1.0 and reg.expectation_stats() == (2, 0), "the basis state is still pending"
        run_batch(qc, reg, gates)
        call_loop(qc, twin, gates)
        got = reg.read()
        same(got, twin.read())
    e = np.zeros(2 << (L + M)); e[2] = 1.0
    same(got, ref_loop(e, L + M, gates))


def test_compact_result_is_expanded_first(qc):
    L, M, Cn, a = 15, 5, 21, 2                                      # (the compact chain runs from n = 20 on)
    p1, p2 = pool1(qc), pool2(qc)
    gates = [(p1[0], 19), (p2[0], (2, 17)), (p1[2], 5, 12), (p2[4], (8, 9), 0), (p1[3], 3)]
    with qc.Register(L, M) as reg, qc.Register(L, M) as twin:
        for r in (reg, twin):
            qc.reset_register(r); qc.quantum_computation(Cn, a, r)
        run_batch(qc, reg, gates)
        call_loop(qc, twin, gates)
        got, want = bits(reg.read()), bits(twin.read())
        qc.reset_register(twin); qc.quantum_computation(Cn, a, twin)
        before = bits(twin.read())
    assert np.array_equal(got, want) and not np.array_equal(got, before)


@pytest.mark.parametrize("mode", [1, 2])
def test_queued_gates_are_flushed_first(qc, mode):
    L, M = 10, 4
    n = L + M
    gates = list_14(qc)
    with qc.Register(L, M) as reg, qc.Register(L, M) as twin:
        for r in (reg, twin):
            r.set_fusion(mode)
            r.fill_random(8)

        def queue(r):
            for q in (0, 3, n - 1):
                qc.hadamard_gate(q, r)
            qc.c_phase_shift_gate(3, n - 1, 0.7, r)

        queue(reg)
        s0 = reg.fusion_stats()
        reg.flush()
        flush_counts = tuple(x - y for x, y in zip(reg.fusion_stats(), s0))
        assert flush_counts != (0, 0)
        queue(twin); twin.flush()
        queue(reg); queue(twin)
        before = reg.fusion_stats()
        run_batch(qc, reg, gates)
        assert tuple(x - y for x, y in zip(reg.fusion_stats(), before)) == flush_counts, "nothing is counted for the gates"
        call_loop(qc, twin, gates)
        qc.hadamard_gate(1, reg); qc.hadamard_gate(1, twin)         # queued behind it
        same(reg.read(), twin.read())


def test_nonfinite_register(qc, ob):
    n = 6
    a = state(n, 21)
    a[2 * 37] = np.inf
    a[2 * 5] = -0.0
    p1, p2 = pool1(qc), pool2(qc)
    gates = [(p1[0], 2), (p1[1], 0, 5), (p2[1], (1, 4)), (p2[0], (5, 3), 0), (p1[2], 5, 2), (p2[3], (0, 2), 1), (p1[4], 3)]
    m = RegisterModel(ob, n, 0)
    with qc.Register(n, 0) as reg:
        reg.write(a); m.write(a)
        qc.gate_batch(gates, reg)
        assert reg.gate_batch_stats() == (len(gates), 0)            # gate by gate, through the calls' own strict paths
        want = ref_loop(a, n, gates)
        assert np.any(np.isnan(want))
        same_with_nans(reg.read(), want)
        m.a = want
        assert m.holds_nonfinite()
        qc.hadamard_gate(2, reg); m.hadamard_gate(2)                # the flag is kept: still the strict gate, the oracle's products
        same_with_nans(reg.read(), m.a)


# ---- arguments --------------------------------------------------------------------------------------------------------------

def records(qc, gates):
    from quantumcomputer_amd import _lib
    recs = (_lib.Gate * len(gates))()
    for rec, g in zip(recs, gates):
        U, t, c = parts(g)
        u = one_qubit_ref.matrix8(U) if len(t) == 1 else two_qubit_ref.matrix32(U)
        rec.ntargets, rec.control, rec.qubit0, rec.qubit1 = len(t), (-1 if c is None else c), t[0], (t[1] if len(t) == 2 else 0)
        rec.u[:u.size] = u.tolist()
    return recs


def test_refusals_in_their_order_touch_nothing(qc):
    lib = qc.lib()
    batch = lib.qcx_gate_batch
    p1, p2 = pool1(qc), pool2(qc)
    good = [(p1[0], 1), (p2[0], (11, 3)), (p1[2], 7, 2), (p2[1], (0, 5), 9), (p1[3], 8)]
    err = lambda: lib.qcx_last_error().decode()
    with qc.Register(12, 0) as reg:
        reg.set_fusion(1)
        reg.fill_random(1)
        a0 = reg.read()
        r = records(qc, good); r[2].u[8] = 5.0; r[0].qubit1 = 99    # a one-target gate is its first 8 doubles and qubit0
        assert batch(reg._h, 5, r) == 0
        same(reg.read(), ref_loop(a0, 12, good))
        run_batch(qc, reg, good[:2])
        after = bits(reg.read())
        qc.hadamard_gate(4, reg)                                    # one gate in the queue
        stats, queued = reg.gate_batch_stats(), reg.fusion_stats()
        assert stats == (1, 2)
        assert batch(None, 5, records(qc, good)) == 2               # QCX_BAD_ARGUMENTS
        assert batch(reg._h, 5, None) == 2
        r = records(qc, good); r[3].ntargets = 3; r[0].qubit0 = 12; r[1].u[0] = 2.0
        assert batch(reg._h, 5, r) == 2 and "gate 3" in err()       # the target count before any matrix and any qubit
        r[3].ntargets = 0
        assert batch(reg._h, 5, r) == 2 and "gate 3" in err()
        r[3].ntargets = 2
        assert batch(reg._h, 5, r) == 2 and "gate 1" in err() and "component 0" in err()      # a matrix before any qubit
        for bad in (float("nan"), float("inf"), -1.0000001):
            r = records(qc, good); r[4].qubit0 = 12; r[1].u[31] = bad
            assert batch(reg._h, 5, r) == 2 and "gate 1" in err() and "component 31" in err()
        for field, value in (("qubit0", 12), ("qubit0", 3), ("qubit1", 1 << 31), ("control", 12), ("control", 11), ("control", 3)):
            r = records(qc, good); setattr(r[1], field, value)
            assert batch(reg._h, 5, r) == 6 and "gate 1" in err(), (field, value)      # QCX_BAD_QUBIT
        r = records(qc, good); r[4].control = 8
        assert batch(reg._h, 5, r) == 6 and "gate 4" in err()
        assert reg.gate_batch_stats() == stats and reg.fusion_stats() == queued, "state and queue untouched"
        with pytest.raises(ValueError):
            qc.gate_batch([(p1[0], (1, 2))], reg)                   # a 2x2 matrix on two targets
        with pytest.raises(ValueError):
            qc.gate_batch([(p1[0], (1, 2, 3))], reg)
        assert reg.fusion_stats() == queued
        want = ref_loop(ref_loop(after.view(np.float64), 12, [(qc.GATES["H"], 4)]), 12, [])
        got = reg.read()
        assert np.max(np.abs(got - want)) <= 1e-15                  # (the queued Hadamard, flushed by the read, and nothing else)
        # the launch alone: a hot mask that is not the plan's, or does not hold a gate's high target, is refused
        reg.set_fusion(0)
        dev = C.c_void_p(lib.qcx_device_pointer(reg._h))
        reg.synchronize()
        held = bits(reg.read())
        run = lib.qcx_shard_gate_run
        one = records(qc, [(p1[0], 8)])
        assert run(None, 12, 0xF00, 1, one, None) == 2
        assert run(dev, 12, 0x700, 1, one, None) == 2
        assert run(dev, 12, 0xF01, 1, one, None) == 2
        assert run(dev, 12, 0xF00, 0, one, None) == 2
        assert run(dev, 13, 0x1E00, 1, one, None) == 2              # qubit 8 is outside that tile
        assert run(dev, 12, 0xF00, 11, records(qc, [(p2[0], (0, 1))] * 11), None) == 2      # 44 units
        one[0].qubit0 = 12
        assert run(dev, 12, 0xF00, 1, one, None) == 6
        assert np.array_equal(bits(reg.read()), held)
    with qc.Register(13, 0, shards=2, devices=[0, 0]) as sh:        # two virtual shards on device 0
        sh.fill_random(3)
        before = bits(sh.read())
        assert batch(sh._h, 5, records(qc, good)) == 7              # QCX_UNSUPPORTED
        r = records(qc, good); r[0].qubit0 = 13
        assert batch(sh._h, 5, r) == 6                              # the qubits are looked at first
        assert np.array_equal(bits(sh.read()), before)


def test_no_gates(qc):
    n = 14
    gates = list_14(qc)
    with qc.Register(n, 0) as reg, qc.Register(n, 0) as twin:
        for r in (reg, twin):
            r.set_fusion(1)
            r.fill_random(2)
        run_batch(qc, reg, gates[:2]); call_loop(qc, twin, gates[:2])
        qc.hadamard_gate(4, reg); qc.hadamard_gate(4, twin)
        before = reg.fusion_stats()
        assert qc.lib().qcx_gate_batch(reg._h, 0, None) == 0
        qc.gate_batch([], reg)
        assert reg.fusion_stats() == before, "queued gates stay queued"
        assert reg.gate_batch_stats() == (0, 0)
        same(reg.read(), twin.read())


def test_the_shard_form_is_the_launch_alone(qc):
    n = 13
    lib = qc.lib()
    p1, p2 = pool1(qc), pool2(qc)
    gates = [(p2[0], (12, 9)), (p1[0], 3, 8), (p2[1], (6, 11), 10), (p1[3], 11)]
    with qc.Register(n, 0) as reg:
        reg.fill_random(2)
        a = reg.read()
        dev = C.c_void_p(lib.qcx_device_pointer(reg._h))
        reg.synchronize()
        assert lib.qcx_shard_gate_run(dev, n, 0x1A00 | 0x400, 4, records(qc, gates), None) == 0      # (the default stream: ordered with the register's)
        same(reg.read(), ref_loop(a, n, gates))


# ---- physics ----------------------------------------------------------------------------------------------------------------

def test_forward_qft_then_the_inverse_gives_the_state_back(qc):
    """the adjoint of inverse_QFT's own gate sequence, as a gate list: H and c_one_qubit_gate(phase(-theta))"""
    n = 13
    H = qc.GATES["H"]
    gates = []
    for l in range(n):
        gates += [(qc.phase(-math.pi / (1 << (l - k))), k, l) for k in range(l)] + [(H, l)]
    a = state(n, 31)
    with qc.Register(n, 0) as reg:
        reg.write(a)
        run_batch(qc, reg, gates)
        mid = reg.read()
        qc.inverse_QFT(reg)
        got = reg.read()
    assert np.max(np.abs(mid - a)) > 1e-3
    assert np.max(np.abs(got - a)) <= 1e-12 * np.max(np.abs(a))


def test_hadamards_give_hadamard_gates_bits(qc):
    n = 13
    with qc.Register(n, 0) as reg, qc.Register(n, 0) as twin:
        reg.fill_random(4); twin.fill_random(4)
        run_batch(qc, reg, [(qc.GATES["H"], q) for q in range(n)])
        for q in range(n):
            qc.hadamard_gate(q, twin)
        same(reg.read(), twin.read())
