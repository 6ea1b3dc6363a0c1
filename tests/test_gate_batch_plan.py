"""CPU: the pass plan of qcx_gate_batch (include/qcx_plan.h: qcx_gate_batch_plan) against the rule restated in a few lines of
Python: a run of consecutive gates shares a pass while their units (1 per one-target gate, 4 per two-target gate) fit the width
and their targets at and above qubit 8 fit four hot bits.  Controls never count.  A gate always fits an empty pass.  No GPU
needed."""
import ctypes as C

import numpy as np
import pytest


def popcount(v):
    return bin(v).count("1")


def plan_rule(gates, n, width):
    """gates: [(target_mask, units), ...] -> (pass_of_gate, [hot_mask, ...])"""
    nhot = min(4, max(n, 8) - 8)
    pass_of, passes = [], []
    H, used = None, 0                                               # H is None: no pass is open

    def close():
        nonlocal H
        q = 8
        while popcount(H) < nhot:
            if not H >> q & 1:
                H |= 1 << q
            q += 1
        passes.append(H)
        H = None

    for mask, units in gates:
        hx = mask >> 8 << 8
        if H is not None and not (used + units <= width and popcount(H | hx) <= 4):
            close()
        if H is None:
            H, used = 0, 0                                          # (the gate that opens a pass is not asked whether it fits)
        H |= hx
        used += units
        pass_of.append(len(passes))
    if H is not None:
        close()
    return pass_of, passes


def entries(gates, control=None):
    """the (U, targets[, control]) entries gate_batch_plan takes, from (target_mask, units) pairs; U is not looked at"""
    out = []
    for mask, units in gates:
        t = tuple(q for q in range(64) if mask >> q & 1)
        out.append((None, t) if control is None else (None, t, control))
    return out


def check_plan(qc, gates, n, width):
    got_of, got = qc.gate_batch_plan(entries(gates), n, width)
    want_of, want = plan_rule(gates, n, width)
    assert got_of == want_of and got == want, (n, width, gates)
    # what the kernel relies on, stated without the rule
    assert got_of == sorted(got_of) and set(got_of) == set(range(len(got)))
    nhot = min(4, max(n, 8) - 8)
    for p, hot in enumerate(got):
        members = [gates[k] for k in range(len(gates)) if got_of[k] == p]
        assert members and (sum(u for _, u in members) <= width or len(members) == 1)
        assert popcount(hot) == nhot and hot & 0xFF == 0 and hot >> n == 0
        assert all((m >> 8 << 8) & ~hot == 0 for m, _ in members)   # every target lies inside the tile
    return got_of, got


def one(q):
    return (1 << q, 1)


def two(q0, q1):
    return (1 << q0 | 1 << q1, 4)


def test_width_is_a_build_constant_that_fits_the_kernel_arguments(qc):
    W = qc.gate_batch_width()
    assert W >= 4 and 80 * W + 64 <= 4096


@pytest.mark.parametrize("width", [1, 4, 5, 40])
def test_random_lists(qc, width):
    rs = np.random.RandomState(width)
    for n in range(1, 35):
        check_plan(qc, [], n, width)
        for _ in range(6):
            gates = []
            for _ in range(int(rs.randint(1, 90))):
                if n >= 2 and rs.randint(0, 3) == 0:
                    q0, q1 = (int(q) for q in rs.choice(n, 2, replace=False))
                    gates.append(two(q0, q1))
                else:
                    lowish = rs.randint(0, 3) == 0                  # often neighbours just above qubit 8, sometimes below
                    gates.append(one(int(rs.randint(0, min(n, 8))) if lowish else int(rs.randint(0, n))))
            check_plan(qc, gates, n, width)


def test_a_gate_always_fits_an_empty_pass(qc):
    of, passes = check_plan(qc, [two(0, 1), one(2), two(9, 3), two(4, 5)], 12, 1)
    assert of == [0, 1, 2, 3] and passes == [0xF00] * 4
    of, _ = check_plan(qc, [one(0), two(0, 1), one(1), one(2)], 12, 4)
    assert of == [0, 1, 2, 2]                                       # 1 + 4 > 4; then 1 + 1 <= 4


def test_the_budget_closes_a_pass(qc):
    W = qc.gate_batch_width()
    for n in (5, 12, 20):
        for run in (W - 1, W, W + 1, 2 * W + 3):
            of, passes = check_plan(qc, [one(3)] * run, n, W)
            assert len(passes) == -(-run // W) and of == [k // W for k in range(run)]
        per = W // 4
        for run in (per, per + 1, 3 * per + 1):
            of, passes = check_plan(qc, [two(1, 4)] * run, n, W)
            assert of == [k // per for k in range(run)]
    of, passes = check_plan(qc, [two(0, 1), one(0), one(1), two(2, 3)], 20, 8)
    assert of == [0, 0, 0, 1] and passes == [0xF00, 0xF00]          # 4 + 1 + 1 + 4 > 8
    of, passes = check_plan(qc, [one(8), one(9), one(10), one(11), one(12)], 20, 4)
    assert of == [0, 0, 0, 0, 1] and passes == [0xF00, 0x1700]      # closed by the budget; the fifth bit opens a tile of its own


def test_a_fifth_hot_bit_closes_a_pass(qc):
    n = 16
    gates = [one(15), two(8, 11), one(13), two(13, 0), two(3, 7), one(10), one(0)]
    of, passes = check_plan(qc, gates, n, 40)
    assert of == [0, 0, 0, 0, 0, 1, 1]
    assert passes == [0xA900, 0x0F00]
    # a two-target gate that would bring bits five and six
    of, passes = check_plan(qc, [one(8), one(9), one(10), two(11, 12), one(8)], n, 40)
    assert of == [0, 0, 0, 1, 1] and passes == [0x0F00, 0x1900 | 0x0200]
    # one high target of the two already hot: it joins
    of, passes = check_plan(qc, [one(8), one(9), one(10), two(10, 12)], n, 40)
    assert of == [0, 0, 0, 0] and passes == [0x1700]


def test_controls_never_constrain(qc):
    n = 20
    gates = [one(8), one(9), one(10), one(11), two(8, 11), one(3)]
    want = qc.gate_batch_plan(entries(gates), n)
    assert want == ([0] * 6, [0xF00])
    for control in (0, 7, 12, 19):
        assert qc.gate_batch_plan(entries(gates, control), n) == want


def test_padding_of_the_hot_set(qc):
    assert check_plan(qc, [one(0)], 30, 40)[1] == [0xF00]
    assert check_plan(qc, [one(29)], 30, 40)[1] == [(1 << 29) | 0x700]
    assert check_plan(qc, [two(8, 9), one(20)], 30, 40)[1] == [(1 << 20) | 0x700]
    assert check_plan(qc, [two(9, 12)], 13, 40)[1] == [0x1200 | 0x100 | 0x400]
    assert check_plan(qc, [two(9, 10), two(11, 12)], 13, 40)[1] == [0x1E00]
    assert check_plan(qc, [one(9)], 10, 40)[1] == [0x300]
    assert check_plan(qc, [one(0)], 3, 40)[1] == [0]


@pytest.mark.parametrize("n", range(1, 13))
def test_up_to_12_qubits_the_tile_is_the_register(qc, n):
    W = qc.gate_batch_width()
    rs = np.random.RandomState(n)
    gates = [one(int(q)) for q in rs.randint(0, n, 2 * W + 5)]
    of, passes = check_plan(qc, gates, n, W)
    whole = ((1 << n) - 1) >> 8 << 8
    assert passes == [whole] * len(passes) and len(passes) == -(-len(gates) // W)       # only W splits passes
    assert of == [k // W for k in range(len(gates))]


# ---- the lists tools/time_gate_batch.py times at n = 30 (DESIGN s4.5l quotes these pass counts) ---------------------------------

def timed_lists(n=30):
    ansatz = [one(q) for q in range(n)] + [two(q, q + 1) for q in range(n - 1)]       # ry on every qubit, then CNOT(q, q + 1)
    qft = []
    for t in range(20, 8, -1):                                      # the forward QFT of qubits 9 .. 20: H, then the phases onto it
        qft += [one(t)] + [one(t)] * (t - 9)                        # (c_one_qubit_gate(c, t, phase): the control does not count)
    return {
        "low32": [one(q % 8) for q in range(32)],
        "hot4": [one(q) for q in range(12, 16)],
        "ansatz": ansatz,
        "qft12": qft,
        "bonds10": [two(8 + k % 3, 9 + k % 3) for k in range(10)],
    }


def test_the_timed_lists_at_30_qubits(qc):
    assert qc.gate_batch_width() == 40, "the counts below are those of W = 40"
    lists = timed_lists()
    assert {k: len(v) for k, v in lists.items()} == {"low32": 32, "hot4": 4, "ansatz": 59, "qft12": 78, "bonds10": 10}
    want = {"low32": 1, "hot4": 1, "ansatz": 13, "qft12": 4, "bonds10": 1}      # (from plan_rule above)
    for name, gates in lists.items():
        assert len(plan_rule(gates, 30, 40)[1]) == want[name], name
        of, passes = check_plan(qc, gates, 30, 40)
        assert len(passes) == want[name], (name, len(passes))
    # the ansatz layer: the rotations take a pass per four qubits above 7, the CNOT chain one per three bonds there
    assert check_plan(qc, lists["ansatz"], 30, 40)[1][:6] == [0xF00, 0xF000, 0xF0000, 0xF00000, 0xF000000, 0x30000300]


def test_plan_arguments(qc):
    lib = qc.lib()
    ms, us, of, n = (C.c_uint64 * 2)(1, 1 << 9 | 2), (C.c_uint * 2)(1, 4), (C.c_ulong * 2)(9, 9), C.c_ulong(9)
    hot = (C.c_uint64 * 2)(9, 9)
    plan = lib.qcx_gate_batch_plan
    assert plan(10, 2, ms, us, 0, of, C.byref(n), hot) == 2            # QCX_BAD_ARGUMENTS: width 0
    assert plan(0, 2, ms, us, 4, of, C.byref(n), hot) == 2             # no qubits
    assert plan(41, 2, ms, us, 4, of, C.byref(n), hot) == 2
    assert plan(10, 2, ms, us, 4, of, None, hot) == 2
    assert plan(10, 2, None, us, 4, of, C.byref(n), hot) == 2
    assert plan(10, 2, ms, None, 4, of, C.byref(n), hot) == 2
    assert plan(10, 2, ms, us, 4, None, C.byref(n), hot) == 2
    assert plan(10, 2, ms, us, 4, of, C.byref(n), None) == 2
    for bad in (0, 2, 3, 5):
        us[1] = bad
        assert plan(10, 2, ms, us, 4, of, C.byref(n), hot) == 2        # a unit cost other than 1 or 4
    us[1] = 4
    assert plan(9, 2, ms, us, 4, of, C.byref(n), hot) == 6             # QCX_BAD_QUBIT: bit 9 of 9 qubits
    us[0], us[1] = 4, 4
    assert plan(10, 2, ms, us, 4, of, C.byref(n), hot) == 6            # one target bit, cost 4
    us[0], us[1] = 1, 1
    assert plan(10, 2, ms, us, 4, of, C.byref(n), hot) == 6            # two target bits, cost 1
    ms[0], us[1] = 0, 4
    assert plan(10, 2, ms, us, 4, of, C.byref(n), hot) == 6            # no target at all
    assert list(of) == [9, 9] and n.value == 9 and list(hot) == [9, 9]
    ms[0] = 1
    assert plan(10, 0, None, None, 4, None, C.byref(n), None) == 0 and n.value == 0
    assert plan(10, 2, ms, us, 4, of, C.byref(n), hot) == 0
    assert list(of) == [0, 1] and n.value == 2 and list(hot) == [0x300, 0x300]
    with pytest.raises(ValueError):
        qc.gate_batch_plan([(None, (1, 2, 3))], 10)
    with pytest.raises(qc.QcxError):
        qc.gate_batch_plan([(None, (1, 1))], 10)
