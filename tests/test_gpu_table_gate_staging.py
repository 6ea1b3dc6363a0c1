"""GPU: the staged upload diagonal_gate, permutation_gate and multi_qubit_gate share (host array -> pinned buffer -> device
buffer on the register's stream, an event before the pinned buffer is written again; StagedUpload in csrc/qcx_api.hip).  The
three calls are interleaved on one register in a fixed seeded order, every caller array is overwritten as soon as its call
returns, the diagonal's table grows and then shrinks again, an identity permutation (no copy, no launch) sits between two real
ones, and one refused call of each kind sits in the middle.  Then the same with two registers alive at once, one of them on a
caller's stream.  Every state must be, bit for bit, what the numpy definitions give (tests/diagonal_ref.py, permutation_ref.py,
multi_qubit_ref.py), and the three *_stats what the plans say of the last accepted call of each kind.

The large table has 2^min(16, n) entries: 2^16 at n = 16, the whole register's 2^13 at n = 13 -- more than the 2^12 the buffer
starts with in either case.  The diagonal over diagonal_host_max_qubits() + 1 qubits is wider than both registers, so what
refuses it is the range check in front of the host form's own limit: a refusal before anything is staged either way."""
import numpy as np
import pytest

import diagonal_ref
import multi_qubit_ref
import permutation_ref
import sequence_replay as sr
from bitwise import random_unitary, same

pytestmark = pytest.mark.gpu

BAD_ARGUMENTS, BAD_QUBIT = 2, 6
_SEQ = {}


def masks_of(rs, n, taken, most=2):
    """up to `most` controls among the qubits not in `taken`, of either polarity"""
    free = [q for q in range(n) if q not in taken]
    cs = [int(q) for q in rs.choice(free, size=min(int(rs.randint(0, most + 1)), len(free)), replace=False)]
    cm = sum(1 << q for q in cs)
    return cm, cm & int(rs.randint(0, 1 << n))


def sequence(n, seed):
    """about 30 calls in a fixed seeded order: [(kind, arguments, expected status)]"""
    rs = np.random.RandomState(seed)

    def diag(num, first=None):
        first = int(rs.randint(0, n - num + 1)) if first is None else first
        return ("diag", (first, num, np.exp(1j * rs.uniform(0, 2 * np.pi, 1 << num))), 0)

    def perm(identity=False):
        num = int(rs.randint(1, 9))
        first = int(rs.randint(0, n - num + 1))
        table = np.arange(1 << num, dtype=np.uint32) if identity else rs.permutation(1 << num).astype(np.uint32)
        return ("perm", (first, num, table) + masks_of(rs, n, range(first, first + num)), 0)

    def multi(k):
        t = tuple(int(q) for q in rs.choice(n, size=k, replace=False))
        U = np.ascontiguousarray(random_unitary(int(rs.randint(1 << 30)), 1 << k).reshape(-1)).view(np.float64).copy()
        return ("multi", (t, U) + masks_of(rs, n, t), 0)

    big = min(16, n)
    twice = np.arange(256, dtype=np.uint32); twice[7] = twice[9]                   # not a bijection
    above = multi(3); above[1][1][5] = 1.5                                         # a matrix component above 1
    wide = qc_host_max() + 1
    ops = [diag(4), perm(), multi(3), diag(big, 0), multi(5), perm(), perm(identity=True), perm(), diag(4),
           ("perm", (2, 8, twice, 0, 0), BAD_ARGUMENTS), perm(),
           (above[0], above[1], BAD_ARGUMENTS), multi(4),
           ("diag", (0, wide, np.zeros(1 << wide, dtype=complex)), BAD_QUBIT), diag(6, 5)]
    kinds = ["multi", "diag", "perm", "perm", "diag", "multi", "diag", "perm", "multi", "diag", "perm", "multi", "diag", "multi", "perm"]
    for kind in kinds:
        ops.append(diag(int(rs.randint(0, 11))) if kind == "diag" else perm() if kind == "perm" else multi(int(rs.randint(3, 6))))
    return ops


def qc_host_max():
    import quantumcomputer_amd
    return quantumcomputer_amd.diagonal_host_max_qubits()


def expected(ob, n, seed):
    """(ops, the state behind each op) for the register that starts as fill_random(seed) leaves it"""
    if (n, seed) not in _SEQ:
        ops = sequence(n, seed)
        a, states = ob.fill_random(n, seed), []
        for kind, args, status in ops:
            if status == 0:
                if kind == "diag":
                    a = diagonal_ref.apply(a, n, *args)
                elif kind == "perm":
                    first, num, table, cm, cv = args
                    a = permutation_ref.apply(a, n, first, num, table, cm, cv)
                else:
                    t, U, cm, cv = args
                    a = multi_qubit_ref.apply(a, n, t, U, cm, cv)
            a.setflags(write=False)
            states.append(a)
        # the arguments are handed to the library as copies (run): these stay as they are
        for _, args, _ in ops:
            for v in args:
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
        _SEQ[(n, seed)] = (ops, states)
    return _SEQ[(n, seed)]


def run(qc, reg, op):
    """one call with caller arrays of its own, overwritten as soon as the call is back; returns the status"""
    kind, args, _ = op
    own = [v.copy() if isinstance(v, np.ndarray) else v for v in args]
    try:
        if kind == "diag":
            qc.diagonal_gate(own[0], own[1], own[2], reg)
        elif kind == "perm":
            qc.permutation_gate(own[0], own[1], own[2], reg, controls=own[3], values=own[4])
        else:
            qc.multi_qubit_gate(own[0], own[1], reg, controls=own[2], values=own[3])
        status = 0
    except qc.QcxError as e:
        status = e.status
    for v in own:
        if isinstance(v, np.ndarray):
            v.fill(3)                     # no table entry, matrix component or permutation value the call could still want
    return status


def check_stats(qc, reg, n, ops):
    last = {kind: [a for k, a, st in ops if k == kind and st == 0][-1] for kind in ("diag", "perm", "multi")}
    first, num, _ = last["diag"]
    st, pl = qc.diagonal_plan(n, first, num)
    assert st == 0 and reg.diagonal_stats() == (pl.form, 1 << num)
    first, num, table, cm, cv = last["perm"]
    st, pl = qc.permutation_plan(n, cm, cv, first, num)
    assert st == 0 and reg.permutation_stats() == (pl.form, int(np.count_nonzero(table != np.arange(1 << num))))
    t, _, cm, cv = last["multi"]
    st, pl = qc.multi_gate_plan(n, cm, cv, t)
    assert st == 0 and reg.multi_qubit_stats() == (pl.form, len(t))


@pytest.mark.parametrize("n", [13, 16])
def test_interleaved_on_one_register(qc, ob, n):
    ops, states = expected(ob, n, 40 + n)
    assert 28 <= len(ops) <= 32 and [st for _, _, st in ops].count(0) == len(ops) - 3
    sizes = [1 << a[1] for k, a, st in ops if k == "diag" and st == 0][:3]
    assert sizes == [16, 1 << min(16, n), 16]
    with qc.Register(n, 0) as reg:
        reg.fill_random(40 + n)
        after_refusal = False
        for j, op in enumerate(ops):
            assert run(qc, reg, op) == op[2], f"call {j}: {op[0]}"
            if after_refusal:                                      # the first accepted call behind a refused one
                same(reg.read(), states[j], f"call {j} ({op[0]}), behind a refused call")
            after_refusal = op[2] != 0
        same(reg.read(), states[-1], "the final state")
        check_stats(qc, reg, n, ops)


def test_two_registers_alternating_one_on_a_callers_stream(qc, ob):
    ctx = {}
    (ops_a, states_a), (ops_b, states_b) = expected(ob, 13, 53), expected(ob, 16, 56)
    with qc.Register(13, 0) as ra, qc.Register(16, 0) as rb:
        sr.set_stream(rb, 1, ctx)                                  # one non-blocking stream of PyTorch's, alive until rb is closed
        ra.fill_random(53); rb.fill_random(56)
        for j, (oa, ob_) in enumerate(zip(ops_a, ops_b)):
            assert run(qc, ra, oa) == oa[2] and run(qc, rb, ob_) == ob_[2], f"call {j}"
        same(ra.read(), states_a[-1], "the register on its own stream")
        same(rb.read(), states_b[-1], "the register on the caller's stream")
        check_stats(qc, ra, 13, ops_a)
        check_stats(qc, rb, 16, ops_b)
        sr.set_stream(rb, 0, ctx)


def test_a_register_that_staged_nothing_closes(qc, ob):
    with qc.Register(13, 0) as reg:
        reg.fill_random(5)
        qc.hadamard_gate(3, reg)
        assert reg.diagonal_stats() == (0, 0) and reg.permutation_stats() == (0, 0) and reg.multi_qubit_stats() == (0, 0)
    with qc.Register(13, 0) as reg:                                # ... and the next one starts empty too
        reg.fill_random(5)
        a = ob.fill_random(13, 5)
        d = np.exp(1j * np.linspace(0, 1, 16))
        qc.diagonal_gate(2, 4, d, reg)
        same(reg.read(), diagonal_ref.apply(a, 13, 2, 4, d))
