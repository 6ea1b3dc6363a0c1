"""CPU: tests/multi_qubit_ref.py, the definition of qcx_mc_multi_qubit_gate, against everything it must agree with: the
definitions of the one- and two-qubit gates under a control mask (bit for bit), the kron and controlled embeddings of a 4x4
matrix as 8x8 ones (bit for bit), the dense operator in extended precision (to a derived bound), the permutation definition (bit
for bit), the formula on -0, Inf and NaN, and fused_matrix against the loop of the small definitions.  No GPU needed."""
import itertools

import numpy as np
import pytest

import mc_gate_ref
import multi_qubit_ref as mq
import permutation_ref
from bitwise import random_unitary, same, same_with_nans

U53 = 2.0 ** -53


def finite_state(n, seed):
    """a random state of n qubits with no zero component"""
    rs = np.random.RandomState(seed)
    a = rs.standard_normal(2 << n)
    a[a == 0] = 0.5
    return a / np.sqrt(np.sum(a * a))


def row_bound(k, amax):
    """What a row of 2^k columns may differ by from the exact sum, per component, to first order: every column costs four
    roundings -- two products, their difference (or sum), the accumulation -- each at most 2^-53 relative to a quantity that a
    unitary (every |m_rc| <= 1) keeps of the order of max|amp|:  2^k * 4 * 2^-53 * max|amp|."""
    return (1 << k) * 4 * U53 * amax


def test_k1_and_k2_are_the_mc_definitions():
    forms = mc_gate_ref.forms1(4) + mc_gate_ref.forms2(4)
    assert len(forms) == 216
    state = finite_state(4, 1)
    state[3] = -0.0; state[8] = 0.0; state[17] = np.inf; state[20] = np.nan
    for j, (targets, cm, cv) in enumerate(forms):
        U = random_unitary(100 + j, 1 << len(targets))
        if j % 5 == 0:
            U = U.copy(); U[0, -1] = 0.0; U[-1, 0] = -0.0
        same_with_nans(mq.apply(state, 4, targets, U, cm, cv), mc_gate_ref.apply(state, 4, targets, U, cm, cv), (targets, cm, cv))
    fin = finite_state(4, 2)
    for j, (targets, cm, cv) in enumerate(forms):
        U = random_unitary(400 + j, 1 << len(targets))
        same(mq.apply(fin, 4, targets, U, cm, cv), mc_gate_ref.apply(fin, 4, targets, U, cm, cv), (targets, cm, cv))


def test_kron_and_controlled_embeddings_for_every_ordered_triple():
    """kron(I2, U4) on (t0, t1, t2) is U4 on (t0, t1): the eight-column rows hold U4's four entries and four exact zeros, whose
    products are +-0 and change no sum of a finite state without -0; controlled(U4) likewise fires where t2 reads 1 and has the
    identity's rows (one 1 and seven zeros) elsewhere"""
    n = 5
    state = finite_state(n, 3)
    for j, (t0, t1, t2) in enumerate(itertools.permutations(range(n), 3)):
        U4 = random_unitary(700 + j, 4)
        same(mq.apply(state, n, (t0, t1, t2), np.kron(np.eye(2), U4)), mc_gate_ref.apply2(state, n, t0, t1, U4), (t0, t1, t2))
        cU = np.eye(8, dtype=complex); cU[4:, 4:] = U4
        same(mq.apply(state, n, (t0, t1, t2), cU), mc_gate_ref.apply2(state, n, t0, t1, U4, 1 << t2, 1 << t2), ("controlled", t0, t1, t2))
        free = [q for q in range(n) if q not in (t0, t1, t2)]
        cm, cv = (1 << free[0]) | (1 << free[1]), 1 << free[j % 2]
        same(mq.apply(state, n, (t0, t1, t2), np.kron(np.eye(2), U4), cm, cv), mc_gate_ref.apply2(state, n, t0, t1, U4, cm, cv), ("masked", t0, t1, t2))


@pytest.mark.parametrize("k", [3, 4, 5])
def test_against_the_dense_operator_in_extended_precision(k):
    n = 6
    rs = np.random.RandomState(k)
    worst = 0.0
    for rep in range(6):
        targets = [int(q) for q in rs.permutation(n)[:k]]
        free = [q for q in range(n) if q not in targets]
        cm = sum(1 << c for c in free[:rep % (len(free) + 1)])
        cv = cm & int(rs.randint(1 << n))
        U = random_unitary(50 * k + rep, 1 << k)
        state = finite_state(n, 10 * k + rep)
        got = mq.apply(state, n, targets, U, cm, cv).view(np.complex128)
        op = mq.dense_operator(n, targets, U, cm, cv).astype(np.clongdouble)
        want = op @ state.view(np.complex128).astype(np.clongdouble)
        err = float(max(np.max(np.abs((got - want).real)), np.max(np.abs((got - want).imag))))
        bound = row_bound(k, float(np.max(np.abs(state))))
        print(f"k={k} targets={targets} mask={cm:#x} values={cv:#x}: max component error {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (k, targets, cm, cv, err, bound)
        worst = max(worst, err / bound)
    assert worst > 0.0


def test_a_permutation_matrix_is_the_permutation_definition():
    """one 1 per row, every other product an exact +-0: on a finite state pure movement with -0 made +0, as permutation_ref has it"""
    rs = np.random.RandomState(9)
    n = 7
    state = finite_state(n, 9)
    state[5] = -0.0; state[40] = 0.0
    for k, first in [(1, 0), (2, 3), (3, 0), (3, 4), (4, 2), (5, 0), (5, 2)]:
        perm = rs.permutation(1 << k)
        U = np.zeros((1 << k, 1 << k))
        U[perm, np.arange(1 << k)] = 1.0                        # |c> -> |perm[c]>
        free = [q for q in range(n) if not first <= q < first + k]
        for cm, cv in [(0, 0), (1 << free[0], 1 << free[0]), ((1 << free[0]) | (1 << free[-1]), 1 << free[-1])]:
            same(mq.apply(state, n, range(first, first + k), U, cm, cv), permutation_ref.apply(state, n, first, k, perm, cm, cv), (k, first, cm, cv))


def test_minus_zero_inf_and_nan_by_the_formula():
    n, targets, cm, cv = 5, (3, 0, 4), 0b00100, 0b00100
    U = random_unitary(77, 8)
    U = U.copy(); U[2, 5] = 0.0
    state = finite_state(n, 5)
    re, im = state[0::2], state[1::2]
    re[0b00100] = -0.0; im[0b00101] = np.inf; re[0b11100] = np.nan          # in firing groups
    re[0b00001] = -0.0; im[0b01000] = -np.inf; im[0b10011] = np.nan; im[0b00010] = -0.0   # outside them
    got = mq.apply(state, n, targets, U, cm, cv)
    m = mq.ascending_matrix(targets, U)
    want = np.empty_like(state)
    st = sorted(targets)
    with np.errstate(all="ignore"):
        for i in range(1 << n):
            if (i & cm) != cv:
                x, y = re[i], im[i]
                want[2 * i], want[2 * i + 1] = 0.0 + ((1.0 * x) - (0.0 * y)), 0.0 + ((1.0 * y) + (0.0 * x))
                continue
            r = sum(((i >> st[j]) & 1) << j for j in range(3))
            i0 = i & ~sum(1 << q for q in st)
            sr, si = np.float64(0.0), np.float64(0.0)
            for c in range(8):
                j = i0 | sum(((c >> b) & 1) << st[b] for b in range(3))
                sr = sr + ((m[r, c, 0] * re[j]) - (m[r, c, 1] * im[j]))
                si = si + ((m[r, c, 0] * im[j]) + (m[r, c, 1] * re[j]))
            want[2 * i], want[2 * i + 1] = sr, si
    same_with_nans(got, want)
    g = got.view(np.complex128)
    assert np.signbit(state[2 * 0b00001]) and not np.signbit(got[2 * 0b00001])          # an identity row turns -0 into +0
    assert np.isnan(g[0b01000].real) and np.isinf(g[0b01000].imag)                      # 0 * Inf poisons the other component
    assert np.all(np.isnan(got[[2 * i + c for i in range(32) if (i & cm) == cv and (i & 0b00110) == 0b00100 for c in (0, 1)]]))


X = np.array([[0, 1], [1, 0]], dtype=complex)
Z = np.diag([1, -1]).astype(complex)
S = np.diag([1, 1j])
CNOT = np.array([[1, 0, 0, 0], [0, 0, 0, 1], [0, 0, 1, 0], [0, 1, 0, 0]], dtype=complex)      # qubit0 controls qubit1
SWAP = np.eye(4, dtype=complex)[[0, 2, 1, 3]]


def test_fused_matrix_of_dyadic_gates_is_exact(qc):
    """X, CNOT, SWAP, Z and S have one entry of {1, -1, i} per row: every product of the block and of the loop is exact, so on a
    state without zeros the block and the gate-by-gate definitions agree bit for bit"""
    n = 6
    targets = (4, 1, 5, 2)
    gates = [(X, 1), (CNOT, (4, 2)), (S, 5), (SWAP, (1, 5)), (Z, 2, 4), (CNOT, (5, 1), 2), (S, 4, 1), (X, 2), (SWAP, (2, 4), 5)]
    F = qc.fused_matrix(gates, targets)
    assert F.shape == (16, 16) and np.array_equal(np.abs(F).sum(axis=1), np.ones(16))
    state = finite_state(n, 11)
    same(mq.apply(state, n, targets, F), mq.apply_gate_list(state, n, gates))
    same(mq.apply(state, n, targets, F, 1 << 3, 0), _loop_under(state, n, gates, 1 << 3, 0))
    with pytest.raises(ValueError):
        qc.fused_matrix([(X, 0)], targets)
    with pytest.raises(ValueError):
        qc.fused_matrix([(X, 1, 3)], targets)
    with pytest.raises(ValueError):
        qc.fused_matrix(gates, (1, 1, 2))


def _loop_under(state, n, gates, cm, cv):
    """the loop of the small definitions with every gate under the extra controls (cm, cv) as well"""
    for g in gates:
        tg = tuple(g[1]) if np.ndim(g[1]) else (g[1],)
        c = (1 << g[2]) if len(g) > 2 else 0
        state = mc_gate_ref.apply(state, n, tg, g[0], cm | c, cv | c)
    return state


def test_fused_matrix_of_random_gates_to_the_derived_bound(qc):
    """The block and the loop are the same operator with different roundings.  Per component, to first order in 2^-53 and with
    max|amp| for every magnitude: the loop's gate g adds row_bound(k_g); the block's one call adds row_bound(k); and the block's
    matrix carries the roundings of its own products -- each of the G numpy products rounds an entry as a row of 2^k columns
    does, and an entry error e moves an amplitude by at most 2^k e max|amp| -- so G * row_bound(k) more.  The state's norm is kept
    by unitaries, so max|amp| <= 1 serves for every stage."""
    n, k = 6, 4
    targets = (5, 0, 3, 2)
    rs = np.random.RandomState(21)
    gates = []
    for j in range(10):
        if j % 2:
            q = [int(x) for x in rs.permutation(targets)[:3]]
            gates.append((random_unitary(900 + j, 4), (q[0], q[1])) if j % 4 == 1 else (random_unitary(900 + j, 4), (q[0], q[1]), q[2]))
        else:
            q = [int(x) for x in rs.permutation(targets)[:2]]
            gates.append((random_unitary(900 + j, 2), q[0]) if j % 4 == 0 else (random_unitary(900 + j, 2), q[0], q[1]))
    F = qc.fused_matrix(gates, targets)
    F = np.clip(F.real, -1, 1) + 1j * np.clip(F.imag, -1, 1)
    state = finite_state(n, 22)
    got, want = mq.apply(state, n, targets, F), mq.apply_gate_list(state, n, gates)
    err = float(np.max(np.abs(got - want)))
    bound = sum(row_bound(1 if np.ndim(g[1]) == 0 else len(g[1]), 1.0) for g in gates) + row_bound(k, 1.0) + len(gates) * row_bound(k, 1.0)
    print(f"fused block against the loop of {len(gates)} gates: max component difference {err:.3e}, bound {bound:.3e}")
    assert 0.0 < err <= bound
