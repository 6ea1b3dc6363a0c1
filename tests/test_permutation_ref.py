"""CPU: tests/permutation_ref.py, the numpy definition of qcx_permutation_gate, against everything that already says what it must
be: its own dense matrix, the mc gates' definition (X, CNOT, Toffoli, SWAP, Fredkin, negative controls included), the oracle's
controlled modular multiply, and the formula of its rows on -0, Inf and NaN; and the table helpers of the package.  No GPU needed."""
import itertools

import numpy as np
import pytest

import mc_gate_ref as mr
import permutation_ref as pr
from bitwise import bits, same, same_with_nans

X = np.array([[0, 1], [1, 0]], dtype=complex)
SWAP = np.eye(4, dtype=complex)[[0, 2, 1, 3]]


def random_state(n, seed):
    rs = np.random.RandomState(seed)
    return rs.uniform(-0.5, 0.5, 2 << n)


def masks(n, first, num, most=2):
    """every control set of up to `most` qubits outside the range, in every polarity"""
    free = [q for q in range(n) if not first <= q < first + num]
    yield 0, 0
    for k in range(1, most + 1):
        for cs in itertools.combinations(free, k):
            for pol in range(1 << k):
                yield sum(1 << c for c in cs), sum(1 << c for j, c in enumerate(cs) if (pol >> j) & 1)


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_apply_is_the_dense_matrix(n):
    rs = np.random.RandomState(n)
    a = random_state(n, 10 + n)
    for first in range(n + 1):
        for num in range(n - first + 1):
            for cm, cv in masks(n, first, num, most=n):
                perm = rs.permutation(1 << num)
                got = pr.apply(a, n, first, num, perm, cm, cv).view(np.complex128)
                d = pr.dense(n, first, num, perm, cm, cv)
                assert np.array_equal(d.sum(0), np.ones(1 << n)) and np.array_equal(d.sum(1), np.ones(1 << n))
                assert np.array_equal(got, d @ a.view(np.complex128)), (n, first, num, cm, cv)      # (one term per row: exact)
                if num:
                    k0 = int(perm[0])                                        # |0> of the range goes to |perm[0]>
                    e = np.zeros(2 << n); e[2 * cv] = 1.0
                    assert pr.apply(e, n, first, num, perm, cm, cv)[2 * (cv | (k0 << first))] == 1.0


@pytest.mark.parametrize("n", [3, 5])
def test_x_cnot_toffoli_swap_fredkin_are_the_mc_gates(n):
    a = random_state(n, 20 + n)
    for q in range(n):
        for cm, cv in masks(n, q, 1):                                        # X, CNOT, Toffoli, each polarity
            same(pr.apply(a, n, q, 1, [1, 0], cm, cv), mr.apply1(a, n, q, X, cm, cv), f"X on {q} under {cm:#x}/{cv:#x}")
    for q in range(n - 1):
        for cm, cv in masks(n, q, 2, most=1):                                # SWAP, Fredkin
            same(pr.apply(a, n, q, 2, [0, 2, 1, 3], cm, cv), mr.apply2(a, n, q, q + 1, SWAP, cm, cv), f"SWAP on {q} under {cm:#x}/{cv:#x}")


@pytest.mark.parametrize("Cn,a,M", [(15, 7, 4), (21, 2, 5)])
def test_the_oracles_controlled_modular_multiply(qc, ob, Cn, a, M):
    n = M + 5
    for ctl in (M, n - 1):                                                   # just above the M register, and well above it
        state = ob.random_state(n, 3 + ctl)
        want = state.copy()
        ob.camodc(want, n, M, Cn, a, ctl)
        got = pr.apply(state, n, 0, M, qc.modmul_table(a, Cn, M), 1 << ctl, 1 << ctl)
        same(got, want, f"C={Cn} a={a} M={M} ctl={ctl}")
        assert not np.array_equal(bits(got), bits(state))


def test_finite_states_are_moved_and_negative_zero_becomes_positive():
    n, first, num = 6, 1, 3
    rs = np.random.RandomState(5)
    perm = rs.permutation(1 << num)
    a = random_state(n, 6)
    a[rs.randint(0, a.size, a.size // 3)] = -0.0
    a[rs.randint(0, a.size, 8)] = 0.0
    a[7] = 5e-324; a[9] = -1.7976931348623157e308                            # a subnormal and the largest double move unchanged
    for cm, cv in ((0, 0), (1, 1), (1 << 5, 0), (0x21, 0x20)):
        got = pr.apply(a, n, first, num, perm, cm, cv)
        assert not np.any((got == 0) & np.signbit(got))
        src = pr.source(n, first, num, perm, cm, cv)
        moved = a.view(np.complex128)[src].view(np.float64)
        same(got, np.where(moved == 0, 0.0, moved), "pure movement, +0 for every zero")
        assert np.array_equal(got[got != 0], moved[moved != 0])


def test_inf_and_nan_poison_the_other_component():
    n, first, num = 5, 2, 2
    perm = [2, 0, 3, 1]
    a = random_state(n, 7)
    a[2 * 3] = np.inf                   # real part of amplitude 3: its imaginary part becomes 0 * inf = NaN
    a[2 * 9 + 1] = -np.inf
    a[2 * 20] = np.nan
    a[2 * 30] = np.inf; a[2 * 30 + 1] = np.inf
    for cm, cv in ((0, 0), (1, 1), (1, 0), (0x10, 0x10)):
        got = pr.apply(a, n, first, num, perm, cm, cv)
        src = pr.source(n, first, num, perm, cm, cv)
        x = a.view(np.complex128)[src]
        with np.errstate(invalid="ignore"):
            want_re = 0.0 + ((1.0 * x.real) - (0.0 * x.imag))
            want_im = 0.0 + ((1.0 * x.imag) + (0.0 * x.real))
        same_with_nans(got[0::2], want_re)
        same_with_nans(got[1::2], want_im)
        dst = {int(np.flatnonzero(src == s)[0]): s for s in (3, 9, 20, 30)}
        g = got.view(np.complex128)
        for d, s in dst.items():                                             # identity rows and moved rows alike
            if s == 3:
                assert g[d].real == np.inf and np.isnan(g[d].imag)
            elif s == 9:
                assert np.isnan(g[d].real) and g[d].imag == -np.inf
            else:
                assert np.isnan(g[d].real) and np.isnan(g[d].imag)
        finite = np.ones(1 << n, bool); finite[list(dst)] = False
        assert np.all(np.isfinite(got.view(np.complex128)[finite]))


def test_a_table_and_its_inverse_restore_the_bits():
    n = 7
    rs = np.random.RandomState(8)
    a = random_state(n, 9)
    for first, num, cm, cv in ((0, 7, 0, 0), (2, 4, 0x41, 0x01), (3, 1, 0x06, 0x06), (5, 0, 1, 1)):
        perm = rs.permutation(1 << num)
        b = pr.apply(a, n, first, num, perm, cm, cv)
        same(pr.apply(b, n, first, num, pr.inverse(perm, num), cm, cv), a)


def test_table_helpers(qc):
    # modmul: k -> a k mod C below C, the identity above
    t = qc.modmul_table(7, 15, 4)
    assert t.dtype == np.uint32 and list(t) == [(7 * k) % 15 for k in range(15)] + [15]
    assert list(qc.modmul_table(2, 21, 5))[:21] == [(2 * k) % 21 for k in range(21)] and list(qc.modmul_table(2, 21, 5))[21:] == list(range(21, 32))
    assert list(qc.modmul_table(23, 21, 5)) == list(qc.modmul_table(2, 21, 5))
    for bad in ((3, 21, 5), (2, 33, 5), (2, 0, 5)):
        with pytest.raises(ValueError):
            qc.modmul_table(*bad)
    # modadd
    assert list(qc.modadd_table(3, 3)) == [(k + 3) % 8 for k in range(8)]
    assert list(qc.modadd_table(-1, 3)) == [(k - 1) % 8 for k in range(8)]
    assert list(qc.modadd_table(3, 3, modulus=5)) == [3, 4, 0, 1, 2, 5, 6, 7]
    with pytest.raises(ValueError):
        qc.modadd_table(1, 3, modulus=9)
    # the xor oracle: x in the low nx bits
    f = [3, 0, 1, 2]
    t = qc.xor_oracle_table(f, 2, 2)
    for x in range(4):
        for y in range(4):
            assert t[x | (y << 2)] == x | ((y ^ f[x]) << 2)
    with pytest.raises(ValueError):
        qc.xor_oracle_table([4, 0, 0, 0], 2, 2)
    with pytest.raises(ValueError):
        qc.xor_oracle_table([0, 0, 0], 2, 2)
    # every helper gives a bijection
    for t, num in ((qc.modmul_table(7, 15, 4), 4), (qc.modadd_table(5, 6, modulus=61), 6), (qc.xor_oracle_table(f, 2, 2), 4), (qc.qubit_permutation_table([2, 0, 1]), 3)):
        pr.table(t, num)
    with pytest.raises(ValueError):
        qc.qubit_permutation_table([0, 0, 1])


def test_qubit_permutation_table_is_a_transpose():
    import quantumcomputer_amd as qc
    n, first = 6, 1
    a = random_state(n, 11).view(np.complex128)
    for order in ([3, 2, 1, 0], [1, 2, 3, 0], [0, 1, 2, 3], [2, 0, 3, 1]):
        num = len(order)
        got = pr.apply(a.view(np.float64), n, first, num, qc.qubit_permutation_table(order)).view(np.complex128)
        # axes of the reshaped state: axis j is qubit n - 1 - j.  new qubit first + order[j] holds what qubit first + j held
        where = list(range(n))
        for j, q in enumerate(order):
            where[first + q] = first + j
        axes = [n - 1 - where[n - 1 - ax] for ax in range(n)]
        want = np.transpose(a.reshape([2] * n), axes).reshape(-1)
        assert np.array_equal(got, want), order
    assert list(qc.qubit_permutation_table(range(3)[::-1])) == [0, 4, 2, 6, 1, 5, 3, 7]                # the bit reversal
