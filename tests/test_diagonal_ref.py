"""tests/diagonal_ref.py IS the definition of qcx_diagonal_gate; this file pins it from the outside: bit for bit against the
committed definitions it specialises to -- the Z-type Pauli rotation (finite and Inf/NaN states), the one- and two-qubit gates
with diagonal matrices and Z under n - 1 controls (finite states) -- against the dense operator, and on what it promises about
-0 and num = 0.  Host only."""
import numpy as np

import diagonal_ref as dr
import mc_gate_ref
import one_qubit_ref
import pauli_cases
import pauli_rotation_ref as prr
import two_qubit_ref
from bitwise import bits, same, same_with_nans


def unit_table(rs, num):
    ph = rs.uniform(-np.pi, np.pi, 1 << num)
    return np.clip(np.cos(ph), -1, 1) + 1j * np.clip(np.sin(ph), -1, 1)


def z_rotation_table(n, z_mask, theta):
    """exp(-i theta/2 Z..Z) as a table over all n qubits: (c, -s) where popcount(i & z_mask) is even, (c, s) where it is odd"""
    c, s = prr.polar(np.float64(theta) / np.float64(2.0))
    odd = np.array([bin(i & z_mask).count("1") & 1 for i in range(1 << n)], dtype=bool)
    return np.where(odd, complex(c, s), complex(c, -s))


def test_z_rotations_bit_for_bit_finite_and_nonfinite():
    rs = np.random.RandomState(1)
    for trial in range(120):
        n = int(rs.randint(1, 8))
        z = int(rs.randint(0, 1 << n))
        theta = float(rs.uniform(-7, 7))
        for finite in (True, False):
            a = pauli_cases.adversarial(n, 100 + trial, finite=finite)
            want = prr.apply(a, n, 0, z, theta)
            got = dr.apply(a, n, 0, n, z_rotation_table(n, z, theta))
            same_with_nans(got, want, f"n={n} z={z:#x} theta={theta} finite={finite}")
            # the same through the narrowest range that covers the string
            if z:
                lo, hi = (z & -z).bit_length() - 1, z.bit_length()
                sub = z_rotation_table(hi - lo, z >> lo, theta)
                same_with_nans(dr.apply(a, n, lo, hi - lo, sub), want, f"n={n} z={z:#x} range [{lo}, {hi})")


def test_one_qubit_diagonal_matrices():
    n = 6
    rs = np.random.RandomState(2)
    for q in range(n):
        a = pauli_cases.adversarial(n, 20 + q, finite=True)
        for t in (unit_table(rs, 1), np.array([1.0, -1.0]), np.array([0.0, 1j]), np.array([0.25 - 0.5j, -1.0 + 0j])):
            t = np.asarray(t, dtype=complex)
            want = one_qubit_ref.apply(a, n, q, np.diag(t))
            same(dr.apply(a, n, q, 1, t), want, f"q={q} diag={t}")


def test_two_qubit_diagonal_matrices():
    n = 6
    rs = np.random.RandomState(3)
    for q in range(n - 1):
        a = pauli_cases.adversarial(n, 40 + q, finite=True)
        theta = float(rs.uniform(-7, 7))
        c, s = prr.polar(theta)
        for t in (np.array([1.0, 1.0, 1.0, complex(c, s)]), unit_table(rs, 2)):
            # two_qubit_ref's matrix index is bit(q0) + 2 * bit(q1): with (q0, q1) = (q, q + 1) that is the table's k
            want = two_qubit_ref.apply(a, n, q, q + 1, np.diag(t))
            same(dr.apply(a, n, q, 2, t), want, f"q={q} diag={t}")


def test_z_under_all_other_controls():
    Z = np.array([[1, 0], [0, -1]], dtype=complex)
    for n in (2, 3, 5, 7):
        a = pauli_cases.adversarial(n, 60 + n, finite=True)
        t = np.ones(1 << n, dtype=complex)
        t[-1] = -1.0
        for q in range(n):
            cm = ((1 << n) - 1) & ~(1 << q)
            want = mc_gate_ref.apply1(a, n, q, Z, cm, cm)
            same(dr.apply(a, n, 0, n, t), want, f"n={n} target {q}")


def test_against_the_dense_operator():
    """1e-14 on O(1) amplitudes"""
    rs = np.random.RandomState(4)
    for trial in range(200):
        n = int(rs.randint(1, 7))
        first = int(rs.randint(0, n + 1))
        num = int(rs.randint(0, n - first + 1))
        t = unit_table(rs, num)
        a = rs.uniform(-1, 1, 2 << n)
        want = dr.dense(n, first, num, t) @ a.view(np.complex128)
        assert np.max(np.abs(dr.apply(a, n, first, num, t).view(np.complex128) - want)) <= 1e-14, (n, first, num)


def test_entry_index_is_lsb_first():
    assert list(dr.entry_index(3, 1, 2)) == [0, 0, 1, 1, 2, 2, 3, 3]
    assert list(dr.entry_index(3, 0, 1)) == [0, 1] * 4
    assert list(dr.entry_index(2, 2, 0)) == [0] * 4


def test_no_negative_zero():
    rs = np.random.RandomState(5)
    for n in (1, 3, 5):
        a = pauli_cases.adversarial(n, n, finite=True)
        a[rs.randint(0, a.size, a.size // 2)] = -0.0
        for first in range(n + 1):
            for num in range(n - first + 1):
                for t in (unit_table(rs, num), -np.ones(1 << num, dtype=complex), np.zeros(1 << num, dtype=complex), np.full(1 << num, -1j)):
                    out = dr.apply(a, n, first, num, t)
                    assert not np.any((out == 0) & np.signbit(out)), (n, first, num)
    all_neg = np.full(2 << 3, -0.0)
    assert np.array_equal(bits(dr.apply(all_neg, 3, 0, 3, unit_table(rs, 3))), np.zeros(16, dtype=np.uint64))


def test_num_zero_is_the_global_factor():
    a = pauli_cases.adversarial(4, 9, finite=True)
    c, s = prr.polar(-0.45)
    want = np.empty_like(a)
    want[0::2] = 0.0 + (c * a[0::2] - s * a[1::2])
    want[1::2] = 0.0 + (c * a[1::2] + s * a[0::2])
    for first in range(5):
        same(dr.apply(a, 4, first, 0, [c, s]), want, f"first={first}")
    same(dr.apply(a, 4, 0, 0, [c, s]), prr.apply(a, 4, 0, 0, 0.9), "the empty Pauli string")


def test_an_inf_stays_in_its_row():
    n = 5
    rs = np.random.RandomState(6)
    for trial in range(50):
        k = int(rs.randint(0, 32))
        a = rs.standard_normal(2 << n)
        a[2 * k + int(rs.randint(0, 2))] = np.inf
        first = int(rs.randint(0, n + 1)); num = int(rs.randint(0, n - first + 1))
        out = dr.apply(a, n, first, num, unit_table(rs, num)).view(np.complex128)
        bad = ~(np.isfinite(out.real) & np.isfinite(out.imag))
        want = np.zeros(32, dtype=bool); want[k] = True
        assert np.array_equal(bad, want), (first, num, k)
    # zero components are multiplied out: 0 * Inf = NaN
    a = np.zeros(4); a[0] = np.inf
    out = dr.apply(a, 1, 0, 1, np.array([1j, 1.0]))
    assert np.isnan(out[0]) and out[1] == np.inf                     # re = 0 * Inf - 1 * 0, im = 0 * 0 + 1 * Inf
