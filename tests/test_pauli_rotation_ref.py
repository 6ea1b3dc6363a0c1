"""tests/pauli_rotation_ref.py IS the definition of qcx_pauli_rotation; this file pins it from the outside: against the dense
cos(theta/2) I - i sin(theta/2) P, bit for bit against the committed one- and two-qubit definitions for one- and two-letter
strings, and on what it promises about -0, Inf and NaN.  Host only."""
import itertools

import numpy as np
import pytest

import one_qubit_ref
import pauli_rotation_ref as prr
import two_qubit_ref
from bitwise import bits
from pauli_ref import pauli_masks

THETAS = [0.0, np.pi, -0.7, 7.5, 1e-9, np.pi / 2]                   # 0, pi, a negative value, one above 2 pi


def finite_adversarial(n, seed):
    """mixed binades, subnormals, +-0 -- test_gpu_pauli_expectation.adversarial(finite=True), restated for the host"""
    rs = np.random.RandomState(seed)
    a = rs.standard_normal(2 << n) * 2.0 ** rs.randint(-40, 40, 2 << n)
    k = a.size
    m = max(1, k // 16)
    a[rs.randint(0, k, m)] = 5e-324 * rs.randint(1, 1000, m)
    a[rs.randint(0, k, m)] = 0.0
    a[rs.randint(0, k, m)] = -0.0
    return a


def dense(n, x, z, theta):
    p = np.eye(1, dtype=complex)
    for q in range(n):                                               # qubit 0 is the lowest index bit: the last kron factor
        l = "IXZY"[(x >> q & 1) + 2 * (z >> q & 1)]
        p = np.kron(prr.PAULI[l], p)
    return np.cos(theta / 2) * np.eye(1 << n) - 1j * np.sin(theta / 2) * p


def test_against_the_dense_matrix():
    """1e-14 on O(1) amplitudes, n <= 5, random strings and angles"""
    rs = np.random.RandomState(1)
    for trial in range(400):
        n = int(rs.randint(1, 6)) if trial < 200 else 5
        x, z = int(rs.randint(0, 1 << n)), int(rs.randint(0, 1 << n))
        theta = float(rs.uniform(-7, 7))
        a = rs.uniform(-1, 1, 2 << n)
        want = dense(n, x, z, theta) @ a.view(np.complex128)
        assert np.max(np.abs(prr.apply(a, n, x, z, theta).view(np.complex128) - want)) <= 1e-14, (n, x, z, theta)


@pytest.mark.parametrize("letter", ["X", "Y", "Z"])
def test_one_letter_is_the_one_qubit_gate(letter):
    n = 5
    for q, theta in itertools.product(range(n), THETAS):
        a = finite_adversarial(n, 10 * q + 1)
        c, s = prr.polar(theta / 2)
        want = one_qubit_ref.apply(a, n, q, prr.matrices(letter, c, s))
        got = prr.apply(a, n, *pauli_masks({q: letter}, n), theta)
        assert np.array_equal(bits(got), bits(want)), (letter, q, theta)


@pytest.mark.parametrize("l0,l1", list(itertools.product("XYZ", repeat=2)))
def test_two_letters_are_the_two_qubit_gate(l0, l1):
    n = 5
    for (q0, q1), theta in itertools.product(((0, 1), (1, 0), (1, 4), (4, 1), (3, 2), (0, 4)), THETAS):
        a = finite_adversarial(n, 7 * q0 + q1)
        c, s = prr.polar(theta / 2)
        want = two_qubit_ref.apply(a, n, q0, q1, prr.matrix2(l0, l1, c, s))
        got = prr.apply(a, n, *pauli_masks({q0: l0, q1: l1}, n), theta)
        assert np.array_equal(bits(got), bits(want)), (l0, l1, q0, q1, theta)


def test_matrix2_is_the_dense_matrix():
    c, s = prr.polar(0.35)
    for l0, l1 in itertools.product("XYZ", repeat=2):
        x, z = pauli_masks({0: l0, 1: l1}, 2)
        assert np.allclose(prr.matrix2(l0, l1, c, s), dense(2, x, z, 0.7), atol=1e-16)


def test_no_negative_zero():
    rs = np.random.RandomState(3)
    for n in (1, 3, 5):
        a = finite_adversarial(n, n)
        a[rs.randint(0, a.size, a.size // 2)] = -0.0
        for x, z in itertools.product(range(1 << n), repeat=2) if n < 5 else [(0, 0), (0, 31), (5, 3), (31, 31), (16, 16)]:
            for theta in THETAS:
                out = prr.apply(a, n, x, z, theta)
                assert not np.any((out == 0) & np.signbit(out)), (n, x, z, theta)
    all_neg = np.full(2 << 3, -0.0)
    for x, z in itertools.product(range(8), repeat=2):
        assert np.array_equal(bits(prr.apply(all_neg, 3, x, z, 0.3)), np.zeros(16, dtype=np.uint64))


def test_an_inf_reaches_two_rows_only():
    n = 5
    rs = np.random.RandomState(4)
    for trial in range(100):
        x, z = int(rs.randint(0, 32)), int(rs.randint(0, 32))
        k = int(rs.randint(0, 32))
        a = rs.standard_normal(2 << n)
        a[2 * k + int(rs.randint(0, 2))] = np.inf
        out = prr.apply(a, n, x, z, float(rs.uniform(-3, 3))).view(np.complex128)
        bad = ~(np.isfinite(out.real) & np.isfinite(out.imag))
        want = np.zeros(32, dtype=bool); want[k] = want[k ^ x] = True
        assert np.array_equal(bad, want), (x, z, k)


def test_theta_then_minus_theta():
    rs = np.random.RandomState(5)
    for n in (1, 4, 9):
        a = rs.standard_normal(2 << n)
        a /= np.linalg.norm(a)
        for trial in range(20):
            x, z = int(rs.randint(0, 1 << n)), int(rs.randint(0, 1 << n))
            theta = float(rs.uniform(-7, 7))
            b = prr.apply(prr.apply(a, n, x, z, theta), n, x, z, -theta)
            assert np.max(np.abs(b - a)) <= 1e-12
            assert abs(np.linalg.norm(prr.apply(a, n, x, z, theta)) - 1) <= 1e-12


def test_polar_is_one_sincos():
    assert prr.polar(0.0) == (1.0, 0.0)
    c, s = prr.polar(0.20966817126512538)                            # an argument where glibc's sin and sincos differ
    assert abs(c - np.cos(0.20966817126512538)) <= 2e-16 and abs(s - np.sin(0.20966817126512538)) <= 2e-16


def test_the_empty_string_is_a_global_phase():
    a = finite_adversarial(4, 9)
    c, s = prr.polar(0.45)
    want = np.empty_like(a)
    want[0::2] = 0.0 + (c * a[0::2] - (-s) * a[1::2])
    want[1::2] = 0.0 + (c * a[1::2] + (-s) * a[0::2])
    assert np.array_equal(bits(prr.apply(a, 4, 0, 0, 0.9)), bits(want))
