"""CPU: the definition of a Pauli string's expectation value (tests/pauli_ref.py) against the textbook, and the facts about it
that the GPU kernel rests on: the two leaves of a pair (i, i ^ x_mask) are the same bits, and the empty string is the
marginal's "sum everything"."""
import functools
import itertools

import numpy as np
import pytest

from bitwise import bits
from marginal_ref import marginal_ref
from pauli_ref import pauli_leaves, pauli_masks, pauli_ref, pauli_sum_ref

PAULI = {
    "I": np.eye(2, dtype=complex),
    "X": np.array([[0, 1], [1, 0]], dtype=complex),
    "Y": np.array([[0, -1j], [1j, 0]], dtype=complex),
    "Z": np.array([[1, 0], [0, -1]], dtype=complex),
}


def letters(n, x, z):
    return "".join("IXZY"[(x >> q & 1) | (z >> q & 1) << 1] for q in range(n))


def dense(s):
    """kron-built matrix of the string s (character k = qubit k = index bit k: the LAST kron factor is qubit 0)"""
    return functools.reduce(np.kron, [PAULI[c] for c in reversed(s)])


def adversarial_states(n):
    """interleaved (re, im) states that make products cancel, underflow, overflow and disappear"""
    k = 2 << n
    rs = np.random.RandomState(7 * n + 1)
    out = []
    a = rs.standard_normal(k) * 2.0 ** rs.randint(-40, 40, k)                      # mixed binades
    out.append(a)
    a = rs.randint(-3, 4, k).astype(np.float64)                                    # small integers: the two products are equal
    a[rs.randint(0, k, max(1, k // 8))] = -0.0
    out.append(a)
    a = rs.standard_normal(k) * 2.0 ** rs.randint(-40, 40, k)
    m = max(1, k // 8)
    a[rs.randint(0, k, m)] = 5e-324 * rs.randint(1, 1000, m)                       # subnormals
    a[rs.randint(0, k, m)] = 0.0
    a[rs.randint(0, k, m)] = -0.0
    a[rs.randint(0, k, max(1, k // 16))] = 1e300
    a[rs.randint(0, k, max(1, k // 16))] = -1e300
    out.append(a)
    b = a.copy()
    b[rs.randint(0, k)] = np.inf
    b[rs.randint(0, k)] = -np.inf
    b[rs.randint(0, k)] = np.nan
    out.append(b)
    out.append(np.full(k, 3.0))                                                    # every difference cancels exactly
    return out


def test_value_is_the_textbook_expectation():
    """n = 1 .. 6, every (x_mask, z_mask): vdot(a, P a) of the kron-built dense P, to 1e-12, and that product is real"""
    for n in range(1, 7):
        rs = np.random.RandomState(n)
        a = rs.standard_normal(1 << n) + 1j * rs.standard_normal(1 << n)
        a /= np.linalg.norm(a)
        for x, z in itertools.product(range(1 << n), repeat=2):
            want = np.vdot(a, dense(letters(n, x, z)) @ a)
            assert abs(want.imag) < 1e-12
            assert abs(pauli_ref(a, n, x, z) - want.real) <= 1e-12, (n, x, z)


def test_a_pair_has_one_leaf():
    """leaf_i and leaf_(i ^ x_mask) are the same bits, NaNs in the same places, for every string, on adversarial states"""
    for n in range(1, 6):
        i = np.arange(1 << n)
        for a in adversarial_states(n):
            for x, z in itertools.product(range(1 << n), repeat=2):
                v = pauli_leaves(a, n, x, z)
                w = v[i ^ x]
                nan = np.isnan(v)
                assert np.array_equal(nan, np.isnan(w)), (n, x, z)
                assert np.array_equal(bits(v[~nan]), bits(w[~nan])), (n, x, z)
                assert not np.any(bits(v) == 1 << 63), "a leaf is never -0"


def test_the_empty_string_is_the_marginal_of_nothing():
    for n in range(1, 12):
        for a in adversarial_states(n):
            got, want = pauli_ref(a, n, 0, 0), marginal_ref(a, n, 0, 0)[0]
            assert (np.isnan(got) and np.isnan(want)) or bits(got) == bits(want)


def test_known_values():
    s = 0.5 ** 0.5
    plus, plus_i = np.array([s, s], dtype=complex), np.array([s, 1j * s], dtype=complex)
    one = np.array([0, 1], dtype=complex)
    assert abs(pauli_ref(plus, 1, *pauli_masks("X", 1)) - 1) <= 1e-15
    assert abs(pauli_ref(plus_i, 1, *pauli_masks("Y", 1)) - 1) <= 1e-15
    assert pauli_ref(one, 1, *pauli_masks("Z", 1)) == -1.0
    bell = np.array([s, 0, 0, s], dtype=complex)
    assert [round(pauli_ref(bell, 2, *pauli_masks(p, 2)), 12) for p in ("XX", "YY", "ZZ", "XY", "ZI")] == [1, -1, 1, 0, 0]
    # a basis state: the parity for a Z-type string, +0 for anything else
    k = 0b0110
    e = np.zeros(16, dtype=complex); e[k] = 1
    for x, z in itertools.product(range(16), repeat=2):
        want = 0.0 if x else (-1.0 if bin(k & z).count("1") & 1 else 1.0)
        assert bits(pauli_ref(e, 4, x, z)) == bits(want)


def test_pauli_masks():
    assert pauli_masks("XIZY", 4) == (0b1001, 0b1100)
    assert pauli_masks("xizy", 6) == (0b1001, 0b1100)
    assert pauli_masks("", 3) == (0, 0)
    assert pauli_masks({3: "Y", 0: "X", 2: "Z", 1: "I"}, 4) == (0b1001, 0b1100)
    assert pauli_masks((5, 3), 3) == (5, 3)
    for n in range(1, 6):
        for x, z in itertools.product(range(1 << n), repeat=2):
            s = letters(n, x, z)
            assert pauli_masks(s, n) == (x, z)
            assert pauli_masks({q: c for q, c in enumerate(s)}, n) == (x, z)
    for bad in ("XXXXX", "XA", {4: "X"}, {-1: "Z"}, {0: "Q"}, {0.5: "X"}, (16, 0), (0, 16), (-1, 0)):
        with pytest.raises(ValueError):
            pauli_masks(bad, 4)


def test_the_product_restates_pauli_masks(qc):
    for spec in ("XIZY", "", {3: "Y", 0: "X"}, (9, 12)):
        assert qc.pauli_masks(spec, 4) == pauli_masks(spec, 4)
    for bad in ("XXXXX", "XA", {4: "X"}, (16, 0)):
        with pytest.raises(ValueError):
            qc.pauli_masks(bad, 4)


def test_pauli_sum_is_added_in_order():
    n = 3
    rs = np.random.RandomState(3)
    a = rs.standard_normal(2 << n)
    terms = [(1e16, 0, 0), (1.0, 1, 0), (-1e16, 0, 0), (0.25, 3, 5), (-2.0, 0, 7)]
    total, values = pauli_sum_ref(a, n, terms)
    assert values == [pauli_ref(a, n, x, z) for _, x, z in terms]
    acc = 0.0
    for (c, _, _), v in zip(terms, values):
        acc = acc + c * v
    assert bits(total) == bits(acc)
    back, _ = pauli_sum_ref(a, n, terms[::-1])
    assert bits(back) != bits(total), "the order of the terms is part of the definition"
    assert pauli_sum_ref(a, n, []) == (0.0, []) and bits(pauli_sum_ref(a, n, [])[0]) == 0
