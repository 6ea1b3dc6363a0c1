"""CPU: the definition of qcx_reduced_density_matrix (tests/rdm_ref.py) against the definitions it leans on -- its diagonal is
the marginal bit for bit, one qubit's off-diagonal entry is that qubit's X and Y values, Tr(rho P) is the Pauli string's value
to rounding -- and against plain linear algebra.  No GPU needed."""
import itertools

import numpy as np
import pytest

from bitwise import bits, same_with_nans as same
from marginal_ref import marginal_ref
from pauli_cases import adversarial
from pauli_ref import pauli_ref
from rdm_ref import as_complex, rdm_ref

MINUS_ZERO = np.uint64(1 << 63)
PAULI = {"I": np.eye(2), "X": np.array([[0, 1], [1, 0]]), "Y": np.array([[0, -1j], [1j, 0]]), "Z": np.diag([1.0, -1.0])}


def ranges(n, most=4):
    return [(first, num) for first in range(n + 1) for num in range(min(n - first, most) + 1)]


def normalised(n, seed):
    a = adversarial(n, seed, True).view(np.complex128)
    return a / np.linalg.norm(a)


@pytest.mark.parametrize("finite", [True, False], ids=["finite", "inf-nan"])
@pytest.mark.parametrize("n", range(1, 12))
def test_diagonal_is_the_marginal(n, finite):
    a = adversarial(n, 17 * n, finite)
    for first, num in ranges(n):
        rho = rdm_ref(a, n, first, num)
        same(np.diagonal(rho[:, :, 0]), marginal_ref(a, n, first, num), (n, first, num))
        assert not np.diagonal(rho[:, :, 1]).view(np.uint64).any(), "a diagonal entry's imaginary part is +0"


@pytest.mark.parametrize("finite", [True, False], ids=["finite", "inf-nan"])
@pytest.mark.parametrize("n", range(1, 12))
def test_hermitian_by_construction_and_no_minus_zero(n, finite):
    a = adversarial(n, 19 * n, finite)
    for first, num in ranges(n):
        rho = rdm_ref(a, n, first, num)
        assert rho.shape == (1 << num, 1 << num, 2)
        same(rho[:, :, 0], rho[:, :, 0].T)
        with np.errstate(invalid="ignore"):
            same(np.tril(rho[:, :, 1]), np.tril(0.0 - rho[:, :, 1].T))
        assert not (bits(rho) == MINUS_ZERO).any(), (n, first, num)


@pytest.mark.parametrize("n", range(1, 12))
def test_one_qubit_gives_its_X_and_Y(n):
    """the two leaves of a Pauli pair are the same bits, so level `q` of the Pauli tree is an exact doubling"""
    a = adversarial(n, 23 * n, True)
    for q in range(n):
        rho = rdm_ref(a, n, q, 1)
        assert 2.0 * rho[0, 1, 0] == pauli_ref(a, n, 1 << q, 0), (n, q)
        assert -2.0 * rho[0, 1, 1] == pauli_ref(a, n, 1 << q, 1 << q), (n, q)


@pytest.mark.parametrize("n", range(1, 12))
def test_trace_with_a_pauli_string_is_its_value(n):
    a = normalised(n, 29 * n)
    rs = np.random.RandomState(n)
    for first, num in ranges(n):
        rho = as_complex(rdm_ref(a, n, first, num))
        strings = list(itertools.product("IXYZ", repeat=num))
        if num > 2:
            strings = [strings[i] for i in rs.choice(len(strings), 12, replace=False)]
        for s in strings:
            P = np.eye(1)
            x = z = 0
            for k, p in enumerate(s):                                # qubit first + k is bit k of the matrix index
                P = np.kron(PAULI[p], P)
                x |= (p in "XY") << (first + k)
                z |= (p in "ZY") << (first + k)
            assert abs(np.sum(rho * P.T).real - pauli_ref(a, n, x, z)) <= 1e-12, (n, first, num, s)


@pytest.mark.parametrize("n", range(1, 12))
def test_against_einsum(n):
    rs = np.random.RandomState(31 * n)
    a = rs.standard_normal(1 << n) + 1j * rs.standard_normal(1 << n)
    a /= np.linalg.norm(a)
    for first, num in ranges(n):
        psi = a.reshape(1 << (n - first - num), 1 << num, 1 << first)
        want = np.einsum("hvl,hwl->vw", psi, psi.conj())
        assert np.max(np.abs(as_complex(rdm_ref(a, n, first, num)) - want)) <= 1e-12, (n, first, num)


@pytest.mark.parametrize("finite", [True, False], ids=["finite", "inf-nan"])
def test_the_whole_register_is_the_outer_product(finite):
    """num = n: nothing is summed, every entry is its single leaf"""
    for n in range(1, 5):
        a = adversarial(n, 37 * n, finite).view(np.complex128)
        rho = rdm_ref(a, n, 0, n)
        with np.errstate(over="ignore", invalid="ignore", under="ignore"):
            for v in range(1 << n):
                for w in range(v, 1 << n):
                    same(rho[v, w, 0], 0.0 + (a[v].real * a[w].real + a[v].imag * a[w].imag))
                    if v < w:
                        same(rho[v, w, 1], 0.0 + (a[v].imag * a[w].real - a[v].real * a[w].imag))


@pytest.mark.parametrize("finite", [True, False], ids=["finite", "inf-nan"])
def test_no_qubit_gives_the_norm(finite):
    for n in range(1, 12):
        a = adversarial(n, 41 * n, finite)
        for first in (0, n // 2, n):
            rho = rdm_ref(a, n, first, 0)
            assert rho.shape == (1, 1, 2) and bits(rho[0, 0, 1]) == 0
            same(rho[0, 0, 0], marginal_ref(a, n, 0, 0)[0])
