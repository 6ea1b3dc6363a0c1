"""GPU: the reduced density matrix of a qubit range (qcx_reduced_density_matrix, K16).  Every entry must be, bit for bit, what
tests/rdm_ref.py defines on whatever the state holds (a NaN where the definition gives a NaN), wherever the range lies -- inside
a thread's elements, across the lines of a unit, above the unit --, the state and its lazy forms must stay as they were, and a
few matrices are checked against physics with no reference at all."""
import ctypes as C

import numpy as np
import pytest

from bitwise import bits, same_with_nans as same
from pauli_cases import adversarial
from rdm_ref import rdm_ref

pytestmark = pytest.mark.gpu


def as_pairs(rho):
    """complex128[d, d] as the float64[d, d, 2] of rdm_ref"""
    return np.ascontiguousarray(rho).view(np.float64).reshape(rho.shape + (2,))


def check_ranges(qc, n, a, ranges):
    """every range on the written state a, then: the state is what it was"""
    with qc.Register(n, 0) as reg:
        reg.write(a)
        for first, num in ranges:
            got = reg.reduced_density_matrix(first, num)
            assert got.shape == (1 << num, 1 << num) and got.dtype == np.complex128
            same(as_pairs(got), rdm_ref(a, n, first, num), (n, first, num))
            assert reg.rdm_stats() == (0, 1)
        assert np.array_equal(bits(reg.read()), bits(a)), "the state changed"


def every_range(n, nums):
    return [(first, num) for num in nums if num <= n for first in range(n - num + 1)]


# ---- small registers: one partial unit ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("finite", [True, False], ids=["finite", "inf-nan"])
def test_small_registers_every_range(qc, finite):
    for n in range(1, 6):
        check_ranges(qc, n, adversarial(n, 31 * n, finite), every_range(n, range(0, 5)))


@pytest.mark.parametrize("n", range(6, 12))
def test_partial_unit_every_range(qc, n):
    check_ranges(qc, n, adversarial(n, 37 * n), every_range(n, range(1, 5)))


# ---- full units: the range inside the unit, across its lines, above it --------------------------------------------------------

def test_one_full_unit_every_range(qc):
    check_ranges(qc, 12, adversarial(12, 5), every_range(12, range(0, 5)))


@pytest.mark.parametrize("n", [13, 14])
@pytest.mark.parametrize("finite", [True, False], ids=["finite", "inf-nan"])
def test_around_bit_12(qc, n, finite):
    """inside the unit (first = 0, 3, 7), straddling bit 12 (9, 10, 11), above it (12, 13)"""
    ranges = [(first, num) for first in (0, 3, 7, 9, 10, 11, 12, 13) for num in range(1, 5) if first + num <= n]
    check_ranges(qc, n, adversarial(n, 7 * n + finite, finite), ranges)


def test_nothing_summed_above_the_range(qc):
    check_ranges(qc, 16, adversarial(16, 16), [(12, 4), (0, 4), (8, 4)])


N3 = 25
RANGES_25 = [(0, 1), (11, 1), (24, 1), (0, 2), (11, 2), (23, 2)]


@pytest.fixture(scope="module")
def three_stages(qc):
    """one fill_random state of n = 25, read once, and the matrices the GPU gives on it"""
    with qc.Register(N3, 0) as reg:
        reg.fill_random(5)
        got = [reg.reduced_density_matrix(*r) for r in RANGES_25]
        stats = reg.rdm_stats()
        a = reg.read().view(np.complex128)
    return a, got, stats


@pytest.mark.parametrize("k", range(len(RANGES_25)))
def test_three_stages(three_stages, k):
    a, got, stats = three_stages
    assert stats == (0, 1)
    same(as_pairs(got[k]), rdm_ref(a, N3, *RANGES_25[k]), RANGES_25[k])


def test_four_qubits_of_twenty(qc):
    n = 20
    with qc.Register(n, 0) as reg:
        reg.fill_random(9)
        got = [reg.reduced_density_matrix(first, 4) for first in (0, 10, 16)]
        assert reg.rdm_stats() == (0, 1)
        a = reg.read().view(np.complex128)
    for first, g in zip((0, 10, 16), got):
        same(as_pairs(g), rdm_ref(a, n, first, 4), first)


@pytest.mark.parametrize("n,first,num", [(22, 5, 3), (23, 20, 3), (24, 11, 1)])
def test_groups_of_units(qc, n, first, num):
    """from 22 qubits on a workgroup adds the roots of 2, 4, 8 (and at n = 25, above, 16) consecutive units itself"""
    with qc.Register(n, 0) as reg:
        reg.fill_random(n)
        got = reg.reduced_density_matrix(first, num)
        assert reg.rdm_stats() == (0, 1)
        a = reg.read().view(np.complex128)
    same(as_pairs(got), rdm_ref(a, n, first, num))


# ---- identities that need no reference ----------------------------------------------------------------------------------------

def test_the_diagonal_is_the_marginal(qc):
    for n, finite in ((3, True), (11, False), (12, True), (13, False), (14, True), (18, True)):
        with qc.Register(n, 0) as reg:
            reg.write(adversarial(n, n, finite))
            for first, num in [(0, 0), (0, 1), (n - 1, 1), (1, 2), (n - 3, 3), (0, min(n, 4)), (n - min(n, 4), min(n, 4)), (n // 2, 2)]:
                rho = reg.reduced_density_matrix(first, num)
                same(np.diagonal(rho).real, reg.marginal(first, num), (n, first, num))
                assert not bits(np.diagonal(rho).imag).any()


def test_one_qubit_gives_its_X_and_Y(qc):
    n = 13
    with qc.Register(n, 0) as reg:
        reg.write(adversarial(n, 99, True))
        for q in range(n):
            rho = reg.reduced_density_matrix(q, 1)
            assert 2.0 * rho[0, 1].real == reg.expectation({q: "X"}), q
            assert -2.0 * rho[0, 1].imag == reg.expectation({q: "Y"}), q


# ---- physics --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [3, 12, 14])
def test_product_state(qc, n):
    """|+> on every qubit: every range gives the all-1/2^num matrix, pure, no entropy"""
    with qc.Register(n, 0) as reg:
        reg.write(np.eye(1, 2 << n)[0])
        for q in range(n):
            qc.hadamard_gate(q, reg)
        for first, num in every_range(n, range(0, 5)):
            rho = reg.reduced_density_matrix(first, num)
            assert np.max(np.abs(rho - 0.5 ** num)) <= 1e-12, (first, num)
            assert abs(qc.purity(rho) - 1) <= 1e-12 and abs(qc.von_neumann_entropy(rho)) <= 1e-12


@pytest.mark.parametrize("n,q", [(3, 0), (3, 1), (12, 3), (12, 10), (14, 5), (14, 11), (14, 12)])
def test_bell_pair(qc, n, q):
    """(|00> + |11>) / sqrt 2 on the qubits (q, q + 1): one of them alone is maximally mixed, the pair is the Bell projector"""
    bell = np.zeros((4, 4)); bell[np.ix_([0, 3], [0, 3])] = 0.5
    with qc.Register(n, 0) as reg:
        reg.write(np.eye(1, 2 << n)[0])
        qc.one_qubit_gate(q, qc.GATES["H"], reg)
        qc.two_qubit_gate(q, q + 1, qc.GATES2["CNOT"], reg)
        for one in (q, q + 1):
            rho = reg.reduced_density_matrix(one, 1)
            assert np.max(np.abs(rho - np.eye(2) / 2)) <= 1e-12
            assert abs(qc.von_neumann_entropy(rho) - 1) <= 1e-12 and abs(qc.purity(rho) - 0.5) <= 1e-12
        pair = reg.reduced_density_matrix(q, 2)
        assert np.max(np.abs(pair - bell)) <= 1e-12
        assert abs(qc.von_neumann_entropy(pair)) <= 1e-12 and abs(qc.purity(pair) - 1) <= 1e-12


@pytest.mark.parametrize("n,first", [(3, 1), (12, 5), (14, 11)])
def test_expectation_matrix(qc, n, first):
    rs = np.random.RandomState(n)
    M = rs.standard_normal((4, 4)) + 1j * rs.standard_normal((4, 4))
    M = M + M.conj().T
    with qc.Register(n, 0) as reg:
        reg.fill_random(7)
        got = reg.expectation_matrix(first, M)
        psi = reg.read().view(np.complex128).reshape(1 << (n - first - 2), 4, 1 << first)
    want = np.einsum("hvl,vw,hwl->", psi.conj(), M, psi)
    assert isinstance(got, complex) and abs(got - want) <= 1e-12
    with pytest.raises(ValueError):
        reg.expectation_matrix(0, np.eye(3))


# ---- lazy forms and modes -----------------------------------------------------------------------------------------------------

def compact_stat(qc, reg, name):
    v = C.c_ulong(0)
    assert getattr(qc.lib(), name)(reg._h, C.byref(v)) == 0
    return int(v.value)


def test_pending_basis_state(qc, ob):
    n = 14
    with qc.Register(n - 4, 4) as reg:
        qc.reset_register(reg)                                       # pending basis state |1>
        e = np.zeros(2 << n); e[2] = 1.0
        for first, num in [(0, 0), (0, 1), (0, 4), (1, 3), (12, 2), (10, 4)]:
            got = reg.reduced_density_matrix(first, num)
            same(as_pairs(got), rdm_ref(e, n, first, num), (first, num))
            want = np.zeros((1 << num, 1 << num), dtype=np.complex128)
            vk = (1 >> first) & ((1 << num) - 1)
            want[vk, vk] = 1.0
            assert np.array_equal(bits(as_pairs(got)), bits(as_pairs(want)))
            assert reg.rdm_stats() == (2, 0)
        reg.marginal(0, 2)
        assert reg.marginal_stats() == (2, 0), "the basis state is still pending"
        qc.hadamard_gate(3, reg)                                     # no longer a basis state: a kernel reads the register
        ob.hadamard(e, n, 3)
        same(as_pairs(reg.reduced_density_matrix(2, 3)), rdm_ref(e, n, 2, 3))
        assert reg.rdm_stats() == (0, 1)
        assert np.array_equal(bits(reg.read()), bits(e))


def test_compact_result_is_expanded_first(qc, ob):
    """reset + quantum_computation(15, 7) at M = 4, on the smallest L register whose result stays compact"""
    L, M = 12, 4
    n = L + M
    ranges = [(0, 4), (2, 3), (M, 2), (n - 1, 1), (9, 4), (0, 0)]
    with qc.Register(L, M) as reg:
        k0 = compact_stat(qc, reg, "qcx_compact_stats")
        qc.reset_register(reg); qc.quantum_computation(15, 7, reg)
        assert compact_stat(qc, reg, "qcx_compact_stats") == k0 + 1, "the circuit's result is not in its compact form"
        c0 = compact_stat(qc, reg, "qcx_compact_measure_stats")
        got = []
        for r in ranges:
            got.append(reg.reduced_density_matrix(*r))
            assert reg.rdm_stats() == (3, 1)
        assert compact_stat(qc, reg, "qcx_compact_measure_stats") == c0
        idx = qc.measure_state(reg, 0.61)                            # the lazy form is as it was: the measurement scans it
        assert compact_stat(qc, reg, "qcx_compact_measure_stats") == c0 + 1
        collapsed = reg.read()
    with qc.Register(L, M) as reg:
        qc.reset_register(reg); qc.quantum_computation(15, 7, reg)
        state = reg.read()
    for r, g in zip(ranges, got):
        same(as_pairs(g), rdm_ref(state, n, *r), r)
    assert abs(np.trace(got[0]) - 1) <= 1e-12
    w = state.copy()
    assert idx == ob.measure(w, n, 0.61)
    assert np.array_equal(bits(collapsed), bits(w))


def test_queued_gates_are_flushed_first(qc, ob):
    n = 14
    want = np.zeros(2 << n); ob.reset(want, n)
    with qc.Register(n - 4, 4) as reg:
        reg.set_fusion(1)
        qc.reset_register(reg)
        for q in (0, 3, n - 1):
            qc.hadamard_gate(q, reg)
            ob.hadamard(want, n, q)
        qc.c_phase_shift_gate(3, n - 1, 0.7, reg)
        ob.cphase(want, n, 3, n - 1, 0.7)
        for first, num in [(0, 4), (3, 1), (10, 4), (n - 1, 1)]:
            same(as_pairs(reg.reduced_density_matrix(first, num)), rdm_ref(want, n, first, num), (first, num))
            assert reg.rdm_stats() == (0, 1)
        assert np.array_equal(bits(reg.read()), bits(want))


def test_nonfinite_register(qc, ob):
    n = 13
    a = ob.random_state(n, 21)
    a[2 * 700] = np.inf
    a[2 * 5] = -0.0
    with qc.Register(n, 0) as reg:
        reg.write(a)
        for first, num in [(0, 0), (0, 4), (8, 2), (9, 4), (12, 1)]:
            same(as_pairs(reg.reduced_density_matrix(first, num)), rdm_ref(a, n, first, num), (first, num))
        qc.hadamard_gate(2, reg)                                     # still the strict gate: the oracle's products, NaN/Inf included
        w = a.copy(); ob.hadamard(w, n, 2)
        got = reg.read()
        gn, wn = np.isnan(got), np.isnan(w)
        assert np.array_equal(gn, wn)
        assert np.array_equal(bits(got[~gn]), bits(w[~wn]))


# ---- arguments ------------------------------------------------------------------------------------------------------------------

def test_arguments(qc):
    lib = qc.lib()
    most = qc.rdm_max_qubits()
    assert most >= 4
    out = (C.c_double * (2 << (2 * most + 2)))()
    with qc.Register(12, 0) as reg:
        reg.fill_random(1)
        before = bits(reg.read())
        assert lib.qcx_reduced_density_matrix(None, 0, 1, out) == 2            # QCX_BAD_ARGUMENTS
        assert lib.qcx_reduced_density_matrix(reg._h, 0, 1, None) == 2
        assert lib.qcx_reduced_density_matrix(reg._h, 12, 1, out) == 6         # QCX_BAD_QUBIT
        assert lib.qcx_reduced_density_matrix(reg._h, 9, 4, out) == 6
        assert lib.qcx_reduced_density_matrix(reg._h, 13, 0, out) == 6
        assert lib.qcx_reduced_density_matrix(reg._h, 12 - most, most + 1, out) == 6
        assert lib.qcx_reduced_density_matrix(reg._h, 0, most + 1, out) == 7   # QCX_UNSUPPORTED
        assert lib.qcx_reduced_density_matrix(reg._h, 12, 0, out) == 0
        assert lib.qcx_rdm_last_stats(None, None, None) == 2
        assert lib.qcx_rdm_last_stats(reg._h, None, None) == 0
        assert np.array_equal(bits(reg.read()), before)
        with pytest.raises(ValueError):
            reg.reduced_density_matrix(-1, 1)
        with pytest.raises(qc.QcxError):
            reg.reduced_density_matrix(0, most + 1)
    with qc.Register(13, 0, shards=2, devices=qc.spread_devices(2)) as sh:     # virtual shards on one GPU
        sh.fill_random(3)
        before = bits(sh.read())
        assert lib.qcx_reduced_density_matrix(sh._h, 0, 1, out) == 7           # QCX_UNSUPPORTED
        assert lib.qcx_reduced_density_matrix(sh._h, 13, 1, out) == 7          # ... before the range is looked at
        assert np.array_equal(bits(sh.read()), before)
