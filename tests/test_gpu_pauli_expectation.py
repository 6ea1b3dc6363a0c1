"""GPU: the expectation value of a Pauli string (qcx_pauli_expectation, K14).  Every value must be, bit for bit, what
tests/pauli_ref.py defines on whatever the state holds (a NaN where the definition gives a NaN), in both shapes of the first
stage -- the partner amplitude inside the tile, and in another tile --, the state and its lazy forms must stay as they were,
and a few values are checked against physics with no reference at all."""
import ctypes as C
import itertools

import numpy as np
import pytest

from bitwise import bits, same_with_nans as same
from pauli_cases import PAIR_13, TILE_13, adversarial, g_of, with_every_g
from pauli_ref import pauli_masks, pauli_ref, pauli_sum_ref

pytestmark = pytest.mark.gpu

T = 12                                                              # the first stage's tiles: the 12 lowest index bits


def check_strings(qc, n, a, strings):
    """every string on the written state a, then: the state is what it was"""
    with qc.Register(n, 0) as reg:
        reg.write(a)
        for x, z in strings:
            same(reg.expectation((x, z)), pauli_ref(a, n, x, z))
            assert reg.expectation_stats() == (0, 1)
        assert np.array_equal(bits(reg.read()), bits(a)), "the state changed"


# ---- small registers: a partial tile ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("finite", [True, False], ids=["finite", "inf-nan"])
def test_small_registers_every_string(qc, finite):
    for n in range(1, 6):
        check_strings(qc, n, adversarial(n, 31 * n, finite), list(itertools.product(range(1 << n), repeat=2)))


@pytest.mark.parametrize("finite", [True, False], ids=["finite", "inf-nan"])
def test_small_registers_random_strings(qc, finite):
    for n in range(6, 12):
        rs = np.random.RandomState(1000 + n)
        strings = [(int(rs.randint(0, 1 << n)), int(rs.randint(0, 1 << n))) for _ in range(64)]
        check_strings(qc, n, adversarial(n, 31 * n, finite), strings)


# ---- the edges of the two shapes ---------------------------------------------------------------------------------------------

def test_one_full_tile(qc):
    n = 12
    xs = [0, 1, 0x7, 0x8, 0x100, 0x800, 0xF00, 0xFFF, 0xA53]
    check_strings(qc, n, adversarial(n, 5, True), with_every_g(xs, n, 1))
    check_strings(qc, n, adversarial(n, 6), [(0, 0), (0xA53, 0x11), (0, 0xFFF)])


def test_two_tiles(qc):
    n = 13
    tile, pair = with_every_g(TILE_13, n, 2), with_every_g(PAIR_13, n, 3)
    assert all(x >> T == 0 for x, _ in tile) and all(x >> T for x, _ in pair)
    assert {g_of(x, z) for x, z in tile} == {0, 1, 2, 3} == {g_of(x, z) for x, z in pair}
    check_strings(qc, n, adversarial(n, 7, True), tile + pair)
    check_strings(qc, n, adversarial(n, 8), [(0, 0), (0x1000, 0), (0x1FFF, 0x1FFF), (0x130, 0x1030)])


def test_pairs_whose_partner_is_not_the_neighbour(qc):
    n = 14
    xs = [0x1000, 0x2000, 0x3000, 0x2007, 0x3081, 0x1F00, 0x3FFF, 0x0FFF]
    strings = with_every_g(xs, n, 4)
    assert {g_of(x, z) for x, z in strings if x >> T} == {0, 1, 2, 3}
    check_strings(qc, n, adversarial(n, 9, True), strings)


N3 = 25                                                             # the first size with three stages (12 + 12 + 1 bits)
STRINGS_25 = [(0, 0), (0, (1 << N3) - 1), (0x20, 0x1000001), (1 << 24, 0), (0x1FFFFFF, 0x0AAAAAA), (0x1800F03, 0x1000F01)]


@pytest.fixture(scope="module")
def three_stages(qc):
    """one fill_random state of n = 25, read once, and the six values the GPU gives on it"""
    with qc.Register(N3, 0) as reg:
        reg.fill_random(5)
        got = [reg.expectation(s) for s in STRINGS_25]
        stats = reg.expectation_stats()
        a = reg.read().view(np.complex128)
    return a, got, stats


@pytest.mark.parametrize("k", range(len(STRINGS_25)))
def test_three_stages(three_stages, k):
    a, got, stats = three_stages
    assert stats == (0, 1)
    same(got[k], pauli_ref(a, N3, *STRINGS_25[k]))


# ---- cross-checks that need no reference ------------------------------------------------------------------------------------

def test_the_empty_string_is_the_marginal_of_nothing(qc):
    for n, finite in ((3, True), (11, True), (12, False), (13, True), (14, False), (18, True)):
        with qc.Register(n, 0) as reg:
            reg.write(adversarial(n, n, finite))
            same(reg.expectation((0, 0)), reg.marginal(0, 0)[0])


def test_uniform_superposition(qc):
    """H on every qubit of a basis state: an X-only string gives +-1, anything with a Z or a Y gives 0.  From |0..0> every
    qubit is |+> and every X-only string gives 1.  reset_register leaves |0..01> (the reference's start state), so qubit 0
    becomes |-> and an X on it brings a factor -1: "X" * n gives -1 there, X's on the other qubits alone give 1."""
    for n, from_reset in itertools.product((3, 12, 14), (False, True)):
        with qc.Register(n, 0) as reg:
            if from_reset:
                qc.reset_register(reg)
            else:
                reg.write(np.eye(1, 2 << n)[0])
            for q in range(n):
                qc.hadamard_gate(q, reg)
            x0 = -1 if from_reset else 1
            assert abs(reg.expectation("X" * n) - x0) <= 1e-12
            assert abs(reg.expectation({n - 1: "X"}) - 1) <= 1e-12 and abs(reg.expectation({0: "X", n - 1: "X"}) - x0) <= 1e-12
            assert abs(reg.expectation("IX" + "X" * (n - 2)) - 1) <= 1e-12
            for s in ("Z", "X" * (n - 1) + "Z", "ZX", {n - 1: "Z"}, {0: "Z", n - 1: "Z"}, "Z" * n, {n - 1: "Y"}, {0: "X", n - 1: "Y"}):
                assert abs(reg.expectation(s)) <= 1e-12, (n, s)


def test_bell_pair(qc):
    """(|00> + |11>) / sqrt 2 on two qubits of the register: XX = ZZ = 1, YY = -1 -- inside a tile and across two tiles"""
    for n, q0, q1 in ((2, 0, 1), (12, 3, 11), (14, 3, 13), (14, 12, 13)):
        with qc.Register(n, 0) as reg:
            reg.write(np.eye(1, 2 << n)[0])
            qc.one_qubit_gate(q0, qc.GATES["H"], reg)
            qc.two_qubit_gate(q0, q1, qc.GATES2["CNOT"], reg)
            for p, want in (("X", 1), ("Z", 1), ("Y", -1)):
                assert abs(reg.expectation({q0: p, q1: p}) - want) <= 1e-12, (n, q0, q1, p)
            assert abs(reg.expectation({q0: "X", q1: "Y"})) <= 1e-12 and abs(reg.expectation({q0: "Z"})) <= 1e-12


# ---- lazy forms and modes ---------------------------------------------------------------------------------------------------

def test_pending_basis_state(qc):
    n = 14
    rs = np.random.RandomState(14)
    strings = [(0, 0), (0, 1), (0, 0x3FFF), (0, 0x2AAA), (1, 0), (1, 1), (0x1000, 0), (0x1003, 0x1001)]
    strings += [(int(rs.randint(0, 2)) * int(rs.randint(1, 1 << n)), int(rs.randint(0, 1 << n))) for _ in range(24)]
    with qc.Register(n - 4, 4) as reg:
        for k in (1, 0, 0x2A51):
            if k == 1:
                qc.reset_register(reg)                               # pending basis state |1>
            else:
                e = np.zeros(2 << n); e[2 * k] = 1.0                 # a collapse leaves the pending basis state k
                reg.write(e)
                assert qc.measure_state(reg, 0.5) == k
            e = np.zeros(2 << n); e[2 * k] = 1.0
            for x, z in strings:
                got = reg.expectation((x, z))
                assert bits(got) == bits(pauli_ref(e, n, x, z)), (k, x, z)
                assert bits(got) == bits(0.0 if x else (-1.0) ** bin(k & z).count("1"))
                assert reg.expectation_stats() == (2, 0)             # ... and it is still pending at the next call
            assert np.array_equal(bits(reg.read()), bits(e))
        qc.reset_register(reg)
        qc.hadamard_gate(0, reg)                                     # no longer a basis state: a kernel reads the register
        assert abs(reg.expectation("X") + 1) <= 1e-12                # (H|1> = |->)
        assert reg.expectation_stats() == (0, 1)


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
        for s in ({0: "X", 3: "Y", n - 1: "X"}, {3: "X", n - 1: "Y"}, {0: "X"}, {1: "Z"}):
            same(reg.expectation(s), pauli_ref(want, n, *pauli_masks(s, n)))
            assert reg.expectation_stats() == (0, 1)
        assert abs(reg.expectation({0: "X"}) + 1) <= 1e-12 and abs(reg.expectation({1: "Z"}) - 1) <= 1e-12      # (qubit 0: H|1> = |->)
        assert np.array_equal(bits(reg.read()), bits(want))


def test_compact_result_is_expanded_first(qc, ob):
    L, M, Cn, a = 15, 5, 21, 2                                      # (the compact chain runs from n = 20 on)
    n = L + M
    strings = [(0, 0), (0, 1 << M), (1 << (n - 1), 0), (0x3 << M, 0x1F), (0x81234, 0x80F31)]

    def compact_measures(reg):
        v = C.c_ulong(0)
        assert qc.lib().qcx_compact_measure_stats(reg._h, C.byref(v)) == 0
        return int(v.value)

    with qc.Register(L, M) as flushed:
        qc.reset_register(flushed); qc.quantum_computation(Cn, a, flushed)
        flushed.flush()
        want = [flushed.expectation(s) for s in strings]
        assert flushed.expectation_stats() == (0, 1)
        state = flushed.read()
    same(want, [pauli_ref(state, n, x, z) for x, z in strings])
    assert abs(want[0] - 1) <= 1e-12
    with qc.Register(L, M) as reg:
        qc.reset_register(reg); qc.quantum_computation(Cn, a, reg)
        c0 = compact_measures(reg)
        for s, w in zip(strings, want):
            same(reg.expectation(s), w)
            assert reg.expectation_stats() == (3, 1)
        assert compact_measures(reg) == c0
        idx = qc.measure_state(reg, 0.61)                           # the lazy form is as it was: the measurement scans it
        assert compact_measures(reg) == c0 + 1
        w = state.copy()
        assert idx == ob.measure(w, n, 0.61)
        assert np.array_equal(bits(reg.read()), bits(w))


def test_nonfinite_register(qc, ob):
    n = 13
    a = ob.random_state(n, 21)
    a[2 * 700] = np.inf
    a[2 * 5] = -0.0
    b = a.copy()
    b[2 * 3000 + 1] = np.nan
    strings = [(0, 0), (0, 0x1FFF), (0x1000, 0), (0x4, 0x4), (0x1234, 0x0F0F), (0x2BC ^ 0x1000, 0x1000)]
    for state in (a, b):
        with qc.Register(n, 0) as reg:
            reg.write(state)
            for x, z in strings:
                same(reg.expectation((x, z)), pauli_ref(state, n, x, z))
            qc.hadamard_gate(2, reg)                                # still the strict gate: the oracle's products, NaN/Inf included
            w = state.copy(); ob.hadamard(w, n, 2)
            got = reg.read()
            gn, wn = np.isnan(got), np.isnan(w)
            assert np.array_equal(gn, wn)
            assert np.array_equal(bits(got[~gn]), bits(w[~wn]))
    assert np.isinf(pauli_ref(a, n, 0, 0)) and not np.isnan(pauli_ref(a, n, 0x1000, 0)), "the Inf state gives more than NaNs"


# ---- sums of strings --------------------------------------------------------------------------------------------------------

def test_expectation_sum(qc):
    n = 13
    a = adversarial(n, 77, True)
    terms = [(1e16, ""), (0.5, {0: "Z", 12: "Z"}), (-1e16, (0, 0)), (-0.3, "XYZ" * 4 + "X"), (2.0, (0x1030, 0x0031))]
    ref_terms = [(c,) + pauli_masks(p, n) for c, p in terms]
    want_total, want_values = pauli_sum_ref(a, n, ref_terms)
    with qc.Register(n, 0) as reg:
        reg.write(a)
        total, values = reg.expectation_sum(terms)
        assert reg.expectation_stats() == (0, 5)
        same(values, want_values)
        same(total, want_total)
        # values may be NULL
        lib = qc.lib()
        xs = (C.c_uint64 * 5)(*[t[1] for t in ref_terms]); zs = (C.c_uint64 * 5)(*[t[2] for t in ref_terms])
        cs = (C.c_double * 5)(*[t[0] for t in ref_terms])
        tot = C.c_double(-1.0)
        assert lib.qcx_pauli_expectation_sum(reg._h, 5, xs, zs, cs, None, C.byref(tot)) == 0
        same(tot.value, want_total)
        # no term: +0.0, nothing runs
        reg.set_fusion(1)
        qc.hadamard_gate(0, reg)
        g0 = reg.fusion_stats()
        total, values = reg.expectation_sum([])
        assert bits(total) == 0 and values.size == 0
        assert reg.expectation_stats() == (0, 0) and reg.fusion_stats() == g0


# ---- arguments --------------------------------------------------------------------------------------------------------------

def test_arguments(qc):
    lib = qc.lib()
    out = C.c_double(0.0)
    one = (C.c_uint64 * 1)(0)
    high = (C.c_uint64 * 1)(1 << 12)
    cf = (C.c_double * 1)(1.0)
    with qc.Register(12, 0) as reg:
        reg.fill_random(1)
        before = bits(reg.read())
        assert lib.qcx_pauli_expectation(None, 0, 0, C.byref(out)) == 2                 # QCX_BAD_ARGUMENTS
        assert lib.qcx_pauli_expectation(reg._h, 0, 0, None) == 2
        assert lib.qcx_pauli_expectation(reg._h, 1 << 12, 0, C.byref(out)) == 6         # QCX_BAD_QUBIT
        assert lib.qcx_pauli_expectation(reg._h, 0, 1 << 12, C.byref(out)) == 6
        assert lib.qcx_pauli_expectation(reg._h, 0, 1 << 63, C.byref(out)) == 6
        assert lib.qcx_pauli_expectation(reg._h, 1 << 11, 1 << 11, C.byref(out)) == 0
        assert lib.qcx_pauli_expectation_sum(None, 1, one, one, cf, None, C.byref(out)) == 2
        assert lib.qcx_pauli_expectation_sum(reg._h, 1, one, one, cf, None, None) == 2
        assert lib.qcx_pauli_expectation_sum(reg._h, 0, None, None, None, None, None) == 2
        assert lib.qcx_pauli_expectation_sum(reg._h, 1, None, one, cf, None, C.byref(out)) == 2
        assert lib.qcx_pauli_expectation_sum(reg._h, 1, one, None, cf, None, C.byref(out)) == 2
        assert lib.qcx_pauli_expectation_sum(reg._h, 1, one, one, None, None, C.byref(out)) == 2
        assert lib.qcx_pauli_expectation_sum(reg._h, 1, high, one, cf, None, C.byref(out)) == 6
        assert lib.qcx_pauli_expectation_sum(reg._h, 1, one, high, cf, None, C.byref(out)) == 6
        assert lib.qcx_pauli_expectation_sum(reg._h, 0, None, None, None, None, C.byref(out)) == 0 and bits(out.value) == 0
        assert lib.qcx_expectation_last_stats(None, None, None) == 2
        assert lib.qcx_expectation_last_stats(reg._h, None, None) == 0
        assert np.array_equal(bits(reg.read()), before)
        with pytest.raises(ValueError):
            reg.expectation("X" * 13)
    with qc.Register(13, 0, shards=4, devices=qc.spread_devices(4)) as sh:             # virtual shards on one GPU
        sh.fill_random(3)
        before = bits(sh.read())
        assert lib.qcx_pauli_expectation(sh._h, 1, 2, C.byref(out)) == 7                # QCX_UNSUPPORTED
        assert lib.qcx_pauli_expectation_sum(sh._h, 1, one, one, cf, None, C.byref(out)) == 7
        assert np.array_equal(bits(sh.read()), before)
