"""GPU: qcx_pauli_expectation_batch (K14b) -- the terms of a call that share an x_mask from one read of the state.  Every value
must be, bit for bit, what tests/pauli_ref.py defines and what qcx_pauli_expectation gives for that term alone (a NaN where the
definition has one), in every shape of the first stage, for full and for split groups, with even and odd powers of i in one
pass; the reads must be the plan's passes; the state and its lazy forms must stay as they were."""
import ctypes as C
import itertools

import numpy as np
import pytest

from bitwise import bits, same_with_nans as same
from pauli_cases import PAIR_13, TILE_13, adversarial, g_of, with_every_g
from pauli_ref import pauli_masks, pauli_ref, pauli_sum_ref

pytestmark = pytest.mark.gpu

T = 12                                                              # the first stage's tiles: the 12 lowest index bits


def reads_of(qc, strings):
    return qc.pauli_batch_plan([x for x, _ in strings])[1]


def check_batch(qc, n, a, strings, against_single=False):
    """all strings in one call on the written state a, against the definition term by term; then: the state is what it was"""
    with qc.Register(n, 0) as reg:
        reg.write(a)
        _, values = reg.expectation_batch([(1.0, s) for s in strings])
        assert reg.expectation_stats() == (0, reads_of(qc, strings))
        same(values, [pauli_ref(a, n, x, z) for x, z in strings], f"n = {n}")
        if against_single:
            same(values, [reg.expectation(s) for s in strings], f"n = {n}, term by term")
        assert np.array_equal(bits(reg.read()), bits(a)), "the state changed"


# ---- small registers: a partial tile ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("finite", [True, False], ids=["finite", "inf-nan"])
def test_small_registers_every_string(qc, finite):
    for n in range(1, 5):
        check_batch(qc, n, adversarial(n, 31 * n, finite), list(itertools.product(range(1 << n), repeat=2)))


@pytest.mark.parametrize("finite", [True, False], ids=["finite", "inf-nan"])
def test_small_registers_full_groups(qc, finite):
    for n in range(6, 12):
        rs = np.random.RandomState(2000 + n)
        xs = [0, 1 << (n - 1)] + [int(rs.randint(1, 1 << n)) for _ in range(3)]
        strings = [(xs[rs.randint(len(xs))], int(rs.randint(0, 1 << n))) for _ in range(64)]
        check_batch(qc, n, adversarial(n, 31 * n, finite), strings)


# ---- the edges of the three shapes --------------------------------------------------------------------------------------------

def test_one_and_two_full_tiles(qc):
    xs12 = [0, 1, 0x7, 0x8, 0x100, 0x800, 0xF00, 0xFFF, 0xA53]
    check_batch(qc, 12, adversarial(12, 5, True), with_every_g(xs12, 12, 1), True)
    check_batch(qc, 12, adversarial(12, 6), [(0, 0), (0xA53, 0x11), (0, 0xFFF), (0xA53, 0xFFF)])
    n = 13
    strings = with_every_g(TILE_13, n, 2) + with_every_g(PAIR_13, n, 3)
    # even and odd powers of i in one pass, and the three shapes in one call
    for x in (0x7, 0xFFF, 0x1007, 0x1FFF):
        assert {g_of(x, z) for xx, z in strings if xx == x} == {0, 1, 2, 3}
    assert {0 if x == 0 else 1 + (x >> T) for x, _ in strings} == {0, 1, 2}
    check_batch(qc, n, adversarial(n, 7, True), strings, True)
    check_batch(qc, n, adversarial(n, 8), [(0, 0), (0x1000, 0), (0x1FFF, 0x1FFF), (0x130, 0x1030), (0x1000, 0x1000), (0, 0x1FFF)])


def test_pairs_whose_partner_is_not_the_neighbour(qc):
    n = 14
    xs = [0x1000, 0x2000, 0x3000, 0x2007, 0x3081, 0x1F00, 0x3FFF, 0x0FFF]
    strings = with_every_g(xs, n, 4)
    assert {g_of(x, z) for x, z in strings if x >> T} == {0, 1, 2, 3}
    check_batch(qc, n, adversarial(n, 9, True), strings, True)


@pytest.mark.parametrize("count", ["W", "W + 1", "2 W + 3"])
def test_full_and_split_groups(qc, count):
    n = 13
    W = qc.pauli_batch_width()
    k = {"W": W, "W + 1": W + 1, "2 W + 3": 2 * W + 3}[count]
    rs = np.random.RandomState(k)
    strings = []
    for _ in range(k):                                              # the three shapes take turns: every pass is found again
        for x in (0, 0x130, 0x1130):
            while True:
                s = (x, int(rs.randint(0, 1 << n)))
                if s not in strings:
                    break
            strings.append(s)
    a = adversarial(n, 40 + k, True)
    with qc.Register(n, 0) as reg:
        reg.write(a)
        _, values = reg.expectation_batch([(1.0, s) for s in strings])
        assert reg.expectation_stats() == (0, reads_of(qc, strings)) == (0, 3 * -(-k // W))
        same(values, [reg.expectation(s) for s in strings])
        assert reg.expectation_stats() == (0, 1)
        same(values, [pauli_ref(a, n, x, z) for x, z in strings])
        assert np.array_equal(bits(reg.read()), bits(a))


def test_duplicates_and_order(qc):
    n = 13
    strings = with_every_g([0, 0x5, 0x1F00], n, 11)
    strings = strings + strings[:5] + [strings[2]] * 3
    a = adversarial(n, 12, True)
    perm = np.random.RandomState(3).permutation(len(strings))
    with qc.Register(n, 0) as reg:
        reg.write(a)
        _, values = reg.expectation_batch([(1.0, s) for s in strings])
        same(values, [pauli_ref(a, n, x, z) for x, z in strings])
        _, permuted = reg.expectation_batch([(1.0, strings[k]) for k in perm])
        same(permuted, values[perm])
        assert np.array_equal(bits(reg.read()), bits(a))


# ---- three stages -----------------------------------------------------------------------------------------------------------

N3 = 25                                                             # the first size with three stages (12 + 12 + 1 bits)
# (test_gpu_pauli_expectation.STRINGS_25)
STRINGS_25 = [(0, 0), (0, (1 << N3) - 1), (0x20, 0x1000001), (1 << 24, 0), (0x1FFFFFF, 0x0AAAAAA), (0x1800F03, 0x1000F01)]
AGAINST_REF_25 = [1, 2, 4]                                          # one term per shape


def test_three_stages(qc):
    rs = np.random.RandomState(25)
    strings = list(STRINGS_25)
    for x in (0, 1 << 24):
        strings += [(x, int(rs.randint(0, 1 << N3))) for _ in range(20)]
    with qc.Register(N3, 0) as reg:
        reg.fill_random(5)
        _, values = reg.expectation_batch([(1.0, s) for s in strings])
        assert reg.expectation_stats() == (0, reads_of(qc, strings)) == (0, 5)
        same(values, [reg.expectation(s) for s in strings])
        a = reg.read().view(np.complex128)
    for k in AGAINST_REF_25:
        same(values[k], pauli_ref(a, N3, *strings[k]))


# ---- totals -----------------------------------------------------------------------------------------------------------------

def test_totals(qc):
    n = 13
    a = adversarial(n, 77, True)
    terms = [(1e16, ""), (0.5, {0: "Z", 12: "Z"}), (-1e16, (0, 0)), (-0.3, "XYZ" * 4 + "X"), (2.0, (0x1030, 0x0031)),
             (0.0, {3: "Z"}), (0.25, (0x1030, 0x1001)), (-7.0, "XYZ" * 4 + "Y")]
    ref_terms = [(c,) + pauli_masks(p, n) for c, p in terms]
    want_total, want_values = pauli_sum_ref(a, n, ref_terms)
    with qc.Register(n, 0) as reg:
        reg.write(a)
        total, values = reg.expectation_batch(terms)
        assert reg.expectation_stats() == (0, reads_of(qc, [t[1:] for t in ref_terms])) == (0, 3)
        same(values, want_values)
        same(total, want_total)
        same([total], [reg.expectation_sum(terms)[0]])
        # an infinite coefficient: Inf * value, and NaN where the value is 0
        inf_terms = terms[:4] + [(np.inf, (0, 0)), (-np.inf, {0: "Z", 12: "Z"})] + terms[4:]
        want_total, want_values = pauli_sum_ref(a, n, [(c,) + pauli_masks(p, n) for c, p in inf_terms])
        total, values = reg.expectation_batch(inf_terms)
        same(values, want_values)
        same(total, want_total)
        # values may be NULL
        lib = qc.lib()
        k = len(ref_terms)
        xs = (C.c_uint64 * k)(*[t[1] for t in ref_terms]); zs = (C.c_uint64 * k)(*[t[2] for t in ref_terms])
        cs = (C.c_double * k)(*[t[0] for t in ref_terms])
        tot = C.c_double(-1.0)
        assert lib.qcx_pauli_expectation_batch(reg._h, k, xs, zs, cs, None, C.byref(tot)) == 0
        same(tot.value, pauli_sum_ref(a, n, ref_terms)[0])
        assert np.array_equal(bits(reg.read()), bits(a))


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
            for _ in range(2):                                       # ... and it is still pending at the next call
                _, values = reg.expectation_batch([(1.0, s) for s in strings])
                assert reg.expectation_stats() == (2, 0)
                same(values, [pauli_ref(e, n, x, z) for x, z in strings])
                same(values, [0.0 if x else (-1.0) ** bin(k & z).count("1") for x, z in strings])
            assert np.array_equal(bits(reg.read()), bits(e))
        qc.reset_register(reg)
        qc.hadamard_gate(0, reg)                                     # no longer a basis state: a kernel reads the register
        _, values = reg.expectation_batch([(1.0, "X"), (1.0, "Z")])
        assert abs(values[0] + 1) <= 1e-12 and abs(values[1]) <= 1e-12
        assert reg.expectation_stats() == (0, 2)


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
        specs = [{0: "X", 3: "Y", n - 1: "X"}, {3: "X", n - 1: "Y"}, {0: "X"}, {1: "Z"}, {0: "X", 3: "X", n - 1: "Y"}, {2: "Z", 5: "Z"}]
        _, values = reg.expectation_batch([(1.0, s) for s in specs])
        assert reg.expectation_stats() == (0, 4)
        same(values, [pauli_ref(want, n, *pauli_masks(s, n)) for s in specs])
        assert abs(values[2] + 1) <= 1e-12 and abs(values[3] - 1) <= 1e-12       # (qubit 0: H|1> = |->)
        assert np.array_equal(bits(reg.read()), bits(want))


def test_compact_result_is_expanded_first(qc, ob):
    L, M, Cn, a = 15, 5, 21, 2                                      # (the compact chain runs from n = 20 on)
    n = L + M
    strings = [(0, 0), (0, 1 << M), (1 << (n - 1), 0), (0x3 << M, 0x1F), (0x81234, 0x80F31), (0, 0x1F), (1 << (n - 1), 1 << (n - 1))]

    def compact_measures(reg):
        v = C.c_ulong(0)
        assert qc.lib().qcx_compact_measure_stats(reg._h, C.byref(v)) == 0
        return int(v.value)

    with qc.Register(L, M) as flushed:
        qc.reset_register(flushed); qc.quantum_computation(Cn, a, flushed)
        flushed.flush()
        want = [flushed.expectation(s) for s in strings]
        state = flushed.read()
    with qc.Register(L, M) as reg:
        qc.reset_register(reg); qc.quantum_computation(Cn, a, reg)
        c0 = compact_measures(reg)
        for _ in range(2):                                           # it stays compact: the second call finds what the first did
            _, values = reg.expectation_batch([(1.0, s) for s in strings])
            assert reg.expectation_stats() == (3, reads_of(qc, strings)) == (3, 4)
            same(values, want)
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
    strings = [(0, 0), (0, 0x1FFF), (0x1000, 0), (0x4, 0x4), (0x1234, 0x0F0F), (0x2BC ^ 0x1000, 0x1000), (0x1000, 0x1FFF), (0x4, 0)]
    for state in (a, b):
        with qc.Register(n, 0) as reg:
            reg.write(state)
            _, values = reg.expectation_batch([(1.0, s) for s in strings])
            same(values, [pauli_ref(state, n, x, z) for x, z in strings])
            qc.hadamard_gate(2, reg)                                # still the strict gate: the oracle's products, NaN/Inf included
            w = state.copy(); ob.hadamard(w, n, 2)
            got = reg.read()
            gn, wn = np.isnan(got), np.isnan(w)
            assert np.array_equal(gn, wn)
            assert np.array_equal(bits(got[~gn]), bits(w[~wn]))


# ---- arguments --------------------------------------------------------------------------------------------------------------

def test_arguments(qc):
    lib = qc.lib()
    out = C.c_double(0.0)
    one = (C.c_uint64 * 1)(0)
    cf = (C.c_double * 1)(1.0)
    ok3, bad3 = (C.c_uint64 * 3)(0, 1, 0), (C.c_uint64 * 3)(0, 1, 1 << 12)
    cf3, val3 = (C.c_double * 3)(1.0, 1.0, 1.0), (C.c_double * 3)(7.0, 7.0, 7.0)
    batch = lib.qcx_pauli_expectation_batch
    with qc.Register(12, 0) as reg:
        reg.fill_random(1)
        before = bits(reg.read())
        assert batch(None, 1, one, one, cf, None, C.byref(out)) == 2                    # QCX_BAD_ARGUMENTS
        assert batch(reg._h, 1, one, one, cf, None, None) == 2
        assert batch(reg._h, 0, None, None, None, None, None) == 2
        assert batch(reg._h, 1, None, one, cf, None, C.byref(out)) == 2
        assert batch(reg._h, 1, one, None, cf, None, C.byref(out)) == 2
        assert batch(reg._h, 1, one, one, None, None, C.byref(out)) == 2
        assert np.array_equal(bits(reg.read()), before)
        # a bad mask in the last term: nothing ran -- the statistics and the queued gates are what they were
        reg.expectation((1, 1))
        assert reg.expectation_stats() == (0, 1)
        reg.set_fusion(1)
        qc.hadamard_gate(0, reg)
        g0 = reg.fusion_stats()
        assert batch(reg._h, 3, bad3, ok3, cf3, val3, C.byref(out)) == 6                # QCX_BAD_QUBIT
        assert batch(reg._h, 3, ok3, bad3, cf3, val3, C.byref(out)) == 6
        assert list(val3) == [7.0, 7.0, 7.0]
        assert reg.expectation_stats() == (0, 1) and reg.fusion_stats() == g0
        # no term: +0.0, nothing runs
        out.value = -1.0
        assert batch(reg._h, 0, None, None, None, None, C.byref(out)) == 0 and bits(out.value) == 0
        total, values = reg.expectation_batch([])
        assert bits(total) == 0 and values.size == 0
        assert reg.expectation_stats() == (0, 0) and reg.fusion_stats() == g0
        with pytest.raises(ValueError):
            reg.expectation_batch([(1.0, "X" * 13)])
    with qc.Register(13, 0, shards=4, devices=qc.spread_devices(4)) as sh:             # virtual shards on one GPU
        sh.fill_random(3)
        before = bits(sh.read())
        assert batch(sh._h, 1, one, one, cf, None, C.byref(out)) == 7                   # QCX_UNSUPPORTED
        assert np.array_equal(bits(sh.read()), before)
