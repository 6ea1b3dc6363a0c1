"""GPU: the rotation about a Pauli string, exp(-i theta/2 P) (qcx_pauli_rotation, K15).  Every state must be, bit for bit, what
tests/pauli_rotation_ref.py defines on whatever the register held (a NaN exactly where the definition has one), in all three
shapes of the kernel -- no partner, the partner inside the tile, the partner in another tile --, behind every lazy form the
library keeps a state in, and a few results are checked against the existing gates and against physics with no reference."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

import pauli_rotation_ref as prr
from bitwise import bits, same_with_nans as same
from pauli_cases import PAIR_13, TILE_13, adversarial, g_of, with_every_g
from pauli_ref import pauli_masks, pauli_ref
from register_model import RegisterModel

pytestmark = pytest.mark.gpu

T = 12                                                              # the kernel's tiles: the 12 lowest index bits
THETAS = [0.0, math.pi, -0.7, 7.5, 0.3]                             # 0, pi, a negative value, one above 2 pi


def no_negative_zero(a):
    return not np.any((a == 0) & np.signbit(a))


def check_chained(qc, n, a, strings, run=None):
    """the strings one after the other on ONE register that starts as `a`, a read-back after every call, each compared with the
    definition on what the register held before it.  run: the start state is written again after every `run` calls (a NaN
    spreads to every row within a few strings; this keeps finite rows in the comparison)"""
    with qc.Register(n, 0) as reg:
        reg.write(a)
        have = a
        for k, (x, z) in enumerate(strings):
            if run and k and k % run == 0:
                reg.write(a)
                have = a
            theta = THETAS[k % len(THETAS)]
            qc.pauli_rotation((x, z), theta, reg)
            want = prr.apply(have, n, x, z, theta)
            have = reg.read()
            same(have, want)
            assert no_negative_zero(have[~np.isnan(have)]), (n, x, z)


def check_each(qc, n, a, strings):
    """every string on the freshly written state a"""
    check_chained(qc, n, a, strings, run=1)


# ---- small registers: a partial tile ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("finite", [True, False], ids=["finite", "inf-nan"])
def test_small_registers_every_string(qc, finite):
    for n in range(1, 6):
        strings = list(itertools.product(range(1 << n), repeat=2))
        check_chained(qc, n, adversarial(n, 31 * n, finite), strings, run=None if finite else 4)


@pytest.mark.parametrize("finite", [True, False], ids=["finite", "inf-nan"])
def test_small_registers_random_strings(qc, finite):
    for n in range(6, 12):
        rs = np.random.RandomState(1000 + n)
        strings = [(int(rs.randint(0, 1 << n)), int(rs.randint(0, 1 << n))) for _ in range(64)]
        check_chained(qc, n, adversarial(n, 31 * n, finite), strings, run=None if finite else 4)


# ---- the edges of the three shapes -------------------------------------------------------------------------------------------

def test_one_full_tile(qc):
    n = 12
    xs = [0, 1, 0x7, 0x8, 0x100, 0x800, 0xF00, 0xFFF, 0xA53]
    check_each(qc, n, adversarial(n, 5, True), with_every_g(xs, n, 1))
    check_each(qc, n, adversarial(n, 6), [(0, 0), (0xA53, 0x11), (0, 0xFFF)])
    check_chained(qc, n, adversarial(n, 5, True), with_every_g(xs, n, 11))


def test_two_tiles(qc):
    n = 13
    tile, pair = with_every_g(TILE_13, n, 2), with_every_g(PAIR_13, n, 3)
    assert all(x >> T == 0 for x, _ in tile) and all(x >> T for x, _ in pair)
    assert {g_of(x, z) for x, z in tile} == {0, 1, 2, 3} == {g_of(x, z) for x, z in pair}
    check_each(qc, n, adversarial(n, 7, True), tile + pair)
    check_each(qc, n, adversarial(n, 8), [(0, 0), (0x1000, 0), (0x1FFF, 0x1FFF), (0x130, 0x1030)])


def test_pairs_whose_partner_is_not_the_neighbour(qc):
    n = 14
    xs = [0x1000, 0x2000, 0x3000, 0x2007, 0x3081, 0x1F00, 0x3FFF, 0x0FFF]
    strings = with_every_g(xs, n, 4)
    assert {g_of(x, z) for x, z in strings if x >> T} == {0, 1, 2, 3}
    check_each(qc, n, adversarial(n, 9, True), strings)


# The grid is capped at 2048 workgroups (as K14's): n = 25 has 2^13 tiles and 2^12 pairs of tiles, so a workgroup takes more
# than one unit in every shape.  One string per shape.
N_BIG = 25
STRINGS_BIG = [(0, 0x1AAAAAA), (0x0000A53, 0x1000F01), (0x1800F03, 0x0AAAAAA)]


@pytest.fixture(scope="module")
def big_state(qc):
    """one fill_random state of n = 25, read once"""
    with qc.Register(N_BIG, 0) as reg:
        reg.fill_random(5)
        return reg.read()


@pytest.mark.parametrize("k", range(len(STRINGS_BIG)))
def test_more_than_one_unit_per_workgroup(qc, big_state, k):
    x, z = STRINGS_BIG[k]
    assert (x == 0, 0 < x < 1 << T, x >> T != 0) == tuple(k == s for s in range(3))
    assert (1 << (N_BIG - T)) // (2 if x >> T else 1) > 2048
    with qc.Register(N_BIG, 0) as reg:
        reg.fill_random(5)
        qc.pauli_rotation((x, z), THETAS[2 + k], reg)
        got = reg.read()
    want = prr.apply(big_state, N_BIG, x, z, THETAS[2 + k])
    assert np.array_equal(bits(got), bits(want))
    assert not np.array_equal(bits(got), bits(big_state))


def test_grid_caps_that_do_not_divide_the_units(qc):
    """prot_grid_cap = 1 and 3 at n = 14: one workgroup walks every unit, and three share four tiles / two pairs unevenly"""
    n = 14
    a = adversarial(n, 19, True)
    try:
        for cap in (1, 3):
            qc.tune(prot_grid_cap=cap)
            check_each(qc, n, a, [(0, 0x2AAA), (0xA53, 0x3011), (0x3081, 0x1085), (0x1000, 0x1000)])
    finally:
        qc.tune(prot_grid_cap=2048)


# ---- cross-checks that need no reference ------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [12, 14])
def test_one_letter_is_the_one_qubit_gate(qc, n):
    a = adversarial(n, 40 + n, True)
    with qc.Register(n, 0) as reg, qc.Register(n, 0) as twin:
        for k, (q, letter) in enumerate(itertools.product(range(n), "XYZ")):
            theta = THETAS[k % len(THETAS)]
            c, s = qc.polar(theta / 2)
            reg.write(a); twin.write(a)
            qc.pauli_rotation({q: letter}, theta, reg)
            qc.one_qubit_gate(q, prr.matrices(letter, c, s), twin)
            assert np.array_equal(bits(reg.read()), bits(twin.read())), (n, q, letter, theta)


@pytest.mark.parametrize("n", [12, 14])
def test_two_letters_are_the_two_qubit_gate(qc, n):
    a = adversarial(n, 50 + n, True)
    pairs = [(0, 1), (1, 0), (2, 7), (11, 3), (5, 11), (n - 1, 0), (3, n - 1), (n - 1, n - 2)]
    with qc.Register(n, 0) as reg, qc.Register(n, 0) as twin:
        for k, ((q0, q1), (l0, l1)) in enumerate(itertools.product(pairs, itertools.product("XYZ", repeat=2))):
            theta = THETAS[k % len(THETAS)]
            c, s = qc.polar(theta / 2)
            reg.write(a); twin.write(a)
            qc.pauli_rotation({q0: l0, q1: l1}, theta, reg)
            qc.two_qubit_gate(q0, q1, prr.matrix2(l0, l1, c, s), twin)
            assert np.array_equal(bits(reg.read()), bits(twin.read())), (n, q0, q1, l0, l1, theta)


# ---- physics ------------------------------------------------------------------------------------------------------------------

def test_rx_from_the_zero_state(qc):
    n = 14
    for q, theta in itertools.product((0, 5, 11, 13), (0.0, 0.4, -1.3, math.pi / 2, 7.5)):
        with qc.Register(n, 0) as reg:
            reg.write(np.eye(1, 2 << n)[0])
            qc.pauli_rotation({q: "X"}, theta, reg)
            assert abs(reg.expectation({q: "Z"}) - math.cos(theta)) <= 1e-12, (q, theta)
            assert abs(reg.expectation({q: "Y"}) + math.sin(theta)) <= 1e-12, (q, theta)


def test_expectation_of_the_axis_is_unchanged(qc):
    n = 14
    rs = np.random.RandomState(3)
    strings = [(0, 0x2001), (0x5, 0x4), (0x1000, 0x3000), (0x3FFF, 0x2AAA)]
    strings += [(int(rs.randint(0, 1 << n)), int(rs.randint(0, 1 << n))) for _ in range(8)]
    with qc.Register(n, 0) as reg:
        reg.fill_random(9)
        norm = reg.norm2()
        for k, s in enumerate(strings):
            before = reg.expectation(s)
            qc.pauli_rotation(s, THETAS[k % len(THETAS)] + 0.1, reg)
            assert abs(reg.expectation(s) - before) <= 1e-12, s
        assert abs(reg.norm2() - norm) <= 1e-12


def test_zz_is_cnot_rz_cnot(qc):
    n = 14
    for a, b in ((0, 1), (3, 11), (13, 2), (12, 13)):
        theta = 0.1 + 0.37 * a
        with qc.Register(n, 0) as reg, qc.Register(n, 0) as twin:
            reg.fill_random(4); twin.fill_random(4)
            qc.pauli_rotation({a: "Z", b: "Z"}, theta, reg)
            qc.two_qubit_gate(a, b, qc.GATES2["CNOT"], twin)
            qc.one_qubit_gate(b, qc.rz(theta), twin)
            qc.two_qubit_gate(a, b, qc.GATES2["CNOT"], twin)
            assert np.max(np.abs(reg.read() - twin.read())) <= 1e-12, (a, b)


# ---- lazy forms and modes ---------------------------------------------------------------------------------------------------

def test_pending_basis_state(qc):
    n = 14
    strings = [(0, 0), (0, 0x2A51), (1, 1), (0x1000, 0), (0x1003, 0x3001), (0x2A51, 0x0F0F)]
    with qc.Register(n - 4, 4) as reg:
        for k, (x, z) in itertools.product((1, 0x2A51), strings):
            if k == 1:
                qc.reset_register(reg)                               # pending basis state |1>
            else:
                e = np.zeros(2 << n); e[2 * k] = 1.0                 # a collapse leaves the pending basis state k
                reg.write(e)
                assert qc.measure_state(reg, 0.5) == k
            assert reg.expectation((0, 0)) == 1.0 and reg.expectation_stats() == (2, 0), "the basis state is still pending"
            e = np.zeros(2 << n); e[2 * k] = 1.0
            qc.pauli_rotation((x, z), 0.9, reg)
            same(reg.read(), prr.apply(e, n, x, z, 0.9))


def queue_some_gates(qc, ob, reg, want, n):
    for q in (0, 3, n - 1):
        qc.hadamard_gate(q, reg)
        ob.hadamard(want, n, q)
    qc.c_phase_shift_gate(3, n - 1, 0.7, reg)
    ob.cphase(want, n, 3, n - 1, 0.7)


def test_queued_gates_are_flushed_first(qc, ob):
    n = 14
    with qc.Register(n - 4, 4) as reg:
        reg.set_fusion(1)
        reg.fill_random(8)
        want = ob.fill_random(n, 8)
        queue_some_gates(qc, ob, reg, want, n)
        s0 = reg.fusion_stats()
        reg.flush()
        flush_counts = tuple(x - y for x, y in zip(reg.fusion_stats(), s0))
        assert flush_counts != (0, 0)
        for x, z in ((0, 0x2009), (0x9, 0x8), (0x2008, 0x2001)):
            reg.fill_random(8)
            want = ob.fill_random(n, 8)
            queue_some_gates(qc, ob, reg, want, n)
            before = reg.fusion_stats()
            qc.pauli_rotation((x, z), -0.7, reg)
            assert tuple(x_ - y_ for x_, y_ in zip(reg.fusion_stats(), before)) == flush_counts, "nothing is counted for the rotation"
            want = prr.apply(want, n, x, z, -0.7)
            qc.hadamard_gate(1, reg); ob.hadamard(want, n, 1)        # queued behind it
            same(reg.read(), want)


def test_mode_2_gives_the_bits_of_mode_0(qc):
    n = 14
    for x, z in ((0, 0x3FFF), (0xA53, 0x11), (0x3081, 0x2080)):
        got = []
        for mode in (0, 2):
            with qc.Register(n, 0) as reg:
                reg.set_fusion(mode)
                reg.fill_random(6)
                a = reg.read()
                qc.pauli_rotation((x, z), 7.5, reg)
                got.append(reg.read())
        assert np.array_equal(bits(got[0]), bits(got[1]))
        same(got[0], prr.apply(a, n, x, z, 7.5))


def test_compact_result_is_expanded_first(qc):
    L, M, Cn, a = 15, 5, 21, 2                                      # (the compact chain runs from n = 20 on)
    n = L + M
    for x, z in ((0, 0x81234), (0x3 << M, 0x1F), (0x81234, 0x80F31)):
        with qc.Register(L, M) as flushed:
            qc.reset_register(flushed); qc.quantum_computation(Cn, a, flushed)
            flushed.flush()
            state = flushed.read()
            qc.pauli_rotation((x, z), 0.3, flushed)
            want = flushed.read()
        with qc.Register(L, M) as reg:
            qc.reset_register(reg); qc.quantum_computation(Cn, a, reg)
            qc.pauli_rotation((x, z), 0.3, reg)
            got = reg.read()
        assert np.array_equal(bits(got), bits(want))
        same(got, prr.apply(state, n, x, z, 0.3))
        assert not np.array_equal(bits(got), bits(state))


def test_nonfinite_register(qc, ob):
    n = 13
    a = ob.random_state(n, 21)
    a[2 * 700] = np.inf
    a[2 * 5] = -0.0
    b = a.copy()
    b[2 * 3000 + 1] = np.nan
    strings = [(0, 0), (0, 0x1FFF), (0x1000, 0), (0x4, 0x4), (0x1234, 0x0F0F), (0x2BC ^ 0x1000, 0x1000)]
    for state in (a, b):
        for x, z in strings:
            with qc.Register(n, 0) as reg:
                reg.write(state)
                qc.pauli_rotation((x, z), -0.7, reg)
                w = prr.apply(state, n, x, z, -0.7)
                got = reg.read()
                same(got, w)
                bad = ~np.isfinite(got.view(np.complex128).real) | ~np.isfinite(got.view(np.complex128).imag)
                assert set(np.flatnonzero(bad)) <= {700, 700 ^ x, 3000, 3000 ^ x} and bad[700] and bad[700 ^ x]
                qc.hadamard_gate(2, reg)                            # the flag is kept: still the strict gate, the oracle's products
                ob.hadamard(w, n, 2)
                same(reg.read(), w)


def test_negative_zeros_do_not_survive(qc, ob):
    n = 13
    rs = np.random.RandomState(12)
    a = ob.random_state(n, 22)
    a[rs.randint(0, a.size, a.size // 2)] = -0.0
    for state in (a, np.full(2 << n, -0.0)):
        for x, z in ((0, 0), (0, 0x1001), (0x41, 0x1040), (0x1000, 0x1000), (0x1FFF, 0)):
            with qc.Register(n, 0) as reg:
                reg.write(state)
                qc.pauli_rotation((x, z), 0.3, reg)
                got = reg.read()
                assert no_negative_zero(got), (x, z)
                w = prr.apply(state, n, x, z, 0.3)
                same(got, w)
                qc.hadamard_gate(12, reg)                           # nothing is owed to the next gate
                ob.hadamard(w, n, 12)
                same(reg.read(), w)


# ---- a short random sequence -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [1, 2])
def test_random_sequence(qc, ob, seed):
    n = 13
    rs = np.random.RandomState(500 + seed)
    m = RegisterModel(ob, n, 0)
    with qc.Register(n, 0) as reg:
        reg.set_fusion([-1, 0, 1][seed % 3])
        reg.fill_random(seed); m.fill_random(seed)
        for step in range(40):
            k = int(rs.randint(0, 10))
            if k < 5:
                x = int(rs.randint(0, 1 << n)) if rs.randint(0, 4) else 0
                if rs.randint(0, 3) == 0:
                    x &= 0xFFF
                z, theta = int(rs.randint(0, 1 << n)), float(rs.uniform(-7, 7))
                qc.pauli_rotation((x, z), theta, reg)
                m.a = prr.apply(m.a, n, x, z, theta)
            elif k == 5:
                q = int(rs.randint(0, n))
                qc.hadamard_gate(q, reg); m.hadamard_gate(q)
            elif k == 6:
                c, t = (int(v) for v in rs.choice(n, 2, replace=False))
                theta = float(rs.uniform(-3, 3))
                qc.c_phase_shift_gate(c, t, theta, reg); m.c_phase_shift_gate(c, t, theta)
            elif k == 7:
                q = int(rs.randint(0, n))
                U, _ = np.linalg.qr(rs.standard_normal((2, 2)) + 1j * rs.standard_normal((2, 2)))
                qc.one_qubit_gate(q, U, reg); m.one_qubit_gate(q, U)
            elif k == 8:
                x, z = int(rs.randint(0, 1 << n)), int(rs.randint(0, 1 << n))
                same(reg.expectation((x, z)), pauli_ref(m.a, n, x, z))
            else:
                first = int(rs.randint(0, n))
                outcome = int(np.argmax(m.marginal(first, 1)))
                p, status = m.postselect(first, 1, outcome)
                assert status == 0
                same(reg.postselect(first, 1, outcome), p)
            if step % 4 == 3:
                same(reg.read(), m.a)
        same(reg.read(), m.a)


# ---- arguments --------------------------------------------------------------------------------------------------------------

def test_arguments(qc):
    lib = qc.lib()
    with qc.Register(12, 0) as reg:
        reg.fill_random(1)
        before = bits(reg.read())
        assert lib.qcx_pauli_rotation(1, 0, 0.5, None) == 2                             # QCX_BAD_ARGUMENTS
        assert lib.qcx_pauli_rotation(1, 0, float("nan"), reg._h) == 2
        assert lib.qcx_pauli_rotation(1, 0, float("inf"), reg._h) == 2
        assert lib.qcx_pauli_rotation(0, 0, float("-inf"), reg._h) == 2
        assert lib.qcx_pauli_rotation(1 << 12, 0, 0.5, reg._h) == 6                     # QCX_BAD_QUBIT
        assert lib.qcx_pauli_rotation(0, 1 << 12, 0.5, reg._h) == 6
        assert lib.qcx_pauli_rotation(0, 1 << 63, 0.5, reg._h) == 6
        assert lib.qcx_pauli_rotation(1 << 63, 0, 0.5, reg._h) == 6
        assert np.array_equal(bits(reg.read()), before)
        with pytest.raises(ValueError):
            qc.pauli_rotation("X" * 13, 0.5, reg)
        assert np.array_equal(bits(reg.read()), before)
        assert lib.qcx_pauli_rotation(1 << 11, 1 << 11, 0.5, reg._h) == 0
        assert not np.array_equal(bits(reg.read()), before)
        assert lib.qcx_shard_pauli_rotation(None, 12, 1, 0, 1.0, 0.0, None) == 2
        dev = C.c_void_p(lib.qcx_device_pointer(reg._h))
        assert lib.qcx_shard_pauli_rotation(dev, 12, 1 << 12, 0, 1.0, 0.0, None) == 6
    with qc.Register(13, 0, shards=4, devices=qc.spread_devices(4)) as sh:             # virtual shards on one GPU
        sh.fill_random(3)
        before = bits(sh.read())
        assert lib.qcx_pauli_rotation(1, 2, 0.5, sh._h) == 7                            # QCX_UNSUPPORTED
        assert np.array_equal(bits(sh.read()), before)


def test_the_shard_form_is_the_launch_alone(qc):
    """qcx_shard_pauli_rotation on the register's own memory, c and s given: the bits of the definition with those c and s"""
    n = 13
    lib = qc.lib()
    with qc.Register(n, 0) as reg:
        reg.fill_random(2)
        a = reg.read()
        c, s = qc.polar(0.45)
        dev = C.c_void_p(lib.qcx_device_pointer(reg._h))
        reg.synchronize()
        assert lib.qcx_shard_pauli_rotation(dev, n, 0x1041, 0x0043, c, s, None) == 0      # (the default stream: ordered with the register's)
        same(reg.read(), prr.apply_cs(a, n, 0x1041, 0x0043, c, s))
