"""GPU: a diagonal operator on a qubit range from a table (qcx_diagonal_gate / qcx_diagonal_gate_device, K18).  Every state must
be, bit for bit, what tests/diagonal_ref.py defines on whatever the register held (a NaN exactly where the definition has one),
in every form of the kernel -- one entry per tile, uniform entries inside a tile, an entry per lane, the partial tile --, with
the table in host and in device memory, behind every lazy form the library keeps a state in; a few results are checked against
the existing gates and against physics with no reference."""
import ctypes as C
import math

import numpy as np
import pytest

import diagonal_ref as dr
import pauli_rotation_ref as prr
import sequence_replay as sr
from bitwise import bits, same_with_nans as same
from pauli_cases import adversarial

pytestmark = pytest.mark.gpu

BAD_ARGUMENTS, BAD_QUBIT, UNSUPPORTED = 2, 6, 7


def no_negative_zero(a):
    return not np.any((a == 0) & np.signbit(a))


def unit_table(rs, num):
    """random phases, with a few entries that are exact: 1, -1, i, 0"""
    ph = rs.uniform(-np.pi, np.pi, 1 << num)
    t = np.clip(np.cos(ph), -1, 1) + 1j * np.clip(np.sin(ph), -1, 1)
    special = [1.0, -1.0, 1j, 0.0]
    for k in rs.randint(0, 1 << num, min(4, 1 << num)):
        t[k] = special[int(rs.randint(0, 4))]
    return t


def check_chained(qc, n, a, shapes, seed, run=None):
    """the shapes (first, num), each with a table of its own, one after the other on ONE register that starts as `a`, a read-back
    after every call, each compared with the definition on what the register held before it.  run: the start state is written
    again after every `run` calls"""
    rs = np.random.RandomState(seed)
    with qc.Register(n, 0) as reg:
        reg.write(a)
        have = a
        for k, (first, num) in enumerate(shapes):
            if run and k and k % run == 0:
                reg.write(a)
                have = a
            t = unit_table(rs, num)
            qc.diagonal_gate(first, num, t, reg)
            want = dr.apply(have, n, first, num, t)
            have = reg.read()
            same(have, want, f"n={n} first={first} num={num}")
            assert no_negative_zero(have[~np.isnan(have)]), (n, first, num)
            st, pl = qc.diagonal_plan(n, first, num)
            assert reg.diagonal_stats() == (pl.form, 1 << num)


def check_each(qc, n, a, shapes, seed):
    check_chained(qc, n, a, shapes, seed, run=1)


def every_shape(n):
    return [(first, num) for first in range(n + 1) for num in range(n - first + 1)]


# ---- small registers: a partial tile ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("finite", [True, False], ids=["finite", "inf-nan"])
def test_small_registers_every_range(qc, finite):
    for n in range(1, 6):
        check_chained(qc, n, adversarial(n, 31 * n, finite), every_shape(n), 10 + n)


@pytest.mark.parametrize("finite", [True, False], ids=["finite", "inf-nan"])
def test_small_registers_random_ranges(qc, finite):
    for n in range(6, 12):
        rs = np.random.RandomState(1000 + n)
        shapes = [(0, n), (n, 0), (n - 1, 1)]
        if n > 8:
            shapes += [(8, n - 8), (8, 1), (n - 1, 0)]
        for _ in range(24):
            first = int(rs.randint(0, n + 1))
            shapes.append((first, int(rs.randint(0, n - first + 1))))
        check_chained(qc, n, adversarial(n, 31 * n, finite), shapes, 20 + n, run=None if finite else 6)


# ---- the edges of the forms --------------------------------------------------------------------------------------------------

def test_one_full_tile(qc):
    n = 12
    shapes = [(0, 12), (0, 1), (7, 2), (8, 4), (11, 1), (3, 0)]
    check_each(qc, n, adversarial(n, 5, True), shapes, 1)
    check_each(qc, n, adversarial(n, 6), shapes, 2)
    check_chained(qc, n, adversarial(n, 5, True), shapes, 3)


@pytest.mark.parametrize("n", [13, 14])
def test_tiles_with_different_entries(qc, n):
    shapes = [s for s in [(0, 13), (0, 14), (3, 11), (10, 4), (11, 2), (12, 1), (12, 2), (13, 1)] if s[0] + s[1] <= n]
    assert len(shapes) == (3 if n == 13 else 8)                     # n = 13: (0, 13), (11, 2), (12, 1)
    check_each(qc, n, adversarial(n, 7 + n, True), shapes, 4)
    check_each(qc, n, adversarial(n, 8 + n), shapes, 5)


@pytest.mark.parametrize("lds", [0, 1])
def test_grid_caps_that_do_not_divide_the_units(qc, lds):
    """diag_grid_cap = 3 and 5 at n = 16: 16 tiles, shared unevenly; with diag_lds the per-lane form's other variant"""
    n = 16
    a = adversarial(n, 19, True)
    shapes = [(0, 16), (0, 12), (2, 9), (5, 7), (7, 9), (8, 4), (9, 7), (12, 4), (15, 1), (4, 0)]
    try:
        qc.tune(diag_lds=lds)
        for cap in (3, 5):
            qc.tune(diag_grid_cap=cap)
            check_each(qc, n, a, shapes, 6 + cap)
    finally:
        qc.tune(diag_grid_cap=2048, diag_lds=0)


# The grid is capped at 2048 workgroups: n = 25 has 2^13 tiles, so a workgroup takes more than one unit.  One shape per form, and
# the per-lane form both with a table that a tile covers and with one it does not.
N_BIG = 25
SHAPES_BIG = [(14, 6), (9, 5), (2, 8), (3, 15)]


@pytest.fixture(scope="module")
def big_state(qc):
    """one fill_random state of n = 25, read once"""
    with qc.Register(N_BIG, 0) as reg:
        reg.fill_random(5)
        return reg.read()


@pytest.mark.parametrize("k", range(len(SHAPES_BIG)))
def test_more_than_one_unit_per_workgroup(qc, big_state, k):
    first, num = SHAPES_BIG[k]
    st, pl = qc.diagonal_plan(N_BIG, first, num)
    assert st == 0 and pl.form == (0, 1, 2, 2)[k] and pl.units > pl.grid == 2048
    t = unit_table(np.random.RandomState(70 + k), num)
    with qc.Register(N_BIG, 0) as reg:
        reg.fill_random(5)
        qc.diagonal_gate(first, num, t, reg)
        got = reg.read()
    want = dr.apply(big_state, N_BIG, first, num, t)
    assert np.array_equal(bits(got), bits(want))
    assert not np.array_equal(bits(got), bits(big_state))


def test_the_host_maximum(qc):
    n = 20
    assert qc.diagonal_host_max_qubits() == n
    t = unit_table(np.random.RandomState(8), n)
    with qc.Register(n, 0) as reg:
        reg.fill_random(2)
        a = reg.read()
        qc.diagonal_gate(0, n, t, reg)
        t[:] = 0                                                     # the caller may reuse the table at once
        got = reg.read()
    same(got, dr.apply(a, n, 0, n, unit_table(np.random.RandomState(8), n)))


def test_host_tables_back_to_back(qc):
    """the second call's copy must not overtake the first call's kernel, nor its host copy the first call's transfer"""
    n = 16
    rs = np.random.RandomState(9)
    tabs = [(0, 16, unit_table(rs, 16)), (3, 2, unit_table(rs, 2)), (0, 16, unit_table(rs, 16)), (8, 8, unit_table(rs, 8))]
    with qc.Register(n, 0) as reg:
        reg.fill_random(3)
        want = reg.read()
        for first, num, t in tabs:
            qc.diagonal_gate(first, num, t.copy(), reg)
        for first, num, t in tabs:
            want = dr.apply(want, n, first, num, t)
        same(reg.read(), want)


# ---- the table in device memory ----------------------------------------------------------------------------------------------

def test_device_tables(qc):
    import torch
    n = 14
    rs = np.random.RandomState(11)
    a = adversarial(n, 23, True)
    with qc.Register(n, 0) as reg, qc.Register(n, 0) as twin:
        for first, num in ((0, 14), (2, 9)):
            t = unit_table(rs, num)
            dev = torch.from_numpy(t).cuda()
            torch.cuda.synchronize()
            reg.write(a); twin.write(a)
            qc.diagonal_gate(first, num, dev, reg)
            qc.diagonal_gate(first, num, t, twin)
            got = reg.read()
            same(got, dr.apply(a, n, first, num, t))
            assert np.array_equal(bits(got), bits(twin.read()))
            assert reg.diagonal_stats() == twin.diagonal_stats()
            # an integer pointer
            reg.write(a)
            qc.diagonal_gate(first, num, int(dev.data_ptr()), reg)
            assert np.array_equal(bits(reg.read()), bits(got))
        # what the wrapper refuses by itself
        with pytest.raises(TypeError):
            qc.diagonal_gate(0, 2, torch.zeros(4, dtype=torch.complex64).cuda(), reg)
        with pytest.raises(ValueError):
            qc.diagonal_gate(0, 2, torch.zeros(8, dtype=torch.complex128).cuda(), reg)
        with pytest.raises(ValueError):
            qc.diagonal_gate(0, 2, torch.zeros(4, dtype=torch.complex128), reg)
        with pytest.raises(ValueError):
            qc.diagonal_gate(0, 2, torch.zeros(8, dtype=torch.complex128).cuda()[::2], reg)


def test_device_table_refusals(qc):
    import torch
    n = 14
    lib = qc.lib()
    with qc.Register(n, 0) as reg:
        reg.fill_random(4)
        before = bits(reg.read())
        ptr = reg.device_pointer()
        # overlap with the register's buffer: its start, its middle, and a range that ends inside it
        for address, num in ((ptr, 3), (ptr + 16 * 5000, 0), (ptr + (16 << n) - 16, 0)):
            assert lib.qcx_diagonal_gate_device(0, num, C.c_void_p(address), reg._h) == BAD_ARGUMENTS
            assert b"overlaps" in lib.qcx_last_error()
            assert np.array_equal(bits(reg.read()), before)
        # a host address
        host = np.ones(2 << 4)
        assert lib.qcx_diagonal_gate_device(0, 4, host.ctypes.data_as(C.c_void_p), reg._h) == BAD_ARGUMENTS
        assert b"not device memory" in lib.qcx_last_error()
        assert np.array_equal(bits(reg.read()), before)
        # an Inf, a NaN and a component above 1
        for bad in (complex(np.inf, 0), complex(0, np.nan), complex(0, -1.0000001)):
            t = np.ones(1 << 9, dtype=complex)
            t[300] = bad
            dev = torch.from_numpy(t).cuda()
            torch.cuda.synchronize()
            with pytest.raises(qc.QcxError) as e:
                qc.diagonal_gate(1, 9, dev, reg)
            assert e.value.status == BAD_ARGUMENTS
            assert np.array_equal(bits(reg.read()), before)
        # NULL, and a range past the register
        small = torch.ones(4, dtype=torch.complex128).cuda()
        torch.cuda.synchronize()
        assert lib.qcx_diagonal_gate_device(0, 2, None, reg._h) == BAD_ARGUMENTS
        assert lib.qcx_diagonal_gate_device(0, 2, C.c_void_p(small.data_ptr()), None) == BAD_ARGUMENTS
        assert lib.qcx_diagonal_gate_device(13, 2, C.c_void_p(small.data_ptr()), reg._h) == BAD_QUBIT
        assert np.array_equal(bits(reg.read()), before)
        qc.diagonal_gate(5, 2, small, reg)                           # and the register still works
        same(reg.read(), dr.apply(before.view(np.float64), n, 5, 2, np.ones(4, dtype=complex)))


# ---- cross-checks against the existing gates ---------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [12, 14])
def test_equivalences(qc, n):
    rs = np.random.RandomState(30 + n)
    a = adversarial(n, 40 + n, True)
    Z = np.array([[1, 0], [0, -1]], dtype=complex)
    with qc.Register(n, 0) as reg, qc.Register(n, 0) as twin:
        def both(diag_call, gate_call, what):
            reg.write(a); twin.write(a)
            diag_call(reg); gate_call(twin)
            assert np.array_equal(bits(reg.read()), bits(twin.read())), (n, what)
        for q in range(n):
            t = unit_table(rs, 1)
            both(lambda r: qc.diagonal_gate(q, 1, t, r), lambda r: qc.one_qubit_gate(q, np.diag(t), r), ("one_qubit_gate", q))
        for q in list(range(n - 1)):
            theta = float(rs.uniform(-7, 7))
            both(lambda r: qc.diagonal_phase(q, 2, [0.0, 0.0, 0.0, theta], r), lambda r: qc.c_phase_shift_gate(q, q + 1, theta, r),
                 ("c_phase_shift_gate", q))
        ones = np.ones(1 << n, dtype=complex)
        ones[-1] = -1.0
        for q in (0, 5, 9, n - 1):
            cm = ((1 << n) - 1) & ~(1 << q)
            both(lambda r: qc.diagonal_gate(0, n, ones, r), lambda r: qc.mc_one_qubit_gate(cm, q, Z, r), ("Z under n - 1 controls", q))


@pytest.mark.parametrize("n", [12, 14])
def test_z_strings_are_the_pauli_rotation(qc, n):
    rs = np.random.RandomState(50 + n)
    for finite in (True, False):
        a = adversarial(n, 60 + n, finite)
        with qc.Register(n, 0) as reg, qc.Register(n, 0) as twin:
            for z in (0, 1, 0x800, (1 << n) - 1, int(rs.randint(0, 1 << n)), 0xF0 | 1 << (n - 1)):
                theta = float(rs.uniform(-7, 7))
                c, s = qc.polar(theta / 2)
                i = np.arange(1 << n, dtype=np.uint64) & np.uint64(z)
                for sh in (32, 16, 8, 4, 2, 1):
                    i ^= i >> np.uint64(sh)
                t = np.where((i & np.uint64(1)).astype(bool), complex(c, s), complex(c, -s))
                reg.write(a); twin.write(a)
                qc.diagonal_gate(0, n, t, reg)
                qc.pauli_rotation((0, z), theta, twin)
                same(reg.read(), twin.read(), f"n={n} z={z:#x}")


# ---- physics with no reference -----------------------------------------------------------------------------------------------

def test_grover_two_iterations(qc):
    n = 10
    marked = 0x2B5
    oracle = np.ones(1 << n, dtype=complex); oracle[marked] = -1.0
    flip = np.ones(1 << n, dtype=complex); flip[0] = -1.0            # -(2 |0><0| - 1): the diffusion up to a global sign
    with qc.Register(n, 0) as reg:
        reg.write(np.eye(1, 2 << n)[0])
        for q in range(n):
            qc.hadamard_gate(q, reg)
        for _ in range(2):
            qc.diagonal_gate(0, n, oracle, reg)
            for q in range(n):
                qc.hadamard_gate(q, reg)
            qc.diagonal_gate(0, n, flip, reg)
            for q in range(n):
                qc.hadamard_gate(q, reg)
        p = reg.marginal(0, n)
    assert abs(p[marked] - math.sin(5 * math.asin(2.0 ** -5)) ** 2) <= 1e-12


def test_one_qaoa_layer_on_a_ring(qc):
    n = 10
    gamma, beta = 0.37, 0.81
    x = np.arange(1 << n)
    cut = sum(((x >> q) ^ (x >> ((q + 1) % n))) & 1 for q in range(n)).astype(np.float64)      # MaxCut on the 10-ring
    rx = np.array([[math.cos(beta), -1j * math.sin(beta)], [-1j * math.sin(beta), math.cos(beta)]])
    with qc.Register(n, 0) as reg:
        reg.write(np.eye(1, 2 << n)[0])
        for q in range(n):
            qc.hadamard_gate(q, reg)
        qc.diagonal_phase(0, n, -gamma * cut, reg)
        for q in range(n):
            qc.one_qubit_gate(q, rx, reg)
        got = float(np.dot(reg.marginal(0, n), cut))
    psi = np.full(1 << n, 2.0 ** (-n / 2), dtype=complex) * np.exp(-1j * gamma * cut)
    psi = psi.reshape([2] * n)
    for axis in range(n):
        psi = np.moveaxis(np.tensordot(rx, psi, axes=([1], [axis])), 0, axis)
    want = float(np.dot(np.abs(psi.reshape(-1)) ** 2, cut))
    assert abs(got - want) <= 1e-12 and abs(want - n / 2) > 0.1


# ---- lazy forms and modes ---------------------------------------------------------------------------------------------------

SHAPES_14 = [(0, 0), (0, 14), (2, 9), (9, 4), (12, 2)]


def test_pending_basis_state(qc):
    n = 14
    rs = np.random.RandomState(80)
    with qc.Register(n - 4, 4) as reg:
        for k in (1, 0x2A51):
            for first, num in SHAPES_14:
                if k == 1:
                    qc.reset_register(reg)                           # pending basis state |1>
                else:
                    e = np.zeros(2 << n); e[2 * k] = 1.0             # a collapse leaves the pending basis state k
                    reg.write(e)
                    assert qc.measure_state(reg, 0.5) == k
                assert reg.expectation((0, 0)) == 1.0 and reg.expectation_stats() == (2, 0), "the basis state is still pending"
                e = np.zeros(2 << n); e[2 * k] = 1.0
                t = unit_table(rs, num)
                qc.diagonal_gate(first, num, t, reg)
                same(reg.read(), dr.apply(e, n, first, num, t))


def queue_some_gates(qc, ob, reg, want, n):
    for q in (0, 3, n - 1):
        qc.hadamard_gate(q, reg)
        ob.hadamard(want, n, q)
    qc.c_phase_shift_gate(3, n - 1, 0.7, reg)
    ob.cphase(want, n, 3, n - 1, 0.7)


def test_queued_gates_are_flushed_first(qc, ob):
    import torch
    n = 14
    rs = np.random.RandomState(81)
    with qc.Register(n - 4, 4) as reg:
        reg.set_fusion(1)
        reg.fill_random(8)
        want = ob.fill_random(n, 8)
        queue_some_gates(qc, ob, reg, want, n)
        s0 = reg.fusion_stats()
        reg.flush()
        flush_counts = tuple(x - y for x, y in zip(reg.fusion_stats(), s0))
        assert flush_counts != (0, 0)
        for k, (first, num) in enumerate(SHAPES_14):
            t = unit_table(rs, num)
            reg.fill_random(8)
            want = ob.fill_random(n, 8)
            queue_some_gates(qc, ob, reg, want, n)
            before = reg.fusion_stats()
            if k % 2:
                dev = torch.from_numpy(t).cuda()
                torch.cuda.synchronize()
                qc.diagonal_gate(first, num, dev, reg)
            else:
                qc.diagonal_gate(first, num, t, reg)
            assert tuple(x_ - y_ for x_, y_ in zip(reg.fusion_stats(), before)) == flush_counts, "nothing is counted for the diagonal"
            want = dr.apply(want, n, first, num, t)
            qc.hadamard_gate(1, reg); ob.hadamard(want, n, 1)        # queued behind it
            same(reg.read(), want)


def test_mode_2_gives_the_bits_of_mode_0(qc):
    n = 14
    rs = np.random.RandomState(82)
    for first, num in SHAPES_14:
        t = unit_table(rs, num)
        got = []
        for mode in (0, 2):
            with qc.Register(n, 0) as reg:
                reg.set_fusion(mode)
                reg.fill_random(6)
                a = reg.read()
                qc.diagonal_gate(first, num, t, reg)
                got.append(reg.read())
        assert np.array_equal(bits(got[0]), bits(got[1]))
        same(got[0], dr.apply(a, n, first, num, t))


def test_compact_result_is_expanded_first(qc):
    L, M, Cn, a = 15, 5, 21, 2                                      # (the compact chain runs from n = 20 on)
    n = L + M
    rs = np.random.RandomState(83)
    for first, num in ((0, 12), (M, 9), (13, 7)):
        t = unit_table(rs, num)
        with qc.Register(L, M) as flushed:
            qc.reset_register(flushed); qc.quantum_computation(Cn, a, flushed)
            flushed.flush()
            state = flushed.read()
            qc.diagonal_gate(first, num, t, flushed)
            want = flushed.read()
        with qc.Register(L, M) as reg:
            qc.reset_register(reg); qc.quantum_computation(Cn, a, reg)
            qc.diagonal_gate(first, num, t, reg)
            got = reg.read()
        assert np.array_equal(bits(got), bits(want))
        same(got, dr.apply(state, n, first, num, t))
        assert not np.array_equal(bits(got), bits(state))


def test_nonfinite_register_keeps_its_flag(qc, ob):
    n = 13
    rs = np.random.RandomState(84)
    a = ob.random_state(n, 21)
    a[2 * 700] = np.inf
    a[2 * 5] = -0.0
    b = a.copy()
    b[2 * 3000 + 1] = np.nan
    for state in (a, b):
        for first, num in ((0, 0), (0, 13), (3, 6), (9, 3), (12, 1)):
            t = unit_table(rs, num)
            with qc.Register(n, 0) as reg:
                reg.write(state)
                qc.diagonal_gate(first, num, t, reg)
                w = dr.apply(state, n, first, num, t)
                got = reg.read()
                same(got, w)
                bad = ~np.isfinite(got.view(np.complex128).real) | ~np.isfinite(got.view(np.complex128).imag)
                assert set(np.flatnonzero(bad)) <= {700, 3000} and bad[700]
                qc.hadamard_gate(2, reg)                            # the flag is kept: still the strict gate, the oracle's products
                ob.hadamard(w, n, 2)
                same(reg.read(), w)


def test_negative_zeros_do_not_survive(qc, ob):
    n = 13
    rs = np.random.RandomState(12)
    a = ob.random_state(n, 22)
    a[rs.randint(0, a.size, a.size // 2)] = -0.0
    for state in (a, np.full(2 << n, -0.0)):
        for first, num in ((0, 0), (0, 13), (3, 6), (9, 3), (12, 1)):
            t = unit_table(rs, num)
            with qc.Register(n, 0) as reg:
                reg.write(state)
                qc.diagonal_gate(first, num, t, reg)
                got = reg.read()
                assert no_negative_zero(got), (first, num)
                w = dr.apply(state, n, first, num, t)
                same(got, w)
                qc.hadamard_gate(12, reg)                           # nothing is owed to the next gate
                ob.hadamard(w, n, 12)
                same(reg.read(), w)


def test_on_a_callers_stream(qc):
    import torch
    n = 14
    rs = np.random.RandomState(85)
    ctx = {}
    with qc.Register(n, 0) as reg:
        sr.set_stream(reg, 1, ctx)
        reg.fill_random(7)
        want = reg.read()
        for k, (first, num) in enumerate(SHAPES_14 + SHAPES_14):
            t = unit_table(rs, num)
            if k % 2:
                dev = torch.from_numpy(t).cuda()
                torch.cuda.synchronize()
                qc.diagonal_gate(first, num, dev, reg)
                del dev                                              # the register holds the table until it synchronises
            else:
                qc.diagonal_gate(first, num, t, reg)
            want = dr.apply(want, n, first, num, t)
            if k == 4:
                sr.set_stream(reg, 0, ctx)                           # back on its own stream, in mid-sequence
        same(reg.read(), want)


# ---- arguments --------------------------------------------------------------------------------------------------------------

def test_arguments_in_the_documented_order(qc):
    lib = qc.lib()
    ones = np.ones(2 << 21)                                          # (1, 1) in every entry: fits any num up to 21
    p = ones.ctypes.data_as(C.c_void_p)
    with qc.Register(12, 0) as reg:
        reg.fill_random(1)
        before = bits(reg.read())
        assert lib.qcx_diagonal_gate(0, 1, p, None) == BAD_ARGUMENTS
        assert lib.qcx_diagonal_gate(0, 1, None, reg._h) == BAD_ARGUMENTS
        assert lib.qcx_diagonal_gate(13, 0, None, reg._h) == BAD_ARGUMENTS             # NULL before the range
        for first, num in ((0, 13), (12, 1), (13, 0), (5, 8), (0xFFFFFFFF, 1), (1, 0xFFFFFFFF)):
            assert lib.qcx_diagonal_gate(first, num, p, reg._h) == BAD_QUBIT, (first, num)
        for k, v in ((0, 1.0000001), (5, float("nan")), (8191, float("-inf")), (4096, -1.0000001)):
            t = np.ones(2 << 12)
            t[k] = v
            assert lib.qcx_diagonal_gate(0, 12, t.ctypes.data_as(C.c_void_p), reg._h) == BAD_ARGUMENTS
            msg = lib.qcx_last_error().decode()
            assert f"entry {k >> 1}'s {'imaginary' if k & 1 else 'real'} part" in msg, msg
            t[1] = 2.0                                               # the range comes before the entries
            assert lib.qcx_diagonal_gate(1, 12, t.ctypes.data_as(C.c_void_p), reg._h) == BAD_QUBIT
        with pytest.raises(ValueError):
            qc.diagonal_gate(0, 3, np.ones(4), reg)
        with pytest.raises(qc.QcxError):
            qc.diagonal_gate(0, 1, [1.0, 2.0], reg)
        assert np.array_equal(bits(reg.read()), before)
        assert lib.qcx_diagonal_gate(0, 12, p, reg._h) == 0
        assert lib.qcx_shard_diagonal(None, 12, 0, 1, p, None) == BAD_ARGUMENTS
        dev = C.c_void_p(lib.qcx_device_pointer(reg._h))
        assert lib.qcx_shard_diagonal(dev, 12, 12, 1, dev, None) == BAD_QUBIT
    with qc.Register(21, 0) as reg:                                  # wider than the host form takes
        reg.fill_random(2)
        before = bits(reg.read(0, 4096))
        assert lib.qcx_diagonal_gate(0, 21, p, reg._h) == BAD_ARGUMENTS
        assert b"qcx_diagonal_gate_device" in lib.qcx_last_error()
        ones[0] = 2.0                                                # the size limit comes before the entries
        assert lib.qcx_diagonal_gate(0, 21, p, reg._h) == BAD_ARGUMENTS
        assert b"qcx_diagonal_gate_device" in lib.qcx_last_error()
        assert np.array_equal(bits(reg.read(0, 4096)), before)
        ones[0] = 1.0
    with qc.Register(13, 0, shards=4, devices=qc.spread_devices(4)) as sh:             # virtual shards on one GPU
        sh.fill_random(3)
        before = bits(sh.read())
        assert lib.qcx_diagonal_gate(2, 3, p, sh._h) == UNSUPPORTED
        ones[3] = 2.0                                                # the entries come before the kind of register
        assert lib.qcx_diagonal_gate(2, 3, p, sh._h) == BAD_ARGUMENTS
        assert lib.qcx_diagonal_gate(12, 2, p, sh._h) == BAD_QUBIT
        assert np.array_equal(bits(sh.read()), before)


def test_the_shard_form_is_the_launch_alone(qc):
    """qcx_shard_diagonal on the register's own memory with a table the caller placed: the bits of the definition"""
    import torch
    n = 13
    lib = qc.lib()
    t = unit_table(np.random.RandomState(86), 6)
    dev_t = torch.from_numpy(t).cuda()
    torch.cuda.synchronize()
    with qc.Register(n, 0) as reg:
        reg.fill_random(2)
        a = reg.read()
        dev = C.c_void_p(lib.qcx_device_pointer(reg._h))
        reg.synchronize()
        assert lib.qcx_shard_diagonal(dev, n, 9, 4, C.c_void_p(dev_t.data_ptr()), None) == 0      # (the default stream: ordered with the register's)
        same(reg.read(), dr.apply(a, n, 9, 4, t[:16]))


def test_phase_table_is_polar(qc):
    th = np.array([0.0, 0.20966817126512538, -7.5, math.pi, 1e-300])
    t = qc.phase_table(th)
    for k, v in enumerate(th):
        c, s = qc.polar(v)
        assert t[k].real == c and t[k].imag == s
    assert qc.phase_table([]).size == 0
