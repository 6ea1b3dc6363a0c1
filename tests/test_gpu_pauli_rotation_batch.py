"""GPU: a list of Pauli rotations in as few passes as locality allows (qcx_pauli_rotation_batch, K15b).  The state afterwards
must be, bit for bit, what the loop of tests/pauli_rotation_ref.apply over the list leaves (a NaN exactly where the definition
has one) -- in both variants of the kernel, on the partial tile of a small register, on tiles that are not the 12 lowest index
bits, across passes closed by the width, by a fifth hot bit and by a wide term, and behind every lazy form the library keeps a
state in.  The passes a call ran are the plan's every time."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

import pauli_rotation_ref as prr
from bitwise import bits, same_with_nans as same
from pauli_cases import adversarial, g_of, with_every_g
from register_model import RegisterModel

pytestmark = pytest.mark.gpu

THETAS = [0.0, math.pi, -0.7, 7.5, 0.3]                             # 0, pi, a negative value, one above 2 pi


def with_thetas(strings, shift=0):
    return [((x, z), THETAS[(k + shift) % len(THETAS)]) for k, (x, z) in enumerate(strings)]


def ref_loop(a, n, terms):
    for (x, z), theta in terms:
        a = prr.apply(a, n, x, z, theta)
    return a


def run_batch(qc, reg, terms):
    """the call, and its passes against the plan"""
    qc.pauli_rotation_batch(terms, reg)
    _, passes = qc.pauli_rotation_batch_plan(terms, reg.num_qubits)
    assert reg.rotation_batch_stats() == (len(passes), sum(kind for kind, _ in passes))
    return passes


def check_lists(qc, n, a, lists, chained=True):
    """every list on ONE register that starts as `a`, a read-back after every call, each compared with the loop of the definition
    on what the register held before it; chained=False: the start state is written again before every list"""
    kinds = []
    with qc.Register(n, 0) as reg:
        reg.write(a)
        have = a
        for k, terms in enumerate(lists):
            if k and not chained:
                reg.write(a)
                have = a
            kinds += run_batch(qc, reg, terms)
            want = ref_loop(have, n, terms)
            have = reg.read()
            same(have, want, f"n = {n}, list {k}")
            assert not np.any((have == 0) & np.signbit(have)), (n, k)
    return kinds


def hot_of(qubits):
    return sum(1 << q for q in qubits)


def strings_in_tile(rs, n, hot, count, diagonal=False):
    """(x, z) with x inside the tile of bits 0-7 and `hot`, z anywhere"""
    out = []
    for _ in range(count):
        x = 0 if diagonal else int(rs.randint(0, 1 << n)) & (0xFF | hot)
        out.append((x, int(rs.randint(0, 1 << n))))
    return out


# ---- small registers: one partial tile ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("finite", [True, False], ids=["finite", "inf-nan"])
def test_small_registers_every_string_in_lists_of_3(qc, finite):
    for n in range(1, 6):
        strings = list(itertools.product(range(1 << n), repeat=2))
        strings += strings[:(-len(strings)) % 3]
        lists = [with_thetas(strings[k:k + 3], k) for k in range(0, len(strings), 3)]
        check_lists(qc, n, adversarial(n, 31 * n, finite), lists, chained=finite)


@pytest.mark.parametrize("finite", [True, False], ids=["finite", "inf-nan"])
def test_partial_tile_random_lists_of_40(qc, finite):
    for n in range(6, 12):
        rs = np.random.RandomState(2000 + n)
        lists = [with_thetas([(int(rs.randint(0, 1 << n)), int(rs.randint(0, 1 << n))) for _ in range(40)], k) for k in range(2)]
        lists.append(with_thetas([(0, int(rs.randint(0, 1 << n))) for _ in range(40)]))           # the variant without LDS
        kinds = check_lists(qc, n, adversarial(n, 37 * n, finite), lists, chained=False)
        assert kinds == [(0, hot_of(range(8, n)))] * (3 * -(-40 // qc.pauli_rotation_batch_width()))      # only the width splits a list


# ---- one tile, and tiles that are not the low 12 bits ----------------------------------------------------------------------

def test_one_full_tile(qc):
    n = 12
    W = qc.pauli_rotation_batch_width()
    rs = np.random.RandomState(12)
    high = with_every_g([0xF00, 0x100, 0x800, 0xA00, 0xF53, 0xFFF], n, 1)                         # x on bits 8 .. 11
    diag = strings_in_tile(rs, n, 0xF00, W + 5, diagonal=True)
    exch = [(x or 0x801, z) for x, z in strings_in_tile(rs, n, 0xF00, W + 3)]
    a = adversarial(n, 5, True)
    assert check_lists(qc, n, a, [with_thetas(high)], chained=False) == [(0, 0xF00)] * -(-len(high) // W)
    assert check_lists(qc, n, a, [with_thetas(diag), with_thetas(exch, 2)]) == [(0, 0xF00)] * 4  # W splits both lists
    check_lists(qc, n, adversarial(n, 6), [with_thetas(high[:6]), with_thetas(diag[:5]), with_thetas(exch[:5])], chained=False)


@pytest.mark.parametrize("hot", [(9, 10, 11, 12), (8, 10, 11, 12)], ids=["9-12", "8,10-12"])
def test_two_tiles_one_bit_outside(qc, hot):
    n = 13
    H = hot_of(hot)
    outside = 0x1F00 & ~H
    rs = np.random.RandomState(H)
    xs = [H, 1 << hot[0], 1 << hot[3], H | 0xFF, (1 << hot[1]) | 0x5, 0x80, (1 << hot[2]) | (1 << hot[3]) | 0x13]
    strings = [(x, z | outside) for x, z in with_every_g(xs, n, 3)] + strings_in_tile(rs, n, H, 6) + [(0, outside), (0, 0x1FFF)]
    assert {g_of(x, z) for x, z in strings} == {0, 1, 2, 3}
    for a in (adversarial(n, 7, True), adversarial(n, 8)):
        assert check_lists(qc, n, a, [with_thetas(strings)], chained=False) == [(0, H)] * -(-len(strings) // qc.pauli_rotation_batch_width())
    diag = [(0, z) for _, z in strings[:9]]
    assert check_lists(qc, n, adversarial(n, 9, True), [with_thetas(diag)]) == [(0, 0xF00)]      # (no x bit: the padded set)


def test_scattered_hot_set_and_every_way_a_pass_closes(qc):
    n = 16
    H = hot_of((8, 11, 13, 15))
    outside = 0xFF00 & ~H                                           # qubits 9, 10, 12, 14
    rs = np.random.RandomState(16)
    a = adversarial(n, 11, True)
    # z bits on every outside qubit, all four g
    xs = [H, 0x8000, 0x0100 | 0x2000, H | 0xFF, 0x0800 | 0x41, 0x3]
    run1 = [(x, z | outside) for x, z in with_every_g(xs, n, 5)]
    assert {g_of(x, z) for x, z in run1} == {0, 1, 2, 3} and len(run1) <= qc.pauli_rotation_batch_width()
    assert check_lists(qc, n, a, [with_thetas(run1)], chained=False) == [(0, H)]
    # a fifth hot bit arrives mid-list
    run2 = strings_in_tile(rs, n, H, 5) + [(H, 0x1234), (0x0200 | 0x7, 0xFFFF), (0x1200 | 0x40, 0x00FF)] + strings_in_tile(rs, n, 0x1200, 4)
    kinds = check_lists(qc, n, a, [with_thetas(run2, 1)], chained=False)
    assert kinds[0] == (0, H) and len(kinds) == 2 and kinds[1][1] & 0x1200 == 0x1200
    # one wide term between two runs
    wide = (0xF900 | 0x21, 0x8421)
    run3 = strings_in_tile(rs, n, H, 4) + [wide] + strings_in_tile(rs, n, hot_of((9, 10, 12, 14)), 4, diagonal=False)
    run3[0] = (H, run3[0][1])
    run3[-1] = (hot_of((9, 10, 12, 14)) | 0x80, run3[-1][1])
    for state in (a, adversarial(n, 12)):
        assert check_lists(qc, n, state, [with_thetas(run3, 3)], chained=False) == [(0, H), (1, 0), (0, hot_of((9, 10, 12, 14)))]
    # a sweep: every g on strings over the whole register, whatever passes that takes
    sweep = with_every_g([0xFFFF, 0xA900, 0x00FF, 0x5400 | 0x1, 0x8001, 0x0180, 0x1E00, 0x3F00], n, 7)
    kinds = check_lists(qc, n, a, [with_thetas(sweep)], chained=False)
    assert sum(kind for kind, _ in kinds) >= 3 and len(kinds) >= 5


# ---- more units than workgroups -----------------------------------------------------------------------------------------------
# The grid is capped at 2048 workgroups (K15's prot_grid_cap): n = 25 has 2^13 tiles, so a workgroup walks four units.  One list
# per variant, against the same list issued term by term through qc.pauli_rotation on a second register.
N_BIG = 25
BIG_LISTS = {
    "all-Z": [(0, 0x1AAAAAA), (0, 0x3), (0, 0x180), (0, 0x1800), (0, 0x1000008), (0, 0x1FFFFFF), (0, 1 << 24), (0, 0), (0, 0x300000)],
    "bonds": [s for q in (20, 21, 22) for s in ((3 << q, 0), (3 << q, 3 << q), (0, 3 << q))],         # XX, YY, ZZ per bond
}


@pytest.mark.parametrize("which", sorted(BIG_LISTS))
def test_more_than_one_unit_per_workgroup(qc, which):
    terms = with_thetas(BIG_LISTS[which], 2)
    with qc.Register(N_BIG, 0) as reg, qc.Register(N_BIG, 0) as twin:
        reg.fill_random(5); twin.fill_random(5)
        passes = run_batch(qc, reg, terms)
        assert passes == [(0, 0xF00 if which == "all-Z" else 0xF00000)] and (1 << (N_BIG - 12)) > 2048
        for pauli, theta in terms:
            qc.pauli_rotation(pauli, theta, twin)
        got, want = bits(reg.read()), bits(twin.read())
    assert np.array_equal(got, want)


def test_grid_caps_that_do_not_divide_the_units(qc):
    """prot_grid_cap = 1 and 3 at n = 14: one workgroup walks all four units, and three share them unevenly"""
    n = 14
    a = adversarial(n, 19, True)
    rs = np.random.RandomState(14)
    lists = [with_thetas(strings_in_tile(rs, n, 0x2900 | 0x400, 7)), with_thetas(strings_in_tile(rs, n, 0, 7, diagonal=True), 1)]
    try:
        for cap in (1, 3):
            qc.tune(prot_grid_cap=cap)
            check_lists(qc, n, a, lists, chained=False)
    finally:
        qc.tune(prot_grid_cap=2048)


# ---- lazy forms and modes, against the model driven term by term ------------------------------------------------------------------

LIST_14 = with_thetas([(0, 0x2A51), (0x1003, 0x3001), (0x1, 0x1), (0x2A51, 0x0F0F), (0x3F00, 0x0001), (0, 0), (0x2000, 0x2000), (0x00FF, 0x3FFF)])


def model_apply(m, terms):
    for (x, z), theta in terms:
        m.pauli_rotation(x, z, theta)


def test_pending_basis_state(qc, ob):
    L, M = 10, 4
    n = L + M
    with qc.Register(L, M) as reg:
        for k in (1, 0x2A51):
            m = RegisterModel(ob, L, M)
            if k == 1:
                qc.reset_register(reg); m.reset_register()           # pending basis state |1>
            else:
                e = np.zeros(2 << n); e[2 * k] = 1.0                 # a collapse leaves the pending basis state k
                reg.write(e); m.write(e)
                assert qc.measure_state(reg, 0.5) == k == m.measure_state(0.5)
            assert reg.expectation((0, 0)) == 1.0 and reg.expectation_stats() == (2, 0), "the basis state is still pending"
            run_batch(qc, reg, LIST_14)
            model_apply(m, LIST_14)
            same(reg.read(), m.a)


def test_compact_result_is_expanded_first(qc, ob):
    L, M, Cn, a = 15, 5, 21, 2                                      # (the compact chain runs from n = 20 on)
    terms = with_thetas([(0, 0x81234), (0x3 << M, 0x1F), (0x81234, 0x80F31), (0xF0000, 0xFFFFF), (0x700, 0)])
    m = RegisterModel(ob, L, M)
    m.reset_register(); m.quantum_computation(Cn, a)
    before = m.a.copy()
    with qc.Register(L, M) as reg:
        qc.reset_register(reg); qc.quantum_computation(Cn, a, reg)
        run_batch(qc, reg, terms)
        got = reg.read()
    model_apply(m, terms)
    same(got, m.a)
    assert not np.array_equal(bits(got), bits(before))


@pytest.mark.parametrize("mode", [1, 2])
def test_queued_gates_are_flushed_first(qc, ob, mode):
    L, M = 10, 4
    n = L + M
    m = RegisterModel(ob, L, M)
    with qc.Register(L, M) as reg:
        reg.set_fusion(mode)
        reg.fill_random(8); m.fill_random(8)

        def queue():
            for q in (0, 3, n - 1):
                qc.hadamard_gate(q, reg); m.hadamard_gate(q)
            if mode == 1:                                           # (mode 2 merges phases and is then not the oracle's bits)
                qc.c_phase_shift_gate(3, n - 1, 0.7, reg); m.c_phase_shift_gate(3, n - 1, 0.7)

        queue()
        s0 = reg.fusion_stats()
        reg.flush()
        flush_counts = tuple(x - y for x, y in zip(reg.fusion_stats(), s0))
        assert flush_counts != (0, 0)
        queue()
        before = reg.fusion_stats()
        run_batch(qc, reg, LIST_14)
        assert tuple(x - y for x, y in zip(reg.fusion_stats(), before)) == flush_counts, "nothing is counted for the rotations"
        model_apply(m, LIST_14)
        qc.hadamard_gate(1, reg); m.hadamard_gate(1)                # queued behind it
        same(reg.read(), m.a)


def test_after_device_pointer(qc, ob):
    L, M = 10, 4
    m = RegisterModel(ob, L, M)
    with qc.Register(L, M) as reg:
        reg.set_fusion(1)
        reg.fill_random(3); m.fill_random(3)
        qc.hadamard_gate(13, reg); m.hadamard_gate(13)
        assert reg.device_pointer() != 0
        run_batch(qc, reg, LIST_14)
        model_apply(m, LIST_14)
        same(reg.read(), m.a)
        assert reg.device_pointer() != 0
        run_batch(qc, reg, LIST_14[:3])
        model_apply(m, LIST_14[:3])
        same(reg.read(), m.a)


def test_nonfinite_register(qc, ob):
    n = 13
    a = ob.random_state(n, 21)
    a[2 * 700] = np.inf
    a[2 * 5] = -0.0
    b = a.copy()
    b[2 * 3000 + 1] = np.nan
    terms = with_thetas([(0, 0x1FFF), (0x1000, 0), (0x4, 0x4), (0x1234, 0x0F0F), (0, 0)], 1)
    for state in (a, b):
        m = RegisterModel(ob, n, 0)
        with qc.Register(n, 0) as reg:
            reg.write(state); m.write(state)
            run_batch(qc, reg, terms)
            model_apply(m, terms)
            same(reg.read(), m.a)
            assert m.holds_nonfinite()
            qc.hadamard_gate(2, reg); m.hadamard_gate(2)            # the flag is kept: still the strict gate, the oracle's products
            same(reg.read(), m.a)


# ---- arguments --------------------------------------------------------------------------------------------------------------

def arrays(terms):
    xs = (C.c_uint64 * len(terms))(*[x for (x, _), _ in terms])
    zs = (C.c_uint64 * len(terms))(*[z for (_, z), _ in terms])
    th = (C.c_double * len(terms))(*[t for _, t in terms])
    return xs, zs, th


def test_refusals_touch_nothing(qc):
    lib = qc.lib()
    batch = lib.qcx_pauli_rotation_batch
    good = with_thetas([(1, 0), (0x800, 0x3), (0, 0x7), (0x30, 0x30), (0x3, 0)], 1)
    with qc.Register(12, 0) as reg:
        reg.fill_random(1)
        before = bits(reg.read())
        run_batch(qc, reg, good[:2])
        after = bits(reg.read())
        stats = reg.rotation_batch_stats()
        assert not np.array_equal(after, before) and stats == (1, 0)
        xs, zs, th = arrays(good)
        assert batch(None, 5, xs, zs, th) == 2                      # QCX_BAD_ARGUMENTS
        assert batch(reg._h, 5, None, zs, th) == 2
        assert batch(reg._h, 5, xs, None, th) == 2
        assert batch(reg._h, 5, xs, zs, None) == 2
        for bad in (float("nan"), float("inf"), float("-inf")):
            th[3] = bad
            assert batch(reg._h, 5, xs, zs, th) == 2
            assert "term 3" in lib.qcx_last_error().decode()
        th[3] = 0.5
        xs[4] = 1 << 12
        assert batch(reg._h, 5, xs, zs, th) == 6                    # QCX_BAD_QUBIT
        xs[4], zs[2] = 3, 1 << 63
        assert batch(reg._h, 5, xs, zs, th) == 6
        assert np.array_equal(bits(reg.read()), after) and reg.rotation_batch_stats() == stats
        with pytest.raises(ValueError):
            qc.pauli_rotation_batch([("X" * 13, 0.5)], reg)
        assert np.array_equal(bits(reg.read()), after)
        # the launch alone: a hot mask that is not the plan's, or does not hold a term's partner, is refused
        dev = C.c_void_p(lib.qcx_device_pointer(reg._h))
        reg.synchronize()
        one = (C.c_double * 1)(1.0)
        x1, z1 = (C.c_uint64 * 1)(0x100), (C.c_uint64 * 1)(0)
        run = lib.qcx_shard_pauli_rotation_run
        assert run(None, 12, 0xF00, 1, x1, z1, one, one, None) == 2
        assert run(dev, 12, 0x700, 1, x1, z1, one, one, None) == 2
        assert run(dev, 12, 0xF01, 1, x1, z1, one, one, None) == 2
        assert run(dev, 12, 0xF00, 0, x1, z1, one, one, None) == 2
        assert run(dev, 12, 0xF00, qc.pauli_rotation_batch_width() + 1, x1, z1, one, one, None) == 2
        assert run(dev, 13, 0x1E00, 1, x1, z1, one, one, None) == 2      # bit 8 is outside that tile
        x1[0] = 1 << 12
        assert run(dev, 12, 0xF00, 1, x1, z1, one, one, None) == 6
        assert np.array_equal(bits(reg.read()), after)
    with qc.Register(13, 0, shards=4, devices=qc.spread_devices(4)) as sh:             # virtual shards on one GPU
        sh.fill_random(3)
        before = bits(sh.read())
        xs, zs, th = arrays(good)
        assert batch(sh._h, 5, xs, zs, th) == 7                                        # QCX_UNSUPPORTED
        assert np.array_equal(bits(sh.read()), before)


def test_no_terms(qc, ob):
    n = 14
    m = RegisterModel(ob, n, 0)
    with qc.Register(n, 0) as reg:
        reg.set_fusion(1)
        reg.fill_random(2); m.fill_random(2)
        run_batch(qc, reg, LIST_14[:1])
        model_apply(m, LIST_14[:1])
        qc.hadamard_gate(4, reg); m.hadamard_gate(4)
        before = reg.fusion_stats()
        assert qc.lib().qcx_pauli_rotation_batch(reg._h, 0, None, None, None) == 0
        qc.pauli_rotation_batch([], reg)
        assert reg.fusion_stats() == before, "queued gates stay queued"
        assert reg.rotation_batch_stats() == (0, 0)
        same(reg.read(), m.a)


def test_the_shard_form_is_the_launch_alone(qc):
    """qcx_shard_pauli_rotation_run on the register's own memory, c and s given per term: the definition with those c and s"""
    n = 13
    lib = qc.lib()
    strings = [(0x1041, 0x0043), (0, 0x1FFF), (0x0A00, 0x0B00)]
    cs = [qc.polar(t) for t in (0.45, -1.1, 2.0)]
    with qc.Register(n, 0) as reg:
        reg.fill_random(2)
        a = reg.read()
        dev = C.c_void_p(lib.qcx_device_pointer(reg._h))
        reg.synchronize()
        xs, zs = (C.c_uint64 * 3)(*[x for x, _ in strings]), (C.c_uint64 * 3)(*[z for _, z in strings])
        c, s = (C.c_double * 3)(*[v[0] for v in cs]), (C.c_double * 3)(*[v[1] for v in cs])
        assert lib.qcx_shard_pauli_rotation_run(dev, n, 0x1A00 | 0x100, 3, xs, zs, c, s, None) == 0      # (the default stream: ordered with the register's)
        for (x, z), (ck, sk) in zip(strings, cs):
            a = prr.apply_cs(a, n, x, z, ck, sk)
        same(reg.read(), a)


# ---- with no reference ------------------------------------------------------------------------------------------------------

def heisenberg_step(n, theta):
    out = []
    for q in range(n - 1):
        both = 3 << q
        out += [((both, 0), theta), ((both, both), theta), ((0, both), theta)]
    return out


def test_norm_is_kept_and_the_inverse_list_gives_the_state_back(qc):
    n = 16
    terms = heisenberg_step(n, 0.37) + [((0xFFFF, 0x5A5A), 1.1)] + [((1 << q, 0), -0.9) for q in range(n)]
    with qc.Register(n, 0) as reg:
        reg.fill_random(9)
        a = reg.read()
        norm = reg.norm2()
        run_batch(qc, reg, terms)
        assert abs(reg.norm2() - norm) <= 1e-12
        assert np.max(np.abs(reg.read() - a)) > 1e-4
        for pauli, theta in [((0x00FF, 0x0F0F), 0.8), ((0xA900, 0xFFFF), -2.2), ((0, 0x8001), 0.3), ((0xFFFF, 0), 7.5)]:
            reg.write(a)
            run_batch(qc, reg, [(pauli, theta), (pauli, -theta)])
            assert np.max(np.abs(reg.read() - a)) <= 1e-14, pauli


def dense(n, x, z, theta):
    """cos(theta/2) I - i sin(theta/2) P, P = the kron of the letters (qubit 0 is the lowest index bit)"""
    P = np.eye(1, dtype=complex)
    for q in range(n):
        letter = "IXZY"[(x >> q & 1) + 2 * (z >> q & 1)]
        P = np.kron(prr.PAULI[letter], P)
    return math.cos(theta / 2) * np.eye(1 << n) - 1j * math.sin(theta / 2) * P


def test_six_qubits_against_dense_matrices(qc):
    n = 6
    rs = np.random.RandomState(6)
    v = rs.standard_normal(1 << n) + 1j * rs.standard_normal(1 << n)
    v /= np.linalg.norm(v)
    terms = [((int(rs.randint(0, 1 << n)), int(rs.randint(0, 1 << n))), float(rs.uniform(-7, 7))) for _ in range(40)]
    with qc.Register(n, 0) as reg:
        reg.write(np.ascontiguousarray(v).view(np.float64))
        run_batch(qc, reg, terms)
        got = reg.read().view(np.complex128)
    for (x, z), theta in terms:
        v = dense(n, x, z, theta) @ v
    assert np.max(np.abs(got - v)) <= 1e-13
