"""GPU: the general gates and the observers on a register of 2^33 amplitudes (128 GiB; QCX_TEST_NWIDE, default 33) -- the smallest
register with an amplitude index >= 2^32, a pair count of 2^32 (0 as a uint32), indices with bit 31 set (where an int turns
negative), a qubit 32 and a mask bit 32.  A `1u << q`, an unsigned count, an (unsigned) cast of a mask, an int lane offset or a grid
computed in 32 bits passes every test on registers of up to 30 qubits and corrupts a state of this size.

Nothing of this size visits the host.  tests/wide_windows.py turns the register into SUB-CUBES of 8 to 16 qubits that numpy holds
(qubits 0-7 plus whatever a call names, a fixed pattern `cold` on the others), and the numpy definitions of tests/*_ref.py,
unchanged, say what each sub-cube must hold; tests/test_wide_windows.py pins on the CPU why that is valid.  Every comparison is on
uint64 views: the module has no tolerance.

  a. gates on the dense fill_random state: four sub-cubes each -- cold with bit N-1 set and N-2 clear, the reverse, all zeros and
     all ones; the last two begin and end with the plain 256-amplitude windows at the two ends of the register;
  b. observers on a state that is zero outside one 12-qubit sub-cube (the arithmetic and the high index bits);
  c. observers on the uniform superposition, where a pairwise tree over identical leaves is exact power-of-two scaling (every tile
     is visited exactly once);
  d. refusals at this width.

One module-wide register, never a twin.  With TOP = N - 1 and SUB = N - 2 the cases read as the 32 and 31 of the default size."""
import ctypes as C
import os

import numpy as np
import pytest

import collapse_ref
import one_qubit_ref
import pauli_ref
import two_qubit_ref
import wide_windows as ww
from marginal_ref import marginal_ref
from rdm_ref import rdm_ref

pytestmark = pytest.mark.gpu

N = int(os.environ.get("QCX_TEST_NWIDE", "33"))
TOP, SUB = N - 1, N - 2
FULL = (1 << N) - 1
BAD_QUBIT, UNSUPPORTED = 6, 7
LOW8 = list(range(8))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


class Wide:
    """the module's register and what it holds at the moment (so that the observer tests prepare a state once)"""

    def __init__(self, reg):
        self.reg, self.holds = reg, None


@pytest.fixture(scope="module")
def wide(qc):
    import torch
    free, total = torch.cuda.mem_get_info()
    need = (16 << N) + (8 << 30)
    print(f"\nwide register: n = {N}, {free} bytes of device memory free, {need} needed")
    if free < need:
        pytest.skip(f"a register of {N} qubits needs {need} bytes of free device memory, {free} are free")
    reg = qc.Register(N, 0)
    yield Wide(reg)
    reg.close()


def cube(*named):
    return sorted(set(LOW8) | {int(q) for q in named})


def colds(S):
    """bit TOP set and SUB clear; the reverse; all zeros; all ones (each without the qubits of S)"""
    free = FULL & ~ww.hot_mask(S)
    a = (0x0A5A5C3C96 | 1 << TOP) & ~(1 << SUB)
    b = (0x15A3C5A369 | 1 << SUB) & ~(1 << TOP)
    return [a & free, b & free, 0, free]


def matrix(seed, d):
    """neither symmetric nor unitary: a swapped row or column shows"""
    rs = np.random.RandomState(seed)
    return rs.uniform(-1, 1, (d, d)) + 1j * rs.uniform(-1, 1, (d, d))


def check_gate(wide, ob, seed, S, run, ref):
    """fill_random(seed), run() on the register, then every sub-cube against ref(mini state, cold)"""
    reg = wide.reg
    wide.holds = None
    assert len(S) <= 16 and S[:8] == LOW8
    reg.fill_random(seed)
    run()
    for cold in colds(S):
        mini = ww.gather_dense(N, seed, S, cold, ob)
        want = ref(mini, cold)
        got = ww.read_subcube(reg, S, cold)
        bad = np.nonzero(bits(got).reshape(-1, 2) != bits(want).reshape(-1, 2))[0]
        assert bad.size == 0, (f"sub-cube S = {S}, cold = {cold:#x}: {bad.size} of {1 << len(S)} amplitudes differ, the first at "
                               f"index {int(ww.embed_indices(S, cold)[bad[0]]):#x}")
    # (the last two sub-cubes start with the register's first 256 amplitudes and end with its last 256)
    assert ww.run_starts(S, 0)[0][0] == 0 and ww.run_starts(S, FULL & ~ww.hot_mask(S))[-1][0] == (1 << N) - 256


# ---- a. gates on the dense state ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("q", [0, 2, 5, 7, 12, SUB, TOP])
def test_one_qubit_gate(qc, ob, wide, q):
    U, S = matrix(100 + q, 2), cube(q)
    check_gate(wide, ob, 4100 + q, S, lambda: qc.one_qubit_gate(q, U, wide.reg),
               lambda mini, cold: one_qubit_ref.apply(mini, len(S), ww.down_qubit(q, S), U))


@pytest.mark.parametrize("c,q", [(TOP, 0), (1, TOP), (TOP, SUB), (SUB, TOP), (2, 1), (12, TOP)])
def test_c_one_qubit_gate(qc, ob, wide, c, q):
    U, S = matrix(200 + 40 * c + q, 2), cube(c, q)
    check_gate(wide, ob, 4200 + 40 * c + q, S, lambda: qc.c_one_qubit_gate(c, q, U, wide.reg),
               lambda mini, cold: one_qubit_ref.apply(mini, len(S), ww.down_qubit(q, S), U, control=ww.down_qubit(c, S)))


@pytest.mark.parametrize("q0,q1", [(0, TOP), (TOP, 0), (SUB, TOP), (2, TOP), (7, SUB), (12, 20)])
def test_two_qubit_gate(qc, ob, wide, q0, q1):
    U, S = matrix(300 + 40 * q0 + q1, 4), cube(q0, q1)
    check_gate(wide, ob, 4300 + 40 * q0 + q1, S, lambda: qc.two_qubit_gate(q0, q1, U, wide.reg),
               lambda mini, cold: two_qubit_ref.apply(mini, len(S), ww.down_qubit(q0, S), ww.down_qubit(q1, S), U))


@pytest.mark.parametrize("c,q0,q1", [(TOP, 0, 1), (TOP, 4, SUB), (TOP, 12, 13), (1, SUB, TOP), (4, SUB, TOP)])
def test_c_two_qubit_gate(qc, ob, wide, c, q0, q1):
    U, S = matrix(400 + 40 * q0 + q1 + c, 4), cube(c, q0, q1)
    check_gate(wide, ob, 4400 + 40 * q0 + q1 + c, S, lambda: qc.c_two_qubit_gate(c, q0, q1, U, wide.reg),
               lambda mini, cold: two_qubit_ref.apply(mini, len(S), ww.down_qubit(q0, S), ww.down_qubit(q1, S), U,
                                                      control=ww.down_qubit(c, S)))


ROTATIONS = {
    # no X or Y: Z on every qubit of the register -- the letters on the cold qubits enter by the sign rule
    "z-on-every-qubit": ({q: "Z" for q in range(N)}, []),
    # the partner inside the tile of the 12 lowest bits, Z on the two highest qubits (SUB in the sub-cube, TOP and 20 cold)
    "partner-in-tile-z-on-top": ({3: "X", 9: "Y", 11: "X", 20: "Z", SUB: "Z", TOP: "Z"}, [9, 11, SUB]),
    # the partner 2^TOP + 2^SUB + 2^5 amplitudes away
    "partner-across-top": ({5: "X", SUB: "Y", TOP: "X"}, [SUB, TOP]),
}


@pytest.mark.parametrize("name", sorted(ROTATIONS))
def test_pauli_rotation(qc, ob, wide, name):
    pauli, extra = ROTATIONS[name]
    x, z = qc.pauli_masks(pauli, N)
    S = cube(*extra)
    assert x & ~ww.hot_mask(S) == 0
    theta = 0.7 + 0.1 * len(name)
    check_gate(wide, ob, 4500 + len(name), S, lambda: qc.pauli_rotation((x, z), theta, wide.reg),
               lambda mini, cold: ww.rotation_on_subcube(mini, S, cold, x, z, theta))


def test_pauli_rotation_batch(qc, ob, wide):
    """one list, three passes: a run whose hot bits include SUB and TOP, a wide term (five x bits above 7) on its own, a run of
    diagonal terms"""
    terms = [({2: "X", SUB: "X", TOP: "Y"}, 0.31), ({TOP: "X", 5: "Z", 20: "Z"}, -0.83), ({0: "Y", SUB: "Y", 9: "Z"}, 1.9),
             ({9: "X", 13: "X", 20: "Y", SUB: "X", TOP: "X", 1: "X", 25: "Z"}, 0.57),
             ({q: "Z" for q in range(N)}, -1.1), ({TOP: "Z", 3: "Z"}, 0.45), ({SUB: "Z", 17: "Z"}, 2.2)]
    masks = [qc.pauli_masks(p, N) for p, _ in terms]
    pass_of, passes = qc.pauli_rotation_batch_plan(terms, N)
    assert pass_of == [0, 0, 0, 1, 2, 2, 2]
    assert passes == [(0, 1 << 8 | 1 << 9 | 1 << SUB | 1 << TOP), (1, 0), (0, 0xF00)]
    S = cube(9, 13, 20, SUB, TOP)
    assert all(x & ~ww.hot_mask(S) == 0 for x, _ in masks)

    def ref(mini, cold):
        for (x, z), (_, theta) in zip(masks, terms):
            mini = ww.rotation_on_subcube(mini, S, cold, x, z, theta)
        return mini

    check_gate(wide, ob, 4600, S, lambda: qc.pauli_rotation_batch(terms, wide.reg), ref)
    assert wide.reg.rotation_batch_stats() == (3, 1)


# ---- b. observers on a state that is zero outside one sub-cube -----------------------------------------------------------------

SB = [0, 1, 2, 3, 4, 5, 12, 13, 14, N - 3, SUB, TOP]            # contiguous ranges at the bottom, across tile bit 12, at the top
KB = len(SB)
COLD_B = (1 << 6 | 1 << 9 | 1 << 17 | 1 << 20 | 1 << 25 | 1 << (N - 5) | 1 << (N - 4))
RANGES = [(0, 3), (12, 3), (N - 3, 3), (TOP, 1)]


def sparse_mini():
    """a random state of KB qubits whose running sum ends at or above 1.0 (so that the draw r = 1.0 is met inside the sub-cube)"""
    rs = np.random.RandomState(33)
    a = rs.uniform(-0.5, 0.5, 2 << KB)
    a[2 * 7], a[2 * 7 + 1] = 0.0, 0.0                            # a zero inside the sub-cube: a tie of the running sum
    a /= np.sqrt(np.sum(a * a))
    if ww.sequential_total(a) < 1.0:
        a *= 1.0 + 2.0 ** -30
    assert ww.sequential_total(a) >= 1.0
    a.setflags(write=False)
    return a


MINI = sparse_mini()


def hold_sparse(qc, wide):
    """reset_register (it leaves the basis state |1>: the M register holds 1), that amplitude cleared, MINI written"""
    if wide.holds != "sparse":
        wide.holds = None
        qc.reset_register(wide.reg)
        wide.reg.write(np.array([0.0, 0.0]), first=1)
        ww.write_subcube(wide.reg, SB, COLD_B, MINI)
        wide.holds = "sparse"
    return wide.reg


def zero_outside(reg):
    """the two ends of the register (neither lies in the sub-cube) hold (+0, +0)"""
    return not bits(reg.read(0, 256)).any() and not bits(reg.read((1 << N) - 256, 256)).any()


def test_sparse_state_is_what_was_written(qc, wide):
    reg = hold_sparse(qc, wide)
    assert np.array_equal(bits(ww.read_subcube(reg, SB, COLD_B)), bits(MINI))
    assert zero_outside(reg)
    for cold in (0, COLD_B ^ 1 << 6, COLD_B | 1 << 7):            # neighbouring sub-cubes
        assert not bits(ww.read_subcube(reg, SB, cold)).any()


# one string per shape of the tiles (mini masks: mini qubits 0-5 are real 0-5, 6-8 real 12-14, 9-11 real N-3, SUB, TOP)
STRINGS = {
    "no-x": (0, 1 << 1 | 1 << 7 | 1 << 11),
    "partner-in-tile": (1 << 0 | 1 << 3 | 1 << 5, 1 << 3 | 1 << 8 | 1 << 10),
    "partner-across-12-and-top-y-on-top": (1 << 2 | 1 << 6 | 1 << 11, 1 << 11 | 1 << 4),
    "partner-across-top-only": (1 << 11, 0),
    "x-on-sub-and-top-z-below": (1 << 10 | 1 << 11, 1 << 9),
    "y-on-sub-and-top": (1 << 10 | 1 << 11 | 1 << 1, 1 << 10 | 1 << 11),
}


@pytest.mark.parametrize("name", sorted(STRINGS))
def test_expectation_sparse(qc, wide, name):
    reg = hold_sparse(qc, wide)
    x, z = STRINGS[name]
    got = reg.expectation((ww.up(x, SB), ww.up(z, SB)))
    want = pauli_ref.pauli_ref(MINI, KB, x, z)
    assert bits(got) == bits(want), (got, want)
    assert reg.expectation_stats()[0] == 0                          # (read from the register itself)


@pytest.mark.parametrize("call", ["expectation_sum", "expectation_batch"])
def test_expectation_terms_sparse(qc, wide, call):
    reg = hold_sparse(qc, wide)
    names = sorted(STRINGS)
    # (terms that share an x_mask share a read in expectation_batch: every string again with other Z letters)
    mini_terms = [(0.5 - 0.37 * k, STRINGS[nm][0], STRINGS[nm][1]) for k, nm in enumerate(names)]
    mini_terms += [(1.25 + k, STRINGS[nm][0], STRINGS[nm][1] ^ (1 << 9 | 1 << 2)) for k, nm in enumerate(names)]
    total, values = getattr(reg, call)([(c, (ww.up(x, SB), ww.up(z, SB))) for c, x, z in mini_terms])
    want_total, want_values = pauli_ref.pauli_sum_ref(MINI, KB, mini_terms)
    assert np.array_equal(bits(values), bits(np.array(want_values))), (values, want_values)
    assert bits(total) == bits(want_total)


@pytest.mark.parametrize("first,num", RANGES)
def test_marginal_sparse(qc, wide, first, num):
    reg = hold_sparse(qc, wide)
    got = reg.marginal(first, num)
    want = marginal_ref(MINI, KB, ww.down_qubit(first, SB), num)
    assert np.array_equal(bits(got), bits(want)), (got, want)
    assert reg.marginal_stats()[0] == 0


@pytest.mark.parametrize("first,num", RANGES)
def test_reduced_density_matrix_sparse(qc, wide, first, num):
    reg = hold_sparse(qc, wide)
    got = reg.reduced_density_matrix(first, num)
    want = rdm_ref(MINI, KB, ww.down_qubit(first, SB), num)
    assert np.array_equal(bits(got.view(np.float64).reshape(want.shape)), bits(want)), (got, want)
    assert reg.rdm_stats()[0] == 0                                  # (read from the register itself)


def draws():
    """0.0, 1.0, plain values, and values at and within 1e-12 of a boundary of the running sum of MINI"""
    p = MINI[0::2] * MINI[0::2] + MINI[1::2] * MINI[1::2]
    cums, cum = [], np.float64(0.0)
    for v in p:
        cum = cum + v
        cums.append(float(cum))
    rs = [0.0, 1.0, 1e-300, 1e-7, 0.25, 0.5, 0.77, 0.999999, cums[-1], 1.5]
    for c in (cums[0], cums[6], cums[7], cums[1 << 9], cums[(1 << 11) - 1], cums[(1 << 11)], cums[-2]):
        rs += [c, float(np.nextafter(c, 0.0)), float(np.nextafter(c, 2.0)), c - 1e-12, c + 1e-12]
    return rs, cums[-1]


def test_sample_states_sparse(qc, ob, wide):
    """every draw 0 < r <= total picks the deposit of the oracle's pick on the mini state, inside the sub-cube; the two ends are
    the definition's as well (wide_windows.embedded_pick): r = 0.0 is met by the first amplitude, index 0, and r = 1.5, beyond the
    total, falls through to the last index of the register"""
    reg = hold_sparse(qc, wide)
    rs, total = draws()
    got = qc.sample_states(reg, rs)
    want = [ww.embedded_pick(N, SB, COLD_B, MINI, r, ob) for r in rs]
    assert [int(v) for v in got] == want
    inside = [int(v) for v, r in zip(got, rs) if 0.0 < r <= total]
    assert len(inside) >= len(rs) - 3 and all(v & ~ww.hot_mask(SB) == COLD_B for v in inside)
    assert len(set(inside)) > 12 and any(v >> TOP & 1 for v in inside) and any(v >> SUB & 1 and not v >> TOP & 1 for v in inside)
    assert int(got[0]) == 0 and int(got[1]) & ~ww.hot_mask(SB) == COLD_B     # r = 0.0: the first amplitude; r = 1.0: inside
    assert rs[9] == 1.5 and int(got[9]) == (1 << N) - 1
    assert np.array_equal(bits(ww.read_subcube(reg, SB, COLD_B)), bits(MINI))   # the state stays as it was


@pytest.mark.parametrize("which", [1, 15, 28, 0])
def test_measure_state_sparse(qc, ob, wide, which):
    """draws[which]: r = 1.0, a boundary of the running sum, one 1e-12 below a boundary, r = 0.0"""
    reg = hold_sparse(qc, wide)
    r = draws()[0][which]
    want = ww.embedded_pick(N, SB, COLD_B, MINI, r, ob)
    wide.holds = None
    assert qc.measure_state(reg, r) == want
    after = np.zeros(2 << KB)
    if which:
        assert want & ~ww.hot_mask(SB) == COLD_B
        after[2 * ww.extract(want, SB)] = 1.0
        assert zero_outside(reg)
    else:
        assert want == 0
        assert np.array_equal(bits(reg.read(0, 256)), bits(np.array([1.0] + [0.0] * 511)))
        assert not bits(reg.read((1 << N) - 256, 256)).any()
    assert np.array_equal(bits(ww.read_subcube(reg, SB, COLD_B)), bits(after))
    assert reg.norm2() == 1.0


@pytest.mark.parametrize("first,num", [(N - 3, 3), (0, 2)])
@pytest.mark.parametrize("r", [0.4, 0.93])
def test_measure_qubits_sparse(qc, wide, first, num, r):
    reg = hold_sparse(qc, wide)
    v, p, after = collapse_ref.measure_ref(MINI, KB, ww.down_qubit(first, SB), num, r)
    wide.holds = None
    outcome, prob = reg.measure_qubits(first, num, r)
    assert outcome == v and bits(prob) == bits(p)
    assert np.array_equal(bits(ww.read_subcube(reg, SB, COLD_B)), bits(after))
    assert zero_outside(reg)
    assert reg.collapse_stats()[0] == 0


@pytest.mark.parametrize("first,num,outcome", [(N - 3, 3, 5), (N - 3, 3, 2), (0, 2, 3)])
def test_postselect_sparse(qc, wide, first, num, outcome):
    reg = hold_sparse(qc, wide)
    p, after = collapse_ref.collapse_ref(MINI, KB, ww.down_qubit(first, SB), num, outcome)
    wide.holds = None
    assert bits(reg.postselect(first, num, outcome)) == bits(p)
    assert np.array_equal(bits(ww.read_subcube(reg, SB, COLD_B)), bits(after))
    assert zero_outside(reg)


# ---- c. observers on the uniform superposition ---------------------------------------------------------------------------------

def uniform_amplitude():
    """Hadamards on every qubit of |0>: c_n = fl(s * c_(n-1)) from 1 (tests/test_wide_windows.py pins this against the oracle)"""
    c = np.float64(1.0)
    for _ in range(N):
        c = c * np.float64(0.70710678118654752440)
    return c


def hold_uniform(qc, wide):
    if wide.holds != "uniform":
        wide.holds = None
        reg = wide.reg
        qc.reset_register(reg)
        reg.write(np.array([1.0, 0.0, 0.0, 0.0]), first=0)          # |0> in place of reset's |1>
        for q in range(N):
            qc.hadamard_gate(q, reg)
        wide.holds = "uniform"
    return wide.reg


def test_uniform_state_windows(qc, wide):
    reg = hold_uniform(qc, wide)
    want = np.zeros(2 << 13)
    want[0::2] = uniform_amplitude()
    rs = np.random.RandomState(3)
    starts = {0, (1 << N) - (1 << 13), 1 << 31, 1 << 32, (1 << 32) - (1 << 13), (1 << 32) | (1 << 31)}
    starts |= {(int(v) << 13) | 1 << 31 for v in rs.randint(0, 1 << (N - 13), 3)} | {(int(v) << 13) | 1 << 32 for v in rs.randint(0, 1 << (N - 13), 3)}
    for s in sorted(s & FULL & ~((1 << 13) - 1) for s in starts):
        assert np.array_equal(bits(reg.read(s, 1 << 13)), bits(want)), s


P_LEAF = uniform_amplitude() * uniform_amplitude()                   # p = fl(c * c): every leaf of every tree

X_ONLY = [{0: "X"}, {3: "X", 12: "X", TOP: "X"}, {SUB: "X", TOP: "X"}, {11: "X", 12: "X"}, {TOP: "X"}]
WITH_Z_OR_Y = [{TOP: "Z"}, {5: "Y"}, {12: "X", SUB: "Y", TOP: "Y"}, {0: "Z", 13: "X", TOP: "X"}, {q: "Z" for q in range(N)},
               {TOP: "Y"}, {11: "Z", 12: "Z", SUB: "X"}]


def test_expectation_uniform(qc, wide):
    reg = hold_uniform(qc, wide)
    whole = P_LEAF * np.float64(2.0) ** N
    for pauli in X_ONLY:
        assert bits(reg.expectation(pauli)) == bits(whole), pauli
    for pauli in WITH_Z_OR_Y:
        assert bits(reg.expectation(pauli)) == bits(0.0), pauli
    total, values = reg.expectation_batch([(1.0, p) for p in X_ONLY + WITH_Z_OR_Y])
    assert np.array_equal(bits(values), bits(np.array([whole] * len(X_ONLY) + [0.0] * len(WITH_Z_OR_Y))))


@pytest.mark.parametrize("first,num", [(0, 3), (11, 3), (N - 3, 3), (TOP, 1), (SUB, 2), (9, 6)])
def test_range_observers_uniform(qc, wide, first, num):
    reg = hold_uniform(qc, wide)
    entry = P_LEAF * np.float64(2.0) ** (N - num)
    got = reg.marginal(first, num)
    assert np.array_equal(bits(got), bits(np.full(1 << num, entry))), got
    if num <= qc.rdm_max_qubits():
        rho = reg.reduced_density_matrix(first, num)
        want = np.zeros((1 << num, 1 << num, 2))
        want[:, :, 0] = entry
        assert np.array_equal(bits(rho.view(np.float64).reshape(want.shape)), bits(want)), rho


# ---- d. refusals at this width ------------------------------------------------------------------------------------------------

def test_refusals_leave_the_state_alone(qc, wide):
    reg = wide.reg
    if wide.holds is None:
        reg.fill_random(9)
    lib = qc.lib()
    start = (1 << N) - 256
    before = reg.read(start, 256)
    out = C.c_double(0.0)
    u2 = np.ascontiguousarray(matrix(1, 2).reshape(-1)).view(np.float64)
    u4 = np.ascontiguousarray(matrix(1, 4).reshape(-1)).view(np.float64)
    p2, p4 = u2.ctypes.data_as(C.c_void_p), u4.ctypes.data_as(C.c_void_p)
    bit = np.array([1 << N], dtype=np.uint64)
    zero, one = np.array([0], dtype=np.uint64), np.array([1.0])
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)                    # noqa: E731
    tot, val = C.c_double(0.0), np.zeros(1)
    calls = {
        # a mask with bit N set
        "expectation x": lambda: lib.qcx_pauli_expectation(reg._h, 1 << N, 0, C.byref(out)),
        "expectation z": lambda: lib.qcx_pauli_expectation(reg._h, 1, 1 << N, C.byref(out)),
        "expectation_sum": lambda: lib.qcx_pauli_expectation_sum(reg._h, 1, ptr(bit), ptr(zero), ptr(one), ptr(val), C.byref(tot)),
        "expectation_batch": lambda: lib.qcx_pauli_expectation_batch(reg._h, 1, ptr(zero), ptr(bit), ptr(one), ptr(val), C.byref(tot)),
        "rotation x": lambda: lib.qcx_pauli_rotation(1 << N, 0, 0.3, reg._h),
        "rotation z": lambda: lib.qcx_pauli_rotation(0, 1 << N | 1 << TOP, 0.3, reg._h),
        "rotation_batch": lambda: lib.qcx_pauli_rotation_batch(reg._h, 1, ptr(bit), ptr(zero), ptr(one)),
        # a qubit number N
        "one_qubit": lambda: lib.qcx_one_qubit_gate(N, p2, reg._h),
        "c_one_qubit target": lambda: lib.qcx_c_one_qubit_gate(0, N, p2, reg._h),
        "c_one_qubit control": lambda: lib.qcx_c_one_qubit_gate(N, 0, p2, reg._h),
        "two_qubit": lambda: lib.qcx_two_qubit_gate(TOP, N, p4, reg._h),
        "c_two_qubit": lambda: lib.qcx_c_two_qubit_gate(N, 0, TOP, p4, reg._h),
        "marginal": lambda: lib.qcx_marginal_probabilities(reg._h, TOP, 2, ptr(val)),
        "rdm": lambda: lib.qcx_reduced_density_matrix(reg._h, N, 1, ptr(np.zeros(8))),
        "measure_qubits": lambda: lib.qcx_measure_qubits_r(reg._h, N, 1, 0.5, C.byref(C.c_ulong(0)), C.byref(out)),
        # a control of 2^31: a bad qubit, not "no control"
        "c_one_qubit 2^31": lambda: lib.qcx_c_one_qubit_gate(1 << 31, 0, p2, reg._h),
        "c_two_qubit 2^31": lambda: lib.qcx_c_two_qubit_gate(1 << 31, 0, 1, p4, reg._h),
    }
    for name, call in calls.items():
        assert call() == BAD_QUBIT, name
    with pytest.raises(qc.QcxError) as e:
        reg.marginal(0, 31)
    assert e.value.status == UNSUPPORTED
    assert np.array_equal(bits(reg.read(start, 256)), bits(before))
