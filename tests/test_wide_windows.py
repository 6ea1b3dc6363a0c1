"""CPU: the statements tests/wide_windows.py makes, on n = 18 registers that numpy holds whole -- tests/test_gpu_wide_registers.py
leans on each of them at 2^33 amplitudes, where nothing can be checked against the whole state.

Every definition is run twice, on the whole register and on the mini register of a sub-cube, and the comparison is on bits:
  * gates on a DENSE state (one_qubit_ref, two_qubit_ref, pauli_rotation_ref with the cold-Z sign rule): the sub-cube of the whole
    result is the result on the mini state;
  * observers on a state that is ZERO outside the sub-cube (pauli_ref, marginal_ref, rdm_ref, collapse_ref, the oracle's measure):
    the value on the whole register is the value on the mini state;
  * gather_dense against a plain slice of the oracle's fill_random state.
No GPU needed."""
import numpy as np
import pytest

import collapse_ref
import one_qubit_ref
import pauli_rotation_ref
import two_qubit_ref
import wide_windows as ww
from marginal_ref import marginal_ref
from pauli_ref import pauli_ref
from rdm_ref import rdm_ref

N = 18
K = 8
SEED = 77


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def random_cold(rs, S, n=N):
    free = [q for q in range(n) if q not in S]
    while True:
        cold = sum(1 << q for q in free if rs.randint(0, 2))
        if cold:
            return cold


def subcubes():
    """(S, cold): random S with and without the top qubit, with and without qubit 0, random non-zero cold; and the two extreme
    patterns, all zeros and all ones"""
    rs = np.random.RandomState(5)
    out = []
    for top in (True, False, True, False):
        while True:
            S = sorted(int(q) for q in rs.choice(N, K, replace=False))
            if (N - 1 in S) == top:
                break
        out.append((S, random_cold(rs, S)))
    S = [0, 1, 2, 3, 9, 10, 16, 17]
    out += [(S, 0), (S, ((1 << N) - 1) & ~ww.hot_mask(S))]
    return out


SUBCUBES = subcubes()
# sub-cubes with contiguous ranges at the bottom, in the middle and at the top (the range observers), cold with several bits
RANGE_CUBES = [(S, 0x2DA5B & ~ww.hot_mask(S)) for S in ([0, 1, 2, 7, 8, 9, 16, 17], [1, 2, 3, 4, 11, 12, 13, 15])]


def ids(cubes):
    return ["S" + "_".join(map(str, S)) + f"-{cold:x}" for S, cold in cubes]


@pytest.fixture(scope="module")
def dense(ob):
    a = ob.fill_random(N, SEED)
    a.setflags(write=False)
    return a


def random_mini(seed, k=K):
    rs = np.random.RandomState(seed)
    a = rs.uniform(-0.5, 0.5, 2 << k)
    return a / np.sqrt(np.sum(a * a))


def matrix(rs, d):
    """neither symmetric nor unitary"""
    return rs.uniform(-1, 1, (d, d)) + 1j * rs.uniform(-1, 1, (d, d))


def test_index_maps():
    rs = np.random.RandomState(1)
    for S, cold in SUBCUBES + RANGE_CUBES:
        idx = ww.embed_indices(S, cold)
        assert idx.dtype == np.uint64 and idx.size == 1 << K
        assert np.all(idx[1:] > idx[:-1])                                   # the map preserves order
        assert np.all(idx & np.uint64(~ww.hot_mask(S) & ((1 << N) - 1)) == np.uint64(cold))
        for m in rs.randint(0, 1 << K, 8):
            m = int(m)
            assert int(idx[m]) == ww.deposit(m, S) | cold
            assert ww.down(ww.up(m, S), S) == m and ww.extract(int(idx[m]), S) == m
        for j, q in enumerate(S):
            assert ww.up_qubit(j, S) == q and ww.down_qubit(q, S) == j and ww.up(1 << j, S) == 1 << q
        starts = ww.run_starts(S, cold)
        run = 1 << ww.run_bits(S)
        assert len(starts) * run == 1 << K
        for r, m in starts:
            assert np.array_equal(idx[m:m + run], np.arange(r, r + run, dtype=np.uint64))
    assert ww.run_bits(list(range(8)) + [12, 32]) == 8 and ww.run_bits([1, 2]) == 0
    big = ww.embed_indices([0, 31, 32], 1 << 33)                            # no 32-bit arithmetic in the helper itself
    assert [int(v) for v in big] == [(1 << 33) | (b0 | b1 << 31 | b2 << 32) for b2 in (0, 1) for b1 in (0, 1) for b0 in (0, 1)]
    with pytest.raises(AssertionError):
        ww.down(1 << 5, [0, 1, 2])
    with pytest.raises(AssertionError):
        ww.check_subcube(N, [0, 1], 1)


@pytest.mark.parametrize("S,cold", SUBCUBES + [(list(range(8)), 0x2A500), (list(range(8)) + [12, 17], 0x0A500)],
                         ids=ids(SUBCUBES) + ["runs-k8", "runs-k10"])
def test_gather_dense_is_a_slice(ob, dense, S, cold):
    got = ww.gather_dense(N, SEED, S, cold, ob)
    assert np.array_equal(bits(got), bits(ww.slice_state(dense, S, cold)))


class FakeRegister:
    """read / write of a register, on a numpy state"""

    def __init__(self, n, state):
        self.num_qubits, self.state, self.calls = n, np.array(state, dtype=np.float64), 0

    def read(self, first, count):
        self.calls += 1
        return self.state[2 * first:2 * (first + count)].copy()

    def write(self, amps, first=0):
        self.calls += 1
        self.state[2 * first:2 * first + amps.size] = amps


def test_read_and_write_subcube(dense):
    S, cold = list(range(6)) + [9, 17], 0x0A540
    reg = FakeRegister(N, dense)
    assert np.array_equal(bits(ww.read_subcube(reg, S, cold)), bits(ww.slice_state(dense, S, cold)))
    assert reg.calls == 4                                                   # runs of 2^6
    mini = random_mini(3)
    reg = FakeRegister(N, np.zeros(2 << N))
    ww.write_subcube(reg, S, cold, mini)
    assert np.array_equal(bits(reg.state), bits(ww.embed_state(N, S, cold, mini)))
    assert np.array_equal(bits(ww.read_subcube(reg, S, cold)), bits(mini))


# ---- gates on a dense state ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,cold", SUBCUBES, ids=ids(SUBCUBES))
def test_one_qubit_gates_map_the_subcube_to_itself(dense, S, cold):
    rs = np.random.RandomState(cold & 0xFFFF)
    mini = ww.slice_state(dense, S, cold)
    U = matrix(rs, 2)
    for t, c in [(S[0], None), (S[-1], None), (S[3], S[-1]), (S[-1], S[0]), (S[2], S[1])]:
        whole = one_qubit_ref.apply(dense, N, t, U, control=c)
        want = one_qubit_ref.apply(mini, K, ww.down_qubit(t, S), U, control=None if c is None else ww.down_qubit(c, S))
        assert np.array_equal(bits(ww.slice_state(whole, S, cold)), bits(want)), (t, c)


@pytest.mark.parametrize("S,cold", SUBCUBES, ids=ids(SUBCUBES))
def test_two_qubit_gates_map_the_subcube_to_itself(dense, S, cold):
    rs = np.random.RandomState(cold & 0xFFFF)
    mini = ww.slice_state(dense, S, cold)
    U = matrix(rs, 4)
    for q0, q1, c in [(S[0], S[-1], None), (S[-1], S[0], None), (S[3], S[4], None), (S[1], S[2], S[-1]), (S[-1], S[-2], S[0]),
                      (S[-1], S[2], S[5])]:
        whole = two_qubit_ref.apply(dense, N, q0, q1, U, control=c)
        want = two_qubit_ref.apply(mini, K, ww.down_qubit(q0, S), ww.down_qubit(q1, S), U,
                                   control=None if c is None else ww.down_qubit(c, S))
        assert np.array_equal(bits(ww.slice_state(whole, S, cold)), bits(want)), (q0, q1, c)


@pytest.mark.parametrize("S,cold", SUBCUBES, ids=ids(SUBCUBES))
def test_pauli_rotations_and_the_cold_z_sign_rule(dense, S, cold):
    rs = np.random.RandomState(cold & 0xFFFF)
    mini = ww.slice_state(dense, S, cold)
    hot, full = ww.hot_mask(S), (1 << N) - 1
    seen = set()
    for trial in range(8):
        x = ww.up(int(rs.randint(0, 1 << K)), S) if trial else 0           # (trial 0: a diagonal string)
        z = int(rs.randint(0, 1 << N)) if trial != 1 else ww.up(int(rs.randint(0, 1 << K)), S)
        if trial == 2:
            z = full                                                        # Z or Y on every qubit
        theta = float(rs.uniform(-3, 3))
        whole = pauli_rotation_ref.apply(dense, N, x, z, theta)
        want = ww.rotation_on_subcube(mini, S, cold, x, z, theta)
        assert np.array_equal(bits(ww.slice_state(whole, S, cold)), bits(want)), (hex(x), hex(z))
        seen.add(bin(z & ~hot & cold).count("1") & 1)
        if z & ~hot == 0:                                                   # no cold letter: the plain definition with carried masks
            plain = pauli_rotation_ref.apply(mini, K, ww.down(x, S), ww.down(z, S), theta)
            assert np.array_equal(bits(plain), bits(want))
    assert seen == {0, 1} or cold == 0                                      # both signs of the rule were met


# ---- observers on a state that is zero outside the sub-cube -------------------------------------------------------------------
@pytest.mark.parametrize("S,cold", SUBCUBES, ids=ids(SUBCUBES))
def test_pauli_expectation_of_an_embedded_state(S, cold):
    rs = np.random.RandomState(cold & 0xFFFF)
    mini = random_mini(cold & 0xFF)
    whole = ww.embed_state(N, S, cold, mini)
    for trial in range(8):
        x, z = int(rs.randint(0, 1 << K)), int(rs.randint(0, 1 << K))
        if trial == 0:
            x = 0
        got, want = pauli_ref(whole, N, ww.up(x, S), ww.up(z, S)), pauli_ref(mini, K, x, z)
        assert bits(got) == bits(want), (hex(x), hex(z))


def ranges_in(S, longest=3):
    return [(first, num) for first in S for num in range(1, longest + 1) if all(first + j in S for j in range(num))]


@pytest.mark.parametrize("S,cold", RANGE_CUBES, ids=ids(RANGE_CUBES))
def test_range_observers_of_an_embedded_state(S, cold):
    mini = random_mini(11 + (cold & 0xFF))
    whole = ww.embed_state(N, S, cold, mini)
    rngs = ranges_in(S)
    assert {num for _, num in rngs} == {1, 2, 3}
    for first, num in rngs:
        f = ww.down_qubit(first, S)
        assert np.array_equal(bits(marginal_ref(whole, N, first, num)), bits(marginal_ref(mini, K, f, num))), (first, num)
        assert np.array_equal(bits(rdm_ref(whole, N, first, num)), bits(rdm_ref(mini, K, f, num))), (first, num)
        P = marginal_ref(mini, K, f, num)
        for outcome in range(1 << num):
            p_whole, a_whole = collapse_ref.collapse_ref(whole, N, first, num, outcome)
            p_mini, a_mini = collapse_ref.collapse_ref(mini, K, f, num, outcome)
            assert bits(p_whole) == bits(p_mini) == bits(P[outcome])
            assert np.array_equal(bits(a_whole), bits(ww.embed_state(N, S, cold, a_mini))), (first, num, outcome)
        for r in (0.0, 0.3, 0.99, 1.0) + tuple(collapse_ref.running_sums(P)):
            assert collapse_ref.choose(marginal_ref(whole, N, first, num), r) == collapse_ref.choose(P, r)


@pytest.mark.parametrize("S,cold", SUBCUBES + RANGE_CUBES, ids=ids(SUBCUBES + RANGE_CUBES))
def test_measurement_pick_of_an_embedded_state(ob, S, cold):
    mini = random_mini(23 + (cold & 0xFF))
    mini[2 * 5], mini[2 * 5 + 1] = 0.0, 0.0                                 # a zero inside the sub-cube: a tie of the running sum
    whole = ww.embed_state(N, S, cold, mini)
    p = mini[0::2] * mini[0::2] + mini[1::2] * mini[1::2]
    cums, cum = [], np.float64(0.0)
    for v in p:
        cum = cum + v
        cums.append(float(cum))
    total = cums[-1]
    assert total == ww.sequential_total(mini)
    draws = [0.0, 5e-324, 1e-9, 0.25, 0.5, 0.999999, total, np.nextafter(total, 2.0), 1.5]
    for c in (cums[0], cums[4], cums[5], cums[100], cums[-2]):
        draws += [c, np.nextafter(c, 0.0), np.nextafter(c, 2.0), c - 1e-12, c + 1e-12]
    inside = 0
    for r in draws:
        want = ob.measure(whole.copy(), N, float(r))
        got = ww.embedded_pick(N, S, cold, mini, float(r), ob)
        assert got == want, (r, got, want)
        if 0.0 < r <= total:
            assert got & ~ww.hot_mask(S) == cold                            # inside the sub-cube
            inside += 1
    assert inside >= 25


def test_uniform_superposition_amplitude(ob):
    """Hadamards on every qubit of the basis state |0> (reset_register leaves |1>: the M register holds 1): every amplitude is the
    same double, c_n = fl(s * c_(n-1)) from c_0 = 1 (what the closed forms of the dense observer tests start from)"""
    n = 10
    a = np.zeros(2 << n)
    ob.reset(a, n)
    assert a[2] == 1.0
    a[2], a[0] = 0.0, 1.0
    for q in range(n):
        ob.hadamard(a, n, q)
    c = np.float64(1.0)
    for _ in range(n):
        c = c * np.float64(0.70710678118654752440)
    assert np.all(bits(a[0::2]) == bits(c)) and np.all(a[1::2] == 0.0)
