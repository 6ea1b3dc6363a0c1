"""Sub-cubes of a register too large for the host: the 2^k amplitudes of an n-qubit register whose index agrees with a fixed
pattern `cold` outside k chosen qubits S, taken as a register of k qubits that numpy holds.  Host only.

S is the ascending list of the k real qubit numbers; mini qubit j is real qubit S[j].  The map

    real(m) = deposit(m, S) | cold          (deposit: bit j of m goes to bit S[j]; cold has no bit of S)

from mini index to real index preserves order, which is what makes the numpy definitions of tests/*_ref.py, unchanged, say
what the sub-cube of the large register must hold:

GATES.  A gate that names only qubits of S maps the sub-cube to itself, and every "ascending column order" decision of the
definitions is the same in both numberings.  one_qubit_ref.apply, two_qubit_ref.apply and pauli_rotation_ref.apply on the mini
state, qubits and masks carried by down(), give the sub-cube of the real result bit for bit -- on any state.  A rotation string
may carry Z letters on cold qubits as well: their parity on `cold` is a constant of the sub-cube, and an odd one negates s
(rotation_on_subcube).

OBSERVERS.  On a state that is ZERO outside the sub-cube every leaf outside it is +0, no node of a pairwise tree is ever -0 and
adding +0 is exact: pauli_ref, marginal_ref, rdm_ref and collapse_ref on the mini state are the definition on the whole register
bit for bit (range qubits inside S; they are neighbours in the mini numbering when they are in the real one).  The sequential
cumulative sum of measure_state / sample_states passes +0 leaves too, so a draw 0 < r <= total picks real(the mini pick); the two
ends differ, and embedded_pick states them: r <= 0 is met by the very first amplitude, index 0, whatever the state, and an r
beyond the total falls through to the LAST index of the register the scan runs on.

tests/test_wide_windows.py pins every one of these statements on n = 18 registers that numpy holds whole."""
import numpy as np

import pauli_rotation_ref


def check_subcube(n, S, cold):
    S = [int(q) for q in S]
    assert S == sorted(set(S)) and (not S or (0 <= S[0] and S[-1] < n)), S
    assert 0 <= cold < 1 << n and cold & hot_mask(S) == 0, (S, hex(cold))
    return S


def hot_mask(S):
    return sum(1 << int(q) for q in S)


def deposit(m, S):
    """bit j of m to bit S[j]: a Python int, or a numpy uint64 array"""
    if isinstance(m, np.ndarray):
        out = np.zeros(m.shape, dtype=np.uint64)
        for j, q in enumerate(S):
            out |= ((m >> np.uint64(j)) & np.uint64(1)) << np.uint64(q)
        return out
    m = int(m)
    assert 0 <= m < 1 << len(S)
    return sum((m >> j & 1) << int(q) for j, q in enumerate(S))


def extract(v, S):
    """bit S[j] of v to bit j (the bits outside S are dropped)"""
    v = int(v)
    return sum((v >> int(q) & 1) << j for j, q in enumerate(S))


def up(mask, S):
    """a mask over the mini qubits, in the real numbering"""
    return deposit(mask, S)


def down(mask, S):
    """a mask over real qubits, all of them in S, in the mini numbering"""
    mask = int(mask)
    assert mask & ~hot_mask(S) == 0, (hex(mask), S)
    return extract(mask, S)


def up_qubit(j, S):
    return int(S[j])


def down_qubit(q, S):
    return [int(s) for s in S].index(int(q))


def embed_indices(S, cold):
    """the real index of every mini index, ascending: uint64[2^k]"""
    assert cold & hot_mask(S) == 0, (S, hex(cold))
    return deposit(np.arange(1 << len(S), dtype=np.uint64), S) | np.uint64(cold)


def run_bits(S):
    """the sub-cube consists of runs of 2^this contiguous amplitudes: the number j of leading qubits with S[j] == j"""
    j = 0
    while j < len(S) and int(S[j]) == j:
        j += 1
    return j


def run_starts(S, cold):
    """(real index, mini index) of the first amplitude of every run, ascending"""
    j = run_bits(S)
    hi = np.arange(1 << (len(S) - j), dtype=np.uint64) << np.uint64(j)
    return [(int(r), int(m)) for r, m in zip(deposit(hi, S) | np.uint64(cold), hi)]


def gather_dense(n, seed, S, cold, ob):
    """the sub-cube of the state fill_random(seed) makes at n qubits, from the oracle's per-index generator: interleaved float64"""
    S = check_subcube(n, S, cold)
    run = 1 << run_bits(S)
    out = np.empty(2 << len(S), dtype=np.float64)
    for r, m in run_starts(S, cold):
        out[2 * m:2 * (m + run)] = ob.fill_random(n, seed, r, run)
    return out


def read_subcube(reg, S, cold):
    """the sub-cube of a register's state through reg.read(start, count): interleaved float64"""
    S = check_subcube(reg.num_qubits, S, cold)
    run = 1 << run_bits(S)
    out = np.empty(2 << len(S), dtype=np.float64)
    for r, m in run_starts(S, cold):
        out[2 * m:2 * (m + run)] = reg.read(r, run)
    return out


def write_subcube(reg, S, cold, mini):
    """mini (interleaved float64, 2 * 2^k) into the sub-cube of a register's state through reg.write(amps, first=)"""
    S = check_subcube(reg.num_qubits, S, cold)
    mini = np.ascontiguousarray(mini, dtype=np.float64)
    assert mini.size == 2 << len(S)
    run = 1 << run_bits(S)
    for r, m in run_starts(S, cold):
        reg.write(mini[2 * m:2 * (m + run)], first=r)


def embed_state(n, S, cold, mini):
    """the n-qubit state that is `mini` on the sub-cube and (+0, +0) outside it (small n only: the CPU tests)"""
    S = check_subcube(n, S, cold)
    full = np.zeros(2 << n, dtype=np.float64)
    idx = embed_indices(S, cold).astype(np.int64)
    mini = np.ascontiguousarray(mini, dtype=np.float64)
    full[2 * idx], full[2 * idx + 1] = mini[0::2], mini[1::2]
    return full


def slice_state(full, S, cold):
    """the sub-cube of a state numpy holds whole"""
    idx = embed_indices(S, cold).astype(np.int64)
    full = np.ascontiguousarray(full, dtype=np.float64)
    out = np.empty(2 << len(S), dtype=np.float64)
    out[0::2], out[1::2] = full[2 * idx], full[2 * idx + 1]
    return out


def rotation_on_subcube(mini, S, cold, x_mask, z_mask, theta):
    """pauli_rotation(x_mask, z_mask, theta) of the large register, on its sub-cube: x_mask inside S; z_mask anywhere -- the Z
    letters on cold qubits see the constant `cold`, and an odd parity there negates s"""
    c, s = pauli_rotation_ref.polar(np.float64(theta) / np.float64(2.0))
    hot = hot_mask(S)
    if bin(z_mask & ~hot & cold).count("1") & 1:
        s = -s
    return pauli_rotation_ref.apply_cs(mini, len(S), down(x_mask, S), down(z_mask & hot, S), c, s)


def sequential_total(mini):
    """the last value of the measurement's running sum over a state: cum = fl(cum + fl(fl(x*x) + fl(y*y))), index ascending"""
    a = np.ascontiguousarray(mini, dtype=np.float64)
    p = a[0::2] * a[0::2] + a[1::2] * a[1::2]
    cum = np.float64(0.0)
    for v in p:
        cum = cum + v
    return float(cum)


def embedded_pick(n, S, cold, mini, r, ob):
    """the index measure_state / sample_states give for the draw r on the n-qubit state that is `mini` on the sub-cube and zero
    outside it, from the oracle's pick on the mini state"""
    S = check_subcube(n, S, cold)
    if r <= 0.0:
        return 0                                             # cum = +0 >= r at the first amplitude of any register
    if not r <= sequential_total(mini):
        return (1 << n) - 1                                  # nothing reaches r: the scan falls through to the last index
    return deposit(ob.measure(np.array(mini, dtype=np.float64), len(S), float(r)), S) | cold
