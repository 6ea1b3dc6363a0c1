"""GPU: qcx_mc_one_qubit_gate / qcx_mc_two_qubit_gate on a register of 2^33 amplitudes (128 GiB; QCX_TEST_NWIDE, default 33): a
target or a control at bit 32, indices with bit 31 set, work numberings whose deposit crosses bit 32.  test_gpu_wide_registers.py's
method: nothing of this size visits the host; tests/wide_windows.py turns the register into sub-cubes of 8 to 16 qubits (qubits
0-7 plus the targets, a fixed pattern `cold` on the others) and tests/mc_gate_ref.py says what each must hold.  The controls
outside a sub-cube are constants of it: where `cold` has their values the sub-cube takes the gate under the controls inside it,
where it has not the sub-cube must come back untouched, bit for bit.  Every comparison is on uint64 views.

With TOP = N - 1, SUB = N - 2 and Q30 = N - 3 the cases read as the 32, 31 and 30 of the default size."""
import os

import numpy as np
import pytest

import mc_gate_ref as mc
import wide_windows as ww

pytestmark = pytest.mark.gpu

N = int(os.environ.get("QCX_TEST_NWIDE", "33"))
TOP, SUB, Q30 = N - 1, N - 2, N - 3
FULL = (1 << N) - 1
LOW8 = list(range(8))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def wide(qc):
    import torch
    free, total = torch.cuda.mem_get_info()
    need = (16 << N) + (8 << 30)
    print(f"\nwide register: n = {N}, {free} bytes of device memory free, {need} needed")
    if free < need:
        pytest.skip(f"a register of {N} qubits needs {need} bytes of free device memory, {free} are free")
    reg = qc.Register(N, 0)
    yield reg
    reg.close()


def matrix(seed, d):
    """neither symmetric nor unitary: a swapped row or column shows"""
    rs = np.random.RandomState(seed)
    return rs.uniform(-1, 1, (d, d)) + 1j * rs.uniform(-1, 1, (d, d))


def cold_patterns(S, cmask, cvals):
    """[(cold, the controls outside S hold their values)]: four base patterns (bit TOP set and SUB clear; the reverse; all zeros;
    all ones -- the last two begin and end with the two ends of the register), each once with the cold controls at their values
    and once with one of them flipped"""
    free = FULL & ~ww.hot_mask(S)
    cold_c = cmask & free
    cbits = [b for b in range(N) if cold_c >> b & 1]
    a = (0x0A5A5C3C96 | 1 << TOP) & ~(1 << SUB)
    b = (0x15A3C5A369 | 1 << SUB) & ~(1 << TOP)
    out = []
    for j, base in enumerate((a & free, b & free, 0, free)):
        sat = (base & ~cold_c) | (cvals & cold_c)
        out.append((sat, True))
        if cbits:
            out.append((sat ^ (1 << cbits[j % len(cbits)]), False))
    return out


CASES = {
    "target-32-under-31-and-5": ((TOP,), {SUB: 1, 5: 1}),
    "target-3-under-not-32-and-31": ((3,), {TOP: 0, SUB: 1}),
    "targets-32-0-under-31-and-1": ((TOP, 0), {SUB: 1, 1: 1}),
    "target-31-under-32-30-12-2": ((SUB,), {TOP: 1, Q30: 1, 12: 1, 2: 1}),
    "target-32-under-not-31": ((TOP,), {SUB: 0}),
    "targets-0-32-under-not-31-and-not-2": ((0, TOP), {SUB: 0, 2: 0}),
}


@pytest.mark.parametrize("case", list(CASES))
def test_gate_under_a_mask(qc, ob, wide, case):
    targets, ctl = CASES[case]
    cmask, cvals = sum(1 << c for c in ctl), sum(1 << c for c, v in ctl.items() if v)
    S = sorted(set(LOW8) | set(targets))
    hot = ww.hot_mask(S)
    U = matrix(sum(targets) + cmask % 1000, 2 * len(targets))
    seed = 5100 + list(CASES).index(case)
    wide.fill_random(seed)
    if len(targets) == 1:
        qc.mc_one_qubit_gate(cmask, targets[0], U, wide, values=cvals)
    else:
        qc.mc_two_qubit_gate(cmask, targets[0], targets[1], U, wide, values=cvals)
    patterns = cold_patterns(S, cmask, cvals)
    assert any(s for _, s in patterns) and any(not s for _, s in patterns)
    for cold, satisfied in patterns:
        mini = ww.gather_dense(N, seed, S, cold, ob)
        if satisfied:
            want = mc.apply(mini, len(S), [ww.down_qubit(q, S) for q in targets], U, ww.down(cmask & hot, S), ww.down(cvals & hot, S))
        else:
            want = mini                                            # untouched, bit for bit
        got = ww.read_subcube(wide, S, cold)
        bad = np.nonzero(bits(got).reshape(-1, 2) != bits(want).reshape(-1, 2))[0]
        assert bad.size == 0, (f"{case}, cold = {cold:#x} ({'controls hold' if satisfied else 'a control fails'}): {bad.size} of "
                               f"{1 << len(S)} amplitudes differ, the first at index {int(ww.embed_indices(S, cold)[bad[0]]):#x}")
