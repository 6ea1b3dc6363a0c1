"""GPU: qcx_mc_multi_qubit_gate on a register of 2^33 amplitudes (128 GiB; QCX_TEST_NWIDE, default 33): targets that straddle
bit 32, five targets spread up to it, and low targets under controls at bits 31 and 32, one of them negative -- tile bases whose
deposit crosses bit 32, indices with bit 31 set.  test_gpu_wide_permutation.py's method: nothing of this size visits the host;
tests/wide_windows.py turns the register into sub-cubes (qubits 0-7 plus the qubits the call names, a fixed pattern `cold` on the
others) and tests/multi_qubit_ref.py says what each must hold.  The controls outside a sub-cube are constants of it: where
`cold` has their values the sub-cube takes the matrix under the controls inside it, where it has not the sub-cube must come
back untouched, bit for bit.  Every comparison is on uint64 views.

With TOP = N - 1 and SUB = N - 2 the cases read as the 32 and 31 of the default size."""
import os

import numpy as np
import pytest

import multi_qubit_ref as mq
import wide_windows as ww
from bitwise import random_unitary

pytestmark = pytest.mark.gpu

N = int(os.environ.get("QCX_TEST_NWIDE", "33"))
TOP, SUB = N - 1, N - 2
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


def cold_patterns(S, cmask, cvals):
    """[(cold, the controls outside S hold their values)]: four base patterns (bit TOP set and SUB clear; the reverse; all zeros;
    all ones), each once with the cold controls at their values and once with one of them flipped"""
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


# (targets, {control: value}, the qubits of the sub-cubes besides 0-7 and the targets)
CASES = {
    "targets-5-31-32": ((5, SUB, TOP), {}, []),
    "targets-9-20-30-31-32": ((9, 20, N - 3, SUB, TOP), {}, []),
    "targets-3-to-6-under-31-and-not-32": ((3, 4, 5, 6), {SUB: 1, TOP: 0}, [SUB]),
    "targets-3-to-6-under-not-31-and-32": ((6, 4, 3, 5), {SUB: 0, TOP: 1}, [TOP]),
}


@pytest.mark.parametrize("case", list(CASES))
def test_matrix_on_a_wide_register(qc, ob, wide, case):
    targets, ctl, extra = CASES[case]
    cmask, cvals = sum(1 << c for c in ctl), sum(1 << c for c, v in ctl.items() if v)
    S = sorted(set(LOW8) | set(targets) | set(extra))
    hot = ww.hot_mask(S)
    U = random_unitary(len(case), 1 << len(targets))
    seed = 5300 + list(CASES).index(case)
    wide.fill_random(seed)
    qc.multi_qubit_gate(targets, U, wide, controls=cmask, values=cvals)
    st, pl = qc.multi_gate_plan(N, cmask, cvals, targets)
    assert st == 0 and wide.multi_qubit_stats() == (pl.form, len(targets))
    patterns = cold_patterns(S, cmask, cvals)
    assert any(s for _, s in patterns) and (not ctl or any(not s for _, s in patterns))
    for cold, satisfied in patterns:
        mini = ww.gather_dense(N, seed, S, cold, ob)
        if satisfied:
            want = mq.apply(mini, len(S), [ww.down_qubit(q, S) for q in targets], U, ww.down(cmask & hot, S), ww.down(cvals & hot, S))
            assert not np.array_equal(bits(want), bits(mini))
        else:
            want = mini                                            # untouched, bit for bit
        got = ww.read_subcube(wide, S, cold)
        bad = np.nonzero(bits(got).reshape(-1, 2) != bits(want).reshape(-1, 2))[0]
        assert bad.size == 0, (f"{case}, cold = {cold:#x} ({'controls hold' if satisfied else 'a control fails'}): {bad.size} of "
                               f"{1 << len(S)} amplitudes differ, the first at index {int(ww.embed_indices(S, cold)[bad[0]]):#x}")
