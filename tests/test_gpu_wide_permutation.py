"""GPU: qcx_permutation_gate on a register of 2^33 amplitudes (128 GiB; QCX_TEST_NWIDE, default 33): a range that crosses bit 32,
and a low range under controls at bits 31 and 32, one of them negative -- tile bases whose deposit crosses bit 32, indices with
bit 31 set.  test_gpu_wide_mc_gates.py's method: nothing of this size visits the host; tests/wide_windows.py turns the register
into sub-cubes (qubits 0-7 plus the range and one of the controls, a fixed pattern `cold` on the others) and
tests/permutation_ref.py says what each must hold.  The controls outside a sub-cube are constants of it: where `cold` has
their values the sub-cube takes the table under the controls inside it, where it has not the sub-cube must come back untouched,
bit for bit.  Every comparison is on uint64 views.

With TOP = N - 1 and SUB = N - 2 the cases read as the 32 and 31 of the default size."""
import os

import numpy as np
import pytest

import permutation_ref as pr
import wide_windows as ww

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


# (first, num, {control: value}, the qubits of the sub-cubes besides 0-7 and the range)
CASES = {
    "range-29-to-32": (N - 4, 4, {}, []),
    "range-8-to-10-under-31-and-not-32": (8, 3, {SUB: 1, TOP: 0}, [SUB]),
    "range-8-to-10-under-not-31-and-32": (8, 3, {SUB: 0, TOP: 1}, [TOP]),
}


@pytest.mark.parametrize("case", list(CASES))
def test_table_on_a_wide_register(qc, ob, wide, case):
    first, num, ctl, extra = CASES[case]
    cmask, cvals = sum(1 << c for c in ctl), sum(1 << c for c, v in ctl.items() if v)
    S = sorted(set(LOW8) | set(range(first, first + num)) | set(extra))
    hot = ww.hot_mask(S)
    perm = np.random.RandomState(len(case)).permutation(1 << num)
    assert int(np.count_nonzero(perm != np.arange(1 << num))) >= (1 << num) - 2
    seed = 5200 + list(CASES).index(case)
    wide.fill_random(seed)
    qc.permutation_gate(first, num, perm, wide, controls=cmask, values=cvals)
    st, pl = qc.permutation_plan(N, cmask, cvals, first, num)
    assert st == 0 and wide.permutation_stats() == (pl.form, int(np.count_nonzero(perm != np.arange(1 << num))))
    patterns = cold_patterns(S, cmask, cvals)
    assert any(s for _, s in patterns) and (not ctl or any(not s for _, s in patterns))
    for cold, satisfied in patterns:
        mini = ww.gather_dense(N, seed, S, cold, ob)
        if satisfied:
            want = pr.apply(mini, len(S), ww.down_qubit(first, S), num, perm, ww.down(cmask & hot, S), ww.down(cvals & hot, S))
            assert not np.array_equal(bits(want), bits(mini))
        else:
            want = mini                                            # untouched, bit for bit
        got = ww.read_subcube(wide, S, cold)
        bad = np.nonzero(bits(got).reshape(-1, 2) != bits(want).reshape(-1, 2))[0]
        assert bad.size == 0, (f"{case}, cold = {cold:#x} ({'controls hold' if satisfied else 'a control fails'}): {bad.size} of "
                               f"{1 << len(S)} amplitudes differ, the first at index {int(ww.embed_indices(S, cold)[bad[0]]):#x}")
