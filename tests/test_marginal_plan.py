"""CPU: the stage plan of qcx_marginal_probabilities (include/qcx_plan.h) -- every summed bit reduced exactly once, stages in
ascending bit order, whole 128-B runs, bounded scratch -- and a numpy emulation of the planned stages against the pinned
summation order (tests/marginal_ref.py) on adversarial states.  No GPU needed."""
import numpy as np
import pytest

from marginal_ref import compact_leaves, emulate_stages, marginal_ref


def popcount(x):
    return bin(int(x)).count("1")


def check_plan(stages, n, first, num, M=0):
    summed = ((1 << n) - 1) & ~(((1 << num) - 1) << first)
    seen, prev_top = 0, -1
    scratch = 0
    for i, s in enumerate(stages):
        assert s.kind == (0 if M == 0 else 2) if i == 0 else s.kind == 1
        if i:
            assert s.in_bits == stages[i - 1].out_bits
        else:
            assert s.in_bits == n - M
        assert popcount(s.tile_mask) == s.T and s.T <= (8 if s.kind == 2 else 12)
        assert s.sum_mask & ~s.tile_mask == 0 and s.tile_mask >> s.in_bits == 0
        cmin = {0: 3, 1: 4, 2: 1}[s.kind]
        assert s.c == min(cmin, s.in_bits) and s.tile_mask & ((1 << s.c) - 1) == (1 << s.c) - 1    # whole 128-B runs
        assert s.out_bits == s.in_bits - popcount(s.sum_mask)
        q = int(s.qubits)
        assert popcount(q) == popcount(s.sum_mask) + (M if i == 0 else 0)
        assert q & seen == 0, "a bit summed twice"
        low = (q & -q).bit_length() - 1 if q else None
        if q:
            assert low > prev_top, "a stage's bits lie below the previous stage's"
            prev_top = q.bit_length() - 1
        seen |= q
        if s.final_stage:
            assert i == len(stages) - 1 and s.out_bits == num
        else:
            assert s.out_offset == scratch
            scratch += 1 << s.out_bits
    assert seen == summed, "not every summed bit is reduced"
    assert stages[-1].final_stage
    # device scratch: the output plus at most 1/512 of the state's bytes
    assert 8 * scratch <= (16 << n) // 512, (n, first, num, scratch)


@pytest.mark.parametrize("n", range(1, 35))
def test_plan_every_range(qc, n):
    for first in range(n + 1):
        for num in range(0, min(n - first, 30) + 1):
            check_plan(qc.marginal_plan(n, first, num), n, first, num)


@pytest.mark.parametrize("M", [2, 4, 5, 8, 12])
def test_compact_plan_every_range(qc, M):
    for n in range(M + 6, 35, 3 if M > 4 else 1):
        for first in range(M, n + 1):
            for num in range(0, min(n - first, 30) + 1):
                check_plan(qc.marginal_plan(n, first, num, M=M), n, first, num, M)


def test_plan_errors(qc):
    from quantumcomputer_amd._lib import QcxError
    for args, status in [((10, 5, 6), 6), ((10, 11, 0), 6), ((34, 0, 31), 7), ((34, 3, 31), 7)]:
        with pytest.raises(QcxError) as e:
            qc.marginal_plan(*args)
        assert e.value.status == status
    with pytest.raises(QcxError):
        qc.marginal_plan(20, 3, 4, M=5)                      # a compact plan needs first >= M


def adversarial(n, seed):
    rs = np.random.RandomState(seed)
    a = rs.standard_normal(2 << n) * 2.0 ** rs.randint(-40, 40, 2 << n)
    k = a.size
    a[rs.randint(0, k, max(1, k // 16))] = 5e-324 * rs.randint(1, 1000, max(1, k // 16))     # subnormals
    a[rs.randint(0, k, max(1, k // 32))] = 1e300                                              # |a|^2 overflows to Inf
    a[rs.randint(0, k, max(1, k // 16))] = 0.0
    a[rs.randint(0, k, max(1, k // 16))] = -0.0
    a[rs.randint(0, k, max(1, k // 64))] = 1e154
    if n >= 4:
        a[rs.randint(0, k)] = np.inf
        a[rs.randint(0, k)] = -np.inf
        a[rs.randint(0, k)] = np.nan
    return a


def same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn)
    assert np.array_equal(got[~gn].view(np.uint64), want[~wn].view(np.uint64))


@pytest.mark.parametrize("n", range(1, 15))
def test_emulated_stages_equal_the_definition(qc, n):
    for seed in (1, 2):
        a = adversarial(n, 100 * n + seed)
        for first in range(n + 1):
            for num in range(n - first + 1):
                same(emulate_stages(qc.marginal_plan(n, first, num), a=a), marginal_ref(a, n, first, num))


def test_definition_differs_from_a_sequential_sum():
    """the pinned order matters: on a random state most outputs differ from a sequential loop's"""
    n, first, num = 14, 5, 4
    a = np.random.RandomState(3).standard_normal(2 << n)
    ref = marginal_ref(a, n, first, num)
    p = (a.reshape(-1, 2) ** 2).sum(axis=1).reshape(1 << (n - first - num), 1 << num, 1 << first)
    seq = np.zeros(1 << num)
    for v in range(1 << num):
        t = 0.0
        for h in range(p.shape[0]):
            for lo in range(p.shape[2]):
                t += p[h, v, lo]
        seq[v] = t
    assert np.count_nonzero(ref != seq) > 0


@pytest.mark.parametrize("M,orbit,cb", [(4, [1, 4, 7, 13], 2), (5, [1, 2, 4, 8, 11, 16], 3), (5, [0, 3, 5, 6, 9, 17, 22, 31], 3),
                                        (6, list(range(0, 64, 5)), 4)])
def test_emulated_compact_stages_equal_the_definition(qc, M, orbit, cb):
    n = M + 8
    rs = np.random.RandomState(M)
    a = np.zeros((1 << (n - M), 1 << M), dtype=np.complex128)
    a[:, orbit] = rs.standard_normal((1 << (n - M), len(orbit))) + 1j * rs.standard_normal((1 << (n - M), len(orbit)))
    a[3, orbit[0]] = np.nan
    a[7, orbit[-1]] = 1e300
    a = a.reshape(-1)
    comp = compact_leaves(a, n, M, orbit, cb)
    for first in range(M, n + 1):
        for num in range(n - first + 1):
            same(emulate_stages(qc.marginal_plan(n, first, num, M=M), compact=(comp, orbit, M)), marginal_ref(a, n, first, num))
