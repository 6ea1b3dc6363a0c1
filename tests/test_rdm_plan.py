"""CPU: the stage plan of qcx_reduced_density_matrix (include/qcx_plan.h: qcx_rdm_plan) -- every summed qubit reduced exactly
once, in ascending order over the stages, all rows through each later stage together, bounded scratch -- and a numpy emulation
of the planned stages against the definition (tests/rdm_ref.py) on adversarial states.  No GPU needed."""
import numpy as np
import pytest

from bitwise import same_with_nans as same
from marginal_ref import _reduce_bits
from pauli_cases import adversarial
from rdm_ref import rdm_ref


def popcount(x):
    return bin(int(x)).count("1")


def check_plan(qc, n, first, num):
    s0, stages = qc.rdm_plan(n, first, num)
    summed = [q for q in range(n) if not first <= q < first + num]
    # stage 0: the lowest summed qubits, all of them below 12 qubits, else those that fill a unit of 2^12 with the range and,
    # from 22 qubits on, up to four more (a workgroup adds the roots of consecutive units)
    assert s0.group_bits == min(max(n - 21, 0), 4)
    assert s0.sum_bits == min(n, 12) - num + s0.group_bits and s0.rest_bits == len(summed) - s0.sum_bits
    assert int(s0.sum_mask) == sum(1 << q for q in summed[:s0.sum_bits])
    assert s0.rows == 4 ** num and s0.row_stride == 1 << s0.rest_bits
    left = summed[s0.sum_bits:]                                      # the column bits of stage 0's output, ascending
    scratch = s0.rows << s0.rest_bits if stages else 0
    assert bool(stages) == bool(left)
    for i, s in enumerate(stages):
        assert s.kind == 1 and s.in_bits == len(left) + 2 * num
        if i:
            assert s.in_bits == stages[i - 1].out_bits
        assert popcount(s.tile_mask) == s.T <= 12 and s.sum_mask & ~s.tile_mask == 0 and s.tile_mask >> s.in_bits == 0
        k = popcount(s.sum_mask)
        assert k >= 1 and int(s.sum_mask) == (1 << k) - 1, "a stage sums the lowest summed bits that are left: no row bit"
        assert s.out_bits == s.in_bits - k
        left = left[k:]
        if s.final_stage:
            assert i == len(stages) - 1 and not left and s.out_bits == 2 * num
        else:
            assert s.out_offset == scratch
            scratch += 1 << s.out_bits
    assert not left, "not every summed qubit is reduced"
    assert s0.scratch == scratch
    # device scratch behind the 4^num results: none up to 12 qubits, else at most (1 + 2^-11) 2^(n + 2 num - 12 - group_bits)
    # doubles
    if n <= 12:
        assert scratch == 0
    else:
        assert scratch * 2048 <= 2049 << (n + 2 * num - 12 - s0.group_bits), (n, first, num, scratch)


@pytest.mark.parametrize("n", range(1, 35))
def test_plan_every_range(qc, n):
    most = qc.rdm_max_qubits()
    assert most >= 4
    for first in range(n + 1):
        for num in range(0, min(n - first, most) + 1):
            check_plan(qc, n, first, num)


def test_plan_errors(qc):
    from quantumcomputer_amd._lib import QcxError
    most = qc.rdm_max_qubits()
    for args, status in [((10, 8, 3), 6), ((10, 11, 0), 6), ((34, 0, most + 1), 7), ((34, 34 - most, most + 1), 6)]:
        with pytest.raises(QcxError) as e:
            qc.rdm_plan(*args)
        assert e.value.status == status


@np.errstate(over="ignore", invalid="ignore", under="ignore")
def emulate(qc, a, n, first, num):
    """the planned stages in numpy: stage 0 per row (the leaves indexed by the summed bits, squeezed), then the marginal stages on
    the rows x columns array; the 4^num components back as rdm_ref lays them out"""
    s0, stages = qc.rdm_plan(n, first, num)
    z = np.ascontiguousarray(a, dtype=np.float64).view(np.complex128).reshape(1 << (n - first - num), 1 << num, 1 << first)
    nv = 1 << num
    rows = []
    for row in range(nv * nv):
        v, w = min(divmod(row, nv)), max(divmod(row, nv))
        p, q = z[:, v, :].reshape(-1), z[:, w, :].reshape(-1)
        leaf = p.real * q.real + p.imag * q.imag if row // nv <= row % nv else p.imag * q.real - p.real * q.imag
        # (as the kernel: a leaf's "0.0 +" waits until stage 0's root -- a signed-zero leaf changes no other node's bits)
        rows.append(0.0 + _reduce_bits(leaf, n - num, (1 << s0.sum_bits) - 1))
    x = np.concatenate(rows)
    assert x.size == s0.rows * s0.row_stride
    for s in stages:
        assert x.size == 1 << s.in_bits
        x = _reduce_bits(x, s.in_bits, int(s.sum_mask))
    t = x.reshape(nv, nv)
    rho = np.zeros((nv, nv, 2))
    for v in range(nv):
        for w in range(v, nv):
            rho[v, w, 0] = rho[w, v, 0] = t[v, w]
            if v < w:
                rho[v, w, 1] = t[w, v]
                rho[w, v, 1] = 0.0 - t[w, v]
    return rho


@pytest.mark.parametrize("finite", [True, False], ids=["finite", "inf-nan"])
@pytest.mark.parametrize("n", range(1, 15))
def test_emulated_stages_equal_the_definition(qc, n, finite):
    a = adversarial(n, 43 * n, finite)
    firsts = range(n + 1) if n <= 12 else (0, 3, 7, 9, 10, 11, 12, 13, 14)
    for first in firsts:
        for num in range(min(n - first, qc.rdm_max_qubits()) + 1):
            same(emulate(qc, a, n, first, num), rdm_ref(a, n, first, num), (n, first, num))
