"""CPU: tests/mc_gate_ref.py, the numpy definition of qcx_mc_one_qubit_gate / qcx_mc_two_qubit_gate, against the definitions it
extends (one_qubit_ref, two_qubit_ref: bit for bit) and against the dense 2^n x 2^n matrix built independently.  No GPU needed."""
import numpy as np
import pytest

import mc_gate_ref as mc
import one_qubit_ref as oq
import two_qubit_ref as tq
from bitwise import minus_zero_state, random_unitary, same


def poisoned(ob, n, seed):
    """-0, Inf, -Inf and NaN components among random ones"""
    a = minus_zero_state(ob, n, seed)
    k = a.size
    a[3 % k] = np.inf
    a[(k // 2 + 1) % k] = np.nan
    a[k - 1] = -np.inf
    return a


@pytest.mark.parametrize("n", range(1, 7))
def test_no_control_and_one_positive_control_are_the_existing_definitions(ob, n):
    """1. every form of the plain and the singly controlled gates at n = 1 .. 6, on fill_random states and on states with -0, Inf
    and NaN: the same bits, NaN payloads included (the operations are the same ones in the same order)"""
    for label, a in (("fill_random", ob.fill_random(n, n)), ("minus zero", minus_zero_state(ob, n, 60 + n)), ("poisoned", poisoned(ob, n, 70 + n))):
        k = 0
        for q in range(n):
            for c in [None] + [c for c in range(n) if c != q]:
                U = random_unitary(100 * n + k, 2); k += 1
                m = 0 if c is None else 1 << c
                same(mc.apply1(a, n, q, U, m, m), oq.apply(a, n, q, U, control=c), f"{label} n={n} c={c} q={q}")
        for q0 in range(n):
            for q1 in range(n):
                if q0 == q1:
                    continue
                for c in [None] + [c for c in range(n) if c not in (q0, q1)]:
                    U = random_unitary(100 * n + k, 4); k += 1
                    m = 0 if c is None else 1 << c
                    same(mc.apply2(a, n, q0, q1, U, m, m), tq.apply(a, n, q0, q1, U, control=c), f"{label} n={n} c={c} q0={q0} q1={q1}")


def dense(n, targets, U, mask, values):
    """projector onto the control pattern (x) U + the identity elsewhere, as a 2^n x 2^n complex matrix in two longdouble parts,
    built entry by entry from the bits of the row and column numbers"""
    N = 1 << n
    U = np.asarray(U, dtype=complex)
    tm = sum(1 << q for q in targets)
    Dr, Di = np.zeros((N, N), dtype=np.longdouble), np.zeros((N, N), dtype=np.longdouble)
    for i in range(N):
        if (i & mask) != values:
            Dr[i, i] = 1
            continue
        for j in range(N):
            if (i ^ j) & ~tm:
                continue
            r = sum(((i >> q) & 1) << b for b, q in enumerate(targets))
            c = sum(((j >> q) & 1) << b for b, q in enumerate(targets))
            Dr[i, j], Di[i, j] = U[r, c].real, U[r, c].imag
    return Dr, Di


def check_dense(a, n, targets, U, mask, values, ulps):
    got = mc.apply(a, n, targets, U, mask, values)
    Dr, Di = dense(n, targets, U, mask, values)
    xr, xi = a[0::2].astype(np.longdouble), a[1::2].astype(np.longdouble)
    wr, wi = Dr @ xr - Di @ xi, Dr @ xi + Di @ xr
    bound = ulps * np.spacing(np.max(np.abs(a)))
    err = max(float(np.max(np.abs(got[0::2] - wr))), float(np.max(np.abs(got[1::2] - wi))))
    assert err <= bound, (targets, mask, values, err, bound)


def test_against_the_dense_matrix(ob):
    """2. n = 5, every (mask, values, target): the definition is the dense operator to the rounding of one complex row in
    binary64, at most 4 ulp of the amplitude scale (the largest input component), for one target and for two alike.  A check of
    the definition, not of the kernels."""
    n = 5
    a = ob.fill_random(n, 17)
    for k, (t, m, v) in enumerate(mc.forms1(n)):
        check_dense(a, n, t, random_unitary(k, 2), m, v, 4)
    for k, (t, m, v) in enumerate(mc.forms2(n)):
        check_dense(a, n, t, random_unitary(1000 + k, 4), m, v, 4)


def test_the_number_of_forms():
    assert sum(len(mc.forms1(n)) for n in range(1, 6)) == 547 and sum(len(mc.forms2(n)) for n in range(1, 6)) == 668
