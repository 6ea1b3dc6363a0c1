"""CPU: tests/one_qubit_ref.py -- the numpy restatement that defines qcx_one_qubit_gate / qcx_c_one_qubit_gate -- is pinned to
the reference's arithmetic through the oracle: with H's entries it must give the oracle's Hadamard on every bit, controlled
with diag(1, polar(theta)) the oracle's controlled phase, on finite states, on states with -0 components and on a state that
holds an Inf (where the zero entries and the identity rows poison, qc_shor.c:393-413).  Both forms of the oracle are asked: the
pairwise layer at n = 1..8 and the literal COO mat-vec of the reference (LiteralRegister) at n <= 5.

Where the Inf sits matters for the controlled-phase comparison, and only there.  The one-qubit gate stores all four entries of
its matrix, the two zeros of diag(1, e^{i theta}) included, while the reference's c_phase_shift_gate stores the diagonal alone
(qc_shor.c:529-562).  On finite states the two give the same bits.  A non-finite amplitude in a control-SET pair meets the
stored zero (0 * Inf = NaN) and poisons its partner, which the phase gate leaves alone: there the two gates differ BY
DEFINITION (test_stored_zero_entries_poison_where_the_phase_gate_does_not pins exactly that difference).  The shared Inf input
therefore puts its Inf into amplitude 0, whose control bit is clear for every (c, q): both gates then run their identity row
over it (Inf stays, the other component becomes NaN).  The Hadamard comparisons, where both sides store four entries, also
take an Inf in the middle of the state."""
import math

import numpy as np
import pytest

import one_qubit_ref as oq
from bitwise import same_with_nans as same

S12 = 0.70710678118654752440          # M_SQRT1_2
H = np.array([[S12, S12], [S12, -S12]], dtype=complex)


def inputs(ob, n):
    """(name, state): two random finite states, one with -0 components (and exact zeros), one with an Inf"""
    out = [("random", ob.random_state(n, 7 + n)), ("random2", ob.random_state(n, 70 + n))]
    z = ob.random_state(n, 17 + n)
    z[0] = -0.0
    z[-1] = -0.0
    z[1::3] = -0.0
    z[2::5] = 0.0
    out.append(("minus zeros", z))
    p = ob.random_state(n, 27 + n)
    p[0] = math.inf                 # amplitude 0: control clear for every (c, q), see the module docstring
    out.append(("one inf", p))
    return out


def inf_inside(ob, n):
    p = ob.random_state(n, 37 + n)
    p[(3 * n) % p.size] = -math.inf
    return ("inf inside", p)


def phase_matrix(ob, theta):
    c, s = ob.polar(theta)
    return np.array([[1.0, 0.0], [0.0, complex(c, s)]], dtype=complex)


THETAS = [math.pi / 2, math.pi / 4, math.pi / 64, -2.3, 0.20966817126512538, math.pi]


@pytest.mark.parametrize("n", range(1, 9))
def test_ref_with_h_entries_is_the_oracles_hadamard(ob, n):
    for name, a in inputs(ob, n) + [inf_inside(ob, n)]:
        for q in range(n):
            want = a.copy(); ob.hadamard(want, n, q)
            same(oq.apply(a, n, q, H), want, f"H n={n} q={q} {name}")


@pytest.mark.parametrize("n", range(2, 9))
def test_ref_controlled_diag_is_the_oracles_cphase(ob, n):
    k = 0
    for name, a in inputs(ob, n):
        for c in range(n):
            for q in range(n):
                if c == q:
                    continue
                theta = THETAS[k % len(THETAS)]; k += 1
                want = a.copy(); ob.cphase(want, n, c, q, theta)
                same(oq.apply(a, n, q, phase_matrix(ob, theta), control=c), want, f"CPHASE n={n} c={c} q={q} {name}")


@pytest.mark.parametrize("n", range(1, 6))
def test_ref_against_the_literal_mat_vec(ob, n):
    """the reference's own algorithm (COO matrix built entry by entry, then the mat-vec over every stored triplet).  The
    phase gate's matrix is taken without explicit zeros (keep_zeros=False: the diagonal alone, which is what the pairwise
    oracle and qcx_c_phase_shift_gate compute on a poisoned state); the Hadamard's has none either way."""
    k = 0
    for name, a in inputs(ob, n) + [inf_inside(ob, n)]:
        lit = ob.LiteralRegister(n, 0, keep_zeros=False)
        try:
            for q in range(n):
                lit.set_state(a); lit.hadamard(q)
                same(oq.apply(a, n, q, H), lit.state().copy(), f"literal H n={n} q={q} {name}")
                if name == "inf inside":
                    continue
                for c in range(n):
                    if c == q:
                        continue
                    theta = THETAS[k % len(THETAS)]; k += 1
                    lit.set_state(a); lit.cphase(c, q, theta)
                    same(oq.apply(a, n, q, phase_matrix(ob, theta), control=c), lit.state().copy(),
                         f"literal CPHASE n={n} c={c} q={q} {name}")
        finally:
            lit.close()


def test_ref_rewrites_every_amplitude_and_leaves_its_input_alone(ob):
    """identity rows: a -0 component of a control-clear amplitude becomes +0, an Inf poisons its amplitude's other component"""
    n = 3
    a = ob.random_state(n, 5)
    a[0] = -0.0                     # index 0: control clear
    a[4] = math.inf                 # index 2 (re): control (qubit 0) clear
    keep = a.copy()
    out = oq.apply(a, n, 1, np.array([[0, 1], [1, 0]], dtype=complex), control=0)
    assert np.array_equal(a.view(np.uint64), keep.view(np.uint64))
    assert out[0] == 0.0 and not np.signbit(out[0])
    assert out[4] == math.inf and np.isnan(out[5])
    # X on the control-set pairs (1, 3) and (5, 7): values swapped (a finite state's products with 1 and 0 change nothing)
    for i0, i1 in ((1, 3), (5, 7)):
        assert out[2 * i0] == a[2 * i1] and out[2 * i0 + 1] == a[2 * i1 + 1]
        assert out[2 * i1] == a[2 * i0] and out[2 * i1 + 1] == a[2 * i0 + 1]


def test_stored_zero_entries_poison_where_the_phase_gate_does_not(ob):
    """the documented difference: an Inf in a control-set pair.  c_phase_shift_gate (diagonal stored alone) leaves the partner
    as it is; the one-qubit gate multiplies its stored zero by the Inf and the partner becomes NaN.  Everything else agrees."""
    n, c, q = 3, 0, 1
    a = ob.random_state(n, 9)
    a[2 * 3] = math.inf             # amplitude 3 = |011>: control set, target set; its partner is amplitude 1
    want = a.copy(); ob.cphase(want, n, c, q, math.pi / 4)
    got = oq.apply(a, n, q, phase_matrix(ob, math.pi / 4), control=c)
    assert np.isfinite(want[2]) and np.isfinite(want[3]) and np.isnan(got[2]) and np.isnan(got[3])
    rest = np.ones(2 << n, dtype=bool); rest[2:4] = False
    same(got[rest], want[rest], "outside the poisoned partner")
