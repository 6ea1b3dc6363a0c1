"""CPU: tests/two_qubit_ref.py -- the numpy restatement that defines qcx_two_qubit_gate / qcx_c_two_qubit_gate -- is pinned to
tests/one_qubit_ref.py (itself pinned to the oracle) by the self-checks the definition admits, and to the oracle's own
Hadamard and controlled phase.  All of them hold bit for bit on finite states without -0: the extra products of an embedded
gate are +-0 and a sum that is not -0 does not change when +-0 is added to it.

  kron(I, U) on (q0, q1)            = one_qubit_gate(q0, U)
  kron(U, I) on (q0, q1)            = one_qubit_gate(q1, U)
  diag(1, 1, 1, e^{i theta})        = c_one_qubit_gate(q0, q1, diag(1, e^{i theta}))  (= the oracle's cphase)
  identity with U in rows / columns {1, 3} = c_one_qubit_gate(q0, q1, U)
  gate(q0, q1, V)                   = gate(q1, q0, P V P),  P = the index swap 1 <-> 2

On a state that holds an Inf the sixteen stored triplets poison the whole quad (0 * Inf = NaN); one case is pinned by hand.
The last test asks the built library for the two entry points: it needs no GPU (a NULL register is refused before anything
touches the device) and fails where the feature is missing."""
import ctypes as C
import math

import numpy as np
import pytest

import one_qubit_ref as oq
import two_qubit_ref as tq
from bitwise import bits, random_unitary, same

S12 = 0.70710678118654752440          # M_SQRT1_2
H = np.array([[S12, S12], [S12, -S12]], dtype=complex)
I2 = np.eye(2, dtype=complex)
P = np.eye(4)[[0, 2, 1, 3]]
BAD_ARGUMENTS = 2


def controlled(U):
    m = np.eye(4, dtype=complex)
    m[np.ix_([1, 3], [1, 3])] = U
    return m


def pairs(n):
    return [(a, b) for a in range(n) for b in range(n) if a != b]


@pytest.fixture(scope="module")
def finite_states(ob):
    """n -> two random finite states and one with exact (+0) zeros; none holds a -0"""
    out = {}
    for n in range(2, 8):
        z = ob.random_state(n, 17 + n)
        z[2::5] = 0.0
        z[0] = 0.0
        out[n] = [("random", ob.random_state(n, 7 + n)), ("random2", ob.random_state(n, 70 + n)), ("zeros", z)]
    return out


@pytest.mark.parametrize("n", range(2, 8))
def test_self_checks_against_the_one_qubit_ref(ob, finite_states, n):
    k = 0
    for name, a in finite_states[n]:
        for q0, q1 in pairs(n):
            k += 1
            U = random_unitary(100 * n + k, 2)
            what = f"n={n} ({q0}, {q1}) {name}"
            same(tq.apply(a, n, q0, q1, np.kron(I2, U)), oq.apply(a, n, q0, U), "kron(I, U) " + what)
            same(tq.apply(a, n, q0, q1, np.kron(U, I2)), oq.apply(a, n, q1, U), "kron(U, I) " + what)
            c, s = ob.polar(math.pi / (1 << (1 + k % 6)))
            D = np.array([[1, 0], [0, complex(c, s)]], dtype=complex)
            same(tq.apply(a, n, q0, q1, np.diag([1, 1, 1, complex(c, s)])), oq.apply(a, n, q1, D, control=q0), "phase diagonal " + what)
            same(tq.apply(a, n, q0, q1, controlled(U)), oq.apply(a, n, q1, U, control=q0), "controlled U " + what)
            V = random_unitary(200 * n + k, 4)
            same(tq.apply(a, n, q0, q1, V), tq.apply(a, n, q1, q0, P @ V @ P), "P V P " + what)


@pytest.mark.parametrize("n", range(3, 8))
def test_controlled_form_is_the_plain_gate_on_the_control_set_half(ob, finite_states, n):
    """... and leaves every other amplitude's bits alone (finite, no -0): checked through the one-qubit ref with two controls
    folded into one (the controlled "U on q1 where q0 reads 1" is U on q1 where c AND q0 read 1)"""
    name, a = finite_states[n][0]
    k = 0
    for c in range(n):
        for q0, q1 in pairs(n):
            if c in (q0, q1):
                continue
            k += 1
            V = random_unitary(300 * n + k, 4)
            got = tq.apply(a, n, q0, q1, V, control=c)
            plain = tq.apply(a, n, q0, q1, V)
            on = np.repeat(((np.arange(1 << n) >> c) & 1) == 1, 2)
            same(got[on], plain[on], f"n={n} c={c} ({q0}, {q1}) control set")
            same(got[~on], a[~on], f"n={n} c={c} ({q0}, {q1}) control clear")


@pytest.mark.parametrize("n", range(2, 7))
def test_ref_gives_the_oracles_hadamard_and_cphase(ob, finite_states, n):
    k = 0
    for name, a in finite_states[n]:
        for q0, q1 in pairs(n):
            k += 1
            what = f"n={n} ({q0}, {q1}) {name}"
            want = a.copy(); ob.hadamard(want, n, q0)
            same(tq.apply(a, n, q0, q1, np.kron(I2, H)), want, "oracle H on qubit0 " + what)
            want = a.copy(); ob.hadamard(want, n, q1)
            same(tq.apply(a, n, q0, q1, np.kron(H, I2)), want, "oracle H on qubit1 " + what)
            theta = [math.pi / 2, math.pi / 4, math.pi / 64, -2.3, 0.20966817126512538, math.pi][k % 6]
            c, s = ob.polar(theta)
            want = a.copy(); ob.cphase(want, n, q0, q1, theta)
            same(tq.apply(a, n, q0, q1, np.diag([1, 1, 1, complex(c, s)])), want, "oracle cphase " + what)


def test_an_inf_poisons_its_quad_as_sixteen_stored_triplets_must(ob):
    """n = 2, the identity matrix, amplitude 0 = (Inf, a): row 0 keeps the Inf (1 * Inf - 0 * a) and its imaginary part meets
    0 * Inf; rows 1 .. 3 multiply their stored zero of column 0 by the Inf in both parts.  Pinned by hand: (Inf, NaN) and six
    NaNs.  With a dense matrix every product with the Inf is +-Inf instead, and a row's imaginary and real parts are +-Inf
    (no NaN unless two infinities of opposite sign meet)."""
    a = ob.random_state(2, 3)
    a[0] = math.inf
    keep = a.copy()
    out = tq.apply(a, 2, 0, 1, np.eye(4))
    assert np.array_equal(bits(a), bits(keep)), "the input is left alone"
    assert out[0] == math.inf and np.isnan(out[1:]).all()
    out = tq.apply(a, 2, 1, 0, np.eye(4))
    assert out[0] == math.inf and np.isnan(out[1:]).all()
    # n = 4, gate on (1, 3): the quad of amplitude 0 is {0, 2, 8, 10}; every other amplitude keeps its bits
    n = 4
    a = ob.random_state(n, 4)
    a[0] = math.inf
    for q0, q1 in ((1, 3), (3, 1)):
        out = tq.apply(a, n, q0, q1, np.eye(4))
        nan = np.isnan(out)
        want = np.zeros(2 << n, dtype=bool)
        for i in (0, 2, 8, 10):
            want[2 * i] = want[2 * i + 1] = True
        want[0] = False
        assert np.array_equal(nan, want) and out[0] == math.inf
        same(out[~want][1:], a[~want][1:], "outside the poisoned quad")
    # the controlled form: amplitude 0 has its control clear, so it takes the identity row alone and its quad stays finite
    out = tq.apply(a, n, 1, 3, np.eye(4), control=0)
    assert out[0] == math.inf and np.isnan(out[1]) and np.isfinite(out[2:]).all()


def test_ref_turns_minus_zero_into_plus_zero_everywhere(ob):
    n = 3
    a = ob.random_state(n, 6)
    a[1::3] = -0.0
    for control in (None, 2):
        out = tq.apply(a, n, 0, 1, np.eye(4), control=control)
        assert not np.any(np.signbit(out) & (out == 0.0))
        same(np.abs(out), np.abs(a) + 0.0, "the identity keeps every value")


def test_null_arguments_are_refused_by_the_library(qc):
    """no GPU needed: the NULL checks come before anything touches a device"""
    lib = qc.lib()
    u = tq.matrix32(np.eye(4))
    up = u.ctypes.data_as(C.c_void_p)
    assert lib.qcx_two_qubit_gate(0, 1, up, None) == BAD_ARGUMENTS
    assert lib.qcx_c_two_qubit_gate(2, 0, 1, up, None) == BAD_ARGUMENTS
    # (the per-shard form is exported too; a NULL amplitude pointer is refused before any launch)
    assert lib.qcx_shard_two_qubit(None, 4, 0, 1, -1, up, None) == BAD_ARGUMENTS
