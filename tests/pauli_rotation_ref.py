"""qcx_pauli_rotation (include/qcx.h), restated in numpy -- this restatement IS the definition: exp(-i theta/2 P) for the
Pauli string P = (x_mask, z_mask) (tests/pauli_ref.py: Y sits on x_mask & z_mask), applied as the reference's sparse mat-vec
applies every gate (qc_shor.c:393-413): the matrix cos(theta/2) I - i sin(theta/2) P as stored triplets, one or two per row,
accumulated in ascending column order from 0.0, complex products spelled out as qc_shor.c:409 / 412, every product and sum
a separate binary64 rounding (numpy never contracts), components that are exactly zero multiplied out like any other.

    (c, s) = polar(fl(theta / 2))                      ONE sincos, as c_phase_shift_gate obtains its factor
    g      = popcount(x_mask & z_mask) mod 4           <i|P|j> = i^g (-1)^popcount(j & z_mask), j = i ^ x_mask
    (er, ei) = -i * i^g * s = (+0, -s), (s, +0), (+0, s), (-s, +0) for g = 0, 1, 2, 3
    entry(i, j) = (er, ei) with its one non-zero component negated when popcount(j & z_mask) is odd; the other stays +0

x_mask != 0, row i, j = i ^ x_mask:  D = (c, +0) * amp[i], O = entry(i, j) * amp[j],
    new[i] = fl(fl(0.0 + D) + O) if i < j else fl(fl(0.0 + O) + D)                                        (component-wise)
x_mask == 0, row i:  m = (c, -s if popcount(i & z_mask) is even else s),  new[i] = fl(0.0 + m * amp[i])   (component-wise)

EVERY amplitude is rewritten, so a result is never -0, and an Inf or a NaN at index k reaches rows k and k ^ x_mask only.
Host only."""
import ctypes as C
import ctypes.util

import numpy as np

from pauli_ref import _parity, pauli_masks

_libm = None


def polar(theta):
    """(cos, sin) as qcx_polar gives them: one glibc sincos call (tests/test_abi_and_build.py pins that the library, the oracle
    and libm agree)"""
    global _libm
    if _libm is None:
        _libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        _libm.sincos.argtypes = [C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        _libm.sincos.restype = None
    sn, cs = C.c_double(), C.c_double()
    _libm.sincos(float(theta), C.byref(sn), C.byref(cs))
    return 1.0 * cs.value, 1.0 * sn.value


def entry(x_mask, z_mask, s):
    """(g, er, ei): the off-diagonal entry -i * i^g * s before its sign"""
    g = bin(x_mask & z_mask).count("1") % 4
    s, zero = np.float64(s), np.float64(0.0)
    return (g,) + ((zero, -s), (s, zero), (zero, s), (-s, zero))[g]


def _mul(mr, mi, xr, xi):
    """m * x as qc_shor.c:409 / 412"""
    return (mr * xr) - (mi * xi), (mr * xi) + (mi * xr)


_PAR16 = None


def _odd(v):
    """popcount(v) & 1 == 1 of every uint64 in v (pauli_ref._parity with a table for the last 16 bits: the n = 25 cases)"""
    global _PAR16
    if _PAR16 is None:
        _PAR16 = _parity(np.arange(1 << 16, dtype=np.uint64)).astype(bool)
    v = v ^ (v >> np.uint64(32))
    v ^= v >> np.uint64(16)
    return _PAR16[v & np.uint64(0xFFFF)]


def apply_cs(state, n, x_mask, z_mask, c, s):
    """the rotation with cos(theta/2) and sin(theta/2) given.  state: interleaved float64 (re, im) pairs, 2 * 2^n of them.
    Returns the new state (the input is left alone)."""
    a = np.ascontiguousarray(state, dtype=np.float64)
    x_mask, z_mask = pauli_masks((x_mask, z_mask), n)
    assert a.size == 2 << n
    re, im = a[0::2], a[1::2]
    c, zero = np.float64(c), np.float64(0.0)
    g, er, ei = entry(x_mask, z_mask, s)
    i = np.arange(1 << n, dtype=np.uint64)
    j = i ^ np.uint64(x_mask)
    odd = _odd(j & np.uint64(z_mask))
    # the entry at column j: its non-zero component (ei for even g, er for odd g) carries the sign, the other stays +0
    mr = np.where(odd, -er, er) if g & 1 else er
    mi = ei if g & 1 else np.where(odd, -ei, ei)
    out = np.empty_like(a)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        if x_mask == 0:
            pr, pi = _mul(c, mi, re, im)                             # one triplet: (c, -+s)
            out[0::2], out[1::2] = zero + pr, zero + pi
        else:
            dr, di = _mul(c, zero, re, im)
            orr, oi = _mul(mr, mi, re[j], im[j])
            first = i < j                                            # ascending column order: the diagonal first where i < j
            out[0::2] = np.where(first, (zero + dr) + orr, (zero + orr) + dr)
            out[1::2] = np.where(first, (zero + di) + oi, (zero + oi) + di)
    return out


def apply(state, n, x_mask, z_mask, theta):
    """qcx_pauli_rotation(x_mask, z_mask, theta) on `state`"""
    return apply_cs(state, n, x_mask, z_mask, *polar(np.float64(theta) / np.float64(2.0)))


def matrices(letter, c, s):
    """the one-qubit matrix c I - i s P of a single letter, built component by component (what one_qubit_ref.apply is given in
    the cross-checks)"""
    return {"X": np.array([[complex(c, 0.0), complex(0.0, -s)], [complex(0.0, -s), complex(c, 0.0)]]),
            "Y": np.array([[complex(c, 0.0), complex(-s, 0.0)], [complex(s, 0.0), complex(c, 0.0)]]),
            "Z": np.array([[complex(c, -s), 0.0], [0.0, complex(c, s)]])}[letter]


PAULI = {"I": np.eye(2, dtype=complex), "X": np.array([[0, 1], [1, 0]], dtype=complex),
         "Y": np.array([[0, -1j], [1j, 0]]), "Z": np.array([[1, 0], [0, -1]], dtype=complex)}


def matrix2(l0, l1, c, s):
    """c I - i s (l1 (x) l0) as the 4x4 matrix two_qubit_gate(q0, q1, .) takes (index = bit(q0) + 2 * bit(q1)), every entry
    built component by component: P's entries are +-1 and +-i, so -i s P has ONE non-zero component per entry, +-s"""
    p = np.kron(PAULI[l1], PAULI[l0])
    m = np.zeros((4, 4), dtype=complex)
    for r in range(4):
        for k in range(4):
            e = -1j * p[r, k]                                        # one of 0, +-1, +-i: exact
            m[r, k] = complex(e.real * s if e.real else 0.0, e.imag * s if e.imag else 0.0)
        m[r, r] = complex(c, m[r, r].imag) if p[r, r] else complex(c, 0.0)
    return m
