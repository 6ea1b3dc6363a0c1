"""The value of qcx_pauli_expectation (include/qcx.h), restated in numpy -- this restatement IS the definition.  Host only.

A Pauli string over n qubits is two masks: x_mask = the qubits that carry X or Y, z_mask = those that carry Z or Y (Y sits on
x_mask & z_mask).  With g = popcount(x_mask & z_mask) mod 4, a = amp[i] and b = amp[i ^ x_mask], every fl() one binary64
rounding (no FMA):

    t      = g even ? fl(fl(a.re*b.re) + fl(a.im*b.im)) : fl(fl(a.im*b.re) - fl(a.re*b.im))
    odd    = (popcount((i ^ x_mask) & z_mask) + (g >> 1)) & 1
    leaf_i = fl(0.0 + (odd ? -t : t))                  (the 0.0 + makes a zero leaf +0)
    value  = the pairwise tree over ALL n index bits, lowest first: marginal_ref(.., first=0, num=0)'s tree on these leaves

leaf_i is Re(conj(a_i) * <i|P|i ^ x_mask> * b); the imaginary parts cancel between i and i ^ x_mask, and the two leaves of such
a pair are the same bits (tests/test_pauli_ref.py pins that: the GPU's pair shape rests on it)."""
import numpy as np


def pauli_masks(spec, n):
    """(x_mask, z_mask) of a Pauli string over n qubits.  spec: a str such as "XIZY" (character k = qubit k, at most n of them,
    the rest I), a dict {qubit: 'X' | 'Y' | 'Z' | 'I'}, or an (x_mask, z_mask) pair, which is only checked."""
    n = int(n)
    if isinstance(spec, str):
        if len(spec) > n:
            raise ValueError(f"a Pauli string of {len(spec)} characters on {n} qubits")
        items = list(enumerate(spec))
    elif isinstance(spec, dict):
        items = list(spec.items())
    else:
        x, z = (int(v) for v in spec)
        if x < 0 or z < 0 or (x | z) >> n:
            raise ValueError(f"masks ({x:#x}, {z:#x}) do not fit {n} qubits")
        return x, z
    x = z = 0
    for q, p in items:
        if isinstance(q, bool) or int(q) != q or not 0 <= int(q) < n:
            raise ValueError(f"qubit {q!r} is not one of the {n} qubits")
        p = p.upper() if isinstance(p, str) else p
        if p not in ("I", "X", "Y", "Z"):
            raise ValueError(f"{p!r} is not one of I, X, Y, Z")
        if p in ("X", "Y"):
            x |= 1 << int(q)
        if p in ("Z", "Y"):
            z |= 1 << int(q)
    return x, z


def _parity(v):
    """popcount(v) & 1 of every uint64 in v"""
    v = v.copy()
    for s in (32, 16, 8, 4, 2, 1):
        v ^= v >> np.uint64(s)
    return v & np.uint64(1)


def _amps(a):
    a = np.asarray(a)
    if a.dtype != np.complex128:
        a = np.ascontiguousarray(a, dtype=np.float64).view(np.complex128)
    return a


@np.errstate(over="ignore", invalid="ignore", under="ignore")
def pauli_leaves(a, n, x_mask, z_mask):
    """leaf_i for every index i: float64[2^n]"""
    a = _amps(a)
    x_mask, z_mask = pauli_masks((x_mask, z_mask), n)
    assert a.size == 1 << n
    g = bin(x_mask & z_mask).count("1") % 4
    i = np.arange(1 << n, dtype=np.uint64)
    j = i ^ np.uint64(x_mask)
    b = a[j]
    if g % 2 == 0:
        t = a.real * b.real + a.imag * b.imag
    else:
        t = a.imag * b.real - a.real * b.imag
    odd = _parity(j & np.uint64(z_mask)) ^ np.uint64(g >> 1)
    return 0.0 + np.where(odd == 1, -t, t)


@np.errstate(over="ignore", invalid="ignore")
def pauli_ref(a, n, x_mask, z_mask):
    """a: complex128[2^n] (or interleaved float64 re/im pairs), index order"""
    v = pauli_leaves(a, n, x_mask, z_mask)
    while v.size > 1:
        v = v[0::2] + v[1::2]                                        # one level per index bit, lowest first
    return float(v[0])


def pauli_sum_ref(a, n, terms):
    """terms: (coeff, x_mask, z_mask) in order.  (total, values): acc = 0.0; acc = fl(acc + fl(c_k * value_k)) term by term"""
    values = [pauli_ref(a, n, x, z) for _, x, z in terms]
    acc = np.float64(0.0)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for (c, _, _), v in zip(terms, values):
            acc = acc + np.float64(c) * np.float64(v)
    return float(acc), values
