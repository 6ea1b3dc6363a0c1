"""qcx_diagonal_gate (include/qcx.h), restated in numpy -- this restatement IS the definition: a diagonal operator on the qubit
range [first, first + num) whose entries come from a table, applied as the reference's sparse mat-vec applies every gate
(qc_shor.c:393-413): one stored triplet per row, accumulated from 0.0, the complex product spelled out as qc_shor.c:409 / 412,
every product and sum a separate binary64 rounding (numpy never contracts), components that are exactly zero multiplied out
like any other.

    d      = 2 * 2^num doubles, (re, im) pairs; entry k belongs to the amplitudes whose bits first .. first+num-1 read k,
             qubit `first` being bit 0 of k
    k(i)   = (i >> first) & (2^num - 1)
    m = d[k(i)], x = amp[i]:
        new.re = fl(0.0 + fl(fl(m.re * x.re) - fl(m.im * x.im)))
        new.im = fl(0.0 + fl(fl(m.re * x.im) + fl(m.im * x.re)))

EVERY amplitude is rewritten, so a result is never -0, and an Inf or a NaN stays in its own row.  num = 0 is the global factor
d[0] and still runs.  Host only."""
import numpy as np


def entry_index(n, first, num):
    """k(i) for every index of an n-qubit register"""
    assert num >= 0 and first >= 0 and first + num <= n
    i = np.arange(1 << n, dtype=np.uint64)
    return ((i >> np.uint64(first)) & np.uint64((1 << num) - 1)).astype(np.int64)


def table(d, num):
    """d as the 2 * 2^num doubles of the C ABI, from those doubles themselves or from 2^num complex values"""
    t = np.asarray(d)
    if np.iscomplexobj(t):
        t = np.ascontiguousarray(t.reshape(-1), dtype=np.complex128).view(np.float64)
    t = np.ascontiguousarray(t, dtype=np.float64).reshape(-1)
    assert t.size == 2 << num, (t.size, num)
    return t


def apply(state, n, first, num, d):
    """state: interleaved float64 (re, im) pairs, 2 * 2^n of them.  Returns the new state (the input is left alone)."""
    a = np.ascontiguousarray(state, dtype=np.float64)
    assert a.size == 2 << n
    t = table(d, num)
    k = entry_index(n, first, num)
    mr, mi = t[0::2][k], t[1::2][k]
    xr, xi = a[0::2], a[1::2]
    zero = np.float64(0.0)
    out = np.empty_like(a)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        out[0::2] = zero + ((mr * xr) - (mi * xi))
        out[1::2] = zero + ((mr * xi) + (mi * xr))
    return out


def dense(n, first, num, d):
    """the operator as a 2^n x 2^n matrix"""
    t = table(d, num).view(np.complex128)
    return np.diag(t[entry_index(n, first, num)])
