"""qcx_one_qubit_gate / qcx_c_one_qubit_gate (include/qcx.h), restated in numpy -- this restatement IS the definition: the
2x2 matrix applied as the reference's sparse mat-vec applies every gate (qc_shor.c:393-413), four stored triplets per index
pair taken in column order, every product and sum a separate binary64 rounding (numpy never contracts), entries that are
exactly zero multiplied out like any other.  EVERY amplitude is rewritten, the identity rows of the controlled form included,
so the restatement also says what happens to -0, Inf and NaN.  Host only."""
import numpy as np


def matrix8(U):
    """the 8 doubles of the C ABI from anything numpy.asarray(U, complex) turns into shape (2, 2): row-major (re, im)"""
    m = np.asarray(U, dtype=complex)
    assert m.shape == (2, 2), m.shape
    return np.ascontiguousarray(m.reshape(4)).view(np.float64).copy()


def _row(m0r, m0i, m1r, m1i, ar, ai, br, bi):
    """(0 + m0 * a) + m1 * b with the complex products spelled out as qc_shor.c:409 / 412"""
    zero = np.float64(0.0)
    re = (zero + ((m0r * ar) - (m0i * ai))) + ((m1r * br) - (m1i * bi))
    im = (zero + ((m0r * ai) + (m0i * ar))) + ((m1r * bi) + (m1i * br))
    return re, im


def apply(state, n, q, U, control=None):
    """state: interleaved float64 (re, im) pairs, 2 * 2^n of them.  Returns the new state (the input is left alone).
    U: a (2, 2) complex matrix, or the 8 doubles themselves."""
    a = np.ascontiguousarray(state, dtype=np.float64)
    assert a.size == 2 << n and 0 <= q < n and (control is None or (0 <= control < n and control != q))
    u = np.asarray(U)
    u = np.ascontiguousarray(u, dtype=np.float64) if u.shape == (8,) else matrix8(U)
    u00r, u00i, u01r, u01i, u10r, u10i, u11r, u11i = (np.float64(x) for x in u)
    re, im = a[0::2], a[1::2]
    idx = np.arange(1 << n, dtype=np.uint64)
    i0 = idx[(idx >> np.uint64(q)) & np.uint64(1) == 0]
    i1 = i0 | (np.uint64(1) << np.uint64(q))
    out = np.empty_like(a)
    ore, oim = out[0::2], out[1::2]
    one, zero = np.float64(1.0), np.float64(0.0)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        # the identity row of every amplitude the gate does not act on: 0 + (1 * x - 0 * y), 0 + (1 * y + 0 * x)
        ore[:] = zero + ((one * re) - (zero * im))
        oim[:] = zero + ((one * im) + (zero * re))
        if control is not None:
            on = (i0 >> np.uint64(control)) & np.uint64(1) == 1
            i0, i1 = i0[on], i1[on]
        ar, ai, br, bi = re[i0], im[i0], re[i1], im[i1]
        ore[i0], oim[i0] = _row(u00r, u00i, u01r, u01i, ar, ai, br, bi)
        ore[i1], oim[i1] = _row(u10r, u10i, u11r, u11i, ar, ai, br, bi)
    return out
