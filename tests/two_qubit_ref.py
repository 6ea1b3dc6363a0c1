"""qcx_two_qubit_gate / qcx_c_two_qubit_gate (include/qcx.h), restated in numpy -- this restatement IS the definition: the
4x4 matrix applied as the reference's sparse mat-vec applies every gate (qc_shor.c:393-413), sixteen stored triplets per index
quad taken in ascending state index, every product and sum a separate binary64 rounding (numpy never contracts), entries that
are exactly zero multiplied out like any other.  Matrix index k = bit(qubit0) + 2 * bit(qubit1); with qubit0 above qubit1 the
matrix is first permuted to P u P (P = the index swap 1 <-> 2), so that column k of the sums is the k-th amplitude of the quad
in ascending index order.  EVERY amplitude is rewritten, the identity rows of the controlled form included, so the
restatement also says what happens to -0, Inf and NaN.  Host only."""
import numpy as np

SWAP12 = [0, 2, 1, 3]


def matrix32(U):
    """the 32 doubles of the C ABI from anything numpy.asarray(U, complex) turns into shape (4, 4): row-major (re, im)"""
    m = np.asarray(U, dtype=complex)
    assert m.shape == (4, 4), m.shape
    return np.ascontiguousarray(m.reshape(16)).view(np.float64).copy()


def apply(state, n, q0, q1, U, control=None):
    """state: interleaved float64 (re, im) pairs, 2 * 2^n of them.  Returns the new state (the input is left alone).
    U: a (4, 4) complex matrix, or the 32 doubles themselves."""
    a = np.ascontiguousarray(state, dtype=np.float64)
    assert a.size == 2 << n and 0 <= q0 < n and 0 <= q1 < n and q0 != q1
    assert control is None or (0 <= control < n and control not in (q0, q1))
    u = np.asarray(U)
    u = np.ascontiguousarray(u, dtype=np.float64) if u.shape == (32,) else matrix32(U)
    m = u.reshape(4, 4, 2)
    if q0 > q1:
        m = m[SWAP12][:, SWAP12]                      # P u P
    lo, hi = min(q0, q1), max(q0, q1)
    re, im = a[0::2], a[1::2]
    idx = np.arange(1 << n, dtype=np.uint64)
    lob, hib = np.uint64(1) << np.uint64(lo), np.uint64(1) << np.uint64(hi)
    i0 = idx[(idx & (lob | hib)) == 0]
    out = np.empty_like(a)
    ore, oim = out[0::2], out[1::2]
    one, zero = np.float64(1.0), np.float64(0.0)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        # the identity row of every amplitude the gate does not act on: 0 + (1 * x - 0 * y), 0 + (1 * y + 0 * x)
        ore[:] = zero + ((one * re) - (zero * im))
        oim[:] = zero + ((one * im) + (zero * re))
        if control is not None:
            i0 = i0[(i0 >> np.uint64(control)) & np.uint64(1) == 1]
        quad = [i0, i0 | lob, i0 | hib, i0 | lob | hib]      # ascending state index
        xr = [re[i] for i in quad]
        xi = [im[i] for i in quad]
        for r in range(4):
            sr = np.zeros(i0.size, dtype=np.float64)
            si = np.zeros(i0.size, dtype=np.float64)
            for k in range(4):
                mr, mi = np.float64(m[r, k, 0]), np.float64(m[r, k, 1])
                sr = sr + ((mr * xr[k]) - (mi * xi[k]))      # qc_shor.c:409
                si = si + ((mr * xi[k]) + (mi * xr[k]))      # qc_shor.c:412
            ore[quad[r]], oim[quad[r]] = sr, si
    return out
