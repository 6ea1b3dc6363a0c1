"""The value of qcx_reduced_density_matrix (include/qcx.h), restated in numpy -- this restatement IS the definition.  Host only.

rho[v][w] = sum over r of amp[r, v] * conj(amp[r, w]) for the qubits [first, first + num), r = the other n - num bits.  For
v <= w, with a = amp[r, v], b = amp[r, w] and every fl() one binary64 rounding (no FMA):

    re-leaf = fl(0.0 + fl(fl(a.re*b.re) + fl(a.im*b.im)))          (v == w: the marginal's p_i)
    im-leaf = fl(0.0 + fl(fl(a.im*b.re) - fl(a.re*b.im)))          (v <  w only; a diagonal entry's imaginary part is +0)

and each computed component is marginal_ref's pairwise tree over r: the summed bits below the range, lowest first, then those
above it.  The lower triangle is the conjugate: the same real part, fl(0.0 - im)."""
import numpy as np


@np.errstate(over="ignore", invalid="ignore", under="ignore")
def rdm_ref(a, n, first, num):
    """a: complex128[2^n] (or interleaved float64 re/im pairs), index order.  Returns float64[2^num, 2^num, 2]: (re, im)."""
    a = np.asarray(a)
    if a.dtype != np.complex128:
        a = np.ascontiguousarray(a, dtype=np.float64).view(np.complex128)
    assert a.size == 1 << n and first + num <= n
    x = a.reshape(1 << (n - first - num), 1 << num, 1 << first)     # (hi, range, lo)
    nv = 1 << num
    rho = np.zeros((nv, nv, 2))
    for v in range(nv):
        for w in range(v, nv):
            p, q = x[:, v, :], x[:, w, :]
            comps = [0.0 + (p.real * q.real + p.imag * q.imag)]
            if v < w:
                comps.append(0.0 + (p.imag * q.real - p.real * q.imag))
            for k, t in enumerate(comps):
                while t.shape[1] > 1:
                    t = t[:, 0::2] + t[:, 1::2]                      # low summed bits, ascending
                t = t[:, 0]
                while t.shape[0] > 1:
                    t = t[0::2] + t[1::2]                            # high summed bits, ascending
                rho[v, w, k] = t[0]
            rho[w, v, 0] = rho[v, w, 0]
            if v < w:
                rho[w, v, 1] = 0.0 - rho[v, w, 1]
    return rho


def as_complex(rho):
    """float64[.., .., 2] -> complex128[.., ..]"""
    return np.ascontiguousarray(rho).view(np.complex128)[..., 0]
