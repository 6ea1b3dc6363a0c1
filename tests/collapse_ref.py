"""qcx_measure_qubits / qcx_postselect_qubits (include/qcx.h), restated in numpy -- this restatement IS the definition: the
probabilities are the pinned tree of tests/marginal_ref.py, the outcome is the reference's scan (qc_shor.c:283-292) applied to
them, and the collapse is two separately rounded products per kept amplitude by s = fl(1 / fl(sqrt(P[outcome]))).  Host only."""
import numpy as np

from marginal_ref import marginal_ref


def choose(P, r):
    """cum = 0; for v = 0 .. len(P) - 2 in order cum = fl(cum + P[v]); the first v with cum >= r, none: len(P) - 1"""
    P = np.asarray(P, dtype=np.float64)
    r = np.float64(r)
    cum = np.float64(0.0)
    with np.errstate(over="ignore", invalid="ignore"):
        for v in range(P.size - 1):
            cum = cum + P[v]
            if cum >= r:
                return v
    return P.size - 1


def running_sums(P):
    """the values `cum` takes in choose(), v = 0 .. len(P) - 2 (an r equal to one of them is a tie: the first v wins)"""
    P = np.asarray(P, dtype=np.float64)
    out, cum = [], np.float64(0.0)
    with np.errstate(over="ignore", invalid="ignore"):
        for v in range(P.size - 1):
            cum = cum + P[v]
            out.append(cum)
    return out


def scale_of(p):
    """s for P[outcome] = p, or None where the state cannot be collapsed (p not a finite number > 0, or s not finite)"""
    p = np.float64(p)
    if not (np.isfinite(p) and p > 0.0):
        return None
    s = np.float64(1.0) / np.sqrt(p)
    return s if np.isfinite(s) else None


def collapse_ref(a, n, first, num, outcome):
    """a: interleaved float64 (re, im) pairs or complex128[2^n].  Returns (P[outcome], a') with a' interleaved float64, or
    (P[outcome], None) in the error case."""
    a = np.asarray(a)
    if a.dtype == np.complex128:
        a = np.ascontiguousarray(a).view(np.float64)
    a = np.ascontiguousarray(a, dtype=np.float64)
    p = marginal_ref(a, n, first, num)[outcome]
    s = scale_of(p)
    if s is None:
        return p, None
    idx = np.arange(1 << n, dtype=np.uint64)
    keep = ((idx >> np.uint64(first)) & np.uint64((1 << num) - 1)) == np.uint64(outcome)
    re, im = a[0::2], a[1::2]
    out = np.zeros_like(a)                                           # every dropped amplitude: (+0, +0)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        out[0::2][keep] = re[keep] * s                               # two separately rounded products, IEEE signs
        out[1::2][keep] = im[keep] * s
    return p, out


def measure_ref(a, n, first, num, r):
    """(outcome, P[outcome], a' or None) of qcx_measure_qubits_r"""
    v = choose(marginal_ref(a, n, first, num), r)
    p, out = collapse_ref(a, n, first, num, v)
    return v, p, out
