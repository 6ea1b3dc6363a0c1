"""Helpers of the bit-exact gate tests (one- and two-qubit gates, Pauli expectation values and rotations): comparisons of
doubles by their bits, and the small inputs these tests share.  A plain module, no test."""
import numpy as np


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(got, want, what=""):
    """bit for bit, a NaN's sign and payload included"""
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, f"{what}: shapes {g.shape} and {w.shape}"
    bad = np.nonzero(g != w)[0]
    assert bad.size == 0, (f"{what}: {bad.size}/{g.size} doubles differ; first at {bad[0]}: got {np.asarray(got)[bad[0]]!r} "
                           f"want {np.asarray(want)[bad[0]]!r}")


def same_with_nans(got, want, what=""):
    """a NaN exactly where the definition has one (its sign and payload are the hardware's business), every other double bit
    for bit; scalars count as arrays of one"""
    got, want = np.atleast_1d(np.ascontiguousarray(got, dtype=np.float64)), np.atleast_1d(np.ascontiguousarray(want, dtype=np.float64))
    assert got.shape == want.shape, f"{what}: shapes {got.shape} and {want.shape}"
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f"{what}: NaN pattern differs at {np.nonzero(gn != wn)[0][:8]}: {got} vs {want}"
    same(got[~gn], want[~wn], what)


def random_unitary(seed, d):
    rs = np.random.RandomState(seed)
    q, r = np.linalg.qr(rs.randn(d, d) + 1j * rs.randn(d, d))
    u = q * (np.diag(r) / np.abs(np.diag(r)))
    return np.clip(u.real, -1.0, 1.0) + 1j * np.clip(u.imag, -1.0, 1.0)       # (rounding may leave a component at 1 + 1 ulp)


def minus_zero_state(ob, n, seed):
    """a state for qcx_state_write with -0 components, exact zeros and cancelling pairs"""
    a = ob.random_state(n, seed)
    a[0] = -0.0
    a[1::7] = -0.0
    a[4::11] = 0.0
    if n >= 2:
        a[6] = -a[2]; a[7] = -a[3]
    return a
