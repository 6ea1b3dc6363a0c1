"""qcx_permutation_gate (include/qcx.h), restated in numpy -- this restatement IS the definition: a classical reversible function
|k> -> |perm[k]> on the qubit range [first, first + num) under the controls (ctrl_mask, ctrl_values), applied as the reference's
sparse mat-vec applies every gate (qc_shor.c:393-413).

    perm     = 2^num integers, a bijection of [0, 2^num); qubit `first` is bit 0 of k
    fires(i) = (i & ctrl_mask) == ctrl_values
    k(i)     = (i >> first) & (2^num - 1)
    The operator is the permutation matrix that sends a firing index i to i with its range bits replaced by perm[k(i)], and
    the identity on every other index.  Every row of it, identity rows included, holds ONE stored triplet, (1, 0), which is
    multiplied out and accumulated from 0.0 (qc_shor.c:409 / 412), every product and sum a separate binary64 rounding.  With
    src(row) = row with its range bits replaced by inv[k(row)] where the row fires (a control bit lies outside the range, so
    a row fires exactly when its source does), src(row) = row where it does not, and x = old[src(row)]:
        new.re = fl(0.0 + fl(fl(1.0 * x.re) - fl(0.0 * x.im)))
        new.im = fl(0.0 + fl(fl(1.0 * x.im) + fl(0.0 * x.re)))

On a finite state this is pure movement, except that a -0 component becomes +0 (0.0 + -0.0 = +0.0; 1.0 * x and x - 0.0 keep
every other value).  With an Inf or a NaN in one component of x the product 0.0 * Inf = NaN poisons the other component, in
the rows that move and in the identity rows alike -- what k_strict_mcu does to its identity rows.  Host only."""
import numpy as np


def table(perm, num):
    """perm as 2^num int64 values, checked to be a bijection"""
    p = np.asarray(perm).reshape(-1).astype(np.int64)
    assert p.size == 1 << num, (p.size, num)
    assert np.array_equal(np.sort(p), np.arange(1 << num)), "not a bijection of [0, 2^num)"
    return p


def inverse(perm, num):
    p = table(perm, num)
    inv = np.empty_like(p)
    inv[p] = np.arange(1 << num, dtype=np.int64)
    return inv


def fires(n, ctrl_mask, ctrl_values):
    i = np.arange(1 << n, dtype=np.uint64)
    return (i & np.uint64(ctrl_mask)) == np.uint64(ctrl_values)


def source(n, first, num, perm, ctrl_mask=0, ctrl_values=0):
    """src(row) for every row of an n-qubit register"""
    ctrl_mask, ctrl_values = int(ctrl_mask), int(ctrl_values)
    assert num >= 0 and first >= 0 and first + num <= n
    rng = ((1 << num) - 1) << first
    assert 0 <= ctrl_mask < (1 << n) and ctrl_values & ~ctrl_mask == 0 and ctrl_mask & rng == 0
    inv = inverse(perm, num)
    i = np.arange(1 << n, dtype=np.int64)
    k = (i >> first) & ((1 << num) - 1)
    moved = (i & ~rng) | (inv[k] << first)
    return np.where(fires(n, ctrl_mask, ctrl_values), moved, i)


def apply(state, n, first, num, perm, ctrl_mask=0, ctrl_values=0):
    """state: interleaved float64 (re, im) pairs, 2 * 2^n of them.  Returns the new state (the input is left alone)."""
    a = np.ascontiguousarray(state, dtype=np.float64)
    assert a.size == 2 << n
    src = source(n, first, num, perm, ctrl_mask, ctrl_values)
    xr, xi = a[0::2][src], a[1::2][src]
    one, zero = np.float64(1.0), np.float64(0.0)
    out = np.empty_like(a)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        out[0::2] = zero + ((one * xr) - (zero * xi))
        out[1::2] = zero + ((one * xi) + (zero * xr))
    return out


def dense(n, first, num, perm, ctrl_mask=0, ctrl_values=0):
    """the operator as a 2^n x 2^n matrix: column i holds its 1 in the row i is sent to"""
    p = table(perm, num)
    rng = ((1 << num) - 1) << first
    f = fires(n, ctrl_mask, ctrl_values)
    m = np.zeros((1 << n, 1 << n))
    for i in range(1 << n):
        row = (i & ~rng) | (int(p[(i >> first) & ((1 << num) - 1)]) << first) if f[i] else i
        m[row, i] = 1.0
    return m


# ---- the numpy emulation of qcx_permutation_plan's walk (the CPU plan test and the GPU tests both use it) ------------------------
def deposit(v, mask):
    """v's bits moved, in order, into the set positions of mask (v: a numpy int64 array or an int)"""
    v = np.asarray(v, dtype=np.int64)
    out = np.zeros_like(v)
    j = 0
    for b in range(64):
        if (int(mask) >> b) & 1:
            out |= ((v >> j) & 1) << b
            j += 1
    return out


def control_placements(n, first, num):
    """(mask, values) of every single control of either polarity outside the range"""
    return [(1 << c, v << c) for c in range(n) if not first <= c < first + num for v in (1, 0)]
