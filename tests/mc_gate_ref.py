"""qcx_mc_one_qubit_gate / qcx_mc_two_qubit_gate (include/qcx.h), restated in numpy -- this restatement IS the definition: the
2x2 or 4x4 matrix on the pairs or quads whose index satisfies (i & ctrl_mask) == ctrl_values, applied as the reference's sparse
mat-vec applies every gate (qc_shor.c:393-413) -- the stored triplets of a row taken in ascending state index, every product and
sum a separate binary64 rounding (numpy never contracts), entries that are exactly zero multiplied out like any other; with
qubit0 above qubit1 the 4x4 matrix is first permuted to P u P (P = the index swap 1 <-> 2).  EVERY amplitude is rewritten: first
all of them through the identity row, then the matching pairs or quads through their rows (one_qubit_ref.apply's way), so the
restatement also says what happens to -0, Inf and NaN.  Host only.

Also here, because the CPU tests of the launch plan and the GPU tests both need them: the numpy emulation of the plan's work
numbering (visited), the seeded stratified draws of (mask, values, targets), and the enumeration of every form of a small
register."""
import itertools

import numpy as np

from one_qubit_ref import matrix8
from two_qubit_ref import SWAP12, matrix32


def _identity_rows(re, im, ore, oim):
    one, zero = np.float64(1.0), np.float64(0.0)
    ore[:] = zero + ((one * re) - (zero * im))
    oim[:] = zero + ((one * im) + (zero * re))


def _check_masks(n, targets, ctrl_mask, ctrl_values):
    ctrl_mask, ctrl_values = int(ctrl_mask), int(ctrl_values)
    assert all(0 <= q < n for q in targets) and len(set(targets)) == len(targets)
    assert 0 <= ctrl_mask < (1 << n) and ctrl_values & ~ctrl_mask == 0 and not any((ctrl_mask >> q) & 1 for q in targets)
    return np.uint64(ctrl_mask), np.uint64(ctrl_values)


def apply1(state, n, q, U, ctrl_mask=0, ctrl_values=0):
    """state: interleaved float64 (re, im) pairs, 2 * 2^n of them.  Returns the new state (the input is left alone).
    U: a (2, 2) complex matrix, or the 8 doubles themselves."""
    a = np.ascontiguousarray(state, dtype=np.float64)
    assert a.size == 2 << n
    cm, cv = _check_masks(n, (q,), ctrl_mask, ctrl_values)
    u = np.asarray(U)
    u = np.ascontiguousarray(u, dtype=np.float64) if u.shape == (8,) else matrix8(U)
    m = [[(np.float64(u[4 * r + 2 * k]), np.float64(u[4 * r + 2 * k + 1])) for k in range(2)] for r in range(2)]
    re, im = a[0::2], a[1::2]
    idx = np.arange(1 << n, dtype=np.uint64)
    bit = np.uint64(1) << np.uint64(q)
    i0 = idx[((idx & bit) == 0) & ((idx & cm) == cv)]
    pair = [i0, i0 | bit]
    out = np.empty_like(a)
    ore, oim = out[0::2], out[1::2]
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        _identity_rows(re, im, ore, oim)
        xr, xi = [re[i] for i in pair], [im[i] for i in pair]
        for r in range(2):
            sr, si = np.zeros(i0.size, dtype=np.float64), np.zeros(i0.size, dtype=np.float64)
            for k in range(2):
                mr, mi = m[r][k]
                sr = sr + ((mr * xr[k]) - (mi * xi[k]))      # qc_shor.c:409
                si = si + ((mr * xi[k]) + (mi * xr[k]))      # qc_shor.c:412
            ore[pair[r]], oim[pair[r]] = sr, si
    return out


def apply2(state, n, q0, q1, U, ctrl_mask=0, ctrl_values=0):
    """the same for two targets; U: a (4, 4) complex matrix with index bit(q0) + 2 * bit(q1), or the 32 doubles themselves"""
    a = np.ascontiguousarray(state, dtype=np.float64)
    assert a.size == 2 << n
    cm, cv = _check_masks(n, (q0, q1), ctrl_mask, ctrl_values)
    u = np.asarray(U)
    u = np.ascontiguousarray(u, dtype=np.float64) if u.shape == (32,) else matrix32(U)
    m = u.reshape(4, 4, 2)
    if q0 > q1:
        m = m[SWAP12][:, SWAP12]                      # P u P
    lo, hi = min(q0, q1), max(q0, q1)
    re, im = a[0::2], a[1::2]
    idx = np.arange(1 << n, dtype=np.uint64)
    lob, hib = np.uint64(1) << np.uint64(lo), np.uint64(1) << np.uint64(hi)
    i0 = idx[((idx & (lob | hib)) == 0) & ((idx & cm) == cv)]
    quad = [i0, i0 | lob, i0 | hib, i0 | lob | hib]      # ascending state index
    out = np.empty_like(a)
    ore, oim = out[0::2], out[1::2]
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        _identity_rows(re, im, ore, oim)
        xr, xi = [re[i] for i in quad], [im[i] for i in quad]
        for r in range(4):
            sr, si = np.zeros(i0.size, dtype=np.float64), np.zeros(i0.size, dtype=np.float64)
            for k in range(4):
                mr, mi = np.float64(m[r, k, 0]), np.float64(m[r, k, 1])
                sr = sr + ((mr * xr[k]) - (mi * xi[k]))
                si = si + ((mr * xi[k]) + (mi * xr[k]))
            ore[quad[r]], oim[quad[r]] = sr, si
    return out


def apply(state, n, targets, U, ctrl_mask=0, ctrl_values=0):
    t = tuple(targets)
    return apply1(state, n, t[0], U, ctrl_mask, ctrl_values) if len(t) == 1 else apply2(state, n, t[0], t[1], U, ctrl_mask, ctrl_values)


# ---- every form of a small register -----------------------------------------------------------------------------------------------
def masks_and_values(n, targets):
    """every (mask, values) over the qubits of an n-qubit register that are no target"""
    free = [q for q in range(n) if q not in targets]
    for k in range(len(free) + 1):
        for cs in itertools.combinations(free, k):
            mask = sum(1 << c for c in cs)
            for pol in range(1 << k):
                yield mask, sum(1 << c for j, c in enumerate(cs) if (pol >> j) & 1)


def forms1(n):
    return [((q,), m, v) for q in range(n) for m, v in masks_and_values(n, (q,))]


def forms2(n):
    return [((q0, q1), m, v) for q0 in range(n) for q1 in range(n) if q0 != q1 for m, v in masks_and_values(n, (q0, q1))]


# ---- seeded, stratified draws -----------------------------------------------------------------------------------------------------
def draws(n, count, seed):
    """`count` seeded draws (targets, mask, values) on n >= 9 qubits, stratified -- the strata are walked round-robin -- over
    the number of targets (1, 2), the class of each target (bits 0-2, 3-5, >= 6), the number of controls (1, 2, 3, all the
    others), where the controls sit (below bit 3, at or above it, anywhere) and their polarity (all 1, all 0, mixed)."""
    rs = np.random.RandomState(seed)
    classes = [list(range(0, 3)), list(range(3, 6)), list(range(6, n))]
    tsets = [(a,) for a in range(3)] + [(a, b) for a in range(3) for b in range(3)]
    strata = [(t, k, pos, pol) for t in tsets for k in (1, 2, 3, -1) for pos in ("low", "high", "mixed") for pol in ("pos", "neg", "mixed")]
    out = []
    order = rs.permutation(len(strata))
    j = 0
    while len(out) < count:
        tcls, k, pos, pol = strata[order[j % len(strata)]]
        j += 1
        while True:
            targets = tuple(int(rs.choice(classes[c])) for c in tcls)
            if len(set(targets)) == len(targets):
                break
        free = [q for q in range(n) if q not in targets]
        if k < 0:
            cs = free
        else:
            pool = [q for q in free if (q < 3 if pos == "low" else q >= 3 if pos == "high" else True)]
            if len(pool) < k:           # (fewer than k qubits below bit 3 are left: fill up from the others)
                pool = pool + [q for q in free if q not in pool][:k - len(pool)]
            cs = [int(c) for c in rs.choice(pool, size=k, replace=False)]
        mask = sum(1 << c for c in cs)
        if pol == "pos":
            vals = mask
        elif pol == "neg":
            vals = 0
        else:
            vals = sum(1 << c for c in cs if rs.randint(2))
        out.append((targets, mask, vals))
    return out


# ---- the plan's numbering, emulated ---------------------------------------------------------------------------------------------------
def deposit(p, runs):
    """p's bits moved, in order, into the positions outside the squeezed runs [(pos, len), ...] (ascending); p: uint64 array"""
    i = np.asarray(p, dtype=np.uint64).copy()
    for pos, ln in runs:
        low = (np.uint64(1) << np.uint64(pos)) - np.uint64(1)
        i = ((i & ~low) << np.uint64(ln)) | (i & low)
    return i


def visited(plan, targets):
    """What a launch of `plan` (a quantumcomputer_amd.McPlan) rewrites: (the base indices of its work items, the lanes'
    predicate, the sorted array of every amplitude index that a lane which passes the predicate computes).  Restates K17's
    kernels: a pair / quad form owns the targets that are squeezed out, a shuffled target is part of the numbering."""
    runs = [(int(plan.run_pos[k]), int(plan.run_len[k])) for k in range(plan.nruns)]
    i = deposit(np.arange(int(plan.count), dtype=np.uint64), runs) | np.uint64(plan.or_const)
    hit = (i & np.uint64(plan.low_mask)) == np.uint64(plan.low_values)
    squeezed = 0
    for pos, ln in runs:
        squeezed |= ((1 << ln) - 1) << pos
    own = [q for q in targets if (squeezed >> q) & 1]          # targets in registers: the lane computes all their rows
    idx = [i[hit]]
    for q in own:
        idx = idx + [x | (np.uint64(1) << np.uint64(q)) for x in idx]
    return i, hit, np.sort(np.concatenate(idx))
