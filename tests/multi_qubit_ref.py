"""qcx_mc_multi_qubit_gate (include/qcx.h), restated in numpy -- this restatement IS the definition: a dense 2^k x 2^k matrix,
k = 1 .. 5, on the groups of 2^k amplitudes whose index satisfies (i & ctrl_mask) == ctrl_values, applied as the reference's
sparse mat-vec applies every gate (qc_shor.c:393-413) -- the stored triplets of a row taken in ascending state index, every
product and sum a separate binary64 rounding (numpy never contracts), entries that are exactly zero multiplied out like any
other.  targets[j] is bit j of the matrix index (two_qubit_gate's LSB convention); the matrix is first permuted to m = P u P
so that row and column c of m are the c-th amplitude of a group in ascending state index (the SWAP12 rule of two_qubit_ref.py
for any k).  EVERY amplitude is rewritten: first all of them through the identity row (mc_gate_ref._identity_rows), then the
firing groups through their rows, so the restatement also says what happens to -0, Inf and NaN.  Host only.

Also here, because the CPU tests and the GPU tests both need them: fused_matrix's loop of the small refs, the numpy emulation
of the launch plan, and the seeded stratified draws of (targets, mask, values)."""
import numpy as np

from mc_gate_ref import _check_masks, _identity_rows

MAX_TARGETS = 5


def matrix_doubles(U, k):
    """the 2 * 4^k doubles of the C ABI from a (2^k, 2^k) complex matrix, or those doubles themselves: row-major (re, im)"""
    u = np.asarray(U)
    d = 1 << k
    if u.shape == (2 * d * d,) and u.dtype.kind == "f":
        return np.ascontiguousarray(u, dtype=np.float64)
    m = np.asarray(U, dtype=complex)
    assert m.shape == (d, d), m.shape
    return np.ascontiguousarray(m.reshape(d * d)).view(np.float64).copy()


def ascending_order(targets):
    """asc[c] = the matrix index of the c-th member of a group in ascending state index: bit j of the matrix index is the bit
    of c that stands for targets[j] (its rank among the targets)"""
    t = [int(q) for q in targets]
    rank = [sorted(t).index(q) for q in t]
    return [sum(((c >> rank[j]) & 1) << j for j in range(len(t))) for c in range(1 << len(t))]


def ascending_matrix(targets, U):
    """m = P u P as an array (2^k, 2^k, 2) of doubles"""
    k = len(targets)
    asc = ascending_order(targets)
    return matrix_doubles(U, k).reshape(1 << k, 1 << k, 2)[asc][:, asc]


def apply(state, n, targets, U, ctrl_mask=0, ctrl_values=0):
    """state: interleaved float64 (re, im) pairs, 2 * 2^n of them.  Returns the new state (the input is left alone)."""
    t = tuple(int(q) for q in targets)
    k = len(t)
    assert 1 <= k <= MAX_TARGETS
    a = np.ascontiguousarray(state, dtype=np.float64)
    assert a.size == 2 << n
    cm, cv = _check_masks(n, t, ctrl_mask, ctrl_values)
    m = ascending_matrix(t, U)
    re, im = a[0::2], a[1::2]
    idx = np.arange(1 << n, dtype=np.uint64)
    tmask = np.uint64(sum(1 << q for q in t))
    i0 = idx[((idx & tmask) == 0) & ((idx & cm) == cv)]
    st = sorted(t)
    member = [i0 | np.uint64(sum(((c >> j) & 1) << st[j] for j in range(k))) for c in range(1 << k)]      # ascending state index
    out = np.empty_like(a)
    ore, oim = out[0::2], out[1::2]
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        _identity_rows(re, im, ore, oim)
        xr, xi = [re[i] for i in member], [im[i] for i in member]
        for r in range(1 << k):
            sr, si = np.zeros(i0.size, dtype=np.float64), np.zeros(i0.size, dtype=np.float64)
            for c in range(1 << k):
                mr, mi = np.float64(m[r, c, 0]), np.float64(m[r, c, 1])
                sr = sr + ((mr * xr[c]) - (mi * xi[c]))      # qc_shor.c:409
                si = si + ((mr * xi[c]) + (mi * xr[c]))      # qc_shor.c:412
            ore[member[r]], oim[member[r]] = sr, si
    return out


def dense_operator(n, targets, U, ctrl_mask=0, ctrl_values=0):
    """the 2^n x 2^n complex matrix of the call, built by index arithmetic alone (no rounding: every entry is one of U's or 0 or 1)"""
    t = [int(q) for q in targets]
    k = len(t)
    u = matrix_doubles(U, k).view(np.complex128).reshape(1 << k, 1 << k)
    N = 1 << n
    op = np.zeros((N, N), dtype=complex)
    tm = sum(1 << q for q in t)
    for i in range(N):
        if (i & ctrl_mask) != ctrl_values:
            op[i, i] = 1.0
            continue
        r = sum(((i >> t[j]) & 1) << j for j in range(k))
        for c in range(1 << k):
            op[i, (i & ~tm) | sum(((c >> j) & 1) << t[j] for j in range(k))] = u[r, c]
    return op


def apply_gate_list(state, n, gates):
    """the loop of the small refs over a list in gate_batch's form [(U, targets[, control]), ...]"""
    import mc_gate_ref
    for g in gates:
        U, tg = g[0], tuple(int(q) for q in (g[1] if np.ndim(g[1]) else (g[1],)))
        c = g[2] if len(g) > 2 and g[2] is not None else None
        cm = 0 if c is None else 1 << int(c)
        state = mc_gate_ref.apply(state, n, tg, U, cm, cm)
    return state


def random_unitary(rs, d):
    q, r = np.linalg.qr(rs.standard_normal((d, d)) + 1j * rs.standard_normal((d, d)))
    return q * (np.diag(r) / np.abs(np.diag(r)))


# ---- seeded, stratified draws ----------------------------------------------------------------------------------------------------
def draws(n, count, seed):
    """`count` seeded draws (targets, mask, values) on n qubits, stratified -- the strata are walked round-robin -- over the
    number of targets (1 .. min(5, n)), the class of the targets (all in bits 0-2 where they fit, from bits 3-5, from bit 6
    upwards, anywhere), their order (ascending or shuffled), the number of controls (0, 1, 2, 3, all the others), where the
    controls sit (below bit 3, at or above it, anywhere) and their polarity (all 1, all 0, mixed)."""
    rs = np.random.RandomState(seed)
    strata = [(k, cls, nc, pos, pol) for k in range(1, min(MAX_TARGETS, n) + 1) for cls in ("low", "mid", "high", "any")
              for nc in (0, 1, 2, 3, -1) for pos in ("low", "high", "mixed") for pol in ("pos", "neg", "mixed")]
    order = rs.permutation(len(strata))
    out, j = [], 0
    while len(out) < count:
        k, cls, nc, pos, pol = strata[order[j % len(strata)]]
        j += 1
        pool = {"low": range(0, 3), "mid": range(3, 6), "high": range(6, n), "any": range(n)}[cls]
        pool = [q for q in pool if q < n]
        first = [int(q) for q in rs.permutation(pool)[:k]]                 # as many of the class as it has ...
        rest = [int(q) for q in rs.permutation([q for q in range(n) if q not in first])]
        targets = first + rest[:k - len(first)]                           # ... filled up from the others
        if rs.randint(2):
            targets = sorted(targets)
        free = [q for q in range(n) if q not in targets]
        if nc < 0:
            cs = free
        else:
            head = [q for q in free if (q < 3 if pos == "low" else q >= 3 if pos == "high" else True)]
            pick = [int(q) for q in rs.permutation(head)] + [q for q in free if q not in head]      # (too few there: fill up from the others)
            cs = pick[:min(nc, len(free))]
        mask = sum(1 << c for c in cs)
        vals = mask if pol == "pos" else 0 if pol == "neg" else sum(1 << c for c in cs if rs.randint(2))
        out.append((tuple(targets), mask, vals))
    return out


# ---- the plan's numbering, emulated -------------------------------------------------------------------------------------------------
def deposit(v, mask):
    """v's bits moved, in order, into the set positions of mask; v: uint64 array"""
    v = np.asarray(v, dtype=np.uint64)
    r = np.zeros_like(v)
    j = 0
    for b in range(64):
        if (int(mask) >> b) & 1:
            r |= ((v >> np.uint64(j)) & np.uint64(1)) << np.uint64(b)
            j += 1
    return r


def emulate(plan, U, state, n, targets):
    """What a launch of `plan` (a quantumcomputer_amd.MultiPlan) leaves of `state`, restating k_multi_tile from the plan's
    fields alone: (the new state, the sorted indices it computed rows for, the number of tiles it read, the number it skipped).
    Each tile is staged, its groups -- the elements with every target_pos bit clear, and their 2^k members -- take the rows of
    the ascending matrix where the element predicate holds, and nothing else is written."""
    k = int(plan.num_targets)
    T = int(plan.T)
    m = ascending_matrix(targets, U)
    a = np.ascontiguousarray(state, dtype=np.float64).copy()
    re, im = a[0::2], a[1::2]
    old_re, old_im = re.copy(), im.copy()
    pos = sorted(int(plan.target_pos[j]) for j in range(k))
    emask = sum(1 << p for p in pos)
    e = np.arange(1 << T, dtype=np.uint64)
    e0 = e[(e & np.uint64(emask)) == 0]
    members = [e0 | np.uint64(sum(((c >> j) & 1) << pos[j] for j in range(k))) for c in range(1 << k)]
    off = [deposit(x, plan.tile_mask) for x in members]
    computed, read, skipped = [], 0, 0
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for u in range(int(plan.units)):
            base = int(deposit(np.array([u], dtype=np.uint64), plan.unit_mask)[0]) | int(plan.or_const)
            if (base & int(plan.unit_mask_low)) != int(plan.unit_values_low):
                skipped += 1
                continue
            read += 1
            idx = [np.uint64(base) | o for o in off]
            fires = (idx[0] & np.uint64(plan.elem_mask)) == np.uint64(plan.elem_values)
            idx = [i[fires] for i in idx]
            xr, xi = [old_re[i] for i in idx], [old_im[i] for i in idx]
            for r in range(1 << k):
                sr, si = np.zeros(idx[0].size), np.zeros(idx[0].size)
                for c in range(1 << k):
                    mr, mi = np.float64(m[r, c, 0]), np.float64(m[r, c, 1])
                    sr = sr + ((mr * xr[c]) - (mi * xi[c]))
                    si = si + ((mr * xi[c]) + (mi * xr[c]))
                re[idx[r]], im[idx[r]] = sr, si
                computed.append(idx[r])
    computed = np.sort(np.concatenate(computed)) if computed else np.zeros(0, dtype=np.uint64)
    return a, computed, read, skipped
