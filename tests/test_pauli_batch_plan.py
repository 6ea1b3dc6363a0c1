"""CPU: the pass plan of qcx_pauli_expectation_batch (include/qcx_plan.h: qcx_pauli_batch_plan) against the rule restated in a few
lines of Python, and the facts about the arithmetic that k_pauli_leaves_batch (K14b) rests on, in numpy against the definition
(tests/pauli_ref.py): one tree serves both tiles of a pair, a leaf's "0.0 +" may wait until the tile's root, and the leaves a
partial tile does not have may be zeros of either sign.  No GPU needed."""
import ctypes as C
import math

import numpy as np
import pytest

from bitwise import bits
from pauli_cases import adversarial
from pauli_ref import _parity, pauli_ref


# ---- the plan ---------------------------------------------------------------------------------------------------------------

def plan_rule(xs, width):
    """term k joins the open pass of its x_mask while that holds fewer than width terms, otherwise it opens a new one"""
    open_pass, passes, np_ = {}, [], 0
    for x in xs:
        if x not in open_pass or open_pass[x][1] >= width:
            open_pass[x] = [np_, 0]
            np_ += 1
        open_pass[x][1] += 1
        passes.append(open_pass[x][0])
    return passes, np_


def check_plan(qc, xs, width):
    got, npasses = qc.pauli_batch_plan(xs, width)
    want, want_n = plan_rule(xs, width)
    assert got == want and npasses == want_n
    assert npasses == sum(math.ceil(xs.count(x) / width) for x in set(xs))
    # numbered in opening order: the first term of pass p comes before the first term of pass p + 1, and no number is skipped
    firsts = [got.index(p) for p in range(npasses)]
    assert firsts == sorted(firsts)
    # a pass holds one x_mask and at most width terms
    for p in range(npasses):
        members = [xs[k] for k in range(len(xs)) if got[k] == p]
        assert len(set(members)) == 1 and 1 <= len(members) <= width


def test_width_is_a_build_constant_in_range(qc):
    assert 8 <= qc.pauli_batch_width() <= 64


@pytest.mark.parametrize("width", [1, 2, 3, None], ids=["1", "2", "3", "W"])
def test_plan_follows_the_rule(qc, width):
    W = qc.pauli_batch_width()
    width = W if width is None else width
    check_plan(qc, [], width)
    check_plan(qc, [5], width)
    for run in (W, W + 1, 2 * W + 3):
        check_plan(qc, [7] * run, width)
        check_plan(qc, [7] * run + [0] * run, width)
    # interleaved: the open pass of an x_mask is found again behind other masks, a full one is not reopened
    check_plan(qc, [0, 1, 0, 2, 1, 0, 0, 2, 2, 2, 1, 0] * 7, width)
    check_plan(qc, [k % 3 for k in range(2 * W + 3)] + [1 << 63, 0, 1 << 63], width)
    rs = np.random.RandomState(width)
    for _ in range(20):
        pool = [int(v) for v in rs.randint(0, 1 << 30, rs.randint(1, 6))]
        check_plan(qc, [pool[rs.randint(len(pool))] for _ in range(rs.randint(1, 4 * W))], width)


def test_default_width_is_the_library_s(qc):
    xs = [3] * (qc.pauli_batch_width() + 1)
    assert qc.pauli_batch_plan(xs) == qc.pauli_batch_plan(xs, qc.pauli_batch_width()) == ([0] * (len(xs) - 1) + [1], 2)


def test_plan_arguments(qc):
    lib = qc.lib()
    xs, out, n = (C.c_uint64 * 2)(1, 1), (C.c_ulong * 2)(9, 9), C.c_ulong(9)
    assert lib.qcx_pauli_batch_plan(2, xs, 0, out, C.byref(n)) == 2          # QCX_BAD_ARGUMENTS: width 0
    assert lib.qcx_pauli_batch_plan(2, xs, 4, out, None) == 2
    assert lib.qcx_pauli_batch_plan(2, None, 4, out, C.byref(n)) == 2
    assert lib.qcx_pauli_batch_plan(2, xs, 4, None, C.byref(n)) == 2
    assert list(out) == [9, 9] and n.value == 9
    assert lib.qcx_pauli_batch_plan(0, None, 4, None, C.byref(n)) == 0 and n.value == 0
    assert lib.qcx_pauli_batch_plan(2, xs, 4, out, C.byref(n)) == 0 and list(out) == [0, 0] and n.value == 1


# ---- the arithmetic K14b rests on -------------------------------------------------------------------------------------------

def zero_heavy(n, seed):
    """pauli_cases.adversarial(.., finite=True) with many more exact zeros of both signs: whole runs, single components, and
    every other amplitude -- so that subtrees of the leaves are zeros throughout, of one sign and of both"""
    a = adversarial(n, seed, True)
    rs = np.random.RandomState(seed + 1000)
    k = a.size
    a[rs.randint(0, k, k // 4)] = 0.0
    a[rs.randint(0, k, k // 4)] = -0.0
    for _ in range(3):
        lo = int(rs.randint(0, k)); ln = int(rs.randint(1, max(2, k // 2)))
        a[lo:lo + ln] = rs.choice([0.0, -0.0]) if rs.randint(2) else rs.choice([0.0, -0.0], min(ln, k - lo))
    if seed % 3 == 0:
        a[::4] = -0.0; a[1::4] = 0.0
    return a


def raw_leaves(a, n, x, z):
    """the definition's signed t, WITHOUT its 0.0 +"""
    c = a.view(np.complex128)
    i = np.arange(1 << n, dtype=np.uint64)
    j = i ^ np.uint64(x)
    b = c[j]
    g = bin(x & z).count("1") % 4
    with np.errstate(all="ignore"):
        t = c.real * b.real + c.imag * b.imag if g % 2 == 0 else c.imag * b.real - c.real * b.imag
    odd = _parity(j & np.uint64(z)) ^ np.uint64(g >> 1)
    return np.where(odd == 1, -t, t)


def tree(v):
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(all="ignore"):
        while v.size > 1:
            v = v[0::2] + v[1::2]
    return v[0]


def batch_value(a, n, x, z, T):
    """what K14b and the later stages compute with tiles of 2^T: per tile the tree of the raw signed leaves and 0.0 + its root,
    in the pair shape (x >> T != 0) ONE tree for tile t and tile t ^ xh; then the definition's tree over the tile roots"""
    leaves = raw_leaves(a, n, x, z).reshape(-1, 1 << T)
    xh = x >> T
    roots = np.empty(leaves.shape[0])
    for t in range(leaves.shape[0]):
        if xh and t > (t ^ xh):
            roots[t] = roots[t ^ xh]
        else:
            roots[t] = 0.0 + tree(leaves[t])
    return tree(roots), roots


STRINGS = {3: "all", 5: "all", 8: 400}


def strings_of(n):
    if STRINGS[n] == "all":
        return [(x, z) for x in range(1 << n) for z in range(1 << n)]
    rs = np.random.RandomState(n)
    fixed = [(0, 0), (0, (1 << n) - 1), (1 << (n - 1), 1 << (n - 1)), ((1 << n) - 1, (1 << n) - 1), (1 << (n - 2), 3), (1, 1)]
    return fixed + [(int(rs.randint(0, 1 << n)), int(rs.randint(0, 1 << n))) for _ in range(STRINGS[n])]


@pytest.mark.parametrize("n", [3, 5, 8])
def test_one_tree_per_pair_and_late_canonicalisation(n):
    T = n - 2                                                       # four tiles: pairs whose partner is and is not the neighbour
    roots_checked = 0
    for seed in range(6 if n == 3 else 3):
        a = zero_heavy(n, 10 * n + seed)
        for x, z in strings_of(n):
            want = pauli_ref(a, n, x, z)
            got, roots = batch_value(a, n, x, z, T)
            assert bits(got) == bits(want), (n, seed, x, z)
            # the tile roots themselves are the definition's: canonical leaves, every tile its own tree
            canon = 0.0 + raw_leaves(a, n, x, z).reshape(-1, 1 << T)
            assert np.array_equal(bits(roots), bits(np.array([tree(r) for r in canon]))), (n, seed, x, z)
            roots_checked += roots.size
    assert roots_checked >= 1000


@pytest.mark.parametrize("n", [1, 3, 5, 8])
def test_missing_leaves_of_a_partial_tile_may_be_zeros_of_either_sign(n):
    """K14b runs a register below 12 qubits as one tile of 2^12 leaves; the ones that do not exist are +0 or -0, by the sign
    rule applied to their index"""
    a = zero_heavy(n, 77 + n)
    idx = np.arange(1 << 12, dtype=np.uint64)
    strings = strings_of(n) if n in STRINGS else [(x, z) for x in range(2) for z in range(2)]
    for x, z in strings[:64]:
        g = bin(x & z).count("1") % 4
        pad_sign = _parity((idx ^ np.uint64(x)) & np.uint64(z)) ^ np.uint64(g >> 1)
        leaves = np.where(pad_sign == 1, -0.0, 0.0)
        leaves[:1 << n] = raw_leaves(a, n, x, z)
        assert bits(0.0 + tree(leaves)) == bits(pauli_ref(a, n, x, z)), (n, x, z)
        leaves[1 << n:] = -0.0
        assert bits(0.0 + tree(leaves)) == bits(pauli_ref(a, n, x, z)), (n, x, z)
