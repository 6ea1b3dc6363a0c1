"""CPU: the pass plan of qcx_pauli_rotation_batch (include/qcx_plan.h: qcx_pauli_rotation_batch_plan) against the rule restated in
a few lines of Python: a run of consecutive terms shares a pass while there are fewer than `width` of them and their x bits at
and above 8 fit four hot bits; a term with more than four such bits is a pass of its own.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest


def popcount(v):
    return bin(v).count("1")


def plan_rule(xs, n, width):
    """(pass_of_term, [(kind, hot_mask), ...])"""
    nhot = min(4, max(n, 8) - 8)
    pass_of, passes = [], []
    H, count = None, 0                                              # H is None: no pass is open

    def close():
        nonlocal H
        q = 8
        while popcount(H) < nhot:
            if not H >> q & 1:
                H |= 1 << q
            q += 1
        passes.append((0, H))
        H = None

    for x in xs:
        hx = x >> 8 << 8
        if popcount(hx) > 4:
            if H is not None:
                close()
            pass_of.append(len(passes))
            passes.append((1, 0))
            continue
        if H is not None and not (count < width and popcount(H | hx) <= 4):
            close()
        if H is None:
            H, count = 0, 0
        H |= hx
        count += 1
        pass_of.append(len(passes))
    if H is not None:
        close()
    return pass_of, passes


def terms_of(xs):
    return [((x, 0), 0.1) for x in xs]


def check_plan(qc, xs, n, width):
    got_of, got = qc.pauli_rotation_batch_plan(terms_of(xs), n, width)
    want_of, want = plan_rule(xs, n, width)
    assert got_of == want_of and got == want, (n, width, xs)
    # what the kernel relies on, stated without the rule
    assert got_of == sorted(got_of) and set(got_of) == set(range(len(got)))
    nhot = min(4, max(n, 8) - 8)
    for p, (kind, hot) in enumerate(got):
        members = [xs[k] for k in range(len(xs)) if got_of[k] == p]
        if kind == 1:
            assert len(members) == 1 and popcount(members[0] >> 8) > 4 and hot == 0
        else:
            assert 1 <= len(members) <= width
            assert popcount(hot) == nhot and hot & 0xFF == 0 and hot >> n == 0
            assert all((x >> 8 << 8) & ~hot == 0 for x in members)      # every partner stays inside the tile
    return got_of, got


def test_width_is_a_build_constant_in_range(qc):
    assert 8 <= qc.pauli_rotation_batch_width() <= 64


@pytest.mark.parametrize("width", [1, 3, 8, None], ids=["1", "3", "8", "W"])
def test_random_lists(qc, width):
    W = qc.pauli_rotation_batch_width()
    width = W if width is None else width
    rs = np.random.RandomState(width)
    for n in range(1, 35):
        check_plan(qc, [], n, width)
        for _ in range(6):
            xs = []
            for _ in range(int(rs.randint(1, 3 * W))):
                kind = rs.randint(0, 8)
                if kind == 0:
                    x = int(rs.randint(0, 1 << 62)) & ((1 << n) - 1)                    # any mask: wide for a large n
                elif kind < 3:
                    x = int(rs.randint(0, 256)) & ((1 << n) - 1)                        # inside the lowest 8 bits
                else:
                    x = int(rs.randint(0, 256)) & ((1 << n) - 1)
                    for q in rs.randint(8, max(n, 9), rs.randint(1, 4)):                 # one to three high bits, often neighbours
                        if q < n:
                            x |= 1 << int(q)
                xs.append(x)
            check_plan(qc, xs, n, width)


def test_width_splits_a_pass(qc):
    W = qc.pauli_rotation_batch_width()
    for n in (5, 12, 20):
        for run in (W - 1, W, W + 1, 2 * W + 3):
            of, passes = check_plan(qc, [3] * run, n, W)
            assert len(passes) == -(-run // W) and of == [k // W for k in range(run)]
    of, passes = check_plan(qc, [0x100, 0x200, 0x400, 0x800, 0x1000], 20, 4)
    assert of == [0, 0, 0, 0, 1] and passes == [(0, 0xF00), (0, 0x1700)]      # closed by the width; the fifth bit opens a tile of its own


def test_fifth_hot_bit_closes_the_pass(qc):
    n = 16
    xs = [0x8000, 0x0900, 0x2000, 0x2801, 0x00FF, 0x0400, 0x0001]
    of, passes = check_plan(qc, xs, n, 32)
    assert of == [0, 0, 0, 0, 0, 1, 1]
    assert passes == [(0, 0xA900), (0, 0x0400 | 0x0100 | 0x0200 | 0x0800)]
    # Z letters never count: only x_mask reaches the plan (the z_mask of a term is whatever)
    assert qc.pauli_rotation_batch_plan([((0x100, 0xFF00), 0.1), ((0x200, 0xF000), 0.2)], n) == ([0, 0], [(0, 0xF00)])


def test_wide_term_in_the_middle(qc):
    n = 20
    xs = [0x100, 0x3, 0x1F00, 0x200, 0xFFFFF, 0x3E000, 0x7]
    of, passes = check_plan(qc, xs, n, 32)
    assert of == [0, 0, 1, 2, 3, 4, 5]
    assert passes == [(0, 0x0F00), (1, 0), (0, 0x0F00), (1, 0), (1, 0), (0, 0x0F00)]
    # four bits at and above 8 are not wide, whatever sits below
    assert check_plan(qc, [0xF0FF, 0xF000], n, 32)[1] == [(0, 0xF000)]


def test_padding_of_the_hot_set(qc):
    assert check_plan(qc, [0], 30, 32)[1] == [(0, 0xF00)]
    assert check_plan(qc, [1 << 29], 30, 32)[1] == [(0, (1 << 29) | 0x700)]
    assert check_plan(qc, [0x300, 1 << 20], 30, 32)[1] == [(0, (1 << 20) | 0x700)]
    assert check_plan(qc, [0x200 | 1 << 12], 13, 32)[1] == [(0, 0x1200 | 0x100 | 0x400)]
    assert check_plan(qc, [0x1E00], 13, 32)[1] == [(0, 0x1E00)]


@pytest.mark.parametrize("n", range(1, 13))
def test_up_to_12_qubits_the_tile_is_the_register(qc, n):
    W = qc.pauli_rotation_batch_width()
    rs = np.random.RandomState(n)
    xs = [int(v) for v in rs.randint(0, 1 << n, 2 * W + 5)] + [(1 << n) - 1]
    of, passes = check_plan(qc, xs, n, W)
    whole = ((1 << n) - 1) >> 8 << 8
    assert passes == [(0, whole)] * len(passes) and len(passes) == -(-len(xs) // W)     # no term is wide, only W splits passes
    assert of == [k // W for k in range(len(xs))]


def heisenberg_step(n):
    """bond by bond: XX, YY, ZZ on (q, q + 1)"""
    out = []
    for q in range(n - 1):
        both = 3 << q
        out += [((both, 0), 0.1), ((both, both), 0.1), ((0, both), 0.1)]
    return out


def ising_step(n):
    """the ZZ layer, then X on every qubit"""
    return [((0, 3 << q), 0.1) for q in range(n - 1)] + [((1 << q, 0), 0.2) for q in range(n)]


def test_trotter_steps_at_30_qubits(qc):
    n = 30
    assert qc.pauli_rotation_batch_width() == 32, "the counts below are those of W = 32"
    W = qc.pauli_rotation_batch_width()
    h, i = heisenberg_step(n), ising_step(n)
    assert (len(h), len(i)) == (87, 59)
    for terms, want in ((h, 7), (i, 7)):
        of, passes = qc.pauli_rotation_batch_plan(terms, n, W)
        assert len(passes) == want and all(kind == 0 for kind, _ in passes)
        assert (of, passes) == plan_rule([p[0] for p, _ in terms], n, W) == qc.pauli_rotation_batch_plan(terms, n)


def test_pauli_forms(qc):
    terms = [("XIZY", 0.1), ({9: "Y", 2: "Z"}, 0.2), ((1 << 13, 5), 0.3)]
    assert qc.pauli_rotation_batch_plan(terms, 14) == ([0, 0, 0], [(0, 0x2700)])
    with pytest.raises(ValueError):
        qc.pauli_rotation_batch_plan([((1 << 14, 0), 0.1)], 14)


def test_plan_arguments(qc):
    lib = qc.lib()
    xs, of, n = (C.c_uint64 * 2)(1, 1 << 9), (C.c_ulong * 2)(9, 9), C.c_ulong(9)
    kind, hot = (C.c_uint * 2)(9, 9), (C.c_uint64 * 2)(9, 9)
    plan = lib.qcx_pauli_rotation_batch_plan
    assert plan(10, 2, xs, 0, of, C.byref(n), kind, hot) == 2          # QCX_BAD_ARGUMENTS: width 0
    assert plan(0, 2, xs, 4, of, C.byref(n), kind, hot) == 2           # no qubits
    assert plan(41, 2, xs, 4, of, C.byref(n), kind, hot) == 2
    assert plan(10, 2, xs, 4, of, None, kind, hot) == 2
    assert plan(10, 2, None, 4, of, C.byref(n), kind, hot) == 2
    assert plan(10, 2, xs, 4, None, C.byref(n), kind, hot) == 2
    assert plan(10, 2, xs, 4, of, C.byref(n), None, hot) == 2
    assert plan(10, 2, xs, 4, of, C.byref(n), kind, None) == 2
    assert plan(9, 2, xs, 4, of, C.byref(n), kind, hot) == 6           # QCX_BAD_QUBIT: bit 9 of 9 qubits
    assert list(of) == [9, 9] and n.value == 9 and list(kind) == [9, 9] and list(hot) == [9, 9]
    assert plan(10, 0, None, 4, None, C.byref(n), None, None) == 0 and n.value == 0
    assert plan(10, 2, xs, 4, of, C.byref(n), kind, hot) == 0
    assert list(of) == [0, 0] and n.value == 1 and kind[0] == 0 and hot[0] == 0x300
