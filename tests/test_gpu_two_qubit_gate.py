"""GPU: qcx_two_qubit_gate / qcx_c_two_qubit_gate (K13, DESIGN s4.5g) against tests/two_qubit_ref.py, the numpy restatement
that defines them, and against the existing pinned kernels.  Every comparison is one of uint64 views: no tolerance anywhere.
(On a poisoned state a NaN must sit exactly where the ref has one; the sign and payload of a NaN are the hardware's business,
as in test_gpu_nonfinite.py.)"""
import ctypes as C
import math

import numpy as np
import pytest

import one_qubit_ref as oq
import two_qubit_ref as tq
from bitwise import bits, minus_zero_state, random_unitary, same, same_with_nans
from collapse_ref import collapse_ref
from marginal_ref import marginal_ref

pytestmark = pytest.mark.gpu

BAD_ARGUMENTS, BAD_QUBIT, UNSUPPORTED = 2, 6, 7
KNOBS = ("u2_variant", "u2_nt", "u2_streams_log2")


NAMES = ["SWAP", "ISWAP", "CNOT", "CZ"]


@pytest.fixture(scope="module")
def states(ob):
    """the inputs of the small-register tests, computed once: n -> (fill_random state (seed n), written state with -0)"""
    return {n: (ob.fill_random(n, n), minus_zero_state(ob, n, 40 + n)) for n in list(range(2, 11)) + [12, 13]}


def ordered(qubits, k):
    """every ordered k-tuple of distinct qubits"""
    out = [()]
    for _ in range(k):
        out = [t + (q,) for t in out for q in qubits if q not in t]
    return out


def cases(n):
    """(c, q0, q1) with c = None for the plain gate: the smallest set that reaches every form (see the issue's list: the single
    quad, partial tiles, the lo 2|3 and hi 5|6 boundaries, controls on both sides of bit 3, streams and several tiles)"""
    if n <= 10:
        out = [(None,) + t for t in ordered(range(n), 2)]
        if 3 <= n <= 7:
            out += ordered(range(n), 3)
        elif n >= 9:
            out += ordered(sorted({0, 2, 3, 5, 6, n - 1}), 3)
        return out
    return [(None,) + t for t in ordered(sorted({0, 1, 2, 3, 5, 6, 7, 11, n - 1}), 2)]


def apply_gate(qc, reg, c, q0, q1, U):
    if c is None:
        qc.two_qubit_gate(q0, q1, U, reg)
    else:
        qc.c_two_qubit_gate(c, q0, q1, U, reg)


def check_forms(qc, reg, n, st, what):
    filled, written = st
    for k, (c, q0, q1) in enumerate(cases(n)):
        U = random_unitary(1000 * n + k, 4)
        reg.fill_random(n)
        apply_gate(qc, reg, c, q0, q1, U)
        same(reg.read(), tq.apply(filled, n, q0, q1, U, control=c), f"{what} n={n} c={c} ({q0}, {q1}) unitary, fill_random")
        name = NAMES[k % len(NAMES)]
        reg.write(written)
        apply_gate(qc, reg, c, q0, q1, qc.GATES2[name])
        same(reg.read(), tq.apply(written, n, q0, q1, qc.GATES2[name], control=c), f"{what} n={n} c={c} ({q0}, {q1}) {name}, written state")


# ---- 1. small registers, every form ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", list(range(2, 11)) + [12, 13])
def test_small_registers_every_form(qc, states, n):
    with qc.Register(n, 0) as reg:
        check_forms(qc, reg, n, states[n], "auto")


# ---- 2. forced forms ---------------------------------------------------------------------------------------------------------

FORCED = [dict(u2_variant=1), dict(u2_variant=1, u2_nt=0, u2_streams_log2=0), dict(u2_streams_log2=3)]


@pytest.mark.parametrize("variant", FORCED, ids=[",".join(f"{k}={v}" for k, v in d.items()) for d in FORCED])
def test_forced_kernel_forms(qc, states, variant):
    defaults = {k: qc.lib().qcx_tune_get(k.encode()) for k in KNOBS}
    try:
        qc.tune(**variant)
        for n in (10, 12):
            with qc.Register(n, 0) as reg:
                check_forms(qc, reg, n, states[n], str(variant))
    finally:
        qc.tune(**defaults)


# ---- 3. self-checks against the existing gates -------------------------------------------------------------------------------

def test_embedded_one_qubit_gates_give_the_pinned_kernels_bits(qc):
    n = 10
    I2 = np.eye(2)
    with qc.Register(n, 0) as reg, qc.Register(n, 0) as twin:
        for k, (q0, q1) in enumerate(ordered(range(n), 2)):
            U = random_unitary(k, 2)
            theta = math.pi / (1 << (1 + k % 6))
            for what, M, run in (
                    ("kron(I, U)", np.kron(I2, U), lambda: qc.one_qubit_gate(q0, U, twin)),
                    ("kron(U, I)", np.kron(U, I2), lambda: qc.one_qubit_gate(q1, U, twin)),
                    ("kron(I, H)", np.kron(I2, qc.GATES["H"]), lambda: qc.hadamard_gate(q0, twin)),
                    ("controlled(U)", qc.controlled(U), lambda: qc.c_one_qubit_gate(q0, q1, U, twin)),
                    ("phase diagonal", np.diag([1, 1, 1, complex(*qc.polar(theta))]), lambda: qc.c_phase_shift_gate(q0, q1, theta, twin))):
                reg.fill_random(5); twin.fill_random(5)
                qc.two_qubit_gate(q0, q1, M, reg)
                run()
                same(reg.read(), twin.read(), f"{what} on ({q0}, {q1})")


def swap_bits(i, a, b):
    d = ((i >> a) ^ (i >> b)) & 1
    return i ^ (d << a) ^ (d << b)


def test_swap_toffoli_and_fredkin_are_exact_permutations(qc, ob):
    n = 10
    a = ob.fill_random(n, 4).reshape(-1, 2)
    idx = np.arange(1 << n)
    X = qc.GATES["X"]
    with qc.Register(n, 0) as reg:
        for q0, q1 in ((0, 1), (2, 7), (9, 3), (6, 5)):
            reg.fill_random(4)
            qc.two_qubit_gate(q0, q1, qc.GATES2["SWAP"], reg)
            same(reg.read(), a[swap_bits(idx, q0, q1)].reshape(-1), f"SWAP ({q0}, {q1})")
        for c, q0, q1 in ((0, 1, 2), (9, 4, 0), (3, 8, 6), (5, 2, 9)):
            reg.fill_random(4)
            qc.c_two_qubit_gate(c, q0, q1, qc.controlled(X), reg)
            both = ((idx >> c) & (idx >> q0) & 1) == 1
            same(reg.read(), a[np.where(both, idx ^ (1 << q1), idx)].reshape(-1), f"Toffoli controls ({c}, {q0}) target {q1}")
            reg.fill_random(4)
            qc.c_two_qubit_gate(c, q0, q1, qc.GATES2["SWAP"], reg)
            on = ((idx >> c) & 1) == 1
            same(reg.read(), a[np.where(on, swap_bits(idx, q0, q1), idx)].reshape(-1), f"Fredkin control {c} on ({q0}, {q1})")


def test_named_gates_are_the_exact_matrices(qc):
    G = qc.GATES2
    assert sorted(G) == sorted(NAMES)
    assert np.array_equal(G["SWAP"], [[1, 0, 0, 0], [0, 0, 1, 0], [0, 1, 0, 0], [0, 0, 0, 1]])
    assert np.array_equal(G["ISWAP"], [[1, 0, 0, 0], [0, 0, 1j, 0], [0, 1j, 0, 0], [0, 0, 0, 1]])
    assert np.array_equal(G["CNOT"], [[1, 0, 0, 0], [0, 0, 0, 1], [0, 0, 1, 0], [0, 1, 0, 0]])
    assert np.array_equal(G["CZ"], np.diag([1, 1, 1, -1]))
    U = random_unitary(1, 2)
    assert np.array_equal(qc.controlled(U), [[1, 0, 0, 0], [0, U[0, 0], 0, U[0, 1]], [0, 0, 1, 0], [0, U[1, 0], 0, U[1, 1]]])
    assert np.array_equal(qc.controlled(qc.GATES["X"]), G["CNOT"])
    with qc.Register(3, 0) as reg:
        for bad in (np.eye(2), np.eye(3), np.zeros(16), np.zeros((2, 16))):
            with pytest.raises(ValueError):
                qc.two_qubit_gate(0, 1, bad, reg)
            with pytest.raises(ValueError):
                qc.c_two_qubit_gate(2, 0, 1, bad, reg)
        V = random_unitary(2, 4)
        reg.fill_random(1); qc.two_qubit_gate(2, 0, V, reg); first = reg.read()
        reg.fill_random(1); qc.two_qubit_gate(2, 0, tq.matrix32(V), reg)          # the 32 doubles themselves
        same(reg.read(), first, "32 doubles")


# ---- 4. fusion modes and lazy forms ------------------------------------------------------------------------------------------

def queue_some_gates(qc, reg, n, M):
    for l in range(n - 1, M - 1, -1):
        qc.hadamard_gate(l, reg)
        for k in range(l - 1, max(M - 1, l - 4), -1):
            qc.c_phase_shift_gate(l, k, math.pi / (1 << (l - k)), reg)


@pytest.mark.parametrize("n", [9, 12])
@pytest.mark.parametrize("mode", [1, 2])
def test_lands_in_issue_order_behind_queued_gates(qc, ob, n, mode):
    """the expected state: what the register holds in this mode before the new gate (read on a first run: in mode 2 that is
    the tolerance mode's own result), then the ref; in mode 1 that reading is also the oracle's, bit for bit"""
    M = 3
    U = random_unitary(n, 4)
    for c, q0, q1 in ((None, 1, n - 2), (None, n - 1, 4), (n - 1, 0, 6), (2, n - 1, 5), (5, 6, 7)):
        with qc.Register(n - M, M) as reg:
            reg.set_fusion(mode)
            reg.fill_random(8)
            queue_some_gates(qc, reg, n, M)
            s0 = reg.fusion_stats()
            base = reg.read()
            flush_counts = tuple(x - y for x, y in zip(reg.fusion_stats(), s0))
            if mode == 1:
                w = ob.fill_random(n, 8)
                for l in range(n - 1, M - 1, -1):
                    ob.hadamard(w, n, l)
                    for k in range(l - 1, max(M - 1, l - 4), -1):
                        ob.cphase(w, n, l, k, math.pi / (1 << (l - k)))
                same(base, w, "queued gates, mode 1")
            reg.fill_random(8)
            queue_some_gates(qc, reg, n, M)
            before = reg.fusion_stats()
            apply_gate(qc, reg, c, q0, q1, U)                  # flushes the queue, then its own kernel
            after = reg.fusion_stats()
            assert tuple(x - y for x, y in zip(after, before)) == flush_counts, "the flush counts what it counted alone: nothing for the new gate"
            want = tq.apply(base, n, q0, q1, U, control=c)
            if mode == 1:
                qc.hadamard_gate(0, reg); ob.hadamard(want, n, 0)          # queued behind it
            same(reg.read(), want, f"mode {mode} n={n} c={c} ({q0}, {q1})")


@pytest.mark.parametrize("n", [9, 12])
@pytest.mark.parametrize("fusion", [-1, 0, 1, 2])
def test_directly_after_reset_register(qc, ob, n, fusion):
    """a pending basis state is written first"""
    w = np.zeros(2 << n); ob.reset(w, n)
    H2 = np.kron(qc.GATES["H"], qc.GATES["H"])
    for c, q0, q1, name, G in ((None, 0, 1, "H x H", H2), (None, n - 1, 0, "CNOT", qc.GATES2["CNOT"]), (0, n - 1, 3, "ISWAP", qc.GATES2["ISWAP"]), (3, 1, 0, "H x H", H2)):
        with qc.Register(n - 4, 4) as reg:
            reg.set_fusion(fusion)
            qc.reset_register(reg)
            apply_gate(qc, reg, c, q0, q1, G)
            same(reg.read(), tq.apply(w, n, q0, q1, G, control=c), f"after reset n={n} fusion={fusion} c={c} ({q0}, {q1}) {name}")


def test_directly_after_quantum_computation(qc, ob):
    """the circuit's result (compact where the circuit leaves it so, which the call's flush expands), then the gate.  The new
    gate adds nothing to the fusion statistics: they move by exactly what qcx_flush alone moves them on a twin register"""
    L, M, Cn, a = 7, 5, 21, 2
    n = L + M
    want = np.zeros(2 << n); ob.reset(want, n); ob.quantum_computation(want, n, M, Cn, a)
    U = random_unitary(77, 4)
    with qc.Register(L, M) as twin:
        qc.reset_register(twin); qc.quantum_computation(Cn, a, twin)
        t0 = twin.fusion_stats()
        twin.flush()
        flush_alone = tuple(x - y for x, y in zip(twin.fusion_stats(), t0))
    for c, q0, q1 in ((None, M + 1, 1), (n - 1, 2, M)):
        with qc.Register(L, M) as reg:
            qc.reset_register(reg); qc.quantum_computation(Cn, a, reg)
            before = reg.fusion_stats()
            apply_gate(qc, reg, c, q0, q1, U)
            assert tuple(x - y for x, y in zip(reg.fusion_stats(), before)) == flush_alone
            same(reg.read(), tq.apply(want, n, q0, q1, U, control=c), f"after quantum_computation c={c} ({q0}, {q1})")


def test_after_postselect_and_seen_by_what_follows(qc, ob):
    n = 9
    a = ob.fill_random(n, 3)
    U = random_unitary(5 * n, 4)
    for c, q0, q1 in ((None, 2, 7), (1, n - 1, 4), (n - 1, 4, 0)):
        with qc.Register(n - 3, 3) as reg:
            reg.fill_random(3)
            p, w = collapse_ref(a, n, 1, 2, 3)
            assert bits(reg.postselect(1, 2, 3))[0] == bits(p)[0]
            apply_gate(qc, reg, c, q0, q1, U)                  # (the collapsed state may hold -0: canonicalised first)
            w = tq.apply(w, n, q0, q1, U, control=c)
            same(reg.read(), w, f"after postselect c={c} ({q0}, {q1})")
            same(reg.marginal(0, 4), marginal_ref(w, n, 0, 4), "marginal sees the new state")
            qc.hadamard_gate(q0, reg); ob.hadamard(w, n, q0)
            same(reg.read(), w, "hadamard_gate behind it")
            apply_gate(qc, reg, c, q1, q0, qc.GATES2["ISWAP"]); w = tq.apply(w, n, q1, q0, qc.GATES2["ISWAP"], control=c)
            r = 0.6 * float(marginal_ref(w, n, 0, 0)[0])
            assert qc.measure_state(reg, r) == ob.measure(w, n, r), "measure_state sees the new state"
            same(reg.read(), w, "collapsed state")


# ---- 5. non-finite states ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("poison", [math.inf, math.nan], ids=["inf", "nan"])
def test_non_finite_states_take_the_strict_pass(qc, ob, poison):
    """the identity rows of the controlled form are multiplied out too (0 * Inf = NaN), the plain forms rewrite every amplitude
    from all sixteen products as they stand, and the register stays strict"""
    n = 9
    U = random_unitary(3, 4)
    for where in (0, 2 * 21 + 1, 2 * 511):                     # component index: controls clear / mixed / every control set
        for c, q0, q1 in ((None, 0, 1), (None, 8, 2), (None, 4, 7), (0, 3, 1), (4, 1, 8), (8, 0, 5), (6, 7, 3)):
            a = ob.random_state(n, 50 + where)
            a[where] = poison
            a[9] = -0.0
            with qc.Register(n, 0) as reg:
                reg.write(a)
                apply_gate(qc, reg, c, q0, q1, U)
                w = tq.apply(a, n, q0, q1, U, control=c)
                same_with_nans(reg.read(), w, f"{poison} at {where}, c={c} ({q0}, {q1})")
                apply_gate(qc, reg, c, q0, q1, qc.GATES2["CNOT"])
                w = tq.apply(w, n, q0, q1, qc.GATES2["CNOT"], control=c)
                same_with_nans(reg.read(), w, "a second gate on the poisoned register")
                qc.hadamard_gate(2, reg); ob.hadamard(w, n, 2)
                same_with_nans(reg.read(), w, "hadamard_gate stays strict")


# ---- 6. errors ---------------------------------------------------------------------------------------------------------------

def test_arguments(qc):
    lib = qc.lib()
    n = 8
    good = tq.matrix32(random_unitary(1, 4))
    gp = good.ctypes.data_as(C.c_void_p)

    def with_component(k, v):
        u = good.copy(); u[k] = v
        return u

    with qc.Register(n, 0) as reg:
        reg.fill_random(2)
        before = reg.read()
        assert lib.qcx_two_qubit_gate(0, 1, None, reg._h) == BAD_ARGUMENTS
        assert lib.qcx_c_two_qubit_gate(2, 1, 0, None, reg._h) == BAD_ARGUMENTS
        assert lib.qcx_two_qubit_gate(0, 1, gp, None) == BAD_ARGUMENTS
        assert lib.qcx_c_two_qubit_gate(2, 1, 0, gp, None) == BAD_ARGUMENTS
        for k, v in ((0, math.nan), (31, math.nan), (3, 1.5), (14, -1.5), (26, math.inf), (1, 1.0000000000000002), (17, -1.0000000000000002)):
            u = with_component(k, v)
            assert lib.qcx_two_qubit_gate(2, 5, u.ctypes.data_as(C.c_void_p), reg._h) == BAD_ARGUMENTS, (k, v)
            assert lib.qcx_c_two_qubit_gate(3, 2, 5, u.ctypes.data_as(C.c_void_p), reg._h) == BAD_ARGUMENTS, (k, v)
        for q0, q1 in ((n, 0), (0, n), (3, 3), (0xFFFFFFFF, 1)):
            assert lib.qcx_two_qubit_gate(q0, q1, gp, reg._h) == BAD_QUBIT, (q0, q1)
        for c, q0, q1 in ((n, 0, 1), (0, n, 1), (0, 1, n), (3, 3, 1), (3, 1, 3), (2, 4, 4), (0xFFFFFFFF, 3, 1), (0x80000000, 3, 1)):
            assert lib.qcx_c_two_qubit_gate(c, q0, q1, gp, reg._h) == BAD_QUBIT, (c, q0, q1)
        same(reg.read(), before, "a refused call touches nothing")
        with pytest.raises(qc.QcxError) as e:
            qc.two_qubit_gate(0, 1, np.diag([1, 1, 2, 1]), reg)
        assert e.value.status == BAD_ARGUMENTS and "component 20" in str(e.value)
        same(reg.read(), before, "a refused matrix touches nothing")
        for v in (1.0, -1.0):                                                        # |.| = 1 exactly is allowed
            u = with_component(9, v)
            assert lib.qcx_two_qubit_gate(2, 5, u.ctypes.data_as(C.c_void_p), reg._h) == 0
            assert lib.qcx_c_two_qubit_gate(0, 2, 5, u.ctypes.data_as(C.c_void_p), reg._h) == 0
    with qc.Register(1, 0) as tiny:                                                  # too small to name distinct qubits
        assert lib.qcx_two_qubit_gate(0, 1, gp, tiny._h) == BAD_QUBIT
        assert lib.qcx_two_qubit_gate(0, 0, gp, tiny._h) == BAD_QUBIT
    with qc.Register(2, 0) as tiny:
        assert lib.qcx_c_two_qubit_gate(2, 0, 1, gp, tiny._h) == BAD_QUBIT
        assert lib.qcx_c_two_qubit_gate(1, 0, 1, gp, tiny._h) == BAD_QUBIT
    with qc.Register(13, 0, shards=2, devices=[0, 0]) as sh:                          # two virtual shards on device 0
        sh.fill_random(3)
        before = sh.read()
        assert lib.qcx_two_qubit_gate(2, 12, gp, sh._h) == UNSUPPORTED
        assert lib.qcx_c_two_qubit_gate(12, 2, 0, gp, sh._h) == UNSUPPORTED
        same(sh.read(), before, "sharded register unchanged")


# ---- 7. 64-bit addressing ----------------------------------------------------------------------------------------------------

def test_n29_windows_beyond_4_gib(qc, ob):
    """n = 29: 8 GiB of amplitudes, the upper half starts at byte offset 2^32.  Windows of 2^12 amplitudes and their partner
    windows 2^28 amplitudes away, read before (and checked against the synthetic fill regenerated on the host) and after,
    against the ref applied to the two windows as one 13-qubit state (qubit 28 is its qubit 12)."""
    import torch
    free, _ = torch.cuda.mem_get_info()
    if free < 10 * 2 ** 30:
        pytest.skip(f"needs 10 GiB of free device memory, {free / 2 ** 30:.1f} GiB are free")
    n, W, top = 29, 1 << 12, 1 << 28
    U = random_unitary(29, 4)
    starts = [0, (1 << 27) + 5 * W, top - W]

    def local(q):
        return None if q is None else (12 if q == 28 else q)

    with qc.Register(n, 0) as reg:
        for c, q0, q1 in ((None, 28, 0), (None, 5, 28), (28, 1, 7)):
            reg.fill_random(29)
            before = [(reg.read(s, W), reg.read(s + top, W)) for s in starts]
            apply_gate(qc, reg, c, q0, q1, U)
            for s, (lo, hi) in zip(starts, before):
                same(lo, ob.fill_random(n, 29, s, W), "the fill"); same(hi, ob.fill_random(n, 29, s + top, W), "the fill, upper half")
                want = tq.apply(np.concatenate([lo, hi]), 13, local(q0), local(q1), U, control=local(c))
                same(reg.read(s, W), want[:2 * W], f"c={c} ({q0}, {q1}) window at {s}")
                same(reg.read(s + top, W), want[2 * W:], f"c={c} ({q0}, {q1}) window at 2^28 + {s}")
