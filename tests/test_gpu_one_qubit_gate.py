"""GPU: qcx_one_qubit_gate / qcx_c_one_qubit_gate (K12, DESIGN s4.5f) against tests/one_qubit_ref.py, the numpy restatement
that defines them.  Every comparison is one of uint64 views: no tolerance anywhere.  (On a poisoned state a NaN must sit
exactly where the ref has one; the sign and payload of a NaN are the hardware's business, as in test_gpu_nonfinite.py.)"""
import ctypes as C
import math

import numpy as np
import pytest

import one_qubit_ref as oq
from bitwise import bits, minus_zero_state, random_unitary, same, same_with_nans
from collapse_ref import collapse_ref, measure_ref
from marginal_ref import marginal_ref

pytestmark = pytest.mark.gpu

BAD_ARGUMENTS, BAD_QUBIT, UNSUPPORTED = 2, 6, 7


NAMES = ["X", "Y", "Z", "S", "T", "H"]


@pytest.fixture(scope="module")
def states(ob):
    """the inputs of the small-register tests, computed once: n -> (fill_random state (seed n), written state with -0)"""
    return {n: (ob.fill_random(n, n), minus_zero_state(ob, n, 40 + n)) for n in list(range(1, 14))}


def forms(n, controlled=True):
    out = [(None, q) for q in range(n)]
    if controlled:
        out += [(c, q) for c in range(n) for q in range(n) if c != q]
    return out


def apply_gate(qc, reg, c, q, U):
    if c is None:
        qc.one_qubit_gate(q, U, reg)
    else:
        qc.c_one_qubit_gate(c, q, U, reg)


def check_forms(qc, reg, n, st, what, controlled=True):
    filled, written = st
    for k, (c, q) in enumerate(forms(n, controlled)):
        U = random_unitary(1000 * n + k, 2)
        reg.fill_random(n)
        apply_gate(qc, reg, c, q, U)
        same(reg.read(), oq.apply(filled, n, q, U, control=c), f"{what} n={n} c={c} q={q} unitary, fill_random")
        G = qc.GATES[NAMES[k % len(NAMES)]]
        reg.write(written)
        apply_gate(qc, reg, c, q, G)
        same(reg.read(), oq.apply(written, n, q, G, control=c), f"{what} n={n} c={c} q={q} {NAMES[k % len(NAMES)]}, written state")


# ---- 1. small registers, every form ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", list(range(1, 11)) + [12, 13])
def test_small_registers_every_form(qc, states, n):
    """n <= 10: every q and every ordered (c, q); 12 and 13: every q.  Reaches the shuffle form (q <= 2 from n = 9), the pair
    form with a partial last tile (n <= 6) and with streams, the whole-line controlled forms (n >= 9) and the squeezed pair form"""
    with qc.Register(n, 0) as reg:
        check_forms(qc, reg, n, states[n], "auto", controlled=n <= 10)


def test_named_gates_are_the_exact_matrices(qc):
    s = 0.70710678118654752440
    c, sn = qc.polar(math.pi / 4)
    G = qc.GATES
    assert sorted(G) == sorted(NAMES)
    assert np.array_equal(G["X"], [[0, 1], [1, 0]]) and np.array_equal(G["Y"], [[0, -1j], [1j, 0]])
    assert np.array_equal(G["Z"], [[1, 0], [0, -1]]) and np.array_equal(G["S"], [[1, 0], [0, 1j]])
    assert np.array_equal(G["H"], [[s, s], [s, -s]]) and np.array_equal(G["T"], [[1, 0], [0, complex(c, sn)]])
    cm, sm = qc.polar(-0.35); cp, sp = qc.polar(0.35)
    assert np.array_equal(qc.rz(0.7), [[complex(cm, sm), 0], [0, complex(cp, sp)]])
    assert np.array_equal(qc.phase(0.7), [[1, 0], [0, complex(*qc.polar(0.7))]])
    with pytest.raises(ValueError):
        with qc.Register(2, 0) as reg:
            qc.one_qubit_gate(0, np.eye(3), reg)


FORCED = [
    dict(h_variant=1, h_ppt=1, h_streams_log2=0), dict(h_variant=1, h_ppt=2, h_streams_log2=3), dict(h_variant=1, h_ppt=1, h_nt=0, h_streams_log2=1),
    dict(h_variant=2, h_wave_r=2, h_streams_log2=2), dict(h_variant=2, h_wave_r=4, h_nt=0, h_streams_log2=0), dict(h_variant=2, h_wave_r=8, h_streams_log2=1),
    dict(ph_lines=0), dict(ph_lines=0, ph_nt=0, ph_streams_log2=0), dict(ph_lines=1, ph_streams_log2=3),
]


@pytest.mark.parametrize("variant", FORCED, ids=[",".join(f"{k}={v}" for k, v in d.items()) for d in FORCED])
def test_forced_kernel_forms(qc, states, variant):
    """every launch form of K12 at n = 10 (and 12, where the wave-tile form with 8 registers per lane applies): pair form for
    every q, wave-tile form with the partner in another lane (q < 6) and in another register (q = 6 .. 8), controlled pair form
    for controls and targets inside a line, with and without nontemporal accesses and streams"""
    keys = ("h_variant", "h_ppt", "h_nt", "h_wave_r", "h_streams_log2", "ph_lines", "ph_nt", "ph_streams_log2")
    defaults = {k: qc.lib().qcx_tune_get(k.encode()) for k in keys}
    try:
        qc.tune(**variant)
        for n in ((10,) if "ph_lines" in variant else (10, 12)):
            with qc.Register(n, 0) as reg:
                check_forms(qc, reg, n, states[n], str(variant), controlled="ph_lines" in variant)
    finally:
        qc.tune(**defaults)


# ---- 2. self-checks against the existing gates -------------------------------------------------------------------------------

def test_h_entries_give_hadamard_gates_bits(qc):
    n = 10
    with qc.Register(n, 0) as reg, qc.Register(n, 0) as twin:
        for q in range(n):
            reg.fill_random(5); twin.fill_random(5)
            qc.one_qubit_gate(q, qc.GATES["H"], reg)
            qc.hadamard_gate(q, twin)
            same(reg.read(), twin.read(), f"H q={q}")


def test_controlled_diagonal_gives_c_phase_shift_gates_bits(qc):
    n = 10
    with qc.Register(n, 0) as reg, qc.Register(n, 0) as twin:
        k = 0
        for c in range(n):
            for q in range(n):
                if c == q:
                    continue
                theta = math.pi / (1 << (1 + k % 6)); k += 1
                reg.fill_random(6); twin.fill_random(6)
                qc.c_one_qubit_gate(c, q, qc.phase(theta), reg)
                qc.c_phase_shift_gate(c, q, theta, twin)
                same(reg.read(), twin.read(), f"phase c={c} q={q} theta=pi/{1 << (1 + (k - 1) % 6)}")


# ---- 3. fusion modes and lazy forms ------------------------------------------------------------------------------------------

def queue_some_gates(qc, reg, n, M):
    for l in range(n - 1, M - 1, -1):
        qc.hadamard_gate(l, reg)
        for k in range(l - 1, max(M - 1, l - 4), -1):
            qc.c_phase_shift_gate(l, k, math.pi / (1 << (l - k)), reg)


@pytest.mark.parametrize("n", [9, 10, 11, 12])
@pytest.mark.parametrize("mode", [1, 2])
def test_lands_in_issue_order_behind_queued_gates(qc, ob, n, mode):
    """the expected state: what the register holds in this mode before the new gate (read on a first run: in mode 2 that is
    the tolerance mode's own result), then the ref; in mode 1 that reading is also the oracle's, bit for bit"""
    M = 3
    U = random_unitary(n, 2)
    for c, q in ((None, 1), (None, n - 2), (n - 1, 0), (2, n - 1), (5, 6)):
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
            apply_gate(qc, reg, c, q, U)                       # flushes the queue, then its own kernel
            after = reg.fusion_stats()
            assert tuple(x - y for x, y in zip(after, before)) == flush_counts, "the flush counts what it counted alone: nothing for the new gate"
            want = oq.apply(base, n, q, U, control=c)
            if mode == 1:
                qc.hadamard_gate(0, reg); ob.hadamard(want, n, 0)          # queued behind it
            same(reg.read(), want, f"mode {mode} n={n} c={c} q={q}")


@pytest.mark.parametrize("n", [9, 12])
@pytest.mark.parametrize("fusion", [-1, 0, 1, 2])
def test_directly_after_reset_register(qc, ob, n, fusion):
    """a pending basis state is written first"""
    w = np.zeros(2 << n); ob.reset(w, n)
    for c, q, name in ((None, 0, "X"), (None, n - 1, "H"), (0, n - 1, "Y"), (3, 1, "X")):
        with qc.Register(n - 4, 4) as reg:
            reg.set_fusion(fusion)
            qc.reset_register(reg)
            apply_gate(qc, reg, c, q, qc.GATES[name])
            same(reg.read(), oq.apply(w, n, q, qc.GATES[name], control=c), f"after reset n={n} fusion={fusion} c={c} q={q}")


def oracle_shor(ob, L, M, Cn, a):
    n = L + M
    w = np.zeros(2 << n); ob.reset(w, n); ob.quantum_computation(w, n, M, Cn, a)
    return w


@pytest.mark.parametrize("L,M", [(7, 5), (15, 5)])
def test_directly_after_quantum_computation(qc, ob, L, M):
    """(15, 5): the circuit leaves its result in the compact form, which the call's flush expands.  The new gate adds nothing to
    the fusion statistics: they move by exactly what qcx_flush alone moves them on a twin register in the same state -- nothing
    at (7, 5); at (15, 5) the compact chain's last pass, which the circuit defers to whoever looks at the state first."""
    n, Cn, a = L + M, 21, 2
    want = oracle_shor(ob, L, M, Cn, a)
    U = random_unitary(77, 2)
    with qc.Register(L, M) as twin:
        qc.reset_register(twin); qc.quantum_computation(Cn, a, twin)
        t0 = twin.fusion_stats()
        twin.flush()
        flush_alone = tuple(x - y for x, y in zip(twin.fusion_stats(), t0))
    if L == 7:
        assert flush_alone == (0, 0)
    for c, q in ((None, M + 1), (n - 1, 2)):
        with qc.Register(L, M) as reg:
            qc.reset_register(reg); qc.quantum_computation(Cn, a, reg)
            before = reg.fusion_stats()
            apply_gate(qc, reg, c, q, U)
            assert tuple(x - y for x, y in zip(reg.fusion_stats(), before)) == flush_alone
            same(reg.read(), oq.apply(want, n, q, U, control=c), f"after quantum_computation n={n} c={c} q={q}")


@pytest.mark.parametrize("n", [9, 11])
def test_after_postselect_and_seen_by_what_follows(qc, ob, n):
    a = ob.fill_random(n, 3)
    U = random_unitary(5 * n, 2)
    for c, q in ((None, 2), (1, n - 1), (n - 1, 4)):
        with qc.Register(n - 3, 3) as reg:
            reg.fill_random(3)
            p, w = collapse_ref(a, n, 1, 2, 3)
            assert bits(reg.postselect(1, 2, 3))[0] == bits(p)[0]
            apply_gate(qc, reg, c, q, U)                       # (the collapsed state may hold -0: canonicalised first)
            w = oq.apply(w, n, q, U, control=c)
            same(reg.read(), w, f"after postselect n={n} c={c} q={q}")
            same(reg.marginal(0, 4), marginal_ref(w, n, 0, 4), "marginal sees the new state")
            rs = [0.0, 0.13, 0.5, 0.77, 0.999, 0.5]
            total = float(marginal_ref(w, n, 0, 0)[0])
            shots = qc.sample_states(reg, [r * total for r in rs])
            assert shots.tolist() == [ob.measure(w.copy(), n, r * total) for r in rs], "sample_states sees the new state"
            qc.hadamard_gate(q, reg); ob.hadamard(w, n, q)
            same(reg.read(), w, "hadamard_gate behind it")
            qc.inverse_QFT(reg); ob.iqft(w, n, 3)
            same(reg.read(), w, "inverse_QFT behind it")
            apply_gate(qc, reg, c, q, qc.GATES["Y"]); w = oq.apply(w, n, q, qc.GATES["Y"], control=c)
            r = 0.6 * float(marginal_ref(w, n, 0, 0)[0])
            assert qc.measure_state(reg, r) == ob.measure(w, n, r), "measure_state sees the new state"
            same(reg.read(), w, "collapsed state")


# ---- 4. measure and reset ----------------------------------------------------------------------------------------------------

def test_measure_one_qubit_then_flip_it_back(qc, ob):
    """measure_qubits on one qubit, X if it read 1: the qubit is |0> again.  Its marginal is then (P, +0) with the second entry
    exactly +0 (every amplitude with the bit set is (+0, +0)) and P the pinned sum of the kept amplitudes (marginal_ref); on the
    basis-derived state -- |1>, H on the qubit, so one amplitude is kept -- P is exactly 1.0."""
    n = 10
    a = ob.fill_random(n, 12)
    X = qc.GATES["X"]
    ones = 0
    with qc.Register(n, 0) as reg:
        for q, r in ((0, 0.2), (0, 0.9), (5, 0.4), (5, 0.95), (9, 0.1), (9, 0.7)):
            reg.fill_random(12)
            v, p, w = measure_ref(a, n, q, 1, r)
            assert reg.measure_qubits(q, 1, r) == (v, float(p))
            if v == 1:
                qc.one_qubit_gate(q, X, reg); w = oq.apply(w, n, q, X)
                ones += 1
            same(reg.read(), w, f"measure-and-reset q={q} r={r}")
            m = reg.marginal(q, 1)
            same(m, marginal_ref(w, n, q, 1))
            assert bits(m)[1] == 0, "the qubit reads 0 with certainty: (+0) for outcome 1"
        assert 0 < ones < 6
        for q, r in ((3, 0.2), (3, 0.8), (7, 0.8)):
            qc.reset_register(reg); qc.hadamard_gate(q, reg)
            b = np.zeros(2 << n); ob.reset(b, n); ob.hadamard(b, n, q)
            v, p, w = measure_ref(b, n, q, 1, r)
            assert reg.measure_qubits(q, 1, r) == (v, float(p))
            if v == 1:
                qc.one_qubit_gate(q, X, reg); w = oq.apply(w, n, q, X)
            same(reg.read(), w)
            assert bits(reg.marginal(q, 1)).tolist() == bits(np.array([1.0, 0.0])).tolist()


# ---- 5. non-finite states ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("poison", [math.inf, math.nan], ids=["inf", "nan"])
def test_non_finite_states_take_the_strict_pass(qc, ob, poison):
    """the identity rows of the controlled form are multiplied out too (0 * Inf = NaN), and the register stays strict"""
    n = 6
    U = random_unitary(3, 2)
    for where in (0, 2 * 21 + 1, 2 * 63):                       # component index: control clear / mixed / control set
        for c, q in ((None, 0), (None, 5), (0, 3), (4, 1), (5, 0)):
            a = ob.random_state(n, 50 + where)
            a[where] = poison
            a[9] = -0.0
            for fusion in (0, 1):
                with qc.Register(n, 0) as reg:
                    reg.set_fusion(fusion)
                    reg.write(a)
                    apply_gate(qc, reg, c, q, U)
                    w = oq.apply(a, n, q, U, control=c)
                    same_with_nans(reg.read(), w, f"{poison} at {where}, c={c} q={q}, fusion {fusion}")
                    apply_gate(qc, reg, c, q, qc.GATES["X"])
                    w = oq.apply(w, n, q, qc.GATES["X"], control=c)
                    same_with_nans(reg.read(), w, "a second gate on the poisoned register")
                    qc.hadamard_gate(2, reg); ob.hadamard(w, n, 2)
                    same_with_nans(reg.read(), w, "hadamard_gate stays strict")


# ---- 6. errors ---------------------------------------------------------------------------------------------------------------

def test_arguments(qc):
    lib = qc.lib()
    n = 8
    good = oq.matrix8(random_unitary(1, 2))
    gp = good.ctypes.data_as(C.c_void_p)

    def with_component(k, v):
        u = good.copy(); u[k] = v
        return u

    with qc.Register(n, 0) as reg:
        reg.fill_random(2)
        before = reg.read()
        assert lib.qcx_one_qubit_gate(0, None, reg._h) == BAD_ARGUMENTS
        assert lib.qcx_c_one_qubit_gate(1, 0, None, reg._h) == BAD_ARGUMENTS
        assert lib.qcx_one_qubit_gate(0, gp, None) == BAD_ARGUMENTS
        assert lib.qcx_c_one_qubit_gate(1, 0, gp, None) == BAD_ARGUMENTS
        for k, v in ((0, math.nan), (7, math.nan), (3, 1.5), (4, -1.5), (6, math.inf), (1, 1.0000000000000002)):
            u = with_component(k, v)
            assert lib.qcx_one_qubit_gate(2, u.ctypes.data_as(C.c_void_p), reg._h) == BAD_ARGUMENTS, (k, v)
            assert lib.qcx_c_one_qubit_gate(3, 2, u.ctypes.data_as(C.c_void_p), reg._h) == BAD_ARGUMENTS, (k, v)
        assert lib.qcx_one_qubit_gate(n, gp, reg._h) == BAD_QUBIT
        assert lib.qcx_c_one_qubit_gate(n, 0, gp, reg._h) == BAD_QUBIT
        assert lib.qcx_c_one_qubit_gate(0, n, gp, reg._h) == BAD_QUBIT
        assert lib.qcx_c_one_qubit_gate(3, 3, gp, reg._h) == BAD_QUBIT
        assert lib.qcx_c_one_qubit_gate(0xFFFFFFFF, 3, gp, reg._h) == BAD_QUBIT
        same(reg.read(), before, "a refused call touches nothing")
        with pytest.raises(qc.QcxError) as e:
            qc.one_qubit_gate(0, [[2, 0], [0, 1]], reg)
        assert e.value.status == BAD_ARGUMENTS and "component 0" in str(e.value)
        u = with_component(0, -1.0)                                                  # |.| = 1 exactly is allowed
        assert lib.qcx_one_qubit_gate(2, u.ctypes.data_as(C.c_void_p), reg._h) == 0
    with qc.Register(13, 0, shards=2, devices=[0, 0]) as sh:                          # two virtual shards on device 0
        sh.fill_random(3)
        before = sh.read()
        assert lib.qcx_one_qubit_gate(2, gp, sh._h) == UNSUPPORTED
        assert lib.qcx_c_one_qubit_gate(12, 2, gp, sh._h) == UNSUPPORTED
        same(sh.read(), before, "sharded register unchanged")


# ---- 7. 64-bit addressing ----------------------------------------------------------------------------------------------------

def test_n29_windows_beyond_4_gib(qc, ob):
    """n = 29: 8 GiB of amplitudes, the upper half starts at byte offset 2^32.  Windows of 2^12 amplitudes and their partner
    windows 2^28 amplitudes away, read before (and checked against the synthetic fill regenerated on the host) and after,
    against the ref applied to the windows alone."""
    import torch
    free, _ = torch.cuda.mem_get_info()
    if free < 10 * 2 ** 30:
        pytest.skip(f"needs 10 GiB of free device memory, {free / 2 ** 30:.1f} GiB are free")
    n, W, top = 29, 1 << 12, 1 << 28
    U = random_unitary(29, 2)
    starts = [0, (1 << 27) + 5 * W, top - W]
    with qc.Register(n, 0) as reg:
        for c, q in ((None, 28), (28, 0), (0, 28)):
            reg.fill_random(29)
            before = [(reg.read(s, W), reg.read(s + top, W)) for s in starts]
            apply_gate(qc, reg, c, q, U)
            for s, (lo, hi) in zip(starts, before):
                same(lo, ob.fill_random(n, 29, s, W), "the fill"); same(hi, ob.fill_random(n, 29, s + top, W), "the fill, upper half")
                if q == 28:                                     # the pair spans the two windows: a 13-qubit state, target 12
                    want = oq.apply(np.concatenate([lo, hi]), 13, 12, U, control=c)
                    wlo, whi = want[:2 * W], want[2 * W:]
                else:                                           # control 28: the lower window stays, the upper one takes U on qubit 0
                    wlo, whi = lo, oq.apply(hi, 12, 0, U)
                same(reg.read(s, W), wlo, f"c={c} q={q} window at {s}")
                same(reg.read(s + top, W), whi, f"c={c} q={q} window at 2^28 + {s}")
