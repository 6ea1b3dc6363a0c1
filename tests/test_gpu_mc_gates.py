"""GPU: qcx_mc_one_qubit_gate / qcx_mc_two_qubit_gate (K17, DESIGN s4.5m) -- a one- or two-qubit gate under any set of control
qubits of either polarity -- against tests/mc_gate_ref.py, the numpy restatement that defines them, and against the existing
calls they generalise.  Every comparison is one of uint64 views: no tolerance anywhere.  (On a poisoned state a NaN must sit
exactly where the ref has one; the sign and payload of a NaN are the hardware's business, as in test_gpu_nonfinite.py.)"""
import ctypes as C
import math

import numpy as np
import pytest

import mc_gate_ref as mc
import one_qubit_ref as oq
import two_qubit_ref as tq
from bitwise import minus_zero_state, random_unitary, same, same_with_nans

pytestmark = pytest.mark.gpu

BAD_ARGUMENTS, BAD_QUBIT, UNSUPPORTED = 2, 6, 7
NAMES1 = ["X", "Y", "Z", "S", "T", "H"]
NAMES2 = ["SWAP", "ISWAP", "CNOT", "CZ"]


@pytest.fixture(scope="module")
def states(ob):
    """the inputs shared by the tests, computed once: n -> (fill_random state (seed n), written state with -0)"""
    return {n: (ob.fill_random(n, n), minus_zero_state(ob, n, 40 + n)) for n in list(range(1, 6)) + [9, 10, 12, 13]}


def mask_of(controls):
    """{qubit: value} -> (mask, values)"""
    return sum(1 << c for c in controls), sum(1 << c for c, v in controls.items() if v)


def apply_gate(qc, reg, t, U, m, v):
    if len(t) == 1:
        qc.mc_one_qubit_gate(m, t[0], U, reg, values=v)
    else:
        qc.mc_two_qubit_gate(m, t[0], t[1], U, reg, values=v)


def check_forms(qc, reg, n, st, forms, what, seed0=0, named=True):
    filled, written = st
    for k, (t, m, v) in enumerate(forms):
        U = random_unitary(seed0 + 1000 * n + k, 2 * len(t))
        reg.fill_random(n)
        apply_gate(qc, reg, t, U, m, v)
        same(reg.read(), mc.apply(filled, n, t, U, m, v), f"{what} n={n} targets={t} mask={m:#x} values={v:#x} unitary, fill_random")
        if named:
            name = NAMES1[k % len(NAMES1)] if len(t) == 1 else NAMES2[k % len(NAMES2)]
            G = qc.GATES[name] if len(t) == 1 else qc.GATES2[name]
            reg.write(written)
            apply_gate(qc, reg, t, G, m, v)
            same(reg.read(), mc.apply(written, n, t, G, m, v), f"{what} n={n} targets={t} mask={m:#x} values={v:#x} {name}, written state")


# ---- 6. exhaustive small registers ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", range(1, 6))
def test_small_registers_every_form(qc, states, n):
    """every (mask, values, target) and every ordered (q0, q1) with every (mask, values): 547 + 668 forms over n = 1 .. 5, each on
    the fill_random state with a seeded unitary and on a written state with -0 with a named gate"""
    with qc.Register(n, 0) as reg:
        check_forms(qc, reg, n, states[n], mc.forms1(n) + mc.forms2(n), "small")


# ---- 7. line forms and their edges ---------------------------------------------------------------------------------------------

def named_cases(n):
    """the cases a .. o (written for n = 10: 9 stands for the top qubit n - 1, 8 for n - 2), and two more at the true boundary of
    the shuffle form: p, exactly 64 work items (one whole wave), q, 32 (the small-count fallback)"""
    T, S = n - 1, n - 2
    others = lambda *t: {c: 1 for c in range(n) if c not in t}
    return {
        "a": ((0,), {1: 1, 2: 1}),
        "b": ((1,), {0: 0, 5: 1, T: 1}),
        "c": ((2,), {c: 1 for c in range(3, n)}),
        "d": ((2,), {c: 1 for c in range(4, n)}),
        "e": ((7,), {0: 1, 1: 1, 2: 1}),
        "f": ((7,), {2: 0}),
        "g": ((T,), {c: 1 for c in [0] + list(range(3, T))}),
        "h": ((5,), {c: (j & 1) for j, c in enumerate(c for c in range(n) if c != 5)}),
        "i": ((3,), {4: 1, 5: 1}),
        "j": ((6,), {S: 0, T: 0}),
        "k": ((0, 1), {2: 1}),
        "l": ((1, S), {0: 1, 2: 0, T: 1}),
        "m": ((4, T), {3: 1, 5: 1, 6: 1}),
        "n": ((0, T), others(0, T)),
        "o": ((T, 0), others(0, T)),
        "p": ((2,), {c: 1 for c in range(6, n)}),
        "q": ((2,), {c: 1 for c in range(5, n)}),
    }


def case_forms(n):
    return [(t,) + mask_of(ctl) for t, ctl in named_cases(n).values()]


def test_named_cases_take_the_forms_they_are_named_for(qc):
    """the plan of the named cases at n = 10 (host code): the shuffle form down to exactly one wave, the fallback below"""
    L = qc._lib
    want = {"a": (L.MC_LINE_SHFL, 1024), "b": (L.MC_LINE_SHFL, 256), "c": (L.MC_PAIR, 4), "d": (L.MC_PAIR, 8), "e": (L.MC_LINE_PAIR, 512),
            "f": (L.MC_LINE_PAIR, 512), "g": (L.MC_PAIR, 4), "h": (L.MC_PAIR, 1), "i": (L.MC_PAIR, 128), "j": (L.MC_PAIR, 128),
            "k": (L.MC_LINES2, 1024), "l": (L.MC_LINES2, 256), "m": (L.MC_QUAD, 32), "n": (L.MC_QUAD, 1), "o": (L.MC_QUAD, 1),
            "p": (L.MC_LINE_SHFL, 64), "q": (L.MC_PAIR, 16)}
    for name, (t, ctl) in named_cases(10).items():
        st, pl = qc.mc_gate_plan(10, *mask_of(ctl), t)
        assert st == 0 and (pl.form, pl.count) == want[name], (name, pl.form, pl.count, pl.kernel)


@pytest.mark.parametrize("n", [9, 10, 12, 13])
def test_line_forms_named_cases_and_draws(qc, states, n):
    """the named cases and 200 seeded draws of the plan tests' generator, under the defaults"""
    with qc.Register(n, 0) as reg:
        check_forms(qc, reg, n, states[n], case_forms(n), "named")
        check_forms(qc, reg, n, states[n], mc.draws(n, 200, 7000 + n), "draw", seed0=50000, named=False)


KNOBS = [dict(mc_generic=1), dict(ph_lines=0), dict(ph_nt=0), dict(u2_nt=0), dict(mc_generic=1, ph_nt=0, u2_nt=0)]


@pytest.mark.parametrize("knobs", KNOBS, ids=[",".join(f"{k}={v}" for k, v in d.items()) for d in KNOBS])
def test_draws_under_the_knobs(qc, states, knobs):
    """the draws at n = 10 again: with no control and one positive control on K17's kernels, with the pair / quad form for every
    draw, and without nontemporal accesses (ph_nt for one target, u2_nt for two)"""
    n = 10
    defaults = {k: qc.lib().qcx_tune_get(k.encode()) for k in ("mc_generic", "ph_lines", "ph_nt", "u2_nt")}
    try:
        qc.tune(**knobs)
        with qc.Register(n, 0) as reg:
            check_forms(qc, reg, n, states[n], mc.draws(n, 200, 7000 + n) + case_forms(n), str(knobs), seed0=50000, named=False)
    finally:
        qc.tune(**defaults)


# ---- 8. old against new ------------------------------------------------------------------------------------------------------------

def test_new_kernels_leave_the_old_kernels_bits(qc):
    """n = 10, mc_generic = 1: every (c, q) of c_one_qubit_gate, every q of one_qubit_gate, a seeded 60 of c_two_qubit_gate's
    (c, q0, q1) and 30 of two_qubit_gate's (q0, q1), each on a twin register; phase(theta) under one positive control against
    c_phase_shift_gate; a Toffoli and a Fredkin against c_two_qubit_gate(CNOT) and c_two_qubit_gate(SWAP)"""
    n = 10
    default = qc.lib().qcx_tune_get(b"mc_generic")
    rs = np.random.RandomState(8)
    triples = [tuple(int(x) for x in rs.choice(n, size=3, replace=False)) for _ in range(60)]
    try:
        qc.tune(mc_generic=1)
        with qc.Register(n, 0) as reg, qc.Register(n, 0) as twin:
            def both(k, new, old, what):
                reg.fill_random(100 + k); twin.fill_random(100 + k)
                new(reg); old(twin)
                same(reg.read(), twin.read(), what)
            k = 0
            for q in range(n):
                U = random_unitary(k, 2); k += 1
                both(k, lambda r: qc.mc_one_qubit_gate(0, q, U, r), lambda r: qc.one_qubit_gate(q, U, r), f"plain q={q}")
                for c in range(n):
                    if c == q:
                        continue
                    U = random_unitary(k, 2); k += 1
                    both(k, lambda r: qc.mc_one_qubit_gate([c], q, U, r), lambda r: qc.c_one_qubit_gate(c, q, U, r), f"c={c} q={q}")
                    theta = math.pi / (1 << (1 + k % 6))
                    both(k, lambda r: qc.mc_one_qubit_gate(1 << c, q, qc.phase(theta), r), lambda r: qc.c_phase_shift_gate(c, q, theta, r),
                         f"phase c={c} q={q}")
            for c, q0, q1 in triples:
                U = random_unitary(k, 4); k += 1
                both(k, lambda r: qc.mc_two_qubit_gate({c}, q0, q1, U, r), lambda r: qc.c_two_qubit_gate(c, q0, q1, U, r), f"c={c} q0={q0} q1={q1}")
            for c, q0, q1 in triples[:30]:
                U = random_unitary(k, 4); k += 1
                both(k, lambda r: qc.mc_two_qubit_gate((), q0, q1, U, r), lambda r: qc.two_qubit_gate(q0, q1, U, r), f"plain q0={q0} q1={q1}")
            X, CNOT, SWAP = qc.GATES["X"], qc.GATES2["CNOT"], qc.GATES2["SWAP"]
            for c0, c1, t in triples[:20] + [(0, 1, 2), (8, 9, 0), (9, 0, 5), (3, 4, 5)]:
                k += 1
                # CNOT: qubit0 controls qubit1
                both(k, lambda r: qc.mc_one_qubit_gate({c0, c1}, t, X, r), lambda r: qc.c_two_qubit_gate(c0, c1, t, CNOT, r), f"Toffoli {c0} {c1} -> {t}")
                both(k, lambda r: qc.mc_two_qubit_gate({c0}, c1, t, SWAP, r), lambda r: qc.c_two_qubit_gate(c0, c1, t, SWAP, r), f"Fredkin {c0}: {c1} {t}")
    finally:
        qc.tune(mc_generic=default)


def test_one_positive_control_is_the_old_launch_by_default(qc, states):
    """mc_generic = 0: no control and one positive control go through one_qubit_gate() / two_qubit_gate() -- the same bits, and
    the refusal carries the new call's name"""
    n = 10
    filled, _ = states[n]
    with qc.Register(n, 0) as reg:
        for t, m in (((0,), 0), ((7,), 1 << 2), ((2, 9), 0), ((9, 2), 1 << 1)):
            U = random_unitary(5, 2 * len(t))
            reg.fill_random(n)
            apply_gate(qc, reg, t, U, m, m)
            same(reg.read(), mc.apply(filled, n, t, U, m, m), f"default route targets={t} mask={m:#x}")
        with pytest.raises(qc.QcxError) as e:
            qc.mc_one_qubit_gate(0, 0, [[2, 0], [0, 1]], reg)
        assert e.value.status == BAD_ARGUMENTS and "mc_one_qubit_gate" in str(e.value) and "component 0" in str(e.value)


# ---- 9. non-finite registers ---------------------------------------------------------------------------------------------------------

def poisoned_states(ob, n):
    big = math.ldexp(1.0, 500)
    out = {}
    for name, vals in (("inf", [math.inf]), ("-inf", [-math.inf]), ("nan", [math.nan]), ("2^500", [big]), ("mixed", [math.inf, math.nan, -big, -math.inf])):
        a = ob.random_state(n, 90 + n + len(name))
        where = [1, 2 * 37, 2 * (1 << (n - 1)) + 5, (2 << n) - 2]           # components: index 0, 37, 2^(n-1) + 2, 2^n - 1
        for j, w in enumerate(where):
            a[w] = vals[j % len(vals)]
        a[9] = -0.0
        out[name] = a
    return out


@pytest.mark.parametrize("n", [9, 11])
def test_non_finite_registers_take_the_strict_pass(qc, ob, n):
    """Inf, -Inf, NaN, a component of 2^500 and a mix, through six masks each (one with a low control, one all-negative): every
    amplitude is rewritten, the identity rows multiplied out (0 * Inf = NaN).  The library has no accessor for the register's
    non-finite flag, so that it stays set is checked through behaviour: a second gate under the same mask and a hadamard_gate
    behind it must match the definitions that rewrite EVERY amplitude -- a pass that left the amplitudes outside the mask alone
    would keep an (Inf, y) there where the strict pass makes it (Inf, NaN).  The six masks run on K17's kernels (mc_generic = 1,
    the mask-free one too); the routed cases -- no control, and one positive control with one and with two targets -- run once more at the default 0,
    through two_qubit_gate()'s plain kernel and the strict twins of c_one_qubit_gate() and c_two_qubit_gate()."""
    T = n - 1
    masks = [((3,), {5: 1, T: 1}), ((T,), {0: 1, 4: 0}), ((0,), {c: 0 for c in range(1, n)}), ((1, T), {2: 1, 6: 0}),
             ((6, 2), {0: 0, 1: 0, 7: 0}), ((4, 5), {})]
    routed = [((4, 5), {}), ((3,), {T: 1}), ((T, 0), {1: 1})]
    default = qc.lib().qcx_tune_get(b"mc_generic")
    assert default == 0
    try:
        for name, a in poisoned_states(ob, n).items():
            for generic, (t, ctl) in [(1, m) for m in masks] + [(0, m) for m in routed]:
                qc.tune(mc_generic=generic)
                m, v = mask_of(ctl)
                U = random_unitary(n + len(name), 2 * len(t))
                with qc.Register(n, 0) as reg:
                    reg.write(a)
                    apply_gate(qc, reg, t, U, m, v)
                    w = mc.apply(a, n, t, U, m, v)
                    same_with_nans(reg.read(), w, f"{name} n={n} targets={t} mask={m:#x} values={v:#x}")
                    G = qc.GATES["X"] if len(t) == 1 else qc.GATES2["CNOT"]
                    apply_gate(qc, reg, t, G, m, v)
                    w = mc.apply(w, n, t, G, m, v)
                    same_with_nans(reg.read(), w, "a second gate on the poisoned register")
                    qc.hadamard_gate(2, reg); ob.hadamard(w, n, 2)
                    same_with_nans(reg.read(), w, "hadamard_gate stays strict")
    finally:
        qc.tune(mc_generic=default)


# ---- 10. fusion modes and lazy forms ---------------------------------------------------------------------------------------------------

def queue_some_gates(qc, reg, n, M):
    for l in range(n - 1, M - 1, -1):
        qc.hadamard_gate(l, reg)
        for k in range(l - 1, max(M - 1, l - 4), -1):
            qc.c_phase_shift_gate(l, k, math.pi / (1 << (l - k)), reg)


def lazy_masks(n):
    T = n - 1
    return [((1,), {0: 0, 5: 1, T: 1}), ((T,), {3: 1, 4: 0}), ((2, T - 1), {0: 1, T: 0, 6: 1})]


@pytest.mark.parametrize("mode", [-1, 0, 1, 2])
def test_lands_in_issue_order_behind_queued_gates(qc, ob, mode):
    """the expected state: what the register holds in this mode before the new gate (read on a first run), then the ref; the
    fusion statistics move by what the flush alone moves them"""
    n, M = 10, 3
    for t, ctl in lazy_masks(n):
        m, v = mask_of(ctl)
        U = random_unitary(n + len(t), 2 * len(t))
        with qc.Register(n - M, M) as reg:
            reg.set_fusion(mode)
            reg.fill_random(8)
            queue_some_gates(qc, reg, n, M)
            s0 = reg.fusion_stats()
            base = reg.read()
            flush_counts = tuple(x - y for x, y in zip(reg.fusion_stats(), s0))
            reg.fill_random(8)
            queue_some_gates(qc, reg, n, M)
            before = reg.fusion_stats()
            apply_gate(qc, reg, t, U, m, v)                       # flushes the queue, then its own kernel
            assert tuple(x - y for x, y in zip(reg.fusion_stats(), before)) == flush_counts, "nothing is counted for the new gate"
            want = mc.apply(base, n, t, U, m, v)
            if mode != 2:
                qc.hadamard_gate(0, reg); ob.hadamard(want, n, 0)          # queued behind it
            same(reg.read(), want, f"mode {mode} targets={t} mask={m:#x} values={v:#x}")


@pytest.mark.parametrize("fusion", [-1, 0, 1, 2])
def test_directly_after_reset_register(qc, ob, fusion):
    """a pending basis state is written first"""
    n = 9
    w = np.zeros(2 << n); ob.reset(w, n)
    for (t, ctl), name in zip(lazy_masks(n) + [((3,), {0: 1, 1: 0})], ("X", "H", "ISWAP", "Y")):
        m, v = mask_of(ctl)
        G = qc.GATES[name] if len(t) == 1 else qc.GATES2[name]
        with qc.Register(n - 4, 4) as reg:
            reg.set_fusion(fusion)
            qc.reset_register(reg)
            apply_gate(qc, reg, t, G, m, v)
            same(reg.read(), mc.apply(w, n, t, G, m, v), f"after reset fusion={fusion} targets={t} mask={m:#x} values={v:#x}")


@pytest.mark.parametrize("L,M", [(7, 5), (15, 5)])
@pytest.mark.parametrize("fusion", [-1, 0, 1, 2])
def test_directly_after_quantum_computation(qc, L, M, fusion):
    """(15, 5): the circuit leaves its result in the compact form, which the call's flush expands.  The expected state is what a
    twin in the same mode reads back, then the ref; the statistics move by what qcx_flush alone moves them on that twin."""
    n, Cn, a = L + M, 21, 2
    with qc.Register(L, M) as twin:
        twin.set_fusion(fusion)
        qc.reset_register(twin); qc.quantum_computation(Cn, a, twin)
        t0 = twin.fusion_stats()
        twin.flush()
        flush_alone = tuple(x - y for x, y in zip(twin.fusion_stats(), t0))
        base = twin.read()
    for t, ctl in lazy_masks(n):
        m, v = mask_of(ctl)
        U = random_unitary(77, 2 * len(t))
        with qc.Register(L, M) as reg:
            reg.set_fusion(fusion)
            qc.reset_register(reg); qc.quantum_computation(Cn, a, reg)
            before = reg.fusion_stats()
            apply_gate(qc, reg, t, U, m, v)
            assert tuple(x - y for x, y in zip(reg.fusion_stats(), before)) == flush_alone
            same(reg.read(), mc.apply(base, n, t, U, m, v), f"after quantum_computation n={n} fusion={fusion} targets={t} mask={m:#x}")


# ---- 11. refusals ------------------------------------------------------------------------------------------------------------------

def test_refusals_on_a_live_register(qc, ob):
    lib = qc.lib()
    n = 10
    g1 = oq.matrix8(random_unitary(1, 2)); p1 = g1.ctypes.data_as(C.c_void_p)
    g2 = tq.matrix32(random_unitary(2, 4)); p2 = g2.ctypes.data_as(C.c_void_p)
    bad1 = g1.copy(); bad1[3] = 1.5
    bad2 = g2.copy(); bad2[31] = math.nan
    one, two = lib.qcx_mc_one_qubit_gate, lib.qcx_mc_two_qubit_gate

    def refused(h):
        assert one(6, 6, 0, None, h) == BAD_ARGUMENTS and two(6, 6, 0, 3, None, h) == BAD_ARGUMENTS
        assert one(6, 6, 0, bad1.ctypes.data_as(C.c_void_p), h) == BAD_ARGUMENTS and "component 3" in lib.qcx_last_error().decode()
        assert two(6, 6, 0, 3, bad2.ctypes.data_as(C.c_void_p), h) == BAD_ARGUMENTS and "component 31" in lib.qcx_last_error().decode()
        assert one(6, 8, 0, p1, h) == BAD_ARGUMENTS and "ctrl_values" in lib.qcx_last_error().decode()
        assert two(6, 1, 0, 3, p2, h) == BAD_ARGUMENTS
        assert one(6, 8, n, bad1.ctypes.data_as(C.c_void_p), h) == BAD_ARGUMENTS, "the matrix comes first"
        assert one(1 << n, 1 << (n + 1), n, p1, h) == BAD_ARGUMENTS, "values outside the mask come before the qubits"
        assert one(6, 6, n, p1, h) == BAD_QUBIT and two(6, 6, 0, n, p2, h) == BAD_QUBIT and two(6, 6, 3, 3, p2, h) == BAD_QUBIT
        assert one(1 << n, 0, 0, p1, h) == BAD_QUBIT and one(1 << 63, 1 << 63, 0, p1, h) == BAD_QUBIT and two(1 << 40, 0, 0, 1, p2, h) == BAD_QUBIT
        assert one(6, 6, 1, p1, h) == BAD_QUBIT and two(6, 6, 0, 2, p2, h) == BAD_QUBIT and two(1, 1, 0, 2, p2, h) == BAD_QUBIT

    assert one(6, 6, 0, p1, None) == BAD_ARGUMENTS and two(6, 6, 0, 3, p2, None) == BAD_ARGUMENTS
    with qc.Register(n, 0) as reg:
        reg.fill_random(2)
        before = reg.read()
        refused(reg._h)
        same(reg.read(), before, "a refused call touches nothing")
        with pytest.raises(ValueError):
            qc.mc_one_qubit_gate([5], 0, np.eye(3), reg)
        with pytest.raises(ValueError):
            qc.mc_two_qubit_gate([5], 0, 1, np.eye(2), reg)
        for controls in ("abc", [64], [-1], 2 ** 64, -1, [1.5], 1.5, None, [True]):
            with pytest.raises(ValueError):
                qc.mc_one_qubit_gate(controls, 0, np.eye(2), reg)
        for values in ({4: 1}, {5: 2}, {5: True}, {5: 0.0}, {5: "1"}, 1 << 4, -1, "1", 1.0):
            with pytest.raises(ValueError):
                qc.mc_one_qubit_gate([5], 0, np.eye(2), reg, values=values)
        same(reg.read(), before, "a malformed argument raises before the C call")
    # the queue is left alone: nothing is flushed by a refused call
    with qc.Register(n - 3, 3) as reg, qc.Register(n - 3, 3) as twin:
        for r in (reg, twin):
            r.set_fusion(1); r.fill_random(4); queue_some_gates(qc, r, n, 3)
        s0 = reg.fusion_stats()
        refused(reg._h)
        assert reg.fusion_stats() == s0, "no flush"
        t0 = twin.fusion_stats()
        twin.flush(); reg.flush()
        assert tuple(x - y for x, y in zip(reg.fusion_stats(), s0)) == tuple(x - y for x, y in zip(twin.fusion_stats(), t0))
        same(reg.read(), twin.read(), "the queued gates ran as if nothing had been asked")
    with qc.Register(13, 0, shards=2, devices=[0, 0]) as sh:                          # two virtual shards on device 0
        sh.fill_random(3)
        before = sh.read()
        assert one(6, 2, 0, p1, sh._h) == UNSUPPORTED and one(0, 0, 0, p1, sh._h) == UNSUPPORTED and one(1 << 12, 1 << 12, 0, p1, sh._h) == UNSUPPORTED
        assert two(6, 2, 0, 3, p2, sh._h) == UNSUPPORTED and two(0, 0, 0, 3, p2, sh._h) == UNSUPPORTED
        assert one(6, 8, 0, p1, sh._h) == BAD_ARGUMENTS and one(6, 6, 13, p1, sh._h) == BAD_QUBIT, "the other checks come first"
        same(sh.read(), before, "sharded register unchanged")


def test_python_controls_and_values(qc, states):
    """the spellings of controls and values name the same gate"""
    n = 10
    filled, _ = states[n]
    U = random_unitary(3, 2)
    want = mc.apply1(filled, n, 4, U, 0b100100010, 0b100000010)
    with qc.Register(n, 0) as reg:
        for controls, values in (([1, 5, 8], {5: 0}), ({8, 5, 1}, 0b100000010), (0b100100010, {1: 1, 5: 0, 8: 1}), (np.array([1, 5, 8]), {5: 0}),
                                 (iter((8, 1, 5)), 0b100000010)):
            reg.fill_random(n)
            qc.mc_one_qubit_gate(controls, 4, U, reg, values=values)
            same(reg.read(), want, f"controls={controls!r} values={values!r}")


# ---- 12. physics -----------------------------------------------------------------------------------------------------------------------

def test_two_grover_iterations(qc, ob):
    """n = 10, one marked index among 2^10: sin(theta) = 2^-5, and after two iterations the marked index is measured with
    probability sin^2(5 theta).  The oracle is Z under n - 1 controls of mixed polarity, the reflection about |0..0> is X Z X under
    n - 1 negative controls between two layers of hadamard_gate.  The GPU equals the numpy run of the same circuit bit for bit
    (compared here once more), so it is allowed what that run deviates from the closed form and nothing of its own: the figure,
    measured on the CPU and recomputed by the test, is 1.04e-16: the numpy run gives 0.024223848595511403, the closed form
    0.0242238485955113 (the marked amplitude 0.15564012527465854 against sin(5 theta) = 0.1556401252746582)."""
    n, marked, t = 10, 0b1011001101, 0
    assert marked >> t & 1
    X, Z = qc.GATES["X"], qc.GATES["Z"]
    omask = ((1 << n) - 1) & ~(1 << t)
    w = np.zeros(2 << n); w[0] = 1.0
    with qc.Register(n, 0) as reg:
        reg.write(w)
        for q in range(n):
            qc.hadamard_gate(q, reg); ob.hadamard(w, n, q)
        for _ in range(2):
            qc.mc_one_qubit_gate(omask, t, Z, reg, values=marked & omask); w = mc.apply1(w, n, t, Z, omask, marked & omask)
            for q in range(n):
                qc.hadamard_gate(q, reg); ob.hadamard(w, n, q)
            qc.one_qubit_gate(t, X, reg); w = oq.apply(w, n, t, X)
            qc.mc_one_qubit_gate(omask, t, Z, reg, values=0); w = mc.apply1(w, n, t, Z, omask, 0)
            qc.one_qubit_gate(t, X, reg); w = oq.apply(w, n, t, X)
            for q in range(n):
                qc.hadamard_gate(q, reg); ob.hadamard(w, n, q)
        got = reg.read()
    same(got, w, "the circuit, against the numpy run")
    closed = math.sin(5 * math.asin(2.0 ** -5)) ** 2
    p_ref = float(w[2 * marked] ** 2 + w[2 * marked + 1] ** 2)
    p_gpu = float(got[2 * marked] ** 2 + got[2 * marked + 1] ** 2)
    allowed = abs(p_ref - closed)
    print(f"Grover: closed form {closed!r}, numpy run {p_ref!r}, deviation {allowed:.3e}")
    assert allowed < 1e-14, "the definition itself is off"
    assert abs(p_gpu - closed) <= allowed
