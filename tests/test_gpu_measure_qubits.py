"""GPU: measure or post-select a qubit range and collapse the state (qcx_measure_qubits / qcx_postselect_qubits, K11).  Outcome,
probability and the whole collapsed state must be, bit for bit, what tests/collapse_ref.py defines on whatever the state holds;
an outcome the state cannot be collapsed onto is an error that leaves everything as it was; the lazy forms behave as
include/qcx.h says; and the collapsed state is an ordinary state for every call that follows."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from collapse_ref import choose, collapse_ref, measure_ref, running_sums
from marginal_ref import marginal_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARGUMENTS, BAD_QUBIT, UNSUPPORTED = 2, 6, 7


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(got, want, what=""):
    """bitwise, NaN matching NaN"""
    got, want = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(want, dtype=np.float64).reshape(-1)
    assert got.shape == want.shape, what
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f"{what}: NaN positions differ"
    bad = np.flatnonzero(bits(got[~gn]) != bits(want[~wn]))
    assert bad.size == 0, f"{what}: {bad.size} values differ, first at {bad[:4]}: {got[~gn][bad[:4]]} vs {want[~wn][bad[:4]]}"


def compact_measures(qc, reg):
    v = C.c_ulong(0)
    assert qc.lib().qcx_compact_measure_stats(reg._h, C.byref(v)) == 0
    return int(v.value)


def spread_state(n, seed, nonfinite=False):
    rs = np.random.RandomState(seed)
    a = rs.standard_normal(2 << n) * 2.0 ** rs.randint(-40, 40, 2 << n)
    k = a.size
    m = max(1, k // 16)
    a[rs.randint(0, k, m)] = 5e-324 * rs.randint(1, 1000, m)           # subnormals
    a[rs.randint(0, k, m)] = 0.0
    a[rs.randint(0, k, m)] = -0.0
    if nonfinite:
        a[rs.randint(0, k, max(1, k // 32))] = 1e300                     # |a|^2 overflows to Inf
        a[rs.randint(0, k, max(1, k // 64))] = 1e154
        if n >= 4:
            a[rs.randint(0, k)] = np.inf
            a[rs.randint(0, k)] = np.nan
    return a


def draws(P, rs):
    """<= 0, above the total, NaN, mid-range values, and running sums themselves (ties: the first v wins)"""
    cums = [c for c in running_sums(P) if np.isfinite(c)]
    out = [0.0, -1.0, float("nan"), float("inf")]
    with np.errstate(over="ignore", invalid="ignore"):
        total = cums[-1] + P[-1] if cums else P[-1]
    if np.isfinite(total) and total > 0:
        out += [float(total) * 2.0, float(total) * float(rs.uniform(0.05, 0.95)), float(total) * float(rs.uniform(0.05, 0.95))]
    if cums:
        out += [float(cums[int(rs.randint(len(cums)))]), float(cums[0]), float(np.nextafter(cums[len(cums) // 2], np.inf))]
    return out


def check_call(reg, a, n, first, num, r=None, outcome=None, reads=1, ref=None):
    """one measure (r) or postselect (outcome) on a register that holds `a`; returns the state it holds afterwards
    (ref: collapse_ref's answer for a postselect, where the caller has it already)"""
    if outcome is None:
        v, p, want = measure_ref(a, n, first, num, r)
        gv, gp, st = reg.measure_qubits(first, num, r, strict=False)
        assert gv == v, (n, first, num, r, gv, v)
    else:
        v = outcome
        p, want = ref if ref is not None else collapse_ref(a, n, first, num, v)
        gp, st = reg.postselect(first, num, v, strict=False)
    same([gp], [p], f"probability n={n} range=({first},{num}) outcome={v}")
    if want is None:
        assert st == BAD_ARGUMENTS, (n, first, num, v, p, st)
        assert reg.collapse_stats() == (0, reads, 0)
        same(reg.read(), a, "an error must leave the state as it was")
        return a
    assert st == 0, (n, first, num, v, p, st)
    assert reg.collapse_stats() == (0, reads, 1)
    same(reg.read(), want, f"state n={n} range=({first},{num}) outcome={v}")
    return want


# ---- 1. every range of small registers -------------------------------------------------------------------------------------

@pytest.mark.parametrize("nonfinite", [False, True])
def test_every_range_small_registers(qc, nonfinite):
    rs = np.random.RandomState(5)
    for n in range(1, 13):
        a = spread_state(n, 31 * n + (7 if nonfinite else 0), nonfinite)
        with qc.Register(n, 0) as reg:
            for first in range(n + 1):
                for num in range(n - first + 1):
                    P = marginal_ref(a, n, first, num)
                    rl = draws(P, rs)
                    if n > 8:
                        rl = [rl[i] for i in rs.choice(len(rl), 3, replace=False)]
                    for r in rl:
                        reg.write(a)
                        check_call(reg, a, n, first, num, r=r)


# ---- 2. post-selection ------------------------------------------------------------------------------------------------------

def test_postselect_every_outcome(qc):
    for n in (3, 6, 9):
        a = spread_state(n, 900 + n)
        v = a.reshape(-1, 2)
        v[(np.arange(1 << n) & 5) == 4] = 0.0                          # outcomes with probability exactly +0
        v[3] = (-0.0, 0.0)
        with qc.Register(n, 0) as reg:
            for first in range(n + 1):
                for num in range(min(4, n - first) + 1):
                    zero_seen = False
                    for outcome in range(1 << num):
                        reg.write(a)
                        check_call(reg, a, n, first, num, outcome=outcome)
                        zero_seen |= marginal_ref(a, n, first, num)[outcome] == 0
                    reg.write(a)
                    p, st = reg.postselect(first, num, 1 << num, strict=False)
                    assert st == BAD_ARGUMENTS
                    same(reg.read(), a)
            with pytest.raises(qc.QcxError) as e:
                reg.write(a)
                reg.postselect(0, 3, 4)
            assert e.value.status == BAD_ARGUMENTS and e.value.outcome == 4 and bits(e.value.probability) == 0
            assert "outcome 4" in str(e.value) and "probability 0" in str(e.value)


# ---- 2b. every launch form of K11 ---------------------------------------------------------------------------------------------

FORCED_N = (9, 10, 11, 13)


def forced_ranges(n):
    out = []
    for first in sorted({0, 1, 2, 3, 4, 5, 6, 7, n}):
        nums = {0, 1, 2, 3, n - 6, n - 5, n - first}
        out += [(first, num) for num in sorted(nums) if 0 <= num and first + num <= n]
    for num in (0, 1, 2, 3, n - 6, n - 5):                                 # first = n - num
        if (n - num, num) not in out:
            out.append((n - num, num))
    return out


@pytest.fixture(scope="module")
def forced_refs(ob):
    """the states of test_forced_kernel_forms and collapse_ref's answers, computed once for all launch forms: a dense state
    (fill_random) and one with -0 amplitudes and outcomes of probability exactly +0"""
    refs = {}
    for n in FORCED_N:
        z = ob.random_state(n, 70 + n)
        v = z.reshape(-1, 2)
        v[np.random.RandomState(n).rand(v.shape[0]) < 0.3] = -0.0
        v[(np.arange(1 << n) & 5) == 4] = 0.0
        v[3] = (-0.0, 0.0)
        for kind, a in (("fill", ob.fill_random(n, 40 + n)), ("zeros", z)):
            calls = []
            for first, num in forced_ranges(n):
                ones = (1 << num) - 1
                for outcome in sorted({ones, (ones * 5 // 8) & ones}):   # the all-ones value and one other (num = 0: the one there is)
                    calls.append((first, num, outcome, collapse_ref(a, n, first, num, outcome)))
            refs[(n, kind)] = (a, calls)
    return refs


@pytest.mark.parametrize("cap", [1, 3, 65536])
@pytest.mark.parametrize("perm", [0, 1])
@pytest.mark.parametrize("upt", [4, 8])
def test_forced_kernel_forms(qc, forced_refs, upt, perm, cap):
    """k_collapse_range<PERM, U> in its four instantiations under a capped grid: with U = 8 a step is 2048 amplitudes, so at
    n = 13 one workgroup walks 4 steps (cap 1) or the steps split 2/1/1 (cap 3) -- the PERM index map beyond its first step --,
    and at n = 9, 10 the only step is partial (the e < count guard).  n == num + 6 (PERM applies) next to n == num + 5 (the
    plain map).  collapse_ref bit for bit."""
    keys = ("collapse_upt", "collapse_perm", "collapse_grid_cap")
    defaults = {k: qc.lib().qcx_tune_get(k.encode()) for k in keys}
    try:
        qc.tune(collapse_upt=upt, collapse_perm=perm, collapse_grid_cap=cap)
        for n in FORCED_N:
            with qc.Register(n, 0) as reg:
                for kind in ("fill", "zeros"):
                    a, calls = forced_refs[(n, kind)]
                    errors = 0
                    for first, num, outcome, ref in calls:
                        if kind == "fill":
                            reg.fill_random(40 + n)
                        else:
                            reg.write(a)
                        check_call(reg, a, n, first, num, outcome=outcome, ref=ref)
                        errors += ref[1] is None
                    assert (errors > 0) == (kind == "zeros")
    finally:
        qc.tune(**defaults)


# ---- 3. circuits against the oracle ----------------------------------------------------------------------------------------

def oracle_shor(ob, L, M, Cn, a):
    n = L + M
    w = np.zeros(2 << n)
    ob.reset(w, n)
    ob.quantum_computation(w, n, M, Cn, a, threads=8)
    return w


@pytest.mark.parametrize("fusion", [-1, 0, 1, 2])
def test_circuits_then_measure(qc, ob, fusion):
    L, M, Cn, a = 9, 5, 21, 2
    n = L + M
    want = oracle_shor(ob, L, M, Cn, a)
    for r1, r2 in ((0.3, 0.6), (0.93, 0.11)):
        with qc.Register(L, M) as reg:
            reg.set_fusion(fusion)
            qc.reset_register(reg)
            qc.quantum_computation(Cn, a, reg)
            w = reg.read() if fusion == 2 else want                     # tolerance mode: exact arithmetic on what the GPU holds
            vM, pM, w1 = measure_ref(w, n, 0, M, r1)
            got = reg.measure_qubits(0, M, r1)
            assert got[0] == vM and bits(got[1]) == bits(pM)
            same(reg.read(), w1, "after measuring M")
            vL, pL, w2 = measure_ref(w1, n, M, L, r2)
            got = qc.measure_qubits(reg, M, L, r2)
            assert got[0] == vL and bits(got[1]) == bits(pL)
            same(reg.read(), w2, "after measuring L")
            assert np.count_nonzero(w2) in (1, 2)
    n = 13
    x = ob.random_state(n, 5)
    w = x.copy(); ob.iqft(w, n, 4, threads=8)
    for first, num, r in ((4, 9, 0.5), (0, 4, 0.2), (3, 5, 0.8), (0, 0, 0.5), (5, 3, 0.4)):
        with qc.Register(n - 4, 4) as reg:
            reg.set_fusion(fusion)
            reg.write(x)
            qc.inverse_QFT(reg)
            base = reg.read() if fusion == 2 else w
            v, p, w1 = measure_ref(base, n, first, num, r)
            got = reg.measure_qubits(first, num, r)
            assert got[0] == v and bits(got[1]) == bits(p)
            same(reg.read(), w1)


# ---- 4. the state is usable afterwards --------------------------------------------------------------------------------------

def gates_after(qc, ob, reg, w, n, M, Cn, first, num):
    """more gates on the GPU register and on the oracle's copy: H on a kept and on a measured qubit, a controlled phase, a modular
    multiply"""
    kept = (first + num) % n if num < n else 0
    meas = first if num else (first + 1) % n
    for q in (kept, meas):
        qc.hadamard_gate(q, reg); ob.hadamard(w, n, q)
    c, t = (n - 1, 0)
    qc.c_phase_shift_gate(c, t, 0.37, reg); ob.cphase(w, n, c, t, 0.37)
    qc.c_amodc_gate(Cn, 4, n - 2, reg); ob.camodc(w, n, M, Cn, 4, n - 2)


@pytest.mark.parametrize("fusion", [-1, 0, 1])
def test_gates_before_and_after(qc, ob, fusion):
    L, M, Cn = 9, 5, 21
    n = L + M
    rs = np.random.RandomState(12)
    for first, num, r in ((0, M, 0.4), (M, L, 0.7), (3, 4, 0.2), (7, 3, 0.9), (0, 0, 0.5), (5, 1, 0.5)):
        x = ob.random_state(n, 40 + first)
        v = x.reshape(-1, 2)
        v[rs.rand(v.shape[0]) < 0.3] = -0.0                             # kept -0 stay -0 through the collapse
        w = x.copy()
        with qc.Register(L, M) as reg:
            reg.set_fusion(fusion)
            reg.write(x)
            for q in (1, n - 1):                                        # queued before the call (mode 1), flushed by it
                qc.hadamard_gate(q, reg); ob.hadamard(w, n, q)
            qc.c_phase_shift_gate(2, 9, -1.1, reg); ob.cphase(w, n, 2, 9, -1.1)
            vv, p, w1 = measure_ref(w, n, first, num, r)
            got = reg.measure_qubits(first, num, r)
            assert got[0] == vv and bits(got[1]) == bits(p)
            w2 = w1.copy()
            gates_after(qc, ob, reg, w2, n, M, Cn, first, num)
            same(reg.read(), w2, f"gates after the collapse, mode {fusion}, range ({first},{num})")
            qc.inverse_QFT(reg); ob.iqft(w2, n, M, threads=8)
            same(reg.read(), w2, f"inverse QFT after the collapse, mode {fusion}")


@pytest.mark.parametrize("fusion", [-1, 0, 1])
def test_inverse_qft_straight_after_a_collapse(qc, ob, fusion):
    L, M = 10, 4
    n = L + M
    x = ob.random_state(n, 77)
    x.reshape(-1, 2)[::3] = (-0.0, 0.0)
    v, p, w1 = measure_ref(x, n, 0, M, 0.55)
    with qc.Register(L, M) as reg:
        reg.set_fusion(fusion)
        reg.write(x)
        assert reg.measure_qubits(0, M, 0.55)[0] == v
        qc.inverse_QFT(reg)
        w = w1.copy(); ob.iqft(w, n, M, threads=8)
        same(reg.read(), w)


def test_observers_see_a_written_state(qc, ob, tmp_path):
    """measure_state, sample_states, marginal, state_save / state_load and the device pointer on the collapsed state agree with
    the same calls on a fresh register that was WRITTEN that state"""
    n = 13
    x = ob.random_state(n, 9)
    x.reshape(-1, 2)[5::7] = (0.0, -0.0)
    rsamp = np.random.RandomState(3).rand(64)
    for first, num, r in ((0, 4, 0.3), (4, 6, 0.8), (2, 11, 0.5)):
        v, p, w1 = measure_ref(x, n, first, num, r)
        with qc.Register(n - 4, 4) as reg, qc.Register(n - 4, 4) as twin:
            reg.write(x)
            assert reg.measure_qubits(first, num, r)[0] == v
            twin.write(w1)
            for fr in ((first, num), (0, 4), (3, 7), (0, 0)):
                same(reg.marginal(*fr), twin.marginal(*fr))
            assert np.array_equal(qc.sample_states(reg, rsamp), qc.sample_states(twin, rsamp))
            assert reg.norm2() == twin.norm2() and reg.total_probability() == twin.total_probability()
            f1, f2 = tmp_path / "a.qcx", tmp_path / "b.qcx"
            reg.save(f1); twin.save(f2)
            assert f1.read_bytes() == f2.read_bytes()
            assert reg.device_pointer() != 0
            same(reg.read(), w1)
            with qc.Register(n - 4, 4) as third:
                third.load(f1)
                qc.hadamard_gate(3, third); qc.hadamard_gate(3, reg)
                same(third.read(), reg.read())
            for rr in (0.2, 0.9):
                reg.write(x); reg.postselect(first, num, v)
                twin.write(w1)
                assert qc.measure_state(reg, rr) == qc.measure_state(twin, rr)
                same(reg.read(), twin.read())


# ---- 5. the textbook order of Shor's circuit --------------------------------------------------------------------------------

@pytest.mark.parametrize("fusion", [-1, 0, 1])
def test_textbook_order(qc, ob, fusion):
    L, M, Cn, a = 9, 5, 21, 2
    n = L + M
    w = np.zeros(2 << n); ob.reset(w, n)
    with qc.Register(L, M) as reg:
        reg.set_fusion(fusion)
        qc.reset_register(reg)
        for l in range(L):
            qc.hadamard_gate(M + l, reg); ob.hadamard(w, n, M + l)
        atox = a % Cn
        for l in range(L):
            qc.c_amodc_gate(Cn, atox, M + l, reg); ob.camodc(w, n, M, Cn, atox, M + l)
            atox = (atox * atox) % Cn
        r = 0.37
        v, p, w1 = measure_ref(w, n, 0, M, r)
        got = reg.measure_qubits(0, M, r)
        assert got[0] == v and bits(got[1]) == bits(p)
        qc.inverse_QFT(reg); ob.iqft(w1, n, M, threads=8)
        same(reg.marginal(M, L), marginal_ref(w1, n, M, L))
        same(reg.read(), w1)


# ---- 6. lazy forms ----------------------------------------------------------------------------------------------------------

def test_pending_basis_state(qc, ob):
    n = 14
    w = np.zeros(2 << n); ob.reset(w, n)
    with qc.Register(n - 4, 4) as reg:
        qc.reset_register(reg)                                          # pending basis state |1>
        for first, num in ((0, 4), (4, 10), (0, 0), (1, 3), (0, n)):
            v = (1 >> first) & ((1 << num) - 1)
            assert reg.measure_qubits(first, num, 0.5) == (v, 1.0)
            assert reg.collapse_stats() == (2, 0, 0)
            assert reg.postselect(first, num, v) == 1.0
            assert reg.collapse_stats() == (2, 0, 0)
            assert reg.marginal(0, 2).tolist() == [0.0, 1.0, 0.0, 0.0] and reg.marginal_stats() == (2, 0)     # still pending
            if num:
                p, st = reg.postselect(first, num, v ^ 1, strict=False)
                assert st == BAD_ARGUMENTS and bits(p) == 0 and reg.collapse_stats() == (2, 0, 0)
                assert reg.marginal_stats() == (2, 0)
        same(reg.read(), w)


def test_compact_result(qc, ob):
    L, M, Cn, a = 15, 5, 21, 2                                          # (the compact chain runs from n = 20 on)
    n = L + M
    want = oracle_shor(ob, L, M, Cn, a)
    for first, num, r, in_place in ((M + 3, 4, 0.41, True), (M, L, 0.7, True), (0, M, 0.3, False), (2, 6, 0.66, False)):
        with qc.Register(L, M) as reg:
            qc.reset_register(reg); qc.quantum_computation(Cn, a, reg)
            c0 = compact_measures(qc, reg)
            v, p, w1 = measure_ref(want, n, first, num, r)
            got = reg.measure_qubits(first, num, r)
            assert got[0] == v and bits(got[1]) == bits(p)
            src, reads, writes = reg.collapse_stats()
            assert (src, writes) == (3, 1) and reads == 1
            assert compact_measures(qc, reg) == c0 + (1 if in_place else 0)
            same(reg.marginal(first, num), marginal_ref(w1, n, first, num))
            assert reg.marginal_stats() == (0, 1)                       # no longer compact
            same(reg.read(), w1)
        with qc.Register(L, M) as reg:                                  # the error case leaves the compact form as it was
            qc.reset_register(reg); qc.quantum_computation(Cn, a, reg)
            c0 = compact_measures(qc, reg)
            p, st = reg.postselect(0, M, 0, strict=False)               # M = 0 is never held
            assert st == BAD_ARGUMENTS and bits(p) == 0
            assert reg.collapse_stats()[2] == 0
            reg.marginal(M, L)
            assert reg.marginal_stats() == (1, 1)                       # still compact: read in place
            same(reg.read(), want)


def test_nonfinite_register(qc, ob):
    n = 13
    a = ob.random_state(n, 21)
    a[2 * 700] = np.inf
    a[2 * 3000 + 1] = np.nan
    a[2 * 5] = -0.0
    with qc.Register(n, 0) as reg:
        reg.write(a)
        v, p, w1 = measure_ref(a, n, 0, 0, 0.5)                         # the total is NaN
        assert w1 is None
        gv, gp, st = reg.measure_qubits(0, 0, 0.5, strict=False)
        assert st == BAD_ARGUMENTS and gv == 0 and np.isnan(gp)
        same(reg.read(), a)
        for outcome, bad in ((0, np.isinf), (2, np.isnan)):             # amplitude 700 holds Inf, amplitude 3000 NaN
            p, w1 = collapse_ref(a, n, 10, 3, outcome)
            assert w1 is None and bad(p)
            check_call(reg, a, n, 10, 3, outcome=outcome)
        with pytest.raises(qc.QcxError) as e:
            reg.measure_qubits(10, 3, 1e-3)                             # the scan stops at value 0, whose probability is Inf
        assert e.value.outcome == 0 and np.isinf(e.value.probability) and "inf" in str(e.value)
        same(reg.read(), a)
        qc.hadamard_gate(2, reg)                                        # still the strict gate: NaN / Inf as the oracle's products
        w = a.copy(); ob.hadamard(w, n, 2)
        same(reg.read(), w)
    # a flagged register whose range probabilities are finite: collapsed, flag kept
    b = ob.random_state(n, 22)
    b[2 * 9] = 1e154                                                    # >= 2^500: flagged, |b|^2 = 1e308 is finite
    with qc.Register(n, 0) as reg:
        reg.write(b)
        w1 = check_call(reg, b, n, 0, 3, outcome=1)
        qc.hadamard_gate(5, reg)
        w = w1.copy(); ob.hadamard(w, n, 5)
        same(reg.read(), w)


# ---- 7. errors --------------------------------------------------------------------------------------------------------------

def test_arguments(qc):
    lib = qc.lib()
    out, p = C.c_ulong(99), C.c_double(-1.0)
    with qc.Register(12, 0) as reg:
        reg.fill_random(1)
        before = reg.read()
        rng = qc.Rng(4)
        assert lib.qcx_measure_qubits_r(reg._h, 0, 3, 0.5, None, C.byref(p)) == BAD_ARGUMENTS
        assert lib.qcx_measure_qubits(reg._h, None, 0, 3, C.byref(out), C.byref(p)) == BAD_ARGUMENTS
        assert lib.qcx_measure_qubits(reg._h, rng._h, 0, 3, None, C.byref(p)) == BAD_ARGUMENTS
        assert lib.qcx_measure_qubits_r(reg._h, 10, 3, 0.5, C.byref(out), C.byref(p)) == BAD_QUBIT
        assert lib.qcx_measure_qubits(reg._h, rng._h, 13, 0, C.byref(out), C.byref(p)) == BAD_QUBIT
        assert lib.qcx_postselect_qubits(reg._h, 12, 1, 0, C.byref(p)) == BAD_QUBIT
        assert lib.qcx_postselect_qubits(reg._h, 2, 2, 4, None) == BAD_ARGUMENTS
        assert (out.value, p.value) == (99, -1.0)
        same(reg.read(), before)
        assert lib.qcx_postselect_qubits(reg._h, 2, 2, 3, None) == 0                  # NULL probability is allowed
        assert lib.qcx_collapse_last_stats(reg._h, None, None, None) == 0
    with qc.Register(31, 0) as big:
        assert lib.qcx_measure_qubits_r(big._h, 0, 31, 0.5, C.byref(out), C.byref(p)) == UNSUPPORTED
    with qc.Register(13, 0, shards=4, devices=qc.spread_devices(4)) as sh:           # virtual shards on one GPU
        sh.fill_random(3)
        before = sh.read()
        rng, twin = qc.Rng(11), qc.Rng(11)
        assert lib.qcx_measure_qubits(sh._h, rng._h, 0, 3, C.byref(out), C.byref(p)) == UNSUPPORTED
        assert lib.qcx_measure_qubits_r(sh._h, 0, 3, 0.5, C.byref(out), C.byref(p)) == UNSUPPORTED
        assert lib.qcx_postselect_qubits(sh._h, 0, 3, 1, C.byref(p)) == UNSUPPORTED
        assert rng.get() == twin.get(), "no draw may be made for a sharded register"
        same(sh.read(), before)


def test_rng_form_makes_one_draw(qc, ob):
    n = 10
    a = ob.random_state(n, 2)
    rng, twin = qc.Rng(123), qc.Rng(123)
    with qc.Register(n, 0) as reg:
        reg.write(a)
        r = twin.uniform()
        v, p, w1 = measure_ref(a, n, 2, 5, r)
        got = reg.measure_qubits(2, 5, rng)
        assert got[0] == v and bits(got[1]) == bits(p)
        same(reg.read(), w1)
        assert rng.get() == twin.get()


def test_num_zero_scales_the_state(qc):
    for n in (1, 7, 12):
        a = spread_state(n, 60 + n)
        with qc.Register(n, 0) as reg:
            for first in (0, n // 2, n):
                reg.write(a)
                total = marginal_ref(a, n, first, 0)[0]
                s = np.float64(1.0) / np.sqrt(total)
                v, p = reg.measure_qubits(first, 0, 0.5)
                assert v == 0 and bits(p) == bits(total)
                with np.errstate(under="ignore"):
                    same(reg.read(), a * s)


# ---- 8. full size -----------------------------------------------------------------------------------------------------------

def test_n30_windows_against_a_twin(qc):
    n = 30
    W = 1 << 16
    with qc.Register(n, 0) as reg, qc.Register(n, 0) as twin:
        twin.fill_random(9)
        for first, num, r in ((12, 4, 0.53), (0, 2, 0.8), (27, 3, 0.3)):
            reg.fill_random(9)
            v, p = reg.measure_qubits(first, num, r)
            assert reg.collapse_stats() == (0, 1, 1)
            P = twin.marginal(first, num)
            assert v == choose(P, r) and bits(p) == bits(P[v])
            s = np.float64(1.0) / np.sqrt(np.float64(p))
            if first >= 16:         # half of the windows inside the kept run, half outside
                inside = [(v << first) + k * ((1 << first) // 4) for k in range(4)]
                other = [(((v + 1 + k) % (1 << num)) << first) + k * W * 3 for k in range(4)]
                starts = inside + other
            else:
                starts = [k * ((1 << n) // 8) + k * W for k in range(7)] + [(1 << n) - W]
            kept_seen = dropped_seen = 0
            for st in starts:
                a = twin.read(st, W)
                idx = np.arange(st, st + W, dtype=np.uint64)
                keep = np.repeat(((idx >> np.uint64(first)) & np.uint64((1 << num) - 1)) == np.uint64(v), 2)
                want = np.where(keep, a * s, 0.0)
                same(reg.read(st, W), want, f"window at {st}, range ({first},{num})")
                kept_seen += int(keep.sum()); dropped_seen += int((~keep).sum())
            assert kept_seen and dropped_seen
            assert abs(reg.norm2() - 1.0) < 1e-12


# ---- the host driver (-P -p) -------------------------------------------------------------------------------------------------

def run_cli(*args):
    subprocess.run(["make", "-C", os.path.join(ROOT, "host"), "-s"], check=True)
    return subprocess.run([os.path.join(ROOT, "host", "qcx_shor"), *args], capture_output=True, text=True, timeout=300)


def test_cli_postselect(qc, ob):
    L, M, Cn, a = 9, 5, 21, 2
    n = L + M
    want = oracle_shor(ob, L, M, Cn, a)
    p4, w1 = collapse_ref(want, n, 0, M, 4)
    m = marginal_ref(w1, n, M, L)
    P = np.zeros(1 << L)
    for v in range(1 << L):
        P[int(format(v, f"0{L}b")[::-1], 2)] = m[v]
    p = run_cli("-C", "21", "-L", "9", "-M", "5", "-a", "2", "-P", "-p", "4", "-j")
    assert p.returncode == 0, p.stdout + p.stderr
    j = json.loads([x for x in p.stdout.splitlines() if x.startswith("{")][-1])
    assert j["postselect_M"] == 4 and j["p_postselect"] == float(p4)
    assert " --- P(M = 4) = %.17g" % p4 in p.stdout
    assert j["top"] == {k: float(P[int(k)]) for k in j["top"]} and len(j["top"]) == 16
    assert max(j["top"].values()) == P.max()
    p = run_cli("-C", "21", "-L", "9", "-M", "5", "-a", "2", "-P", "-p", "3")      # 3 is not a power of 2 mod 21
    assert p.returncode != 0 and "M = 3" in p.stderr and "probability 0" in p.stderr
