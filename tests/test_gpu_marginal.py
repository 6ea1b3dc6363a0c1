"""GPU: the exact outcome distribution of a qubit range (qcx_marginal_probabilities, K10).  Every output must be, bit for bit,
the pinned pairwise tree of tests/marginal_ref.py on whatever the state holds (subnormals, overflow to Inf, +-0, NaN as NaN),
circuit results must match the oracle's state, and the lazy forms must stay as they were: a pending basis state answered with
no kernel, a circuit's compact result read in place and still compact afterwards."""
import ctypes as C
import json
import math
import os
import subprocess

import numpy as np
import pytest

from marginal_ref import marginal_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), "NaN positions differ"
    bad = np.flatnonzero(bits(got[~gn]) != bits(want[~wn]))
    assert bad.size == 0, f"{bad.size} outputs differ, first at {bad[:4]}: {got[~gn][bad[:4]]} vs {want[~wn][bad[:4]]}"


def compact_measures(qc, reg):
    v = C.c_ulong(0)
    assert qc.lib().qcx_compact_measure_stats(reg._h, C.byref(v)) == 0
    return int(v.value)


def adversarial(n, seed):
    rs = np.random.RandomState(seed)
    a = rs.standard_normal(2 << n) * 2.0 ** rs.randint(-40, 40, 2 << n)
    k = a.size
    m = max(1, k // 16)
    a[rs.randint(0, k, m)] = 5e-324 * rs.randint(1, 1000, m)           # subnormals
    a[rs.randint(0, k, max(1, k // 32))] = 1e300                         # |a|^2 overflows to Inf
    a[rs.randint(0, k, m)] = 0.0
    a[rs.randint(0, k, m)] = -0.0
    a[rs.randint(0, k, max(1, k // 64))] = 1e154
    if n >= 4:
        a[rs.randint(0, k)] = np.inf
        a[rs.randint(0, k)] = np.nan
    return a


def oracle_shor(ob, L, M, Cn, a):
    n = L + M
    w = np.zeros(2 << n)
    ob.reset(w, n)
    ob.quantum_computation(w, n, M, Cn, a, threads=8)
    return w


def test_every_range_small_registers(qc):
    """n = 1 .. 14, every (first, num), adversarial states written with qcx_state_write"""
    for n in range(1, 15):
        a = adversarial(n, 31 * n)
        with qc.Register(n, 0) as reg:
            reg.write(a)
            for first in range(n + 1):
                for num in range(n - first + 1):
                    same(reg.marginal(first, num), marginal_ref(a, n, first, num))
                    assert reg.marginal_stats() == (0, 1)
            assert np.array_equal(bits(reg.read()), bits(a)), "the state changed"


def test_table_one_without_sampling_noise(qc, ob):
    """C = 15, L = 3, M = 4, a = 7 (the reference's Table I): x~ = 0, 2, 4, 6 carry 0.2500000000000001 each, the others +0"""
    L, M = 3, 4
    want = oracle_shor(ob, L, M, 15, 7)
    with qc.Register(L, M) as reg:
        qc.reset_register(reg)
        qc.quantum_computation(15, 7, reg)
        same(reg.marginal(M, L), marginal_ref(want, L + M, M, L))
        P = qc.omega_distribution(reg)
    assert [float(P[x]) for x in (0, 2, 4, 6)] == [0.2500000000000001] * 4
    assert all(bits(P[[1, 3, 5, 7]]) == 0)


@pytest.mark.parametrize("fusion", [-1, 0, 1])
def test_circuits_against_the_oracle(qc, ob, fusion):
    L, M, Cn, a = 9, 5, 21, 2
    n = L + M
    want = oracle_shor(ob, L, M, Cn, a)
    with qc.Register(L, M) as reg:
        reg.set_fusion(fusion)
        qc.reset_register(reg)
        qc.quantum_computation(Cn, a, reg)
        for first, num in ((M, L), (0, M), (0, 0), (2, 7), (0, n)):
            same(reg.marginal(first, num), marginal_ref(want, n, first, num))
    # a dense input through inverse_QFT
    n = 13
    x = ob.random_state(n, 5)
    w = x.copy(); ob.iqft(w, n, 4, threads=8)
    with qc.Register(n - 4, 4) as reg:
        reg.set_fusion(fusion)
        reg.write(x)
        qc.inverse_QFT(reg)
        for first, num in ((4, 9), (0, 4), (3, 5), (0, 0)):
            same(reg.marginal(first, num), marginal_ref(w, n, first, num))


def test_pending_basis_state(qc, ob):
    n = 14
    with qc.Register(n - 4, 4) as reg:
        qc.reset_register(reg)                                      # pending basis state |1>
        for first, num in ((0, 4), (4, 10), (0, 0), (1, 3), (0, n)):
            got = reg.marginal(first, num)
            want = np.zeros(1 << num); want[(1 >> first) & ((1 << num) - 1)] = 1.0
            assert np.array_equal(bits(got), bits(want))
            assert reg.marginal_stats() == (2, 0)
        w = np.zeros(2 << n); ob.reset(w, n)
        assert np.array_equal(bits(reg.read()), bits(w))
        qc.hadamard_gate(0, reg)                                     # no longer pending: a kernel reads the register
        reg.marginal(0, 1)
        assert reg.marginal_stats() == (0, 1)
        qc.measure_state(reg, 0.9)                                   # a collapse: pending basis state 1 again
        assert reg.marginal(0, 2).tolist() == [0.0, 1.0, 0.0, 0.0] and reg.marginal_stats() == (2, 0)


def test_queued_gates_fusion_1(qc, ob):
    n = 14
    want = np.zeros(2 << n); ob.reset(want, n)
    with qc.Register(n - 4, 4) as reg:
        reg.set_fusion(1)
        qc.reset_register(reg)
        for q in (0, 3, n - 1):
            qc.hadamard_gate(q, reg)
            ob.hadamard(want, n, q)
        qc.c_phase_shift_gate(3, n - 1, 0.7, reg)
        ob.cphase(want, n, 3, n - 1, 0.7)
        same(reg.marginal(2, 5), marginal_ref(want, n, 2, 5))
        assert reg.marginal_stats() == (0, 1)
        assert np.array_equal(bits(reg.read()), bits(want))


def test_compact_result_read_in_place(qc, ob):
    """behind quantum_computation the result is compact: a range above M is read there (source 1), the state stays compact,
    and a measurement afterwards gives what it gives on a register that skipped the marginal"""
    L, M, Cn, a = 15, 5, 21, 2                                      # (the compact chain runs from n = 20 on)
    n = L + M
    want = oracle_shor(ob, L, M, Cn, a)
    r = 0.377
    with qc.Register(L, M) as plain:
        qc.reset_register(plain); qc.quantum_computation(Cn, a, plain)
        idx_plain = qc.measure_state(plain, r)
    with qc.Register(L, M) as reg:
        qc.reset_register(reg); qc.quantum_computation(Cn, a, reg)
        c0 = compact_measures(qc, reg)
        for first, num in ((M, L), (M + 3, 4), (M + 1, L - 1), (n, 0), (M, 0)):
            same(reg.marginal(first, num), marginal_ref(want, n, first, num))
            assert reg.marginal_stats() == (1, 1)
        assert compact_measures(qc, reg) == c0 + 5
        idx = qc.measure_state(reg, r)                              # still compact: the measurement scans the compact form
        assert compact_measures(qc, reg) == c0 + 6
        assert idx == idx_plain
        w = want.copy(); ob.measure(w, n, r)
        assert np.array_equal(bits(reg.read()), bits(w))


def test_compact_range_inside_the_M_register(qc, ob):
    L, M, Cn, a = 15, 5, 21, 2
    n = L + M
    want = oracle_shor(ob, L, M, Cn, a)
    with qc.Register(L, M) as reg:
        qc.reset_register(reg); qc.quantum_computation(Cn, a, reg)
        c0 = compact_measures(qc, reg)
        got = {}
        for first, num in ((0, M), (2, 6), (0, n), (4, 16), (0, 0)):
            got[first, num] = reg.marginal(first, num)
            same(got[first, num], marginal_ref(want, n, first, num))
            assert reg.marginal_stats() == (3, 1)
        assert compact_measures(qc, reg) == c0                      # nothing scanned the compact form in place ...
        assert qc.measure_state(reg, 0.61) == ob.measure(want.copy(), n, 0.61)
        assert compact_measures(qc, reg) == c0 + 1                  # ... and it is still what the measurement reads
    with qc.Register(L, M) as reg:                                  # the same bits as after an explicit flush
        qc.reset_register(reg); qc.quantum_computation(Cn, a, reg)
        reg.flush()
        for (first, num), g in got.items():
            same(reg.marginal(first, num), g)
            assert reg.marginal_stats() == (0, 1)


def test_nonfinite_register(qc, ob):
    n = 13
    a = ob.random_state(n, 21)
    a[2 * 700] = np.inf
    a[2 * 3000 + 1] = np.nan
    a[2 * 5] = -0.0
    with qc.Register(n, 0) as reg:
        reg.write(a)
        for first, num in ((0, 0), (0, 13), (3, 4), (10, 3), (0, 2)):
            same(reg.marginal(first, num), marginal_ref(a, n, first, num))
        qc.hadamard_gate(2, reg)                                    # still the strict gate: the oracle's products, NaN/Inf included
        w = a.copy(); ob.hadamard(w, n, 2)
        got = reg.read()
        gn, wn = np.isnan(got), np.isnan(w)
        assert np.array_equal(gn, wn)
        assert np.array_equal(bits(got[~gn]), bits(w[~wn]))


def test_arguments(qc):
    lib = qc.lib()
    out = (C.c_double * 8)()
    with qc.Register(12, 0) as reg:
        reg.fill_random(1)
        assert lib.qcx_marginal_probabilities(reg._h, 0, 3, None) == 2          # QCX_BAD_ARGUMENTS
        assert lib.qcx_marginal_probabilities(None, 0, 3, out) == 2
        assert lib.qcx_marginal_probabilities(reg._h, 10, 3, out) == 6          # QCX_BAD_QUBIT
        assert lib.qcx_marginal_probabilities(reg._h, 13, 0, out) == 6
        assert lib.qcx_marginal_probabilities(reg._h, 12, 0, out) == 0
        assert lib.qcx_marginal_last_stats(None, None, None) == 2
    with qc.Register(31, 0) as big:                                            # num > 30
        assert lib.qcx_marginal_probabilities(big._h, 0, 31, out) == 7          # QCX_UNSUPPORTED
    with qc.Register(13, 0, shards=4, devices=qc.spread_devices(4)) as sh:     # virtual shards on one GPU
        sh.fill_random(3)
        before = bits(sh.read())
        assert lib.qcx_marginal_probabilities(sh._h, 0, 3, out) == 7
        assert np.array_equal(bits(sh.read()), before)


def test_n28_dense(qc):
    n = 28
    with qc.Register(n, 0) as reg:
        reg.fill_random(5)
        got = {fr: reg.marginal(*fr) for fr in ((5, 23), (0, 5), (10, 8), (0, 0))}
        a = reg.read()
    for (first, num), g in got.items():
        same(g, marginal_ref(a, n, first, num))


def test_n30_shor_compact_against_flushed(qc):
    L, M = 25, 5
    with qc.Register(L, M) as reg:
        qc.reset_register(reg); qc.quantum_computation(21, 2, reg)
        got = reg.marginal(M, L)
        assert reg.marginal_stats() == (1, 1)
        reg.flush()
        want = reg.marginal(M, L)
        assert reg.marginal_stats() == (0, 1)
    same(got, want)
    assert abs(math.fsum(got) - 1.0) <= 1e-12


@pytest.mark.skipif(int(os.environ.get("QCX_TEST_NMAX", "30")) < 34, reason="n = 34 needs QCX_TEST_NMAX >= 34 (a 256 GiB state)")
def test_n34_shor_L_register(qc):
    L, M = 29, 5
    with qc.Register(L, M) as reg:
        qc.reset_register(reg); qc.quantum_computation(21, 2, reg)
        got = reg.marginal(M, L)
        assert reg.marginal_stats() == (1, 1)
    assert abs(math.fsum(got) - 1.0) <= 1e-12


# ---- the host driver (-P) ----------------------------------------------------------------------------------------------------

def classical():
    lib = C.CDLL(os.path.join(ROOT, "host", "libqcx_classical.so"))
    lib.qcx_period_from_omega.restype = C.c_uint
    lib.qcx_period_from_omega.argtypes = [C.c_double, C.c_uint, C.c_uint, C.c_int]
    lib.qcx_factors_from_period.restype = C.c_int
    lib.qcx_factors_from_period.argtypes = [C.c_uint, C.c_uint, C.c_uint, C.c_int, C.POINTER(C.c_uint)]
    return lib


def expected_probabilities(ob, L, M, Cn, a):
    """p_period / p_factors from the oracle's state, the pinned order and the host's own continued fractions"""
    cl = classical()
    m = marginal_ref(oracle_shor(ob, L, M, Cn, a), L + M, M, L)
    P = np.zeros(1 << L)
    for v in range(1 << L):
        P[int(format(v, f"0{L}b")[::-1], 2)] = m[v]
    pp = pf = 0.0
    f = (C.c_uint * 2)()
    for x in range(1 << L):
        if P[x] == 0.0:
            continue
        per = cl.qcx_period_from_omega(x / float(1 << L), a, Cn, 0)
        if per:
            pp += P[x]
            if cl.qcx_factors_from_period(a, per, Cn, 0, f) == 0 and f[0] != 1 and f[1] != 1:
                pf += P[x]
    return P, pp, pf


def run_cli(*args):
    subprocess.run(["make", "-C", os.path.join(ROOT, "host"), "-s"], check=True)
    p = subprocess.run([os.path.join(ROOT, "host", "qcx_shor"), *args], capture_output=True, text=True, timeout=300)
    return p


def json_line(p):
    return json.loads([x for x in p.stdout.splitlines() if x.startswith("{")][-1])


def test_cli_exact_15(qc, ob):
    p = run_cli("-C", "15", "-L", "3", "-M", "4", "-a", "7", "-s", "1", "-P", "-j")
    assert p.returncode == 0, p.stdout + p.stderr
    j = json_line(p)
    P, pp, pf = expected_probabilities(ob, 3, 4, 15, 7)
    assert abs(j["p_period"] - 0.75) <= 1e-12 and abs(j["p_factors"] - 0.75) <= 1e-12
    assert j["p_period"] == pp and j["p_factors"] == pf
    assert j["top"] == {str(x): float(P[x]) for x in range(8)}
    cl = classical()
    assert cl.qcx_period_from_omega(0.0, 7, 15, 0) == 0 and all(cl.qcx_period_from_omega(x / 8, 7, 15, 0) for x in (2, 4, 6))
    assert " --- Exact probability that one attempt yields a period: 0.75" in p.stdout


def test_cli_exact_21_and_histogram(qc, ob):
    P, pp, pf = expected_probabilities(ob, 9, 5, 21, 2)
    assert abs(pp - 0.833328247070314) <= 1e-12 and abs(float(P[0]) - 0.1666717529296877) <= 1e-15
    p = run_cli("-C", "21", "-L", "9", "-M", "5", "-a", "2", "-P", "-j")
    assert p.returncode == 0, p.stdout + p.stderr
    j = json_line(p)
    assert j["p_period"] == pp and j["p_factors"] == pf and abs(j["p_factors"] - 0.833328247070314) <= 1e-12
    assert j["top"]["0"] == float(P[0]) and len(j["top"]) == 16
    shots = 4096
    p = run_cli("-C", "21", "-L", "9", "-M", "5", "-a", "2", "-s", "7", "-P", "-H", str(shots), "-j")
    assert p.returncode == 0, p.stdout + p.stderr
    j = json_line(p)
    assert j["attempts"] == 1 and j["shots"] == shots and j["p_period"] == pp
    sigma = math.sqrt(pp * (1 - pp) / shots)
    assert abs(j["valid_period_shots"] / shots - pp) <= 5 * sigma


def test_cli_exact_needs_a_trial_integer(qc):
    p = run_cli("-C", "15", "-L", "3", "-M", "4", "-P")
    assert p.returncode != 0 and "-P" in p.stderr
    p = run_cli("-C", "15", "-L", "3", "-M", "4", "-a", "7", "-P", "-g", "2")
    assert p.returncode != 0 and "-P" in p.stderr
