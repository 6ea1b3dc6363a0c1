"""Host only: the definition of qcx_measure_qubits / qcx_postselect_qubits (tests/collapse_ref.py) against itself and the oracle
on small registers, and the parts of the feature that need no GPU: the header declares the four entry points, libqcx.so exports
them, and the host driver refuses -p without -P."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from collapse_ref import choose, collapse_ref, measure_ref, running_sums, scale_of
from marginal_ref import marginal_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("qcx_measure_qubits_r", "qcx_measure_qubits", "qcx_postselect_qubits", "qcx_collapse_last_stats")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def spread_state(n, seed):
    rs = np.random.RandomState(seed)
    a = rs.standard_normal(2 << n) * 2.0 ** rs.randint(-40, 40, 2 << n)
    k = a.size
    m = max(1, k // 16)
    a[rs.randint(0, k, m)] = 5e-324 * rs.randint(1, 1000, m)
    a[rs.randint(0, k, m)] = 0.0
    a[rs.randint(0, k, m)] = -0.0
    return a


def test_choose_is_the_reference_scan():
    P = np.array([0.25, 0.0, 0.5, 0.25])
    assert choose(P, -1.0) == 0 and choose(P, 0.0) == 0                       # r <= 0: the first value, whatever it holds
    assert choose(P, 0.25) == 0 and choose(P, np.nextafter(0.25, 1)) == 2     # a tie goes to the first v; P = 0 is stepped over
    assert choose(P, 0.75) == 2 and choose(P, 0.9) == 3
    assert choose(P, 5.0) == 3 and choose(P, float("nan")) == 3               # above the total, NaN: the last value
    assert choose(np.array([0.7]), 0.3) == 0 and choose(np.array([0.7]), 9.0) == 0     # num = 0: the single outcome
    assert running_sums(P) == [0.25, 0.25, 0.75]
    assert choose(np.array([np.nan, 1.0, 0.0]), 0.5) == 2                     # a NaN running sum never compares >= r


def test_scale():
    assert scale_of(0.0) is None and scale_of(-1.0) is None and scale_of(np.inf) is None and scale_of(np.nan) is None
    assert scale_of(1.0) == 1.0 and scale_of(0.25) == 2.0
    assert scale_of(5e-324) == np.float64(1.0) / np.sqrt(np.float64(5e-324))  # finite: every P > 0 has a finite s
    assert scale_of(0.2500000000000001) == np.float64(1.0) / np.sqrt(np.float64(0.2500000000000001))


def test_collapse_against_itself():
    for n in range(1, 9):
        a = spread_state(n, 17 * n)
        idx = np.arange(1 << n)
        for first in range(n + 1):
            for num in range(n - first + 1):
                P = marginal_ref(a, n, first, num)
                for v in range(1 << num):
                    p, out = collapse_ref(a, n, first, num, v)
                    assert bits(p) == bits(P[v])
                    if out is None:
                        assert not (np.isfinite(p) and p > 0)
                        continue
                    s = np.float64(1.0) / np.sqrt(np.float64(p))
                    keep = ((idx >> first) & ((1 << num) - 1)) == v
                    drop2 = np.repeat(~keep, 2)
                    assert not bits(out)[drop2].any(), "a dropped amplitude is not (+0, +0)"
                    with np.errstate(under="ignore"):
                        assert np.array_equal(bits(out)[~drop2], bits(a[~drop2] * s))
                    again = marginal_ref(out, n, first, num)
                    assert not bits(np.delete(again, v)).any(), "the collapsed state holds another outcome"
                    assert again[v] > 0 or p < 1e-300


def test_minus_zero_is_kept_and_small_products_underflow_to_it():
    a = np.zeros(8)
    a[0], a[1] = -0.0, -5e-324                  # amplitude 0 = (-0, -denormal), amplitude 1 heavy: s < 1
    a[2] = 3.0
    a[4] = 1.0
    p, out = collapse_ref(a, 2, 1, 1, 0)
    assert p == 9.0
    assert bits(out)[0] == 1 << 63 and bits(out)[1] == 1 << 63       # fl(-5e-324 / 3) = -0
    assert out[2] == 1.0 and not bits(out)[4:].any()


def test_error_case_leaves_no_state():
    a = np.zeros(16)
    a[0] = 1.0
    p, out = collapse_ref(a, 3, 0, 2, 1)
    assert bits(p) == 0 and out is None
    a[6] = 1e300                                 # |a|^2 = Inf
    p, out = collapse_ref(a, 3, 0, 2, 3)
    assert np.isinf(p) and out is None
    a[6] = np.nan
    v, p, out = measure_ref(a, 3, 0, 2, 2.0)
    assert v == 3 and np.isnan(p) and out is None


def oracle_shor(ob, L, M, Cn, a):
    n = L + M
    w = np.zeros(2 << n)
    ob.reset(w, n)
    ob.quantum_computation(w, n, M, Cn, a, threads=4)
    return w


def test_measuring_M_then_L_of_the_shor_state_leaves_one_amplitude(ob):
    for (L, M, Cn, a), rs in (((3, 4, 15, 7), (1e-9, 0.3, 0.77, 0.999)), ((9, 5, 21, 2), (0.01, 0.42, 0.9))):
        n = L + M
        w = oracle_shor(ob, L, M, Cn, a)
        v0, p0, w0 = measure_ref(w, n, 0, M, 0.0)                    # r <= 0 stops at M = 0, which the ladder's orbit never holds
        assert v0 == 0 and bits(p0) == 0 and w0 is None
        for r1 in rs:
            vM, pM, w1 = measure_ref(w, n, 0, M, r1)
            assert w1 is not None and 0 < pM <= 1
            assert abs(ob.norm2(w1.copy(), n) - 1.0) < 1e-12
            for r2 in rs:
                vL, pL, w2 = measure_ref(w1, n, M, L, r2)
                assert w2 is not None
                nz = np.flatnonzero((w2[0::2] != 0) | (w2[1::2] != 0))
                assert nz.tolist() == [(vL << M) | vM]
                assert abs(np.hypot(w2[2 * nz[0]], w2[2 * nz[0] + 1]) - 1.0) < 1e-12
                # the joint probability is that of the basis state in the uncollapsed state, to rounding
                i = int(nz[0])
                assert abs(pM * pL - (w[2 * i] ** 2 + w[2 * i + 1] ** 2)) < 1e-12


def test_header_declares_and_library_exports_the_entry_points(qc):
    hdr = open(os.path.join(ROOT, "include", "qcx.h")).read()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in qc._lib.SIGNATURES
    lib = C.CDLL(qc.LIB_PATH)
    for name in NAMES:
        assert getattr(lib, name) is not None
    out, p = C.c_ulong(7), C.c_double(0.5)
    f = qc.lib()
    assert f.qcx_measure_qubits_r(None, 0, 1, 0.5, C.byref(out), C.byref(p)) == 2       # NULL register: QCX_BAD_ARGUMENTS
    assert f.qcx_measure_qubits(None, None, 0, 1, C.byref(out), C.byref(p)) == 2
    assert f.qcx_postselect_qubits(None, 0, 1, 0, C.byref(p)) == 2
    assert f.qcx_collapse_last_stats(None, None, None, None) == 2
    assert (out.value, p.value) == (7, 0.5)
    assert callable(qc.measure_qubits) and callable(qc.postselect_qubits)
    for m in ("measure_qubits", "postselect", "collapse_stats"):
        assert callable(getattr(qc.Register, m))


def test_host_driver_refuses_p_without_P():
    subprocess.run(["make", "-C", os.path.join(ROOT, "host"), "-s"], check=True)
    exe = os.path.join(ROOT, "host", "qcx_shor")
    p = subprocess.run([exe, "-C", "21", "-L", "9", "-M", "5", "-a", "2", "-p", "4"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 2 and "-p" in p.stderr and "-P" in p.stderr
    p = subprocess.run([exe, "-C", "21", "-L", "9", "-M", "5", "-a", "2", "-P", "-p", "x"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 2 and "-p" in p.stderr
    p = subprocess.run([exe, "-C", "21", "-L", "9", "-M", "5", "-a", "2", "-P", "-p", "4", "-g", "2"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 2 and "-P" in p.stderr
