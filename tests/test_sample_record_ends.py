"""CPU: the arithmetic the sampling scan (qcx_sample_states, K4d) rests on, rehearsed without a GPU.

A numpy twin of step 2 of DESIGN s4.5c: records that the scan would redo (EVENTS: start of the sum, binade crossing, tie,
oversized element) carry their exact end; every other record is PLAIN -- its integer increment S under the binade of its exact
start, with no flag and no carry out of the binade.  The segmented scan assembles a plain record's end from the last event's
end plus the integer sum of the plain S since then.  Each assembled end must be, bit for bit, the reference's sequential running
sum (orc_measure_range run to the end of the record), on the adversarial inputs of the measurement tests.  The CLI's -H flag's
argument rules are checked here too (no GPU needed: they are refused before a register exists)."""
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASK = (1 << 52) - 1


def meas_inc(b, e):
    """increment of the running sum in ulps of binade e for p with bits b > 0 (qcx_kernels.h: meas_inc); flag = tie or oversized"""
    ex = (b >> 52) & 0x7ff
    mp = (b & MASK) | ((1 << 52) if ex else 0)
    sh = e - (ex if ex else 1)
    if sh <= 0:
        return 1 << 54, True
    shc = min(sh, 63)
    rem, half = mp & ((1 << shc) - 1), 1 << (shc - 1)
    return (mp >> shc) + (1 if rem > half else 0), rem == half


def dbits(x):
    return int(np.float64(x).view(np.uint64))


def bits_to_d(b):
    return float(np.uint64(b).view(np.float64))


def twin_ends(ob, a, rlog):
    """(assembled ends, exact ends, number of events) for records of 2^rlog amplitudes"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    p = (a[0::2] * a[0::2] + a[1::2] * a[1::2]).view(np.uint64)
    dim, R = p.size, 1 << rlog
    exact, cum = [], 0.0
    for b in range(dim // R):
        _, _, cum = ob.measure_range(a[2 * b * R:], b * R, R, dim, cum, math.inf)     # the reference's additions
        exact.append(cum)
    ends, carry, events, start = [], (False, 0, 0), 0, 0.0
    for b in range(dim // R):
        e = (dbits(start) >> 52) & 0x7ff
        S, flag = 0, False
        for x in p[b * R:(b + 1) * R]:
            if int(x):
                i, f = meas_inc(int(x), e)
                S += i
                flag |= f
        nz = bool(p[b * R:(b + 1) * R].any())
        plain = not nz or (0 < e < 0x7ff and not flag and ((dbits(start) & MASK) | (1 << 52)) + S < (1 << 53))
        if plain:
            carry = (carry[0], carry[1], carry[2] + (S if nz else 0))
        else:
            carry = (True, dbits(exact[b]), 0)
            events += 1
        ev, E, s = carry
        if s == 0:
            v = bits_to_d(E) if ev else 0.0
        else:
            assert ev, "a non-zero plain record before any event"
            K = ((E & MASK) | (1 << 52)) + s
            assert K < (1 << 53)
            v = bits_to_d((E & ~MASK) | (K & MASK))
        ends.append(v)
        start = exact[b]
    return ends, exact, events


def inputs(ob):
    n = 14
    i = np.arange(1 << n, dtype=np.float64)
    cross = np.zeros(2 << n); cross[0::2] = 2.0 ** (-30 + i / 1024.0)            # binade crossings inside records
    ties = np.zeros(2 << n); ties[0] = 1.0; ties[2::2] = 2.0 ** -27; ties[3::2] = 2.0 ** -27   # every addition a tie
    mixed = np.zeros(2 << n); mixed[0] = 1.0; mixed[2::4] = 2.0 ** -27; mixed[3::4] = 2.0 ** -27; mixed[4::4] = 2.0 ** -26
    spikes = ob.random_state(n, 13); spikes[0:64] = 1e-160; spikes[2 * 5000] = 0.9; spikes[2 * 9000 + 1] = -0.7
    sparse = np.zeros(2 << n); sparse[2 * 9001] = 0.6; sparse[2 * 9001 + 1] = 0.8
    rs = np.random.RandomState(3)
    wild = ob.random_state(n, 9) * np.repeat(10.0 ** rs.uniform(-9, 0, 1 << n), 2)
    return dict(dense=ob.random_state(n, 40), cross=cross, ties=ties, mixed=mixed, spikes=spikes, sparse=sparse, wild=wild,
                zero=np.zeros(2 << n))


@pytest.mark.parametrize("rlog", [0, 4, 8, 11])
def test_assembled_record_ends_are_the_sequential_sums(ob, rlog):
    for name, a in inputs(ob).items():
        ends, exact, events = twin_ends(ob, a, rlog)
        got = np.array(ends).view(np.uint64)
        want = np.array(exact).view(np.uint64)
        assert np.array_equal(got, want), f"{name}, records of 2^{rlog}: first difference at {np.argmax(got != want)}"
        if name == "dense" and rlog == 8:
            assert events < len(ends) // 2, "the twin found (almost) no plain records: the test shows nothing"


def test_cli_sample_flag_arguments():
    subprocess.run(["make", "-C", os.path.join(ROOT, "quantumcomputer_amd", "csrc"), "-s"], check=True)
    subprocess.run(["make", "-C", os.path.join(ROOT, "host"), "-s"], check=True)
    exe = os.path.join(ROOT, "host", "qcx_shor")
    p = subprocess.run([exe, "-C", "15", "-L", "3", "-M", "4", "-H", "500"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 2 and "needs a trial integer" in p.stderr and "[-H shots]" in p.stdout
    for bad in ("0", "x", "12y"):
        p = subprocess.run([exe, "-C", "15", "-L", "3", "-M", "4", "-a", "7", "-H", bad], capture_output=True, text=True, timeout=60)
        assert p.returncode == 2 and "positive number of shots" in p.stderr
