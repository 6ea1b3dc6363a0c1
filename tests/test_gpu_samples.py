"""GPU: many measurement shots from one state in one scan (qcx_sample_states, K4d).  Every shot's index must be, bit for bit,
the reference's decision on the UNCOLLAPSED state for its draw r (oracle: orc_measure_range on a copy), whatever the input: ties
at half an ulp, binade crossings inside records, subnormal starts, spikes larger than the running sum, sparse states, and r on
and next to partial sums, repeated, unsorted, <= 0, above the total, NaN.  The state -- and every lazy form of it -- must be left
exactly as it was, and the fast path must read the state once for all shots."""
import ctypes as C
import json
import math
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(params=[0, 8, 9, 10, 13], ids=lambda b: f"record=2^{b}" if b else "record=auto")
def force_parallel(qc, request):
    """the parallel scan even on small registers, with every record size (0: chosen from the register size)"""
    old = {k: qc.lib().qcx_tune_get(k.encode()) for k in ("meas_parallel", "meas_min_log2", "meas_block_log")}
    qc.tune(meas_parallel=1, meas_min_log2=10, meas_block_log=request.param)
    yield
    qc.tune(**old)


@pytest.fixture
def tuned(qc):
    """set knobs for one test, put them back afterwards"""
    saved = {}

    def set_(**kv):
        for k in kv:
            saved.setdefault(k, qc.lib().qcx_tune_get(k.encode()))
        qc.tune(**kv)
    yield set_
    qc.tune(**saved)


def compact_measures(qc, reg):
    v = C.c_ulong(0)
    assert qc.lib().qcx_compact_measure_stats(reg._h, C.byref(v)) == 0
    return int(v.value)


def oracle_index(ob, a, n, r):
    dim = 1 << n
    hit, idx, _ = ob.measure_range(a, 0, dim, dim - 1, 0.0, float(r))
    return idx if hit else dim - 1


def thresholds(a, rs, k=8):
    """r on partial sums and their neighbours, duplicates, unsorted, 0, negative, 1.0, above the total, NaN"""
    p = (a.reshape(-1, 2) ** 2).sum(axis=1)
    cum = np.cumsum(p)
    tot = float(cum[-1])
    out = [0.0, -0.0, -1.0, -1e-300, 1.0, 0.5, 1e-9, 0.999999999, tot, np.nextafter(tot, 0.0), tot * 1.5, 2.0, float("nan"),
           float("inf"), float("-inf")]
    for i in rs.randint(0, cum.size, k):
        out += [float(cum[i]), float(np.nextafter(cum[i], 0.0)), float(np.nextafter(cum[i], 2.0))]
    out += list(rs.uniform(0, tot, 8))
    out += out[15:21]                              # duplicates
    rs.shuffle(out)                                # unsorted
    return out


def check_sample(qc, ob, n, a, rvals, expect_fast=True):
    a = np.ascontiguousarray(a, dtype=np.float64)
    want = [oracle_index(ob, a, n, r) for r in rvals]
    with qc.Register(n, 0) as reg:
        reg.write(a)
        before = bits(reg.read())
        got = qc.sample_states(reg, rvals)
        assert got.dtype == np.uint64 and got.shape == (len(rvals),)
        bad = [(r, int(g), w) for r, g, w in zip(rvals, got, want) if int(g) != w]
        assert not bad, f"n={n}: (r, got, want) {bad[:6]}"
        scans, fb = reg.sample_stats()
        if expect_fast:
            assert (scans, fb) == (1, 0), (scans, fb)
        assert np.array_equal(bits(reg.read()), before)
    return got


@pytest.mark.parametrize("n", [14, 17, 20])
def test_dense_random_states(qc, ob, force_parallel, n):
    rs = np.random.RandomState(n)
    a = ob.random_state(n, 40 + n)
    check_sample(qc, ob, n, a, thresholds(a, rs))


def test_uniform_superposition_and_sparse_states(qc, ob, force_parallel):
    n = 18
    a = np.zeros(2 << n); a[0::2] = 2.0 ** (-n / 2)
    k = [0, 1, 2, 1000, (1 << n) - 2, (1 << n) - 1]
    check_sample(qc, ob, n, a, [x / float(1 << n) for x in k] + [0.3, 0.7, 1.0, 1.5, 0.0, float("nan")])
    b = np.zeros(2 << n); b[2] = 1.0                                # the reset state, written
    check_sample(qc, ob, n, b, [0.0, 0.3, 1.0, 1.1, 1e-300])
    c = np.zeros(2 << n); c[2 * 200001] = 0.6; c[2 * 200001 + 1] = 0.8   # one amplitude far inside
    check_sample(qc, ob, n, c, [1e-300, 0.3, 1.0, 0.36, 1.0000001])
    d = np.zeros(2 << n)                                            # all zero: every r > 0 falls through
    check_sample(qc, ob, n, d, [0.5, 0.0, 1e-320])
    e = np.zeros(2 << n); e[-2] = 1.0                               # weight only on the excluded last index
    check_sample(qc, ob, n, e, [0.5, 0.0, 1.0])


def test_half_ulp_ties_round_to_even(qc, ob, force_parallel):
    n = 16
    a = np.zeros(2 << n); a[0] = 1.0
    a[2::2] = 2.0 ** -27; a[3::2] = 2.0 ** -27                      # p = 2^-53 after p0 = 1: every addition a tie
    check_sample(qc, ob, n, a, [1.0, 1.0 + 2.0 ** -52, 1.0 + 2.0 ** -40, 0.5, 1.0, np.nextafter(1.0, 0.0)])
    b = a.copy(); b[2::2] = 2.0 ** -26; b[3::2] = 2.0 ** -27 * math.sqrt(2)
    check_sample(qc, ob, n, b, [1.0 + 2.0 ** -45, 1.0 + 2.0 ** -38, 1.00000001, 1.0 + 2.0 ** -38])
    c = np.zeros(2 << n); c[0] = 1.0
    c[2::4] = 2.0 ** -27; c[3::4] = 2.0 ** -27
    c[4::4] = 2.0 ** -26
    check_sample(qc, ob, n, c, [1.0 + 2.0 ** -44, 1.0 + 2.0 ** -41, 1.0 + 2.0 ** -39])


def test_binade_crossings_inside_records(qc, ob, force_parallel):
    n = 16
    i = np.arange(1 << n, dtype=np.float64)
    a = np.zeros(2 << n)
    a[0::2] = 2.0 ** (-30 + i / 4096.0)                             # p doubles every 2048 elements
    tot = float(((a[0::2]) ** 2).sum())
    check_sample(qc, ob, n, a, [tot * f for f in (1e-12, 1e-6, 0.01, 0.3, 0.9, 0.999999, 1.0, 1.01)])
    rs = np.random.RandomState(3)
    b = ob.random_state(n, 9) * np.repeat(10.0 ** rs.uniform(-9, 0, 1 << n), 2)   # wild dynamic range
    check_sample(qc, ob, n, b, thresholds(b, rs))


def test_subnormal_start_and_spikes(qc, ob, force_parallel):
    n = 15
    a = ob.random_state(n, 13)
    a[0:64] = 1e-160                                                # p = 2e-320: subnormal partial sums
    a[2 * 5000] = 0.9                                               # spikes larger than the running sum
    a[2 * 20000 + 1] = -0.7
    check_sample(qc, ob, n, a, [1e-322, 4e-320, 1e-300, 0.05, 0.5, 0.81, 1.2, 1.4, 5.0, 0.0, float("nan")])


@pytest.mark.parametrize("knobs", [dict(meas_fast=0), dict(meas_dbg=2), dict(meas_parallel=0)],
                         ids=["walk-alone", "hand-over", "single-wave"])
def test_every_scan_form(qc, ob, tuned, knobs):
    """the record ends from the tree walk alone, from the event list handing over to the walk in mid-scan, and from the
    single-wave chain (a large register scanned sequentially: records of 2^11)"""
    tuned(**{**dict(meas_parallel=1, meas_min_log2=10, meas_block_log=8), **knobs})
    n = 17
    rs = np.random.RandomState(5)
    a = ob.random_state(n, 77)
    check_sample(qc, ob, n, a, thresholds(a, rs))
    i = np.arange(1 << n, dtype=np.float64)
    b = np.zeros(2 << n)
    b[0::2] = 2.0 ** (-30 + i / 8192.0)
    tot = float(((b[0::2]) ** 2).sum())
    check_sample(qc, ob, n, b, [tot * f for f in (1e-12, 1e-6, 0.01, 0.3, 0.9, 0.999999, 1.0, 1.01)])


@pytest.mark.parametrize("n", [3, 9, 11])
def test_small_registers_single_wave(qc, ob, n):
    """below meas_min_log2 the single-wave chain stores every amplitude's running sum"""
    rs = np.random.RandomState(n)
    a = ob.random_state(n, 3 + n)
    check_sample(qc, ob, n, a, thresholds(a, rs, 4))


def test_more_shots_than_one_batch(qc):
    """2^20 + 3 shots: the draws go to the device a batch of 2^20 at a time, so the last three are a second batch.  On the
    uniform superposition of n = 12 every partial sum is exact (k / 4096), so the reference needs no scan: the first index whose
    partial sum is >= r among all but the last, else the last index (numpy's searchsorted)"""
    n, shots = 12, (1 << 20) + 3
    dim = 1 << n
    a = np.zeros(2 * dim); a[0::2] = 2.0 ** (-n / 2)
    cum = np.arange(1, dim, dtype=np.float64) / dim                 # the partial sums behind the indices 0 .. dim - 2
    assert np.array_equal(cum, np.cumsum(np.full(dim, a[0] * a[0]))[:-1]), "exact partial sums"
    rs = np.random.RandomState(5)
    r = rs.uniform(0.0, 1.0, shots)
    edges = np.array([0.0, 1.0, 1.5, 1e-300, -0.25, 0.5, np.nextafter(0.5, 0.0), np.nextafter(0.5, 1.0), cum[0], cum[-1],
                      np.nextafter(cum[-1], 1.0), np.nextafter(cum[-1], 0.0), 1777.0 / dim])
    r[rs.choice(1 << 20, edges.size, replace=False)] = edges        # in the first batch ...
    r[-3:] = [np.nextafter(0.5, 1.0), 1777.0 / dim, 1.0]            # ... and as the whole of the second
    want = np.minimum(np.searchsorted(cum, r, side="left"), dim - 1).astype(np.uint64)
    with qc.Register(n, 0) as reg:
        reg.write(a)
        got = qc.sample_states(reg, r)
        assert reg.sample_stats() == (1, 0), reg.sample_stats()
        assert np.array_equal(bits(reg.read()), bits(a)), "the state changed"
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} shots differ, first (shot, r, got, want): {[(int(i), r[i], int(got[i]), int(want[i])) for i in bad[:6]]}"
    assert got[-3:].tolist() == [dim // 2, 1776, dim - 1] and len(set(got.tolist())) == dim, "every index is hit, the second batch included"


def test_state_untouched_and_measure_afterwards(qc, ob):
    n = 20
    rs = np.random.RandomState(1)
    with qc.Register(n, 0) as reg, qc.Register(n, 0) as fresh:
        reg.fill_random(11)
        fresh.fill_random(11)
        before = bits(reg.read())
        tp = reg.total_probability()
        qc.sample_states(reg, list(rs.uniform(0, 1, 300)))
        assert np.array_equal(bits(reg.read()), before)
        assert reg.total_probability() == tp
        assert qc.measure_state(reg, 0.61803) == qc.measure_state(fresh, 0.61803)
        assert np.array_equal(bits(reg.read()), bits(fresh.read()))


def test_compact_result_stays_compact(qc, ob):
    """right behind quantum_computation the result is compact with its last pass deferred: sampling scans it there (one
    compact measurement more), and read / measure_state afterwards still give the oracle's bits"""
    L, M, Cn, a = 15, 5, 21, 2                                      # (the compact chain runs from n = 20 on: fuse_chain_min_n)
    n = L + M
    want = np.zeros(2 << n); ob.reset(want, n); ob.quantum_computation(want, n, M, Cn, a, threads=8)
    rs = np.random.RandomState(2)
    rvals = thresholds(want, rs)
    with qc.Register(L, M) as reg:
        qc.reset_register(reg); qc.quantum_computation(Cn, a, reg)
        c0 = compact_measures(qc, reg)
        got = qc.sample_states(reg, rvals)
        assert compact_measures(qc, reg) == c0 + 1, "the sample call did not scan the compact form"
        assert [int(g) for g in got] == [oracle_index(ob, want, n, r) for r in rvals]
        assert reg.sample_stats() == (1, 0)
        got2 = qc.sample_states(reg, rvals)                         # still compact: the same answers, one more compact scan
        assert np.array_equal(got, got2) and compact_measures(qc, reg) == c0 + 2
        r = 0.377
        assert qc.measure_state(reg, r) == oracle_index(ob, want, n, r)
        w = want.copy(); ob.measure(w, n, r)
        assert np.array_equal(bits(reg.read()), bits(w))
    with qc.Register(L, M) as reg:                                  # and read() straight after a sample call
        qc.reset_register(reg); qc.quantum_computation(Cn, a, reg)
        qc.sample_states(reg, [0.25, 0.75])
        assert np.array_equal(bits(reg.read()), bits(want))


def test_pending_basis_state_and_queued_gates(qc, ob):
    n = 14
    with qc.Register(n - 4, 4) as reg:
        qc.reset_register(reg)                                      # pending basis state |1>
        got = qc.sample_states(reg, [0.0, -1.0, 0.5, 1.0, np.nextafter(1.0, 2.0), float("nan"), 1e-300])
        assert [int(g) for g in got] == [0, 0, 1, 1, (1 << n) - 1, (1 << n) - 1, 1]
        assert reg.sample_stats() == (0, 0)                         # answered without a scan: nothing was written
        want = np.zeros(2 << n); ob.reset(want, n)
        assert np.array_equal(bits(reg.read()), bits(want))
        qc.measure_state(reg, 0.5)                                  # a collapse: pending basis state 1 again
        assert qc.sample_states(reg, [0.5]).tolist() == [1]
        # fusion 1: gates queued and not flushed -- the sample call observes the state, so they run first
        reg.set_fusion(1)
        qc.reset_register(reg)
        for q in (0, 3, n - 1):
            qc.hadamard_gate(q, reg)
        qc.c_phase_shift_gate(3, n - 1, 0.7, reg)
        for q in (0, 3, n - 1):
            ob.hadamard(want, n, q)
        ob.cphase(want, n, 3, n - 1, 0.7)
        rs = np.random.RandomState(4)
        rvals = thresholds(want, rs, 4)
        got = qc.sample_states(reg, rvals)
        assert [int(g) for g in got] == [oracle_index(ob, want, n, r) for r in rvals]
        assert np.array_equal(bits(reg.read()), bits(want))


def test_nonfinite_register(qc, ob):
    """Inf / NaN written through qcx_state_write: every shot takes its own exact scan; the flag (strict gates) is kept"""
    n = 13
    a = ob.random_state(n, 21)
    a[2 * 700] = np.inf
    a[2 * 3000 + 1] = np.nan
    rvals = [0.0, -1.0, 1e-6, 0.001, 0.5, 2.0, float("nan")]
    with qc.Register(n, 0) as reg:
        reg.write(a)
        before = bits(reg.read())
        got = qc.sample_states(reg, rvals)
        assert [int(g) for g in got] == [oracle_index(ob, a, n, r) for r in rvals]
        assert reg.sample_stats() == (len(rvals), len(rvals))
        assert np.array_equal(bits(reg.read()), before)
        qc.hadamard_gate(2, reg)                                    # still the strict gate: the oracle's products, NaN/Inf included
        w = a.copy(); ob.hadamard(w, n, 2)
        got = reg.read()
        gn, wn = np.isnan(got), np.isnan(w)
        assert np.array_equal(gn, wn)                               # (NaN payloads aside: bit for bit)
        assert np.array_equal(bits(got[~gn]), bits(w[~wn]))


def test_arguments(qc):
    lib = qc.lib()
    with qc.Register(12, 0) as reg:
        reg.fill_random(1)
        rng = qc.Rng(9)
        out = (C.c_ulong * 4)()
        assert lib.qcx_sample_states(reg._h, rng._h, 0, None) == 0          # nothing, and no draw
        assert lib.qcx_sample_states(reg._h, rng._h, 4, None) == 2          # QCX_BAD_ARGUMENTS
        assert lib.qcx_sample_states_r(reg._h, None, 4, out) == 2
        assert lib.qcx_sample_states_r(None, None, 4, out) == 2
        assert rng.uniform() == qc.Rng(9).uniform()
        with pytest.raises(ValueError):
            qc.sample_states(reg, rng)
    with qc.Register(13, 0, shards=4, devices=qc.spread_devices(4)) as sh:
        rng = qc.Rng(9)
        assert lib.qcx_sample_states(sh._h, rng._h, 4, out) == 7           # QCX_UNSUPPORTED, no draw made
        assert lib.qcx_sample_states_r(sh._h, (C.c_double * 1)(0.5), 1, out) == 7
        assert rng.uniform() == qc.Rng(9).uniform()


def rounds(qc, L, M, Cn, a, seed, shots, fusion=0):
    rng = qc.Rng(seed)
    out = []
    with qc.Register(L, M) as reg:
        reg.set_fusion(fusion)
        for _ in range(shots):
            qc.reset_register(reg)
            qc.quantum_computation(Cn, a, reg)
            out.append(qc.measure_state(reg, rng))
    return out


def test_pinned_histogram_through_the_sample_path(qc, ob):
    """the reference's seeded 500-shot histogram (tests/golden): one circuit, 500 samples"""
    L, M = 3, 4
    with qc.Register(L, M) as reg:
        qc.reset_register(reg)
        qc.quantum_computation(15, 7, reg)
        got = qc.sample_states(reg, qc.Rng(12345), 500)
        omegas = [qc.read_omega(int(i), reg) for i in got]
    counts = {w: omegas.count(w) for w in sorted(set(omegas))}
    assert counts == {0.0: 123, 0.25: 113, 0.5: 127, 0.75: 137}
    assert [int(i) for i in got] == rounds(qc, L, M, 15, 7, 12345, 500)


@pytest.mark.parametrize("fusion", [-1, 0, 1, 2])
def test_shots_equal_rounds_n20(qc, fusion):
    L, M, Cn, a = 15, 5, 21, 2
    with qc.Register(L, M) as reg:
        reg.set_fusion(fusion)
        qc.reset_register(reg)
        qc.quantum_computation(Cn, a, reg)
        got = qc.sample_states(reg, qc.Rng(777), 200)
        assert reg.sample_stats() == (1, 0)
    assert [int(i) for i in got] == rounds(qc, L, M, Cn, a, 777, 200, fusion)


def test_cli_histogram(qc):
    subprocess.run(["make", "-C", os.path.join(ROOT, "host"), "-s"], check=True)
    exe = os.path.join(ROOT, "host", "qcx_shor")
    p = subprocess.run([exe, "-C", "15", "-L", "3", "-M", "4", "-a", "7", "-s", "12345", "-H", "500", "-j"],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    line = [x for x in p.stdout.splitlines() if x.startswith("{")][-1]
    j = json.loads(line)
    assert j["shots"] == 500 and j["attempts"] == 1
    assert j["histogram"] == {"0": 123, "2": 113, "4": 127, "6": 137}
    assert 0 <= j["valid_period_shots"] <= 500
    assert " --- x~ = 6, omega = 0.7500000000: 137 shots" in p.stdout


def test_one_read_for_1024_shots_n24(qc, ob):
    n = 24
    rs = np.random.RandomState(24)
    rvals = list(rs.uniform(0, 1, 1024))
    with qc.Register(n, 0) as reg:
        reg.fill_random(5)
        got = qc.sample_states(reg, rvals)
        assert reg.sample_stats() == (1, 0)
        for k in range(0, 1024, 128):                               # a few against the per-shot measurement
            reg.fill_random(5)
            assert int(got[k]) == qc.measure_state(reg, rvals[k])
    L, M = 19, 5
    with qc.Register(L, M) as reg:
        qc.reset_register(reg); qc.quantum_computation(21, 2, reg)
        got = qc.sample_states(reg, qc.Rng(31), 1024)
        assert reg.sample_stats() == (1, 0)
        assert [int(i) for i in got[:6]] == rounds(qc, L, M, 21, 2, 31, 6)
        near = [min(abs(qc.read_omega(int(i), reg) - k / 6.0) for k in range(7)) < 2.0 ** -12 for i in got]
        assert sum(near) > 0.8 * len(near)                         # the period shows: most shots sit on a multiple of 1/6


def test_n30_against_per_shot_scans(qc):
    """the maximum size of one run in the style of test_gpu_maxsize.py: a handful of shots against the measurement scan itself"""
    n = 30
    rvals = [0.1, 0.5, 0.73, 0.999999, 0.5, 1e-12, 2.0]
    with qc.Register(n, 0) as reg:
        reg.fill_random(30)
        got = qc.sample_states(reg, rvals)
        assert reg.sample_stats() == (1, 0)
        ptr = reg.device_pointer()
        for r, g in zip(rvals, got):
            found, index, cum = C.c_int(0), C.c_uint64(0), C.c_double(0.0)
            assert qc.lib().qcx_shard_measure_scan(ptr, n, 0, (1 << n) - 1, 0.0, float(r), C.byref(found), C.byref(index),
                                                   C.byref(cum), None) == 0
            assert int(g) == (int(index.value) if found.value else (1 << n) - 1), r
