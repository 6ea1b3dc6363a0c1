"""CPU: tests/exact_ref.py, the extended-precision truth behind the tolerance mode's accuracy criterion, and the criterion itself.

1. the reference against mpmath at 50 digits, on registers small enough for plain Python loops: agreement to 2^-56;
2. the oracle is double-accurate: at most four roundings per component per gate, e(oracle) <= 4 G 2^-53, on every shape the GPU
   tests use at n <= 16 and one at n = 18;
3. the criterion is sharp: the oracle's own double-precision gate sequence with ONE defect is rejected by
   assert_as_accurate_as_oracle and accepted by the bound the suite had before, max |delta| <= 1e-12 -- the gap it closes."""
import math

import mpmath
import numpy as np
import pytest

import exact_ref as er
import tolerance_cases as tc
import tolerance_twin as tt

TOL = 1e-12                                   # the old bound (tests/test_gpu_tolerance_mode.TOL)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def max_delta(a, b):
    d = np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)
    return float(np.max(np.hypot(d[0::2], d[1::2])))


# ---- 1. against mpmath ---------------------------------------------------------------------------------------------------------

def mp_truth(pairs, n, M, steps):
    """the same gates in mpmath (mp.dps = 50), plain loops over the 2^n amplitudes"""
    mp = mpmath.mp
    z = [mpmath.mpc(mpmath.mpf(float(pairs[2 * i])), mpmath.mpf(float(pairs[2 * i + 1]))) for i in range(1 << n)]
    s = 1 / mpmath.sqrt(mpmath.mpf(2))
    for st in steps:
        if st[0] == "h":
            b = 1 << st[1]
            for i in range(1 << n):
                if not i & b:
                    a0, a1 = z[i], z[i | b]
                    z[i], z[i | b] = (a0 + a1) * s, (a0 - a1) * s
        elif st[0] == "p":
            both = (1 << st[1]) | (1 << st[2])
            w = mpmath.expj(mpmath.mpf(float(st[3])))
            for i in range(1 << n):
                if i & both == both:
                    z[i] = z[i] * w
        else:
            Cn, atox, ctl = st[1:]
            out = [mpmath.mpc(0)] * (1 << n)
            for k in range(1 << n):
                f = k & ((1 << M) - 1)
                j = k
                if (k >> ctl) & 1 and f < Cn:
                    j = (k - f) | (((atox % Cn) * f) % Cn)
                out[j] = out[j] + z[k]
            z = out
    assert mp.dps == 50
    return z


def to_longdouble(z):
    out = np.empty(len(z), dtype=er.CLD)
    out.real = [er.LD(mpmath.nstr(v.real, 30)) for v in z]
    out.imag = [er.LD(mpmath.nstr(v.imag, 30)) for v in z]
    return out


def agreement(T, Z):
    """rel_errors of the long-double truth T against the mpmath result Z (both numbers of exact_ref.rel_errors)"""
    d, t = np.abs(T - Z), np.abs(Z)
    return float(d.max() / t.max()), float(np.sqrt(np.sum(d * d)) / np.sqrt(np.sum(t * t)))


def small_program(rs, n, M, Cn, length):
    steps = []
    for _ in range(length):
        k = rs.randint(0, 10)
        if k < 4:
            steps.append(("h", int(rs.randint(0, n))))
        elif k < 8:
            c, t = (int(v) for v in rs.choice(n, 2, replace=False))
            steps.append(("p", c, t, float(rs.uniform(-3, 3)) if k % 2 else math.pi / (1 << int(rs.randint(1, 30)))))
        else:
            steps.append(("c", Cn, int(rs.randint(1, 4 * Cn)), int(rs.randint(M, n))))
    return steps


MP_CASES = [("iqft n=1", 1, 0, er.iqft_steps(1, 0), 5), ("iqft n=3", 3, 0, er.iqft_steps(3, 0), 5), ("iqft n=4 M=1", 4, 1, er.iqft_steps(4, 1), 6),
            ("iqft n=5", 5, 0, er.iqft_steps(5, 0), 7), ("iqft n=5 M=2", 5, 2, er.iqft_steps(5, 2), 8),
            ("program", 6, 3, small_program(np.random.RandomState(5), 6, 3, 7, 40), 9),
            ("program, multiplies that are no permutation", 6, 3, small_program(np.random.RandomState(6), 6, 3, 6, 40), 10),
            ("shor 15/3/4", 7, 4, er.qcomp_steps(15, 7, 3, 4), None)]


@pytest.mark.parametrize("name,n,M,steps,seed", MP_CASES, ids=[c[0] for c in MP_CASES])
def test_reference_against_mpmath(ob, name, n, M, steps, seed):
    """about 130 long-double roundings of 2^-63 are allowed, far more than 15 to 40 gates can accumulate, and still an eighth of a
    double rounding"""
    if name.startswith("program"):
        assert any(s[0] == "c" for s in steps)
    start = er.basis_state(n, 1) if seed is None else ob.random_state(n, seed)
    with mpmath.workdps(50):
        Z = to_longdouble(mp_truth(start, n, M, steps))
    T = er.truth(start, n, M, steps)
    e = agreement(T, Z)
    print(f"{name}: {len(steps)} gates, long double against mpmath {e[0]:.3e} (max), {e[1]:.3e} (2-norm)")
    assert max(e) <= 2.0 ** -56, e


@pytest.mark.parametrize("n,M", [(3, 0), (5, 0), (5, 2)])
def test_basis_chain_against_mpmath_and_the_dense_truth(n, M):
    for x in range(1 << n):
        W = er.basis_iqft_window(x, n, M, 0, 1 << n)
        T = er.truth(er.basis_state(n, x), n, M, er.iqft_steps(n, M))
        assert np.array_equal(W, T), x                     # the same operations on the one non-zero member of every pair
    x = (1 << n) - 2
    with mpmath.workdps(50):
        Z = to_longdouble(mp_truth(er.basis_state(n, x), n, M, er.iqft_steps(n, M)))
    assert max(agreement(er.basis_iqft_window(x, n, M, 0, 1 << n), Z)) <= 2.0 ** -56
    assert np.array_equal(er.basis_iqft_window(x, n, M, 3, 4), er.basis_iqft_window(x, n, M, 0, 1 << n)[3:7])


def test_rel_errors_and_the_criterion_on_made_up_numbers():
    T = np.array([3 + 4j, 0, 1j, -1], dtype=er.CLD)
    got = np.array([3.0, 4.0, 0.0, 0.0, 0.0, 1.0, -1.0, 0.0])
    assert er.rel_errors(got, T) == (0.0, 0.0)
    got[0] += 5e-3
    e = er.rel_errors(got, T)
    assert abs(e[0] - 1e-3) < 1e-15 and abs(e[1] - 5e-3 / math.sqrt(27)) < 1e-15
    assert er.rel_errors(got, T, where=np.array([False, True, True, True])) == (0.0, 0.0)
    exact = np.array([3.0, 4.0, 0.0, 0.0, 0.0, 1.0, -1.0, 0.0])
    er.assert_as_accurate_as_oracle(exact, got, T, "better than the oracle")
    er.assert_as_accurate_as_oracle(got, got, T, "the oracle against itself")
    with pytest.raises(AssertionError, match="max norm"):
        er.assert_as_accurate_as_oracle(got, exact, T, "worse than an exact oracle")
    worse = exact.copy(); worse[0] += 1.01e-2
    with pytest.raises(AssertionError):
        er.assert_as_accurate_as_oracle(worse, got, T, "more than MARGIN times the oracle's error")
    # the floor: an oracle that is exact allows one double rounding times MARGIN, no more
    near = exact.copy(); near[0] = np.nextafter(3.0, 4.0)
    er.assert_as_accurate_as_oracle(near, exact, T, "one ulp of the largest amplitude")
    far = exact.copy(); far[0] = 3.0 + 8 * np.spacing(3.0)
    with pytest.raises(AssertionError):
        er.assert_as_accurate_as_oracle(far, exact, T, "eight ulps")
    # a truth that is all zeros (a window of a collapsed state): exact zeros pass, anything else does not
    zeros = np.zeros(3, dtype=er.CLD)
    assert er.rel_errors(np.zeros(6), zeros) == (0.0, 0.0)
    er.assert_as_accurate_as_oracle(np.zeros(6), np.zeros(6), zeros, "zeros")
    with pytest.raises(AssertionError):
        er.assert_as_accurate_as_oracle(np.array([0.0, 0.0, 1e-300, 0.0, 0.0, 0.0]), np.zeros(6), zeros, "not quite zeros")
    assert er.MARGIN == 2.0 and er.FLOOR == 2.0 ** -52


# ---- 2. the oracle is double-accurate ------------------------------------------------------------------------------------------

def check_oracle(what, want, T, G):
    e = er.rel_errors(want, T)
    bound = 4 * G * 2.0 ** -53
    print(f"{what}: {G} gates, e(oracle) = {e[0]:.3e} (max) {e[1]:.3e} (2-norm), bound {bound:.3e}")
    assert max(e) <= bound, (what, e, bound)


@pytest.mark.parametrize("n,M", tc.IQFT_SHAPES + [(12, 3), (14, 0), (18, 0)])
def test_oracle_is_double_accurate_on_the_inverse_qft(ob, n, M):
    seed = tc.IQFT_SEED
    want, T, G = tc.iqft_case(ob, n, M, seed)
    assert G == (n - M) * (n - M + 1) // 2
    w = ob.fill_random(n, seed); ob.iqft(w, n, M)
    assert np.array_equal(bits(w), bits(want)), "the gate list is the oracle's inverse_QFT"
    check_oracle(f"iQFT n={n} M={M}", want, T, G)
    if (n, M) in tc.RADIX8_SHAPES or (n, M) == tc.SWITCH_SHAPE:        # the same shapes under the seeds of the other tests
        for seed in {tc.RADIX8_SEED, tc.SWITCH_SEED}:
            check_oracle(f"iQFT n={n} M={M} seed {seed}", *tc.iqft_case(ob, n, M, seed))


@pytest.mark.parametrize("Cn,L,M,a", tc.SHOR_SHAPES)
def test_oracle_is_double_accurate_on_the_shor_circuit(ob, Cn, L, M, a):
    n = L + M
    want, T, G = tc.shor_case(ob, Cn, L, M, a)
    w = np.zeros(2 << n); ob.reset(w, n); ob.quantum_computation(w, n, M, Cn, a)
    assert np.array_equal(bits(w), bits(want)), "the gate list is the oracle's quantum_computation"
    check_oracle(f"Shor {Cn}/{L}/{M}", want, T, G)


@pytest.mark.parametrize("seed", tc.PROGRAM_SEEDS)
def test_oracle_is_double_accurate_on_the_random_programs(ob, seed):
    n = tc.random_program(seed)[0]
    assert n <= 18
    check_oracle(f"program {seed} (n = {n})", *tc.program_case(ob, seed))


def test_oracle_is_double_accurate_on_the_run_merge_edges(ob):
    check_oracle("edges", *tc.edge_case(ob))


TWIN_CASES = [(p, s) for p in tt.PREFIX_KINDS for s in tt.SHAPES if tt.prefix_is_legal(p, s)]


@pytest.mark.parametrize("kind,shape", TWIN_CASES, ids=[tt.key_of(p, s) for p, s in TWIN_CASES])
def test_oracle_is_double_accurate_on_the_twin_prefixes(ob, kind, shape):
    """the prefixes of tests/tolerance_twin.py (n <= 16), whose mode-2 state S is held to the criterion on the GPU"""
    n, M = shape[0] + shape[1], shape[1]
    prefix = tt.prefix_ops(kind, shape)
    G = len(tt.gate_steps(n, M, [op for op in prefix if op[0] in tt.GATE_OPS]))
    check_oracle(tt.key_of(kind, shape), tt.oracle_state(ob, kind, shape)[0], tt.truth_of(ob, shape, prefix), G)


# ---- 3. the criterion is sharp -------------------------------------------------------------------------------------------------

def cphase_polar(a, n, c, t, er_, ei_):
    """orc_pair_cphase with the factor given, not computed: the oracle's sums, so that with the oracle's own (cos, sin) the bits
    are its bits (asserted below)"""
    re, im = a[0::2].copy(), a[1::2].copy()
    idx = np.arange(1 << n)
    sel = (((idx >> c) & 1) == 1) & (((idx >> t) & 1) == 1)
    one, z = np.float64(1.0), np.float64(0.0)
    nr = np.where(sel, 0.0 + ((er_ * re) - (ei_ * im)), 0.0 + ((one * re) - (z * im)))
    ni = np.where(sel, 0.0 + ((er_ * im) + (ei_ * re)), 0.0 + ((one * im) + (z * re)))
    a[0::2], a[1::2] = nr, ni


def run_with(ob, n, M, steps, seed, replace):
    """the oracle's double-precision gate sequence; replace: {position: a callable that applies something else there, or None
    to drop the gate}"""
    a = ob.fill_random(n, seed)
    for k, s in enumerate(steps):
        if k in replace:
            if replace[k] is not None:
                replace[k](a)
        elif s[0] == "h":
            ob.hadamard(a, n, s[1])
        else:
            ob.cphase(a, n, s[1], s[2], s[3])
    return a


def rejected_and_formerly_accepted(bad, want, T, what):
    with pytest.raises(AssertionError, match="relative error"):
        er.assert_as_accurate_as_oracle(bad, want, T, what)
    old = max_delta(bad, want)
    g, o = er.rel_errors(bad, T), er.rel_errors(want, T)
    print(f"{what}: old measure {old:.3e} (<= 1e-12), relative error {g[0]:.3e} / {g[1]:.3e}, the oracle's {o[0]:.3e} / {o[1]:.3e}")
    assert old <= TOL, f"{what}: the old bound would have caught it ({old:.3e})"
    return g, o


@pytest.mark.parametrize("n,M", tc.IQFT_SHAPES + [(18, 0)])
def test_clean_run_passes_and_an_angle_off_by_1e_13_is_rejected(ob, n, M):
    """defect 1: one angle of the top ladder off by 1e-13 rad.  The state moves by some 1e-15 absolute -- a thousand times inside
    1e-12 -- and by 6e-14 to 7e-14 of the largest amplitude, twenty times the threshold"""
    seed = tc.IQFT_SEED
    want, T, G = tc.iqft_case(ob, n, M, seed)
    steps = er.iqft_steps(n, M)
    clean = run_with(ob, n, M, steps, seed, {})
    assert np.array_equal(bits(clean), bits(want))
    er.assert_as_accurate_as_oracle(clean, want, T, "the oracle against itself")
    pos = 1                                                   # H(n-1), then the first phase of its ladder: pi / 2
    assert steps[pos][:2] == ("p", n - 1)
    c, t, th = steps[pos][1:]
    bad = run_with(ob, n, M, steps, seed, {pos: lambda a: ob.cphase(a, n, c, t, th + 1e-13)})
    g, o = rejected_and_formerly_accepted(bad, want, T, f"iQFT n={n} M={M}, one angle off by 1e-13")
    assert g[0] >= 10 * er.MARGIN * max(o[0], er.FLOOR), "caught by a factor of ten or more"


def float32_k(n):
    """the smallest k at which a phase of angle pi / 2^k with its (cos, sin) rounded to float32 still passes 1e-12 absolute.
    Below theta = 2^-12 the float32 cosine is 1, off by theta^2 / 2; the sine is off by at most theta 2^-25.  The amplitudes of
    these states are at most 6 / 2^(n/2) (Gaussian with deviation 2^-(n+1)/2 per component: six deviations of the modulus)"""
    k = 13
    while (6.0 / 2.0 ** (n / 2)) * ((math.pi / 2.0 ** k) ** 2 / 2 + (math.pi / 2.0 ** k) * 2.0 ** -25) > TOL / 2:
        k += 1
    return k


@pytest.mark.parametrize("n,M", tc.IQFT_SHAPES)
def test_a_phase_rounded_to_float32_is_rejected(ob, n, M):
    """defect 2: the (cos, sin) of one phase rounded to float32.  On the angles these ladders hold (down to pi / 2^15) the float32
    cosine is off by up to 3e-8 and the old bound sees it too; the gap opens at the angles a LONGER ladder holds, where the
    float32 cosine is 1.  So the circuit is the inverse QFT with one more phase pi / 2^k behind the top ladder, on (n-1, M), for
    the oracle, the truth and the defective run alike; the defect is the rounding alone"""
    seed, k = tc.IQFT_SEED, float32_k(n)
    assert 17 <= k <= 22
    theta = math.pi / float(1 << k)
    steps = er.iqft_steps(n, M)
    pos = n - M                                               # behind H(n-1) and its n-M-1 phases
    assert steps[pos - 1][:2] == ("p", n - 1) and steps[pos][0] == "h"
    steps.insert(pos, ("p", n - 1, M, theta))
    want, T, G = tc.steps_case(ob, ("iqft+1", n, M, seed, k), lambda: ob.fill_random(n, seed), n, M, steps)
    c64, s64 = ob.polar(theta)
    same = run_with(ob, n, M, steps, seed, {pos: lambda a: cphase_polar(a, n, n - 1, M, np.float64(c64), np.float64(s64))})
    assert np.array_equal(bits(same), bits(want)), "cphase_polar is the oracle's phase"
    c32, s32 = np.float64(np.float32(c64)), np.float64(np.float32(s64))
    assert c32 == 1.0 and c32 != c64 and s32 != s64
    bad = run_with(ob, n, M, steps, seed, {pos: lambda a: cphase_polar(a, n, n - 1, M, c32, s32)})
    rejected_and_formerly_accepted(bad, want, T, f"iQFT n={n} M={M}, pi/2^{k} in float32")
    # and the other half: on an angle of the ladder itself the old bound did catch it
    pos = n - M - 1
    c, t, th = steps[pos][1:]
    assert (c, t) == (n - 1, M)
    c64, s64 = ob.polar(th)
    bad = run_with(ob, n, M, steps, seed, {pos: lambda a: cphase_polar(a, n, c, t, np.float64(np.float32(c64)), np.float64(np.float32(s64)))})
    assert max_delta(bad, want) > TOL
    with pytest.raises(AssertionError):
        er.assert_as_accurate_as_oracle(bad, want, T, "float32 on an angle of the ladder")


def basis_chain_double(ob, x, n, M, first, count, drop=None):
    """the oracle's basis_iqft_window (one scalar chain per output index, its sums in binary64) with the phase `drop` = (l, k)
    left out"""
    i = np.arange(first, first + count, dtype=np.int64)
    s, z0 = np.float64(0.70710678118654752440), np.float64(0.0)
    ar, ai, zeros = np.ones(count), np.zeros(count), np.zeros(count)
    for l in range(n - 1, M - 1, -1):
        out_l = ((i >> l) & 1) == 1
        inp = (x >> l) & 1
        lr, li = (zeros, zeros) if inp else (ar, ai)
        hr, hi = (ar, ai) if inp else (zeros, zeros)
        sh = np.where(out_l, -s, s)
        o_r = (0.0 + ((s * lr) - (z0 * li))) + ((sh * hr) - (z0 * hi))
        o_i = (0.0 + ((s * li) + (z0 * lr))) + ((sh * hi) + (z0 * hr))
        ar, ai = o_r, o_i
        for k in range(l - 1, M - 1, -1):
            if (l, k) == drop:
                continue
            sel = out_l & bool((x >> k) & 1)
            c, sn = (np.float64(v) for v in ob.polar(math.pi / float(1 << (l - k))))
            nr = np.where(sel, 0.0 + ((c * ar) - (sn * ai)), 0.0 + ((1.0 * ar) - (z0 * ai)))
            ni = np.where(sel, 0.0 + ((c * ai) + (sn * ar)), 0.0 + ((1.0 * ai) + (z0 * ar)))
            ar, ai = nr, ni
    mlow = (1 << M) - 1
    out = np.zeros(2 * count)
    keep = (i & mlow) == (x & mlow)
    out[0::2], out[1::2] = np.where(keep, ar, 0.0), np.where(keep, ai, 0.0)
    return out


def test_a_dropped_smallest_angle_phase_is_rejected(ob):
    """defect 3: the smallest-angle phase of the top ladder, pi / 2^(n-1), left out.  On a dense state at n <= 18 it moves the
    amplitudes by 2e-5 of their size or more and the old bound sees it; so the per-index chain on a basis state, one window of
    2^13, with the bound of test_config3_iqft_n28_on_basis_states_within_tolerance, 1e-12 of the amplitude 2^-(n/2).  At n = 28
    that bound rejects the drop as well (pi / 2^27 = 2.3e-8): a ladder has to be 43 qubits long before its last angle is below
    1e-12 rad.  The chain needs no 2^n array, so that is where the gap is shown; at n = 28 the criterion is shown to reject."""
    W = 13
    for n, old_accepts in ((28, False), (43, True)):
        x, first = ((1 << n) - 1) & 0x5A5A5A5A5A5 | 1, ((1 << (n - 1)) | (5 << W))
        want = ob.basis_iqft_window(x, n, 0, first, 1 << W)
        clean = basis_chain_double(ob, x, n, 0, first, 1 << W)
        assert np.array_equal(bits(clean), bits(want)), "the restated chain is the oracle's"
        T = er.basis_iqft_window(x, n, 0, first, 1 << W)
        er.assert_as_accurate_as_oracle(clean, want, T, "the clean chain")
        bad = basis_chain_double(ob, x, n, 0, first, 1 << W, drop=(n - 1, 0))
        with pytest.raises(AssertionError, match="relative error"):
            er.assert_as_accurate_as_oracle(bad, want, T, f"n = {n}: the phase pi/2^{n - 1} dropped")
        old = max_delta(bad, want) / 2.0 ** -(n / 2)
        print(f"n = {n}: the dropped phase moves the window by {old:.3e} of the amplitude scale; relative errors {er.rel_errors(bad, T)}, the oracle's {er.rel_errors(want, T)}")
        assert (old <= TOL) == old_accepts, (n, old)
