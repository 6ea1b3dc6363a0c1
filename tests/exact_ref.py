"""A plain EXTENDED-PRECISION reference of the gate set (numpy.longdouble / numpy.clongdouble, 64-bit mantissa): the truth that
neither the oracle nor the code under test had a hand in.  The tolerance mode (qcx_set_fusion(reg, 2)) is not bit-exact against
the oracle, so its tests need a bound; `max |delta| <= 1e-12` against the oracle is 10^4 to 10^5 above what correct double
arithmetic gives.  Here the bound is the oracle's OWN error against this truth:

    e(got) <= MARGIN * max(e(oracle), 2^-52)          for both numbers of rel_errors

(assert_as_accurate_as_oracle).  The gates are the ideal ones: H with 1/sqrt(2) computed in long double (not M_SQRT1_2), a
controlled phase cos(theta) + i sin(theta) of the double theta the gate receives, the modular multiply of Q:595-660 as an index
map.  tests/test_exact_ref.py checks this module against mpmath at 50 digits and shows the criterion is sharp.  Host only."""
import math

import numpy as np

LD, CLD = np.longdouble, np.clongdouble
assert np.finfo(LD).nmant >= 63, f"numpy.longdouble has a {np.finfo(LD).nmant}-bit mantissa here: no extended precision, no truth"

# the one statement of the criterion's constants.  MARGIN: the merged arithmetic measures 0.95 to 1.11 times the oracle's error
# on the CPU emulator; 2 leaves room for the max norm being an extreme value over 2^n amplitudes and for the device ordering its
# FMAs differently.  FLOOR: one double rounding, for states the oracle reaches almost exactly.
MARGIN = 2.0
FLOOR = 2.0 ** -52


def widen(pairs):
    """interleaved float64 (re, im) pairs -> clongdouble, exactly"""
    a = np.asarray(pairs, dtype=np.float64)
    z = np.empty(a.size // 2, dtype=CLD)
    z.real = a[0::2]
    z.imag = a[1::2]
    return z


def _unit(theta):
    t = LD(float(theta))                       # the double the gate receives, widened
    return CLD(np.cos(t) + 1j * np.sin(t))


def _hadamard(z, n, q):
    s = LD(1) / np.sqrt(LD(2))
    v = z.reshape(1 << (n - 1 - q), 2, 1 << q)
    a0, a1 = v[:, 0, :].copy(), v[:, 1, :].copy()
    v[:, 0, :] = (a0 + a1) * s
    v[:, 1, :] = (a0 - a1) * s


def _cphase(z, n, c, t, theta):
    hi, lo = max(c, t), min(c, t)
    v = z.reshape(1 << (n - 1 - hi), 2, 1 << (hi - lo - 1), 2, 1 << lo)
    v[:, 1, :, 1, :] *= _unit(theta)


def _camodc(z, n, M, Cn, atox, ctl):
    """Q:595-660: index k goes to j, j = k unless the control bit of k is set and f = k mod 2^M < C, then the low M bits of j are
    those of (A f) mod C, A = atox mod C.  A permutation when gcd(A, C) = 1 and C <= 2^M; amplitudes that meet are summed"""
    A = int(atox) % int(Cn)
    idx = np.arange(1 << n, dtype=np.int64)
    f = idx & ((1 << M) - 1)
    moved = (((idx >> ctl) & 1) == 1) & (f < Cn)
    dst = np.where(moved, (idx - f) | (((A * f) % Cn) & ((1 << M) - 1)), idx)
    out = np.zeros_like(z)
    if math.gcd(A, int(Cn)) == 1 and Cn <= (1 << M):
        out[dst] = z
    else:
        np.add.at(out, dst, z)
    z[:] = out


def advance(z, n, M, steps, Cn=None):
    """the gate list applied in place to a clongdouble state: ("h", q), ("p", c, t, theta), ("c", C, atox, ctl) -- or
    ("c", atox, ctl) with the modulus in Cn, as the random programs of the suite write it"""
    assert z.size == 1 << n
    for s in steps:
        if s[0] == "h":
            _hadamard(z, n, s[1])
        elif s[0] == "p":
            _cphase(z, n, s[1], s[2], s[3])
        elif s[0] == "c":
            C_, atox, ctl = s[1:] if len(s) == 4 else (Cn,) + tuple(s[1:])
            _camodc(z, n, M, C_, atox, ctl)
        else:
            raise ValueError(f"unknown step {s!r}")
    return z


def truth(pairs, n, M, steps, Cn=None):
    """the gate list applied to the state given as (re, im) pairs.  Returns clongdouble, read-only"""
    z = advance(widen(pairs), n, M, steps, Cn)
    z.setflags(write=False)
    return z


def iqft_steps(n, M):
    """inverse_QFT(n, M) (Q:678-690): for l = n-1 .. M: H(l), then the ladder of phases pi / 2^(l-k) on (l, k), k = l-1 .. M"""
    steps = []
    for l in range(n - 1, M - 1, -1):
        steps.append(("h", l))
        for k in range(l - 1, M - 1, -1):
            steps.append(("p", l, k, math.pi / float(1 << (l - k))))
    return steps


def qcomp_steps(Cn, a, L, M):
    """quantum_computation(C, a) (Q:712-737) with exact modular powers: the Hadamard layer, the multiplies by a^(2^j), the iQFT"""
    n = L + M
    steps = [("h", l) for l in range(M, n)]
    x = a % Cn
    for l in range(M, n):
        steps.append(("c", Cn, x, l))
        x = (x * x) % Cn
    return steps + iqft_steps(n, M)


def basis_state(n, x=1):
    a = np.zeros(2 << n)
    a[2 * x] = 1.0
    return a


def basis_iqft_window(x, n, M, first, count):
    """amplitudes [first, first + count) of inverse_QFT applied to |x>, one scalar chain per output index (the oracle's
    basis_iqft_window in long double): every Hadamard meets a pair with one non-zero member, bit l is final (the output's) once
    its Hadamard ran, bit k < l still the input's"""
    i = np.arange(first, first + count, dtype=np.int64)
    s = LD(1) / np.sqrt(LD(2))
    z = np.ones(count, dtype=CLD)
    for l in range(n - 1, M - 1, -1):
        out_l = ((i >> l) & 1) == 1
        z *= s
        if (x >> l) & 1:
            z[out_l] = -z[out_l]
        for k in range(l - 1, M - 1, -1):
            if (x >> k) & 1:
                z[out_l] *= _unit(math.pi / float(1 << (l - k)))
    mlow = (1 << M) - 1
    z[(i & mlow) != (x & mlow)] = 0
    z.setflags(write=False)
    return z


def rel_errors(got_pairs, T, where=None):
    """(max_j |got_j - T_j| / max_j |T_j|,  ||got - T||_2 / ||T||_2), on the amplitudes `where` selects when given"""
    g = widen(got_pairs)
    if where is not None:
        g, T = g[where], T[where]
    d = np.abs(g - T)
    t = np.abs(T)
    if not t.any():                            # nothing to be relative to (a window of a collapsed state): exact or not at all
        return (0.0, 0.0) if not d.any() else (math.inf, math.inf)
    return float(d.max() / t.max()), float(np.sqrt(np.sum(d * d)) / np.sqrt(np.sum(t * t)))


def figures(got, oracle_state, T, where=None):
    """the numbers the criterion compares, as a dict (tools/measure_tolerance_accuracy.py writes them down)"""
    g, o = rel_errors(got, T, where), rel_errors(oracle_state, T, where)
    return dict(e_oracle_max=o[0], e_oracle_l2=o[1], e_mode2_max=g[0], e_mode2_l2=g[1],
                ratio_max=g[0] / max(o[0], FLOOR), ratio_l2=g[1] / max(o[1], FLOOR))


def assert_as_accurate_as_oracle(got, oracle_state, T, what, where=None):
    """got is as close to the truth T as the oracle's own double-precision result is, within MARGIN, in both norms.  e(oracle) is
    computed here, from the reference's result, never taken from the code under test"""
    g, o = rel_errors(got, T, where), rel_errors(oracle_state, T, where)
    for name, eg, eo in zip(("max norm", "2-norm"), g, o):
        bound = MARGIN * max(eo, FLOOR)
        assert eg <= bound, f"{what}: relative error {eg:.3e} in the {name}, the oracle's own is {eo:.3e}, allowed {bound:.3e}"
    return g, o


_TRUTHS = {}


def cached(key, make):
    """one truth per (circuit, shape, seed), module-wide: the geometry parametrisations reuse one input several times"""
    if key not in _TRUTHS:
        _TRUTHS[key] = make()
    return _TRUTHS[key]
