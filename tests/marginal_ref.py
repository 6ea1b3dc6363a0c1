"""The summation order of qcx_marginal_probabilities (include/qcx.h), restated in numpy -- this restatement IS the definition --
and an emulator of the planned stages (include/qcx_plan.h: qcx_marginal_plan), the way tests/fuse_emulator.py interprets the
fused-pass records.  Host only."""
import numpy as np


def marginal_ref(a, n, first, num):
    """a: complex128[2^n] (or interleaved float64 re/im pairs), index order.  The pairwise tree over the summed bits, lowest
    first: the low bits below the range, then the high bits above it."""
    a = np.asarray(a)
    if a.dtype != np.complex128:
        a = np.ascontiguousarray(a, dtype=np.float64).view(np.complex128)
    with np.errstate(over="ignore", invalid="ignore"):              # (Inf and NaN propagate by IEEE rules)
        p = a.real * a.real + a.imag * a.imag
    x = p.reshape(1 << (n - first - num), 1 << num, 1 << first)     # (hi, range, lo)
    with np.errstate(over="ignore", invalid="ignore"):
        while x.shape[2] > 1:
            x = x[:, :, 0::2] + x[:, :, 1::2]                        # low summed bits, ascending
        x = x[:, :, 0]
        while x.shape[0] > 1:
            x = x[0::2] + x[1::2]                                    # high summed bits, ascending
    return x[0]


def _reduce_bits(x, m, mask):
    """x: 2^m values, index order; sum out the index bits in `mask`, lowest first, one pairwise level per bit.  Returns the
    values indexed by the remaining bits in ascending order."""
    y = x.reshape([2] * m) if m else x.reshape(())
    left = m
    for b in range(m):                                               # ascending bit order; axis of bit b = left - 1 - rank
        if mask >> b & 1:
            rank = bin(mask & ((1 << b) - 1)).count("1")             # summed bits below b are gone already
            ax = left - 1 - (b - rank)
            y = np.take(y, 0, axis=ax) + np.take(y, 1, axis=ax)
            left -= 1
    return np.ascontiguousarray(y).reshape(-1)


def compact_leaves(a, n, M, orbit, cb):
    """the compact form of a state whose M-register values lie in `orbit` (ascending): (L blocks, 2^cb columns) amplitudes"""
    a = np.asarray(a)
    if a.dtype != np.complex128:
        a = np.ascontiguousarray(a, dtype=np.float64).view(np.complex128)
    blocks = a.reshape(1 << (n - M), 1 << M)
    out = np.zeros((1 << (n - M), 1 << cb), dtype=np.complex128)
    out[:, :len(orbit)] = blocks[:, list(orbit)]
    return out


@np.errstate(over="ignore", invalid="ignore")
def emulate_stages(stages, a=None, compact=None):
    """Run the planned stages on the host.  a: the dense state (kind 0); compact = (amplitudes (blocks, 2^cb), orbit, M) for a
    plan that starts with a compact stage (kind 2): every block's leaves are +0 except at its orbit residues."""
    x = None
    for i, s in enumerate(stages):
        if s.kind == 0:
            z = np.asarray(a)
            if z.dtype != np.complex128:
                z = np.ascontiguousarray(z, dtype=np.float64).view(np.complex128)
            x = z.real * z.real + z.imag * z.imag
        elif s.kind == 2:
            amps, orbit, M = compact
            cols = amps[:, :len(orbit)]
            p = cols.real * cols.real + cols.imag * cols.imag
            full = np.zeros((amps.shape[0], 1 << M))
            full[:, list(orbit)] = p
            x = _reduce_bits(full.reshape(-1), (amps.shape[0].bit_length() - 1) + M, (1 << M) - 1)
        assert x.size == 1 << s.in_bits, (i, x.size, s.in_bits)
        x = _reduce_bits(x, s.in_bits, int(s.sum_mask))
        assert x.size == 1 << s.out_bits
    return x
