"""Inputs the GPU tests of the Pauli-string kernels (K14 expectation values, K15 rotations) share: adversarial states and strings
that reach every shape of the kernels and every power of i.  A plain module, no test."""
import numpy as np


def adversarial(n, seed, finite=False):
    """test_gpu_marginal.adversarial: mixed binades, subnormals, +-0, components whose products overflow, Inf and NaN.  One NaN
    amplitude makes every string's value NaN, so most comparisons run on the `finite` variant, which leaves out what overflows."""
    rs = np.random.RandomState(seed)
    a = rs.standard_normal(2 << n) * 2.0 ** rs.randint(-40, 40, 2 << n)
    k = a.size
    m = max(1, k // 16)
    a[rs.randint(0, k, m)] = 5e-324 * rs.randint(1, 1000, m)           # subnormals
    if not finite:
        a[rs.randint(0, k, max(1, k // 32))] = 1e300                     # products overflow to Inf
    a[rs.randint(0, k, m)] = 0.0
    a[rs.randint(0, k, m)] = -0.0
    if not finite:
        a[rs.randint(0, k, max(1, k // 64))] = 1e154
        if n >= 4:
            a[rs.randint(0, k)] = np.inf
            a[rs.randint(0, k)] = np.nan
    return a


def g_of(x, z):
    return bin(x & z).count("1") % 4


def with_every_g(xs, n, seed):
    """for each x_mask: z_masks that put 0, 1, 2 and 3 (as far as x has the bits) Y's on it, random Z's elsewhere"""
    rs = np.random.RandomState(seed)
    out = []
    for x in xs:
        on = [q for q in range(n) if x >> q & 1]
        for g in range(min(3, len(on)) + 1):
            ys = rs.choice(on, g, replace=False) if g else []
            z = int(rs.randint(0, 1 << n)) & ~x
            for q in ys:
                z |= 1 << int(q)
            out.append((x, z))
    return out


# x_masks of n = 13: no partner, the partner inside the tile (x_low below 8: inside a 128-B line; at or above 8: other lines),
# and bit 12 -- the smallest pair shape -- alone and with such low bits
TILE_13 = [0, 0x5, 0x7, 0x8, 0x130, 0xF00, 0xFFF]
PAIR_13 = [0x1000, 0x1005, 0x1007, 0x1008, 0x1130, 0x1F00, 0x1FFF]
