"""GPU: time-boxed randomised comparison of the fused engine with the oracle -- register sizes, gate mixes, modes, observers and
knob settings drawn at random from one seed.  The suite runs a short, fixed-seed slice; a longer campaign is
    QCX_FUZZ_SECONDS=480 QCX_FUZZ_SEED=$RANDOM python -m pytest tests/test_gpu_fuzz.py -m gpu -x -q -s
(every case prints its own seed first, so a failure names the case to replay with QCX_FUZZ_CASE=<seed>)."""
import math
import os
import time

import numpy as np
import pytest

import exact_ref as er

pytestmark = pytest.mark.gpu

TOL = 1e-12
TRUTH_MAX_N = 20                                    # mode-2 cases up to here carry an extended-precision truth beside the oracle's state
KNOBS = ("fuse_T", "fuse_c", "fuse_x8", "fuse_x8_min_tiles_log2", "fuse_chain", "fuse_chain_min_n", "fuse_chain_dir", "fuse_compact",
         "fuse_compact_lazy", "fuse_expand_fused", "fuse_gen", "fuse_gen_cols", "fuse_plan_cache", "meas_parallel", "meas_min_log2", "meas_block_log", "meas_fast")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(got, want, mode, what, truth=None):
    if mode == 3:                                   # poisoned states: NaN wherever the oracle has one, everything else bit for bit
        gn, wn = np.isnan(got), np.isnan(want)
        assert np.array_equal(gn, wn), f"{what}: NaN pattern differs at {np.nonzero(gn != wn)[0][:6]}"
        bad = np.nonzero(bits(got[~gn]) != bits(want[~wn]))[0]
        assert bad.size == 0, f"{what}: {bad.size} non-NaN doubles differ"
        return
    if mode == 2:
        err = float(np.max(np.abs(got - want)))
        assert err <= TOL, f"{what}: max |delta| {err:.3e}"
        if truth is not None:                       # as accurate against the truth as the oracle's own state (tests/exact_ref.py)
            er.assert_as_accurate_as_oracle(got, want, truth, what)
    else:
        bad = np.nonzero(bits(got) != bits(want))[0]
        assert bad.size == 0, f"{what}: {bad.size} doubles differ, first at {int(bad[0])}: {got[bad[0]]!r} vs {want[bad[0]]!r}"


def gate_mix(rs, n, M, Cn, length, lo, phase_bias):
    """H / CPHASE / C_AMODC on qubits lo .. n-1 (lo = M: nothing touches the M register -- what a compact chain needs)"""
    prog = []
    for _ in range(length):
        k = rs.uniform()
        if k < (1.0 - phase_bias) * 0.8:
            prog.append(("h", int(rs.randint(lo, n))))
        elif k < 0.97 or M == 0 or lo:
            c, t = (int(v) for v in rs.choice(np.arange(lo, n), 2, replace=False))
            th = float(rs.uniform(-3.2, 3.2)) if rs.randint(0, 2) else math.pi / (1 << int(rs.randint(1, 14)))
            prog.append(("p", c, t, th))
        else:
            prog.append(("c", int(rs.randint(1, 4 * Cn)), int(rs.randint(M, n))))
    return prog


def apply(qc, ob, reg, want, n, M, Cn, prog, threads=8, truth=None):
    if truth is not None:
        er.advance(truth, n, M, prog, Cn)
    for g in prog:
        if g[0] == "h":
            qc.hadamard_gate(g[1], reg); ob.hadamard(want, n, g[1], threads)
        elif g[0] == "p":
            qc.c_phase_shift_gate(g[1], g[2], g[3], reg); ob.cphase(want, n, g[1], g[2], g[3], threads)
        else:
            qc.c_amodc_gate(Cn, g[1], g[2], reg); ob.camodc(want, n, M, Cn, g[1], g[2], threads)


def one_case(qc, ob, seed):
    rs = np.random.RandomState(seed)
    Cn, M, a = [(21, 5, 2), (15, 4, 7), (35, 6, 2), (1, 0, 1), (1, 0, 1), (21, 5, 16), (33, 6, 7)][rs.randint(0, 7)]
    n = int(rs.randint(max(M + 6, int(os.environ.get("QCX_FUZZ_NMIN", "10"))), int(os.environ.get("QCX_FUZZ_NMAX", "22")) + 1))
    L = n - M
    mode = int(rs.choice([0, 1, 2]))
    knobs = dict(fuse_T=int(rs.choice([10, 11, 12])), fuse_c=int(rs.choice([3, 4])), fuse_x8=int(rs.randint(0, 4) != 0),
                 fuse_x8_min_tiles_log2=int(rs.choice([0, 2])), fuse_chain=int(rs.randint(0, 4) != 0), fuse_chain_min_n=13,
                 fuse_chain_dir=int(rs.choice([-1, 0, 1])), fuse_compact=int(rs.randint(0, 5) != 0), fuse_compact_lazy=int(rs.randint(0, 3) != 0),
                 fuse_expand_fused=int(rs.randint(0, 4) != 0), fuse_gen=int(rs.randint(0, 6) != 0), fuse_gen_cols=int(rs.randint(0, 6) != 0),
                 fuse_plan_cache=int(rs.randint(0, 4) != 0),
                 meas_parallel=1, meas_min_log2=10, meas_block_log=int(rs.choice([0, 8, 9, 11])), meas_fast=int(rs.randint(0, 4) != 0))
    kind = int(rs.randint(0, 3)) if M else 0
    # one case in five on a register SHARDED by this process (the C host: virtual shards of the one GPU): the exchange step,
    # the relabelling of global qubits, compact circuits on companion registers, measurement across shards
    shards = int(rs.choice([2, 4, 8])) if rs.randint(0, 5) == 0 else 1
    k = shards.bit_length() - 1
    if shards > 1 and n - k - max(M, 6) < 2 * k:
        shards = 1
    poisoned = kind == 0 and shards == 1 and n <= 18 and rs.randint(0, 8) == 0
    tag = f"case {seed}: n={n} M={M} C={Cn} mode={mode} kind={kind} shards={shards} poisoned={int(poisoned)} {knobs}"
    print(tag, flush=True)
    qc.tune(**knobs)
    scale = 1.0
    with (qc.Register(L, M, shards=shards, devices=qc.spread_devices(shards)) if shards > 1 else qc.Register(L, M)) as reg:
        reg.set_fusion(mode)
        # the SAME circuit up to three times on the same register (different states, different observers): the plan cache's case
        reps = int(rs.choice([1, 1, 2, 3]))
        prog0 = gate_mix(rs, n, M, Cn, int(rs.randint(20, 260)), 0, float(rs.choice([0.3, 0.6, 0.9])))
        tail2 = gate_mix(rs, n, M, Cn, int(rs.randint(10, 200)), M, float(rs.choice([0.5, 0.8, 0.95])))
        for rep_i in range(reps):
            truth = None
            tracked = mode == 2 and not poisoned and n <= TRUTH_MAX_N
            if kind == 0 and poisoned:                      # the same on a state with Inf / NaN / overflow-prone components: strict gates (K9)
                want = ob.random_state(n, (seed + rep_i) & 0xFFFF)
                for w_ in rs.choice(2 << n, size=int(rs.randint(1, 5)), replace=False):
                    want[w_] = float(rs.choice([np.inf, -np.inf, np.nan, 1e308, -1.5e308]))
                reg.write(want)
                apply(qc, ob, reg, want, n, M, Cn, prog0[:60])
            elif kind == 0:                                 # a random program on a random dense state
                sd = (seed + 977 * rep_i) & 0xFFFF
                want = ob.fill_random(n, sd); reg.fill_random(sd)
                truth = er.widen(want) if tracked else None
                apply(qc, ob, reg, want, n, M, Cn, prog0, truth=truth)
            else:                                           # behind a reset: the circuit front, then the inverse QFT (1) or a random tail on the L register (2)
                want = np.zeros(2 << n); ob.reset(want, n)
                truth = er.widen(want) if tracked else None
                qc.reset_register(reg)
                if kind == 1:
                    qc.quantum_computation(Cn, a, reg); ob.quantum_computation(want, n, M, Cn, a, threads=8)
                    if tracked:
                        er.advance(truth, n, M, er.qcomp_steps(Cn, a, L, M))
                else:
                    for l in range(M, n):
                        qc.hadamard_gate(l, reg); ob.hadamard(want, n, l, 8)
                    x = a % Cn
                    for l in range(M, n):
                        qc.c_amodc_gate(Cn, x, l, reg); ob.camodc(want, n, M, Cn, x, l, 8); x = (x * x) % Cn
                    if tracked:
                        er.advance(truth, n, M, er.qcomp_steps(Cn, a, L, M)[:2 * L])
                    apply(qc, ob, reg, want, n, M, Cn, tail2, truth=truth)
            # observers, in random order; each must see the reference's state
            for obs in rs.permutation(["read", "norm", "window", "measure", "more"])[:int(rs.randint(1, 5))]:
                cmp_mode = 3 if poisoned else mode
                if poisoned and obs in ("norm", "more"):
                    continue                                # (norm of a NaN state; "more" would run on a collapsed or still poisoned state: covered by the next case)
                if obs == "read":
                    same(reg.read(), want, cmp_mode, tag + " read", truth)
                elif obs == "norm":
                    # (two different summation orders -- the oracle's is the sequential one: 1.1e-11 apart at n = 25 -- so this observer
                    #  only checks that the flush it triggers leaves the right state behind; the reads do the comparing)
                    assert abs(reg.norm2() - ob.norm2(want, n)) < 1e-9, tag + " norm"
                elif obs == "window":
                    s = int(rs.randint(0, (1 << n) - 64)); cnt = int(rs.randint(1, min(1 << n, 5000) - 63))
                    cnt = min(cnt, (1 << n) - s)
                    same(reg.read(s, cnt), want[2 * s:2 * (s + cnt)], cmp_mode, tag + " window", None if truth is None else truth[s:s + cnt])
                elif obs == "measure":
                    r = float(rs.uniform(0, 1)) if rs.randint(0, 4) else float(rs.choice([0.0, 1.0, 1e-9, 0.999999999]))
                    got = qc.measure_state(reg, r)
                    if mode == 2 and not poisoned:
                        # the tolerance mode's probabilities differ in the last bits: the draw must land next to the same boundary
                        cum = np.cumsum((want.reshape(-1, 2) ** 2).sum(axis=1))
                        lo, hi = int(np.searchsorted(cum, r - 1e-9)), int(np.searchsorted(cum, r + 1e-9))
                        assert (r <= 0.0 and got == 0) or lo <= got <= max(hi, lo) or got == (1 << n) - 1, tag + f" measure r={r!r}: {got} not in [{lo}, {hi}]"
                        want[:] = 0.0; want[2 * got] = 1.0
                        truth = er.widen(want) if truth is not None else None
                    else:
                        assert got == ob.measure(want, n, r), tag + f" measure r={r!r}"
                    same(reg.read(), want, 0, tag + " collapsed state")
                    poisoned = False                            # the collapse replaced the state
                else:
                    prog = gate_mix(rs, n, M, Cn, int(rs.randint(1, 60)), 0, 0.6)
                    apply(qc, ob, reg, want, n, M, Cn, prog, truth=truth)
                    same(reg.read(), want, mode, tag + " more gates", truth)
    return scale


def test_randomised_cases_against_the_oracle(qc, ob):
    budget = float(os.environ.get("QCX_FUZZ_SECONDS", "25"))
    master = int(os.environ.get("QCX_FUZZ_SEED", "20260504"))
    only = os.environ.get("QCX_FUZZ_CASE")
    old = {k: qc.lib().qcx_tune_get(k.encode()) for k in KNOBS}
    try:
        if only:
            one_case(qc, ob, int(only))
            return
        rs = np.random.RandomState(master)
        t0, done = time.time(), 0
        while time.time() - t0 < budget or done < 6:
            one_case(qc, ob, int(rs.randint(0, 2 ** 31 - 1)))
            done += 1
        print(f"{done} cases in {time.time() - t0:.1f} s (master seed {master})")
    finally:
        qc.tune(**old)
