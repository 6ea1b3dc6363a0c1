"""GPU: every other call behind the TOLERANCE MODE (qcx_set_fusion(reg, 2)).  The mode's own tests look at a mode-2 register through
read, norm2 and measure_state; here every observer, every unqueued gate, the handed-out pointer, the caller's stream, save /
load and a switch of the mode meet the lazy forms the merged-diagonal engine leaves: a queue planned with merged diagonals, a
compact chain planned for them, a chained result in the second buffer, the radix-8 tolerance kernels.

Mode 2 is not bit-exact against the oracle, but it is deterministic (test_the_trigger_does_not_change_the_bits: that premise is
tested, not assumed), so the state a TWIN register reads back after the same mode-2 work is the exact reference for what the
call under test returns and leaves: tests/tolerance_twin.py (run_pair) replays a schedule of (prefix, follower) pairs that way,
bit for bit, tests/test_tolerance_twin.py pins the schedule on the CPU.  Then four pairs at once from four threads, and three
named chains."""
import time

import numpy as np
import pytest

import exact_ref as er
import register_model as rm
import sequence_replay as sr
import tolerance_twin as tt
from test_gpu_api_sequences import Chain, chain_stats
from test_gpu_concurrent_callers import run_threads

pytestmark = pytest.mark.gpu

CASES = [(p, s) for p in tt.PREFIX_KINDS for s in tt.SHAPES if tt.prefix_is_legal(p, s)]


@pytest.fixture(scope="module")
def sched(ob):
    return tt.schedule(ob)


# ---- the schedule ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind, shape", CASES, ids=[tt.key_of(p, s) for p, s in CASES])
def test_pairs_against_the_twin(qc, ob, tmp_path, sched, kind, shape):
    prefix, near = tt.prefix_ops(kind, shape), tt.oracle_state(ob, kind, shape)[0]
    t0, owed = time.monotonic(), 0
    for knobs, f, follower in sched[(kind, shape)]:
        S = tt.run_pair(qc, ob, shape, knobs, prefix, follower, tmp_path, near=near, kind=f)
        owed += tt.negative_zeros(S) > 0
    print(f"{tt.key_of(kind, shape)}: {len(sched[(kind, shape)])} pairs in {time.monotonic() - t0:.2f} s; the mode-2 state held -0 in {owed} of them")


@pytest.fixture(scope="module")
def shor_20(ob):
    """the oracle's state of the `shor` prefix at n = 20, computed once"""
    return tt.oracle_state(ob, "shor", tt.BIG_SHAPE)[0]


def test_pairs_at_n20_under_the_default_knobs(qc, ob, tmp_path, shor_20):
    """chained passes and the compact chain begin at n = 20 by default: the `shor` prefix, six followers"""
    prefix = tt.prefix_ops("shor", tt.BIG_SHAPE)
    assert [(k, qc.lib().qcx_tune_get(k.encode())) for k in ("fuse_chain_min_n", "fuse_compact_lazy", "fuse_gen", "fuse_gen_cols")] == \
           [("fuse_chain_min_n", 20), ("fuse_compact_lazy", 1), ("fuse_gen", 1), ("fuse_gen_cols", 1)], "the defaults this case is about"
    t0 = time.monotonic()
    for knobs, f, follower in tt.big_case(ob, shor_20):
        tt.run_pair(qc, ob, tt.BIG_SHAPE, knobs, prefix, follower, tmp_path, near=shor_20, kind=f)
    print(f"n = 20: {len(tt.BIG_FOLLOWERS)} pairs in {time.monotonic() - t0:.2f} s")


# ---- the premise ---------------------------------------------------------------------------------------------------------------

def settled(qc, shape, prefix, how, tmp_path):
    L, M = shape[:2]
    with qc.Register(L, M) as reg:
        tt.run_prefix(qc, reg, prefix, tmp_path, {})
        if how == "flush":
            reg.flush()
        elif how == "observer":                                           # a keep-compact observer: a compact result stays compact
            reg.marginal(M, 2)
        return reg.read()


@pytest.mark.parametrize("shape", tt.SHAPES[2:], ids=[f"{s[0]}-{s[1]}" for s in tt.SHAPES[2:]])
def test_the_trigger_does_not_change_the_bits(qc, tmp_path, shape):
    """what settles the pending mode-2 work -- flush() then read(), read() alone, marginal(M, 2) then read() -- leaves the same
    bits: the store and expand paths are copies"""
    old = qc.lib().qcx_tune_get(b"fuse_chain_min_n")
    try:
        for knobs in ({}, dict(fuse_chain_min_n=13)):
            qc.tune(**knobs)
            for kind in tt.PREFIX_KINDS:
                prefix = tt.prefix_ops(kind, shape)
                a, b, c = (sr.bits(settled(qc, shape, prefix, how, tmp_path)) for how in ("flush", "read", "observer"))
                for name, other in (("read() alone", b), ("marginal(M, 2) then read()", c)):
                    bad = np.flatnonzero(a != other)
                    assert bad.size == 0, f"{kind} on {shape} under {knobs}: {name} leaves {bad.size} doubles that flush() then read() does not, first at {bad[:4]}"
    finally:
        qc.tune(fuse_chain_min_n=old)


# ---- four threads ------------------------------------------------------------------------------------------------------------

THREAD_PAIRS = [("iqft", (8, 4, 15, 7), "expect_batch"), ("shor", (11, 5, 21, 2), "marginal"), ("program", (9, 5, 21, 2), "cu1"),
                ("sparse", (13, 0, 1, 1), "devptr")]


def test_four_threads_in_tolerance_mode(qc, ob, tmp_path, sched):
    """four different pairs, one of them on a compact shape, each thread with a twin and a subject of its own, under the default
    knobs (they are process-wide).  The expectations are the single-threaded ones: a twin on this thread gives S and the model
    its values first; a thread's own twin must give the same S"""
    jobs = []
    for kind, shape, f in THREAD_PAIRS:
        follower = next(ops for _, g, ops in sched[(kind, shape)] if g == f)
        prefix, near = tt.prefix_ops(kind, shape), tt.oracle_state(ob, kind, shape)[0]
        twin = tt.run_twin(qc, shape, prefix, tmp_path)
        tt.check_twin(twin, near, prefix, shape, tt.truth_of(ob, shape, prefix))
        ops = tt.pair_ops(shape, follower)
        jobs.append((kind, shape, f, prefix, ops, twin) + tt.expectations(ob, shape, twin[0], ops))
    assert any(rm.compact_shape(j[1]) and j[5][2] == 1 for j in jobs), "one pair behind a compact chain"

    def body(i):
        kind, shape, f, prefix, ops, twin, wants, final = jobs[i]
        def run():
            tmp = tmp_path / f"thread{i}"
            tmp.mkdir(exist_ok=True)
            mine = tt.run_twin(qc, shape, prefix, tmp)
            sr.same(mine[0], twin[0], "this thread's twin against the one that ran alone")
            assert mine[1:3] == twin[1:3], (mine[1:3], twin[1:3])
            tt.run_subject(qc, shape, {}, prefix, f, ops, wants, final, mine, tmp)
        return run

    run_threads([body(i) for i in range(len(jobs))], [f"{j[0]} on {j[1]}, then {j[2]}" for j in jobs], 60.0)


# ---- named chains ------------------------------------------------------------------------------------------------------------

def twin_state(qc, L, M, work):
    """what a fresh register reads back after set_fusion(2) and work(reg, ctx)"""
    ctx = {}
    try:
        with qc.Register(L, M) as reg:
            reg.set_fusion(2)
            work(reg, ctx)
            return reg.read()
    finally:
        ctx.clear()


def test_chain_compact_result_marginal_collapse_then_the_exact_inverse_qft(qc, ob, tmp_path):
    L, M, Cn, a = rm.COMPACT_SHAPES[0]

    def work(reg, ctx):
        qc.reset_register(reg)
        qc.quantum_computation(Cn, a, reg)

    S = twin_state(qc, L, M, work)
    near = tt.oracle_state(ob, "shor", rm.COMPACT_SHAPES[0])[0]
    assert tt.max_delta(S, near) <= tt.TOL
    er.assert_as_accurate_as_oracle(S, near, tt.truth_of(ob, rm.COMPACT_SHAPES[0], tt.prefix_ops("shor", rm.COMPACT_SHAPES[0])), "the compact chain's state")
    with Chain(qc, ob, L, M, 2, tmp_path) as c:
        k0 = sr.compact_chains(qc, c.reg)
        work(c.reg, c.ctx)
        c.m.a = S.copy()
        assert sr.compact_chains(qc, c.reg) == k0, "mode 2 queues the circuit"
        c.do("marginal", 1, 3)                                            # inside M: expanded into the register's stale buffer
        assert sr.compact_chains(qc, c.reg) == k0 + 1, "the observer's flush runs reset + quantum_computation as a compact chain"
        assert c.reg.marginal_stats() == (3, 1)
        v, p, st = c.do("measure_qubits", M, L, 0.61)                     # the whole L register, read from the compact form
        assert st == 0 and c.reg.collapse_stats() == (3, 1, 1)
        c.do("fusion", 0)
        c.do("iqft")                                                      # exact: the oracle's, on the model's collapsed state
        c.state()


def test_chain_inverse_qft_queued_behind_the_handed_out_pointer_on_a_callers_stream(qc, ob, tmp_path):
    L, M = 9, 5

    def work(reg, ctx):
        sr.set_stream(reg, 1, ctx)
        reg.fill_random(3)
        sr.read_through_pointer(reg, 0, 64, ctx)                          # in place from here on: no second buffer, no chain
        qc.inverse_QFT(reg)

    S = twin_state(qc, L, M, work)
    want = ob.fill_random(L + M, 3); ob.iqft(want, L + M, M, 8)
    assert tt.max_delta(S, want) <= tt.TOL and not np.array_equal(sr.bits(S), sr.bits(want))
    er.assert_as_accurate_as_oracle(S, want, tt.truth_from(ob.fill_random(L + M, 3), L + M, M, [("iqft",)]), "the inverse QFT run in place")
    with Chain(qc, ob, L, M, 2, tmp_path) as c:
        p0 = chain_stats(qc, c.reg)
        work(c.reg, c.ctx)
        c.m.a = S.copy()
        got = c.do("prot_batch", 11, 5)
        assert got[0][0] >= 1 and chain_stats(qc, c.reg) == p0, "the queue ran in place"
        c.do("rdm", 10, 4)
        assert c.reg.rdm_stats() == (0, 1)
        c.do("devptr", 0, c.dim)


def zero_half(n, seed):
    """window_data's "negzero" state with every amplitude whose qubit 0 is clear set to (+0, +0): whole pairs of zeros meet the
    merged diagonals of gates that leave qubit 0 alone, and that half stays zero"""
    a = rm.window_data(1 << n, 1 << n, seed, "negzero").reshape(-1, 2)
    a[0::2] = 0.0
    return a.reshape(-1)


def runs_ending_in_a_diagonal(n, ctls, theta=2.0):
    """for each control: a Hadamard, then a run of phases on it with every other qubit but qubit 0 -- the shape of a merged round;
    the last run is not followed by a Hadamard, so what its diagonal leaves is what the state holds.  exp(2i) has a negative real
    and a positive imaginary part: (+0, +0) times it is (-0, +0) in the one complex product of the tolerance kernels"""
    ops = []
    for ctl in ctls:
        ops.append(("h", ctl))
        ops += [("cphase", ctl, t, theta) for t in range(1, n) if t != ctl]
    return ops


def run_gates(qc, reg, ops):
    for op in ops:
        if op[0] == "h":
            qc.hadamard_gate(op[1], reg)
        else:
            qc.c_phase_shift_gate(op[1], op[2], op[3], reg)


@pytest.mark.parametrize("state", ["sparse", "zero-half"])
def test_chain_sparse_state_controlled_gates_meet_the_zeros_mode_2_left(qc, ob, tmp_path, state):
    """the path where a -0 left by a mode-2 pass surfaces: the first exact gates are controlled on qubit 0, whose control-clear
    half is not touched by them, and the reference leaves +0 there.  sparse: the prefix of that name (zeros of either sign
    scattered over the components).  zero-half: the control-clear half of qubit 0 holds nothing but zeros and the mode-2 work
    ends in a merged diagonal -- that state DOES hold -0 (asserted: the chain must make them where the next gate does not act)"""
    shape = (9, 5, 21, 2)
    L, M = shape[:2]
    n = L + M
    prefix = tt.prefix_ops("sparse", shape)
    gates = runs_ending_in_a_diagonal(n, (n - 2, n - 3, M + 1))

    def work(reg, ctx):
        if state == "sparse":
            tt.run_prefix(qc, reg, prefix, tmp_path, ctx)
        else:
            reg.write(zero_half(n, 41))
            run_gates(qc, reg, gates)

    S = twin_state(qc, L, M, work)
    if state == "sparse":
        near, truth = tt.oracle_state(ob, "sparse", shape)[0], tt.truth_of(ob, shape, prefix)
    else:
        m = rm.RegisterModel(ob, L, M)
        m.write(zero_half(n, 41))
        for op in gates:
            rm.apply_to_model(m, op)
        near, truth = m.a, tt.truth_from(zero_half(n, 41), n, M, gates)
        assert not S[0::4].any() and not S[1::4].any(), "the control-clear half of qubit 0 holds nothing but zeros"
        assert tt.negative_zeros(S[0::4]) + tt.negative_zeros(S[1::4]) > 50, "the chain must make -0 where the next gate does not act"
    assert tt.max_delta(S, near) <= tt.TOL and not np.array_equal(sr.bits(S), sr.bits(near))
    er.assert_as_accurate_as_oracle(S, near, truth, f"{state}: the mode-2 state")
    print(f"{state}: the mode-2 state holds {tt.negative_zeros(S)} components that are -0")
    with Chain(qc, ob, L, M, 2, tmp_path) as c:
        work(c.reg, c.ctx)
        c.m.a = S.copy()
        c.do("marginal", 0, 3)                                            # an observer sees the state as it is, -0 and all
        c.do("cu1", 0, n - 1, 4)
        assert tt.negative_zeros(c.m.a) == 0, "the reference's gate leaves canonical zeros"
        c.do("cu2", 0, n - 2, 3, 9)
        c.state()


def test_chain_zeros_mode_2_left_then_the_per_gate_hadamard_in_mode_0(qc, ob, tmp_path):
    """the same state, then a switch to mode 0 and the reference's own gates launched one by one: they act where they act, and
    the zero pass the tolerance flush left owed does the rest"""
    L, M = 8, 4
    n = L + M
    gates = runs_ending_in_a_diagonal(n, (n - 2, M + 1))

    def work(reg, ctx):
        reg.write(zero_half(n, 42))
        run_gates(qc, reg, gates)

    S = twin_state(qc, L, M, work)
    assert tt.negative_zeros(S) > 50, "the chain must make -0"
    for follow in (("cphase", n - 1, 1, 0.4), ("h", n - 1), ("camodc", 15, 7, n - 1)):
        with Chain(qc, ob, L, M, 2, tmp_path) as c:
            work(c.reg, c.ctx)
            c.m.a = S.copy()
            c.do("read", 0, 64)                                           # the -0 are the state until an exact gate runs
            c.do("fusion", 0)
            c.do(*follow)
            assert tt.negative_zeros(c.m.a) == 0
            c.state()


@pytest.mark.parametrize("shards", [2, 4])
def test_sharded_register_owes_the_zero_pass_after_a_tolerance_flush(qc, ob, shards):
    """a register sharded by this process runs the tolerance mode per shard: the same -0, the same owed pass per shard.  The twin
    is a sharded register of the same geometry (another plan gives other bits); the exact gate behind the mode-2 work is a
    controlled phase, which acts on a quarter of the state"""
    L, M = 13, 0
    n = L
    gates = runs_ending_in_a_diagonal(n, (8, 5))

    def settled(more):
        with qc.Register(L, M, shards=shards, devices=qc.spread_devices(shards)) as reg:
            reg.set_fusion(2)
            reg.write(zero_half(n, 43))
            run_gates(qc, reg, gates)
            if more:
                reg.set_fusion(0)
                qc.c_phase_shift_gate(9, 1, 0.4, reg)
            return reg.read()

    S = settled(False)
    m = rm.RegisterModel(ob, L, M)
    m.write(zero_half(n, 43))
    for op in gates:
        rm.apply_to_model(m, op)
    assert tt.max_delta(S, m.a) <= tt.TOL and not np.array_equal(sr.bits(S), sr.bits(m.a))
    er.assert_as_accurate_as_oracle(S, m.a, tt.truth_from(zero_half(n, 43), n, M, gates), f"{shards} shards: the mode-2 state")
    assert tt.negative_zeros(S) > 50, "the chain must make -0"
    m.a = S.copy()
    m.c_phase_shift_gate(9, 1, 0.4)
    assert tt.negative_zeros(m.a) == 0
    sr.same(settled(True), m.a, f"{shards} shards: the state behind the first exact gate")
