"""Every other call behind the TOLERANCE MODE (qcx_set_fusion(reg, 2)): prefixes that leave mode-2 work queued or a mode-2 result in
a lazy form, followers that are one call of every kind, the schedule that deals them out, and run_pair, which replays one
(prefix, follower) pair against a TWIN register.  tests/test_tolerance_twin.py pins the schedule on the CPU,
tests/test_gpu_tolerance_observers.py runs it.

Mode 2 is not bit-exact against the oracle (merged diagonals, FMA: amplitudes within 1e-12), but it is deterministic, and every
other call is defined bit for bit as a function of the state it is given.  So the state S a twin register reads back after the
same mode-2 work is the exact reference: a RegisterModel whose state is set to S must return, and be left with, the very bits the
subject register gives for the follower -- whatever lazy form (a queue planned with merged diagonals, a compact chain, a chained
result in the second buffer, a deferred expanding store) the subject held when the follower arrived.  No tolerance enters but
the one of the mode itself, which only keeps a pair from being vacuous (S is within 1e-12 of the oracle and differs from it in bits)
-- and S itself is held to the criterion of tests/exact_ref.py: against an extended-precision truth of the prefix's gates it is as
accurate as the oracle's state is (truth_of, check_twin).

A mode-2 pass may leave -0 behind (an amplitude (+0, +0) times a merged diagonal F with Re F < 0 <= Im F has the real part
(-0) - (+0) = -0), so a flush that ran merged diagonals owes the zero pass like a state the caller wrote: observers see S as it
is, the next exact gate canonicalises every amplitude.  Every pair therefore ends with a controlled matrix gate in mode 0, which
acts on half of the state only, and the model's gates -- the reference's, which rewrite every amplitude -- say what it must leave.

Host only: imports no GPU code itself."""
import numpy as np

import exact_ref as er
import register_model as rm
import sequence_replay as sr

TOL = 1e-12                                   # tests/test_gpu_tolerance_mode.TOL
SEED = 20261020
PREFIX_KINDS = ("iqft", "shor", "program", "sparse", "collapsed")
FOLLOWER_KINDS = rm.FOLLOWING_V3 + ("prot_batch",)
# (L, M, C, a), the smallest at which each mode-2 path exists: one 2^12 tile with radix-8 tolerance rounds; no M register and pairs
# of tiles for the Pauli kernels; the Shor state with zero columns and no compact chain; the two shapes of the compact chain
SHAPES = [(8, 4, 15, 7), (13, 0, 1, 1), (9, 5, 21, 2)] + rm.COMPACT_SHAPES
BIG_SHAPE = (15, 5, 21, 2)                    # n = 20: chained passes and the compact chain under the DEFAULT knobs
BIG_FOLLOWERS = ("marginal", "measure", "sample", "expect_batch", "rdm", "prot_batch")
KNOBS = [{}, dict(fuse_chain_min_n=13), dict(fuse_chain_min_n=13, fuse_chain_dir=0), dict(fuse_chain_min_n=13, fuse_chain_dir=1),
         dict(fuse_compact_lazy=0), dict(fuse_expand_fused=0), dict(fuse_plan_cache=0), dict(fuse_gen=0), dict(fuse_gen_cols=0),
         dict(fuse_tol_T=0), dict(fuse_q3=0), dict(fuse_x8t=0), dict(fuse_tol_occ=8), dict(fuse_cols_tol=0)]
KNOB_KEYS = sorted({k for d in KNOBS for k in d})
# followers that replace the state without looking at it: the queued mode-2 work may be dropped unrun
REPLACES_STATE = ("reset", "fill")
# observers that leave a compact circuit result compact (and say where they read it)
KEEP_COMPACT = ("measure", "sample", "marginal", "measure_qubits", "postselect", "expect", "expect_sum", "expect_batch", "rdm")
# the last ops of every pair: the first exact gate behind the mode-2 work acts on the control-set half only and must leave
# canonical zeros everywhere (the owed zero pass), then the whole state
def tail_ops(n):
    return [("fusion", 0), ("cu1", n - 1, 0, 7), ("read", 0, 1 << n)]


def key_of(kind, shape):
    return f"{kind}/{shape[0]}-{shape[1]}"


def knobs_are_legal(knobs, shape):
    """as register_model.Config: the two knobs that end compact chains are not used on the compact shapes"""
    return not (rm.compact_shape(shape) and any(k in rm.ENDS_COMPACT_CHAINS for k in knobs))


def prefix_is_legal(kind, shape):
    return not (kind == "shor" and shape[1] == 0)


def pair_is_legal(kind, f, shape):
    return prefix_is_legal(kind, shape) and rm.pair_is_legal("fill", f, shape, False)


# ---- prefixes ----------------------------------------------------------------------------------------------------------------

def prefix_ops(kind, shape):
    """the ops (register_model's tuples) that, run in mode 2, leave merged-diagonal work behind; one list per (kind, shape)"""
    L, M, Cn, a = shape
    n = L + M
    rs = np.random.RandomState(SEED + 1009 * PREFIX_KINDS.index(kind) + 31 * n + M)
    seed = lambda: int(rs.randint(1, 1 << 20))
    if kind == "iqft":                        # queued, merged runs on every control
        return [("fill", seed()), ("iqft",)]
    if kind == "shor":                        # a generated front: a compact chain on the compact shapes, an ordinary chain elsewhere
        return [("reset",), ("qcomp", Cn, a)]
    if kind == "sparse":                      # a quarter of the components exact zeros of either sign
        return [("write", 0, 1 << n, seed(), "negzero"), ("iqft",)]
    if kind == "collapsed":                   # the inverse QFT queued behind a pending basis state
        return [("fill", seed()), ("measure", float(rs.uniform(0.05, 0.95))), ("iqft",)]
    assert kind == "program", kind
    # 30-60 gates as tests/test_gpu_tolerance_mode.test_random_programs_within_tolerance draws them: runs of controlled phases
    # that share a control (one run in two behind a Hadamard on that control, the shape the merged rounds take), Hadamards,
    # modular multiplies where there is an M register
    ops, count = [("fill", seed())], int(rs.randint(30, 61))
    while len(ops) <= count:
        k = int(rs.randint(0, 10))
        if k < 3:
            ops.append(("h", int(rs.randint(0, n))))
        elif k < 8 or M == 0:
            ctl = int(rs.randint(0, n))
            if rs.randint(0, 2):
                ops.append(("h", ctl))
            for _ in range(int(rs.randint(2, 10))):
                t = int(rs.randint(0, n))
                if t != ctl:
                    ops.append(("cphase", ctl, t, float(rs.uniform(-3, 3))))
        else:
            ops.append(("camodc", Cn, int(rs.randint(1, 4 * Cn)), int(rs.randint(M, n))))
    return ops[:count + 1]


def holds_a_merged_run(prefix):
    """a run of >= 2 controlled phases on one control: what mode 2 merges into one diagonal (the circuits hold many)"""
    if any(op[0] in ("iqft", "qcomp") for op in prefix):
        return True
    return any(a[0] == b[0] == "cphase" and a[1] == b[1] for a, b in zip(prefix, prefix[1:]))


_ORACLE = {}


def oracle_state(ob, kind, shape):
    """the prefix on the host model: the exact state its mode-2 result must be within TOL of.  Computed once, never changed"""
    key = (kind, shape)
    if key not in _ORACLE:
        m = rm.RegisterModel(ob, shape[0], shape[1])
        returned = [rm.apply_to_model(m, op) for op in prefix_ops(kind, shape)]
        m.a.setflags(write=False)
        _ORACLE[key] = (m.a, returned)
    return _ORACLE[key]


GATE_OPS = ("h", "cphase", "camodc", "iqft", "qcomp")


def gate_steps(n, M, ops):
    """the gate ops of a prefix in the step form of exact_ref"""
    steps = []
    for op in ops:
        k = op[0]
        if k == "h": steps.append(("h", op[1]))
        elif k == "cphase": steps.append(("p", op[1], op[2], op[3]))
        elif k == "camodc": steps.append(("c", op[1], op[2], op[3]))
        elif k == "iqft": steps += er.iqft_steps(n, M)
        elif k == "qcomp": steps += er.qcomp_steps(op[1], op[2], n - M, M)
        else: raise AssertionError(f"{op!r} is no gate")
    return steps


def truth_from(start, n, M, ops):
    """the extended-precision truth (exact_ref.truth) of the gate ops of a prefix, applied to the pairs `start`"""
    return er.truth(start, n, M, gate_steps(n, M, ops))


def truth_of(ob, shape, prefix):
    """the truth of a prefix, computed once: the calls in front of its first gate (fill, write, reset, a measurement's collapse) make
    the input on the host model, exactly; everything behind must be a gate"""
    def make():
        m = rm.RegisterModel(ob, shape[0], shape[1])
        k = 0
        while k < len(prefix) and prefix[k][0] not in GATE_OPS:
            rm.apply_to_model(m, prefix[k]); k += 1
        return truth_from(m.a, shape[0] + shape[1], shape[1], prefix[k:])
    return er.cached(("twin", tuple(shape), repr(prefix)), make)


# ---- followers ---------------------------------------------------------------------------------------------------------------

def follower_ops(ob, kind, shape, near, rs):
    """one call of `kind` as a short op list, its parameters drawn by register_model's generator on `near`, the oracle's state of
    the prefix (the subject's is within 1e-12 of it: an outcome the one can be collapsed onto is one for the other, and where
    it is not the refused call is what is compared).  The kinds that queue again in mode 2 are not bit-defined there: each
    stands behind a switch to an exact mode"""
    g = rm._Gen(ob, shape, 2, rs, allow_nonfinite=False, vocab=3)
    g.ops, g.m.a, g.pending, g.mode = [], np.array(near), False, 2
    if kind in rm.QUEUED:
        return [("fusion", int(rs.choice([-1, 0, 1]))), g.op_of(kind)]
    if kind == "fusion":
        return [("fusion", int(rs.choice([-1, 0, 1])))]
    if kind == "save":                        # the file must hold the mode-2 result: it is what comes back
        return [("save", 1), ("reset",), ("load", 1)]
    if kind == "load":
        return [("save", 0), ("fill", g.seed()), ("load", 0)]
    if kind == "stream":
        return [("stream", 1)]
    if kind == "prot_batch":
        return [("prot_batch", g.seed(), int(rs.choice([1, 5, 40])))]
    if kind == "postselect":                  # an outcome well inside what the state holds, where there is one
        first, num = g.a_range()
        P = g.m.marginal(first, num)
        likely = np.flatnonzero(P > 1e-6)
        return [("postselect", first, num, int(likely[int(rs.randint(0, likely.size))]) if likely.size else 0)]
    return [g.op_of(kind)]


# ---- the schedule ------------------------------------------------------------------------------------------------------------

def schedule(ob):
    """{(prefix kind, shape): [(knobs, follower kind, follower ops), ...]}: every (prefix kind, follower kind) pair and every
    (shape, follower kind) pair at least once, every knob dict with every prefix kind; pairs a shape makes impossible left out
    as register_model.pair_is_legal does.  Dealt round-robin from one seed, as register_model._schedule deals its pairs"""
    out = {(p, s): [] for p in PREFIX_KINDS for s in SHAPES if prefix_is_legal(p, s)}
    met = set()
    at_knob = {p: 0 for p in PREFIX_KINDS}

    def deal(pi, fi, si):
        p, f, shape = PREFIX_KINDS[pi], FOLLOWER_KINDS[fi], SHAPES[si]
        for k in range(len(KNOBS)):
            knobs = KNOBS[(at_knob[p] + k) % len(KNOBS)]
            if knobs_are_legal(knobs, shape):
                at_knob[p] = (at_knob[p] + k + 1) % len(KNOBS)
                break
        rs = np.random.RandomState(SEED + 7919 * pi + 101 * fi + si)
        out[(p, shape)].append((knobs, f, follower_ops(ob, f, shape, oracle_state(ob, p, shape)[0], rs)))
        met.add((si, fi))

    for pi, p in enumerate(PREFIX_KINDS):
        for fi, f in enumerate(FOLLOWER_KINDS):
            for k in range(len(SHAPES)):              # (a step that changes with the follower: what one shape refuses is spread over the others)
                si = (pi + fi + k * (1 + fi % 4)) % len(SHAPES)
                if pair_is_legal(p, f, SHAPES[si]):
                    deal(pi, fi, si)
                    break
    at = 0                                    # the (shape, follower) pairs the rotation above left out, to the prefix kinds in turn
    for si, shape in enumerate(SHAPES):
        for fi, f in enumerate(FOLLOWER_KINDS):
            if (si, fi) in met:
                continue
            for k in range(len(PREFIX_KINDS)):
                pi = (at + k) % len(PREFIX_KINDS)
                if pair_is_legal(PREFIX_KINDS[pi], f, shape):
                    deal(pi, fi, si)
                    at = (pi + 1) % len(PREFIX_KINDS)
                    break
    # behind a compact chain every keep-compact observer must report the compact source: the `shor` prefix with each of them on
    # a compact shape, the two shapes in turn
    pi = PREFIX_KINDS.index("shor")
    for k, f in enumerate(KEEP_COMPACT):
        if not any(g == f for s in rm.COMPACT_SHAPES for _, g, _ in out[("shor", s)]):
            deal(pi, FOLLOWER_KINDS.index(f), SHAPES.index(rm.COMPACT_SHAPES[k % 2]))
    return out


def big_case(ob, near):
    """the n = 20 case: the `shor` prefix under the default knobs, one follower of each of BIG_FOLLOWERS (short term lists: the
    host references at 2^20 amplitudes dominate)"""
    pairs = []
    for fi, f in enumerate(BIG_FOLLOWERS):
        rs = np.random.RandomState(SEED + 13 * fi)
        ops = follower_ops(ob, f, BIG_SHAPE, near, rs)
        if f == "expect_batch":
            ops = [("expect_batch", ops[0][1], 6)]
        if f == "prot_batch":
            ops = [("prot_batch", ops[0][1], 5)]
        pairs.append(({}, f, ops))
    return pairs


# ---- one pair on the GPU -----------------------------------------------------------------------------------------------------

def max_delta(a, b):
    d = np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)
    return float(np.max(np.hypot(d[0::2], d[1::2])))


def negative_zeros(a):
    return int(np.count_nonzero((a == 0) & np.signbit(a)))


def stats_delta(now, before):
    return tuple(x - y for x, y in zip(now, before))


def run_prefix(qc, reg, prefix, tmp_path, ctx):
    """mode 2, then the prefix; what its calls returned"""
    reg.set_fusion(2)
    return [sr.apply_to_register(qc, reg, op, lambda slot: str(tmp_path / f"prefix_slot{slot}.qcx"), ctx) for op in prefix]


def pass_stats(qc, reg):
    """(passes, gates fused, passes with merged diagonals) so far"""
    return reg.fusion_stats() + (sr.diagonal_passes(qc, reg),)


def run_twin(qc, shape, prefix, tmp_path):
    """(S, pass_stats delta, compact chains, what the prefix's calls returned) of a fresh register: the prefix in mode 2, then
    a read of the whole state"""
    with qc.Register(shape[0], shape[1]) as reg:
        f0, c0 = pass_stats(qc, reg), sr.compact_chains(qc, reg)
        returned = run_prefix(qc, reg, prefix, tmp_path, {})
        S = reg.read()
        return S, stats_delta(pass_stats(qc, reg), f0), sr.compact_chains(qc, reg) - c0, returned


def dense_input(prefix):
    """the merged work of the prefix acts on random dense amplitudes (not on a basis state or the periodic state of a circuit)"""
    return prefix[0][0] in ("fill", "write") and not any(op[0] == "measure" for op in prefix)


def check_twin(twin, near, prefix, shape, truth=None):
    """What keeps a pair from being vacuous, as far as the twin shows it.  The planner keeps a run of phases merged only in a pass
    that can carry the diagonal (rounds form, its tables within the LDS budget, not the by-columns pass of an ordinary chain);
    elsewhere it puts the phases back and the pass is the exact interpreter's.  So the library's own count of passes with merged
    diagonals says what the bits must show: none -- the oracle's bits, exactly; some, on random dense amplitudes -- other bits.
    (On a basis state or a circuit's periodic state the merged products can round as the single ones do: nothing is asked.)
    truth: exact_ref's, of the prefix -- S must be as accurate against it as the oracle's state `near` is."""
    S, stats, chains, _ = twin
    err = max_delta(S, near)
    assert err <= TOL, f"the mode-2 state is {err:.3e} from the oracle's"
    if truth is not None:
        er.assert_as_accurate_as_oracle(S, near, truth, "the mode-2 state S")
    assert holds_a_merged_run(prefix), "a prefix without a run of phases on one control says nothing about mode 2"
    equal = np.array_equal(sr.bits(S), sr.bits(near))
    if stats[2] == 0:
        assert equal, "no pass carried a merged diagonal, and the mode-2 state does not have the oracle's bits"
    elif dense_input(prefix):
        assert not equal, f"{stats[2]} passes carried merged diagonals, and the mode-2 state has the oracle's bits"
    if rm.compact_shape(shape) and prefix[-1][0] == "qcomp":
        assert chains == 1, f"reset + quantum_computation ran as {chains} compact chains"


def expectations(ob, shape, S, ops):
    """what the model gives for `ops` from the state S (assigned, not written: no caller-data semantics enter), and its final state"""
    m = rm.RegisterModel(ob, shape[0], shape[1])
    m.a = np.array(S, dtype=np.float64)
    wants = [rm.apply_to_model(m, op) for op in ops]
    return wants, m.a


def compact_source_is_reported(qc, reg, op, M, got, measures_before):
    """behind a compact chain a keep-compact observer reports the compact source, as tests/test_gpu_api_sequences.py asserts it in
    the exact modes"""
    k = op[0]
    if k == "marginal":
        assert reg.marginal_stats() == ((1, 1) if op[1] >= M else (3, 1)), reg.marginal_stats()
    elif k in ("measure", "sample"):
        assert sr.compact_measures(qc, reg) == measures_before + 1, "the compact form was not what the scan read"
    elif k in ("expect", "expect_sum"):
        assert reg.expectation_stats()[0] == (3 if k == "expect" or op[2] else 0), reg.expectation_stats()
    elif k == "expect_batch":
        assert got[3][0] == (3 if op[2] else 0), got[3]
    elif k == "rdm":
        assert reg.rdm_stats() == (3, 1), reg.rdm_stats()
    elif k in ("measure_qubits", "postselect"):
        assert reg.collapse_stats()[0] == 3, reg.collapse_stats()


def run_subject(qc, shape, knobs, prefix, kind, ops, wants, final, twin, tmp_path):
    """the prefix in mode 2 on a fresh register, then `ops` against `wants` bit for bit; twin: run_twin's result"""
    L, M, Cn, a = shape
    S, twin_stats, twin_chains, twin_returned = twin
    done, ctx = [], {}
    keeps_compact = rm.compact_shape(shape) and prefix[-1][0] == "qcomp" and knobs.get("fuse_compact_lazy", 1) != 0
    try:
        with qc.Register(L, M) as reg:
            f0, c0 = pass_stats(qc, reg), sr.compact_chains(qc, reg)
            returned = run_prefix(qc, reg, prefix, tmp_path, ctx)
            assert repr(returned) == repr(twin_returned), f"the prefix returned {returned!r} here and {twin_returned!r} on the twin"
            for i, (op, want) in enumerate(zip(ops, wants)):
                done.append(op)
                try:
                    measures = sr.compact_measures(qc, reg)
                    got = sr.apply_to_register(qc, reg, op, lambda slot: str(tmp_path / f"slot{slot}.qcx"), ctx)
                    sr.compare(op, got, want)
                    if i == 0 and keeps_compact:
                        compact_source_is_reported(qc, reg, op, M, got, measures)
                    if i == 0 and kind in rm.QUEUED:          # (the switch of the mode ran the prefix; the gate behind it adds its own)
                        assert stats_delta(pass_stats(qc, reg), f0) == twin_stats, (stats_delta(pass_stats(qc, reg), f0), twin_stats)
                except Exception as e:
                    raise AssertionError(f"op {i}: {op!r}\n{type(e).__name__}: {e}") from e
                if op == ("read", 0, 1 << (L + M)) and i + 1 < len(ops) and kind not in rm.QUEUED + REPLACES_STATE:
                    assert stats_delta(pass_stats(qc, reg), f0) == twin_stats, (stats_delta(pass_stats(qc, reg), f0), twin_stats)
                    assert sr.compact_chains(qc, reg) - c0 == twin_chains
            sr.same(reg.read(), final, "the state the pair leaves")
    finally:
        ctx.clear()


def pair_ops(shape, follower):
    n = shape[0] + shape[1]
    return list(follower) + [("read", 0, 1 << n)] + tail_ops(n)


def run_pair(qc, ob, shape, knobs, prefix, follower, tmp_path, near=None, kind=None):
    """One (prefix, follower) pair under `knobs` (set for both registers, restored whatever happens).  Twin register: mode 2, the
    prefix, read -> S.  Model: a RegisterModel whose state is S.  Subject register: mode 2, the same prefix, then the follower,
    a read of the whole state, and the first exact gate (tail_ops) -- everything returned compared with the model bit for bit
    through sequence_replay.compare.  near: the oracle's state of the prefix (computed here when not given); kind: the
    follower's kind (its first op's name when not given).  No way out: a refused follower is a compared pair"""
    if near is None:
        m = rm.RegisterModel(ob, shape[0], shape[1])
        for op in prefix:
            rm.apply_to_model(m, op)
        near = m.a
    kind = kind or follower[-1][0]
    old = {k: qc.lib().qcx_tune_get(k.encode()) for k in KNOB_KEYS}
    try:
        qc.tune(**knobs)
        twin = run_twin(qc, shape, prefix, tmp_path)
        check_twin(twin, near, prefix, shape, truth_of(ob, shape, prefix))
        ops = pair_ops(shape, follower)
        wants, final = expectations(ob, shape, twin[0], ops)
        assert negative_zeros(final) == 0, "the model's gate leaves canonical zeros"
        run_subject(qc, shape, knobs, prefix, kind, ops, wants, final, twin, tmp_path)
    except Exception as e:
        raise AssertionError(f"shape (L, M, C, a) {shape} knobs {knobs}\nprefix = {prefix!r}\nfollower = {follower!r}\n{type(e).__name__}: {e}") from e
    finally:
        qc.tune(**old)
    return twin[0]
