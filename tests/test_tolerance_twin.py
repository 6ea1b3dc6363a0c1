"""CPU: the schedule of tests/tolerance_twin.py (what tests/test_gpu_tolerance_observers.py replays in the tolerance mode) reaches
what it claims, its op lists are the committed ones (tests/golden/tolerance_digests.json), and the new op of the sequence
helpers, prot_batch (qcx_pauli_rotation_batch), is the loop of the single rotation on the model."""
import hashlib
import json
import os

import numpy as np
import pytest

import register_model as rm
import tolerance_twin as tt


@pytest.fixture(scope="module")
def sched(ob):
    return tt.schedule(ob)


def digest(ops):
    return hashlib.sha256(repr(ops).encode()).hexdigest()


def test_schedule_reaches_every_pair_shape_and_knob(sched):
    pairs = [(p, shape, knobs, f) for (p, shape), lst in sched.items() for knobs, f, _ in lst]
    print(f"{len(pairs)} pairs over {len(sched)} (prefix kind, shape) cases, {min(map(len, sched.values()))} to {max(map(len, sched.values()))} per case")
    # (1) every (prefix kind, follower kind) pair
    missing = [(p, f) for p in tt.PREFIX_KINDS for f in tt.FOLLOWER_KINDS if not any(q == p and g == f for q, _, _, g in pairs)]
    assert not missing, missing
    # (2) every (shape, follower kind) pair a shape allows
    missing = [(s, f) for s in tt.SHAPES for f in tt.FOLLOWER_KINDS
               if any(tt.pair_is_legal(p, f, s) for p in tt.PREFIX_KINDS) and not any(t == s and g == f for _, t, _, g in pairs)]
    assert not missing, missing
    impossible = [(s, f) for s in tt.SHAPES for f in tt.FOLLOWER_KINDS if not any(tt.pair_is_legal(p, f, s) for p in tt.PREFIX_KINDS)]
    assert sorted(impossible) == sorted(((13, 0, 1, 1), f) for f in ("camodc", "qcomp")), impossible
    # (3) every knob dict with every prefix kind
    missing = [(p, k) for p in tt.PREFIX_KINDS for k in tt.KNOBS if not any(q == p and kn == k for q, _, kn, _ in pairs)]
    assert not missing, missing
    for p, shape, knobs, f in pairs:
        assert tt.pair_is_legal(p, f, shape) and tt.knobs_are_legal(knobs, shape), (p, shape, knobs, f)
    assert max(map(len, sched.values())) <= 12, "a test of a few seconds holds a dozen pairs at the most"


def test_followers_are_what_the_kinds_say(sched):
    """a follower's list holds its kind's call; the kinds that queue in mode 2 stand behind a switch to an exact mode; no op of
    a follower queues a gate in mode 2; the batches draw all three sizes"""
    sizes = set()
    for (p, shape), lst in sched.items():
        for knobs, f, ops in lst:
            assert f in [op[0] for op in ops], (f, ops)
            if f in rm.QUEUED:
                assert ops[0][0] == "fusion" and ops[0][1] in (-1, 0, 1) and len(ops) == 2, ops
            else:
                assert not any(op[0] in rm.QUEUED for op in ops), ops
            if f == "prot_batch":
                sizes.add(ops[0][2])
            for op in ops:
                if op[0] == "write":
                    assert op[4] in ("plain", "negzero"), op
    assert sizes == {1, 5, 40}, sizes


def test_prefixes_hold_merged_runs_and_the_oracle_state_is_shared(ob):
    for p in tt.PREFIX_KINDS:
        for shape in tt.SHAPES:
            if not tt.prefix_is_legal(p, shape):
                continue
            ops = tt.prefix_ops(p, shape)
            assert ops == tt.prefix_ops(p, shape)
            assert tt.holds_a_merged_run(ops), (p, shape)
            if p == "program":
                gates = ops[1:]
                assert 30 <= len(gates) <= 60 and {g[0] for g in gates} <= {"h", "cphase", "camodc"}
                behind_h = [k for k in range(2, len(ops) - 1) if ops[k - 1] == ("h", ops[k][1]) and ops[k][0] == ops[k + 1][0] == "cphase" and ops[k][1] == ops[k + 1][1]]
                assert behind_h, "a run of phases behind a Hadamard on their control: the shape of a merged round"
    a, _ = tt.oracle_state(ob, "sparse", tt.SHAPES[0])
    assert a is tt.oracle_state(ob, "sparse", tt.SHAPES[0])[0] and not a.flags.writeable
    with pytest.raises(ValueError):
        a[0] = 1.0


def test_schedule_generates_the_committed_op_lists(ob, sched):
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tolerance_digests.json")) as f:
        golden = json.load(f)
    mine = {tt.key_of(p, shape): digest((tt.prefix_ops(p, shape), [(sorted(k.items()), f_, ops) for k, f_, ops in lst])) for (p, shape), lst in sched.items()}
    assert sorted(mine) == sorted(golden["pairs"])
    drifted = [k for k in mine if mine[k] != golden["pairs"][k]]
    assert not drifted, f"the op lists of these cases changed: {drifted}"
    big = tt.big_case(ob, rm_state(ob, tt.BIG_SHAPE))
    assert [f for _, f, _ in big] == list(tt.BIG_FOLLOWERS)
    assert digest([(sorted(k.items()), f_, ops) for k, f_, ops in big]) == golden["big"]
    assert digest([tt.KNOBS, tt.SHAPES, tt.BIG_SHAPE]) == golden["knobs_and_shapes"]


def rm_state(ob, shape):
    m = rm.RegisterModel(ob, shape[0], shape[1])
    for op in tt.prefix_ops("shor", shape):
        rm.apply_to_model(m, op)
    return m.a


def test_rotation_batch_op_is_the_loop_of_the_single_rotation(ob):
    import test_gpu_pauli_rotation_batch as direct
    assert rm.ROTATION_THETAS == direct.THETAS
    n = 13
    shapes = set()
    for seed, k in ((3, 1), (4, 5), (5, 40)):
        terms = rm.rotation_terms(n, seed, k)
        assert len(terms) == k and terms == rm.rotation_terms(n, seed, k)
        assert all(0 <= x < 1 << n and 0 <= z < 1 << n and th in rm.ROTATION_THETAS for (x, z), th in terms)
        shapes |= {rm.mask_shape(x) for (x, _), _ in terms}
        a, b = rm.RegisterModel(ob, n, 0), rm.RegisterModel(ob, n, 0)
        a.fill_random(seed); b.fill_random(seed)
        assert rm.apply_to_model(a, ("prot_batch", seed, k)) is None
        for (x, z), th in terms:
            rm.apply_to_model(b, ("prot", x, z, th))
        assert np.array_equal(a.a.view(np.uint64), b.a.view(np.uint64))
        assert not np.array_equal(a.a, ob.fill_random(n, seed)), "the rotations change the state"
    assert shapes == {0, 1, 2}, "all three unit shapes of the rotation kernel"
