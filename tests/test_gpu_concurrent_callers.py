"""GPU: the library called from several threads at once.  include/qcx.h promises that distinct registers may be used from
distinct threads (one register by one thread at a time; the knobs are process-wide), and the library is written for it: a
per-device workspace -- the look-back slots and the clean-up list of the measurement, the table and the staging buffer of the
modular multiply, the sample buffers, the pinned result words -- that is reallocated as sizes grow, reused across registers and
streams and guarded by one lock per device, a thread-local last error, knob snapshots per call.

Phase 1, on the main thread: every op list runs on the host model (tests/register_model.py) and everything it returns is
recorded.  Phase 2: one Python thread per list replays it on the GPU (tests/sequence_replay.py) against the recorded values,
bit for bit; ctypes releases the GIL, so the calls overlap inside the library.  Every thread has registers, a directory and,
where the ops ask for one, a PyTorch stream of its own; all start on one barrier.  The seeds are ones that run under the
default knobs.

A thread that does not come back is a hang: join() gets 20 times the wall time of the same replay on one thread (measured in the
same test), 60 s at least -- a guard, not a measurement -- and when it runs out the whole session ends (pytest.exit) with
nothing more started on the GPU."""
import ctypes as C
import threading
import time

import numpy as np
import pytest

import register_model as rm
from sequence_replay import apply_to_register, compare, record_ops, run_ops, same

pytestmark = pytest.mark.gpu

THREADS = 4


def plain_seed(ob, want):
    """the first seed without knobs whose Config and op list `want` accepts"""
    for seed in range(rm.NSEEDS_V3):
        cfg = rm.Config(seed)
        if not cfg.knobs and want(cfg, None):
            ops = rm.generate(ob, seed)[1]
            if want(cfg, ops):
                return cfg, ops
    raise AssertionError("no such seed")


def kinds(ops):
    return {op[0] for _, op in ops}


class Job:
    """one thread's work: an op list, what the model gave for it, the registers it runs on"""

    def __init__(self, ob, header, shapes, modes, ops, compact=False):
        self.header, self.shapes, self.modes, self.ops, self.compact = header, shapes, modes, ops, compact
        self.recorded = record_ops(ob, shapes, ops)

    def run(self, qc, ob, tmp):
        tmp.mkdir(exist_ok=True)
        run_ops(qc, ob, self.shapes, self.modes, self.ops, tmp, self.header, compact=self.compact, recorded=self.recorded)


def job_of_seed(ob, cfg, ops):
    return Job(ob, f"{cfg!r} ({len(ops)} ops)", cfg.shapes, cfg.modes, ops, cfg.compact)


def run_threads(bodies, headers, limit):
    """bodies[i]() on a thread of its own, all released by one barrier; the first exception is re-raised here under its header.
    A thread still alive after `limit` seconds ends the session"""
    barrier = threading.Barrier(len(bodies))
    errors = [None] * len(bodies)

    def body(i):
        try:
            barrier.wait()
            bodies[i]()
        except BaseException as e:                                       # (handed to the main thread)
            barrier.abort()
            errors[i] = e

    threads = [threading.Thread(target=body, args=(i,), daemon=True, name=f"caller-{i}") for i in range(len(bodies))]
    deadline = time.monotonic() + limit
    for t in threads:
        t.start()
    for t in threads:
        t.join(max(0.0, deadline - time.monotonic()))
    stuck = [t.name for t in threads if t.is_alive()]
    if stuck:
        pytest.exit(f"concurrent callers: {stuck} did not come back within {limit:.0f} s ({headers}); nothing more is run", returncode=3)
    for i, e in enumerate(errors):
        if e is not None and not isinstance(e, threading.BrokenBarrierError):
            raise AssertionError(f"thread {i}: {headers[i]}\n{type(e).__name__}: {e}") from e
    assert not any(errors), errors


def replay_concurrently(qc, ob, tmp_path, jobs, gates=None):
    """every job once on this thread (the wall time the hang guard is scaled from), then all of them at once.
    gates[i]: an Event thread i waits for before its first op (set by the thread before it)"""
    t0 = time.monotonic()
    for i, job in enumerate(jobs):
        job.run(qc, ob, tmp_path / f"alone{i}")
    alone = time.monotonic() - t0
    limit = max(60.0, 20.0 * alone)

    def body(i):
        def run():
            if gates and gates[i][0] is not None:
                assert gates[i][0].wait(limit), "the thread before this one never got through its first round"
            jobs[i].run(qc, ob, tmp_path / f"thread{i}")
        return run

    for _, event in gates or []:
        event.clear()                                                    # (set by the runs above)
    t0 = time.monotonic()
    run_threads([body(i) for i in range(len(jobs))], [j.header for j in jobs], limit)
    print(f"{len(jobs)} op lists ({sum(len(j.ops) for j in jobs)} ops): {alone:.2f} s one after the other, {time.monotonic() - t0:.2f} s on "
          f"{len(jobs)} threads (limit {limit:.0f} s)")


# ---- (a) four different seeds ------------------------------------------------------------------------------------------------------

def test_four_different_sequences_at_once(qc, ob, tmp_path):
    """a seed with two registers, a compact seed at n = 16, a seed of vocabulary 2 with a handed-out pointer and a caller's
    stream, a seed of vocabulary 3"""
    picks = [plain_seed(ob, lambda c, ops: len(c.shapes) == 2),
             plain_seed(ob, lambda c, ops: c.compact),
             plain_seed(ob, lambda c, ops: c.vocab == 2 and len(c.shapes) == 1 and not c.compact and c.shapes[0][1] >= 4
                        and (ops is None or {"devptr", "stream"} <= kinds(ops))),
             plain_seed(ob, lambda c, ops: c.vocab == 3 and len(c.shapes) == 1 and not c.compact and sum(c.shapes[0][:2]) >= 12
                        and (ops is None or {"rdm", "expect_batch"} <= kinds(ops)))]
    assert len({c.seed for c, _ in picks}) == THREADS
    replay_concurrently(qc, ob, tmp_path, [job_of_seed(ob, c, ops) for c, ops in picks])


# ---- (b) the same seed on every thread -------------------------------------------------------------------------------------------------

def test_the_same_sequence_on_every_thread(qc, ob, tmp_path):
    """sizes, tables and look-back areas are identical: whatever one thread leaves in the workspace fits the next one exactly"""
    cfg, ops = plain_seed(ob, lambda c, ops: c.vocab == 3 and len(c.shapes) == 1 and not c.compact and c.shapes[0][1] >= 4
                          and sum(c.shapes[0][:2]) >= 12 and (ops is None or {"camodc", "measure", "sample", "rdm"} <= kinds(ops)))
    job = job_of_seed(ob, cfg, ops)
    replay_concurrently(qc, ob, tmp_path, [job] * THREADS)


# ---- (c) scratch churn -----------------------------------------------------------------------------------------------------------------

CHURN_SHAPES = [(5, 4, 15, 7), (7, 4, 15, 7), (8, 5, 21, 2), (9, 5, 21, 2)]          # n = 9, 11, 13, 14
CHURN_ROUNDS = 12


def churn_ops(shape, seed):
    """rounds of: a dense state, a modular multiply whose control lies INSIDE the M register (the table path: the per-device
    table and staging buffer), then every call that borrows per-device or per-register scratch, and a measurement"""
    L, M, Cn, a = shape
    n = L + M
    rs = np.random.RandomState(seed)
    ops = []
    for r in range(CHURN_ROUNDS):
        ops.append((0, ("fill", seed + r)))
        ops.append((0, ("camodc", Cn, int(rs.randint(2, 4 * Cn)), int(rs.randint(0, M)))))
        ops.append((0, ("sample", seed + r, 17)))
        num = int(rs.randint(1, min(n, 10) + 1))
        ops.append((0, ("marginal", int(rs.randint(0, n - num + 1)), num)))
        ops.append((0, ("total",)))
        ops.append((0, ("norm2",)))
        num = int(rs.randint(0, rm.RDM_MAX + 1))
        ops.append((0, ("rdm", int(rs.randint(0, n - num + 1)), num)))
        ops.append((0, ("expect_batch", seed + r, int(rs.choice([6, 40])))))
        ops.append((0, ("measure", float(rs.uniform(0, 1)))))
        ops.append((0, ("read", int(rs.randint(0, 1 << (n - 1))), 64)))
    ops.append((0, ("read", 0, 1 << n)))
    return ops


def test_scratch_churn_smallest_register_first(qc, ob, tmp_path):
    """registers of n = 9, 11, 13 and 14: thread k + 1 begins when thread k is through its first round, so every larger register
    makes the workspace grow while the smaller ones are using it"""
    jobs = [Job(ob, f"scratch churn, shape {s}", [s], [(0, -1)[k % 2]], churn_ops(s, 100 * k + 7)) for k, s in enumerate(CHURN_SHAPES)]
    assert all(0 <= op[3] < s[1] for j, s in zip(jobs, CHURN_SHAPES) for _, op in j.ops if op[0] == "camodc"), "controls inside M"
    per_round = (len(jobs[0].ops) - 1) // CHURN_ROUNDS
    events = [threading.Event() for _ in jobs]
    gates = [(events[k - 1] if k else None, events[k]) for k in range(len(jobs))]
    jobs = [ChurnJob(ob, j.header, j.shapes, j.modes, j.ops, per_round, events[k]) for k, j in enumerate(jobs)]
    replay_concurrently(qc, ob, tmp_path, jobs, gates)


class ChurnJob(Job):
    """a Job that sets `event` when the first round of its list is through (run_ops has no hook for that: the list is replayed
    here op by op with the same helpers, on one register in its starting mode)"""

    def __init__(self, ob, header, shapes, modes, ops, per_round, event):
        super().__init__(ob, header, shapes, modes, ops)
        self.per_round, self.event = per_round, event

    def run(self, qc, ob, tmp):
        tmp.mkdir(exist_ok=True)
        (L, M, Cn, a), done = self.shapes[0], []
        try:
            with qc.Register(L, M) as reg:
                reg.set_fusion(self.modes[0])
                ctx = {}
                for i, (_, op) in enumerate(self.ops):
                    done.append(op)
                    try:
                        compare(op, apply_to_register(qc, reg, op, lambda slot: str(tmp / f"slot{slot}.qcx"), ctx), self.recorded[0][i])
                    except Exception as e:
                        raise AssertionError(f"{self.header}\nop {i}: {op!r}\n{type(e).__name__}: {e}\nops = {done!r}") from e
                    if i + 1 == self.per_round:
                        self.event.set()
                same(reg.read(), self.recorded[1][0], "the final state")
        finally:
            self.event.set()                                             # (whatever happened: nobody waits for this thread for ever)


# ---- (d) the last error is the calling thread's ------------------------------------------------------------------------------------------

def test_last_error_is_thread_local(qc):
    """two threads provoke refusals whose texts differ (masks past n, on registers of different n) between barriers; each reads
    its own text, and the main thread's last error is what it was"""
    lib = qc.lib()
    rounds, sizes = 8, (9, 12)
    step = threading.Barrier(len(sizes))
    v = C.c_double(0.0)
    with qc.Register(6, 0) as mine:
        assert lib.qcx_pauli_expectation(mine._h, 1 << 6, 0, C.byref(v)) == rm.BAD_QUBIT
        before = lib.qcx_last_error().decode()
        assert "0x40" in before and "6 qubits" in before, before

        def caller(n):
            def run():
                out = C.c_double(0.0)
                with qc.Register(n, 0) as reg:
                    reg.fill_random(n)
                    for r in range(rounds):
                        x, z = (1 << n) | (r + 1), (r + 1) << 3
                        step.wait()
                        assert lib.qcx_pauli_expectation(reg._h, x, z, C.byref(out)) == rm.BAD_QUBIT
                        step.wait()                                      # (the other thread's refusal has happened as well)
                        text = lib.qcx_last_error().decode()
                        assert f"{x:#x} / {z:#x}" in text and f"the {n} qubits" in text, f"round {r} on n = {n}: {text!r}"
                        assert reg.expectation((r + 1, 0)) == reg.expectation((r + 1, 0))       # (a call that succeeds in between)
                        assert lib.qcx_last_error().decode() == text, "a successful call leaves the last error as it is"
            def guarded():
                try:
                    run()
                except BaseException:
                    step.abort()                                         # (the other thread must not wait for this one)
                    raise
            return guarded

        try:
            run_threads([caller(n) for n in sizes], [f"n = {n}" for n in sizes], 60.0)
        finally:
            step.abort()
        assert lib.qcx_last_error().decode() == before, "another thread's refusal reached the main thread's last error"
