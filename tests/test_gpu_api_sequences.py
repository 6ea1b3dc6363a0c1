"""GPU: random call sequences over the whole API of an unsharded register, and some twenty named chains, against the host model
of tests/register_model.py.  A register carries lazy state between calls (the strict flag, the owed zero pass, the gate queue, a
pending basis state, a compact circuit result, the fusion mode, a handed-out buffer pointer, the caller's stream) and every
entry point settles it in its own way; the files of the single features check each call next to a few hand-picked neighbours,
this one checks chains of them.  Everything a call returns is compared bit for bit (NaN matching NaN) with the model; full
reads are rare, so that the lazy forms live long.

Three vocabularies: the seeds below register_model.NSEEDS_V1 draw from the calls up to the matrix gates and are frozen
(tests/golden/sequence_digests.json); the others add the Pauli calls (expectation, expectation_sum, pauli_rotation), reads
through qcx_device_pointer (after which the register works in place for the rest of its life) and qcx_register_set_stream with
a non-blocking stream of PyTorch's, which is not ordered with the null stream the way the register's own stream is.
The seeds from register_model.NSEEDS on add the batched Pauli sum (expectation_batch) and the reduced density matrix, and run
under launch knobs of the fused engine as well (register_model.KNOBS_FUSED).  The replaying itself is tests/sequence_replay.py.

One seed alone:  QCX_SEQ_CASE=<seed> [QCX_SEQ_OPS=<k>] python -m pytest tests/test_gpu_api_sequences.py -m gpu -q -s -k random
(a failure prints the seed, the index of the failing op and the ops up to it as a Python literal)."""
import ctypes as C
import os

import numpy as np
import pytest

import register_model as rm
from sequence_replay import apply_to_register, bits, compact_chains, compact_measures, compare, run_ops
from sequence_replay import same, status_of  # noqa: F401  (tests/test_gpu_sharded_sequences.py takes them from here)

pytestmark = pytest.mark.gpu

KNOB_KEYS = sorted({k for d in rm.KNOBS_N9 + rm.KNOBS_ANY + rm.KNOBS_V2 + rm.KNOBS_FUSED for k in d})


def measure_last_stats(qc):
    s, b = C.c_uint(0), C.c_uint(0)
    qc.lib().qcx_measure_last_stats(C.byref(s), C.byref(b))
    return s.value, b.value


def chain_stats(qc, reg):
    v = C.c_ulong(0)
    assert qc.lib().qcx_chain_stats(reg._h, C.byref(v)) == 0
    return int(v.value)


# ---- random sequences ----------------------------------------------------------------------------------------------------------

def one_seed(qc, ob, seed, tmp_path):
    cfg, ops = rm.generate(ob, seed)
    limit = os.environ.get("QCX_SEQ_OPS")
    if limit:
        ops = ops[:int(limit)]
    old = {k: qc.lib().qcx_tune_get(k.encode()) for k in KNOB_KEYS}
    try:
        qc.tune(**cfg.knobs)
        run_ops(qc, ob, cfg.shapes, cfg.modes, ops, tmp_path, f"{cfg!r} ({len(ops)} ops)", compact=cfg.compact)
    finally:
        qc.tune(**old)


ONLY = os.environ.get("QCX_SEQ_CASE")


@pytest.mark.parametrize("seed", [int(ONLY)] if ONLY else range(rm.NSEEDS_V3))
def test_random_sequences_against_the_model(qc, ob, tmp_path, seed):
    one_seed(qc, ob, seed, tmp_path)


# ---- named chains ----------------------------------------------------------------------------------------------------------------

class Chain:
    """one register and its model, op by op; do() compares what the call returns and hands it back"""

    def __init__(self, qc, ob, L, M, mode, tmp_path, tag="a"):
        self.qc, self.ob, self.tmp, self.tag = qc, ob, tmp_path, tag
        self.reg = qc.Register(L, M)
        self.reg.set_fusion(mode)
        self.m = rm.RegisterModel(ob, L, M)
        self.n, self.dim = L + M, 1 << (L + M)
        self.done, self.ctx = [], {}

    def do(self, *op):
        self.done.append(op)
        try:
            got = apply_to_register(self.qc, self.reg, op, lambda slot: str(self.tmp / f"{self.tag}_slot{slot}.qcx"), self.ctx)
            compare(op, got, rm.apply_to_model(self.m, op))
        except Exception as e:
            raise AssertionError(f"op {len(self.done) - 1}: {op!r}\n{type(e).__name__}: {e}\nops = {self.done!r}") from e
        return got

    def state(self):
        return self.do("read", 0, self.dim)

    def close(self):
        self.reg.close()
        self.ctx.clear()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def test_chain_postselect_queue_sample_partial_write_controlled_gate(qc, ob, tmp_path):
    with Chain(qc, ob, 9, 5, 1, tmp_path) as c:
        c.do("fill", 11)
        c.do("postselect", 2, 3, 5)                                       # leaves the zero pass owed
        assert c.reg.collapse_stats() == (0, 1, 1)
        p0, g0 = c.reg.fusion_stats()
        c.do("h", 3); c.do("cphase", 4, 9, 0.3); c.do("h", 13); c.do("cphase", 0, 13, -1.2)
        assert c.reg.fusion_stats() == (p0, g0), "mode 1 queues the gates"
        c.do("sample", 5, 9)                                              # settles the queue
        assert c.reg.sample_stats()[0] >= 1
        c.do("write", 1000, 300, 6, "negzero")
        c.do("cu2", 1, 6, 2, 7)
        c.state()


@pytest.fixture(scope="module")
def shor_20(ob):
    """the Shor circuit's result at L = 15, M = 5 (the compact chain runs there), computed once; tests copy it"""
    n = 20
    w = np.zeros(2 << n)
    ob.reset(w, n)
    ob.quantum_computation(w, n, 5, 21, 2, threads=8)
    return w


def compact_start(c, shor_20):
    """reset + quantum_computation on the GPU, the shared oracle result into the model"""
    c.qc.reset_register(c.reg)
    c.qc.quantum_computation(21, 2, c.reg)
    c.m.a = shor_20.copy()
    c.done += [("reset",), ("qcomp", 21, 2)]


def test_chain_compact_marginal_inside_m_keeps_the_compact_form(qc, ob, tmp_path, shor_20):
    with Chain(qc, ob, 15, 5, 0, tmp_path) as c:
        k0 = compact_chains(qc, c.reg)
        compact_start(c, shor_20)
        assert compact_chains(qc, c.reg) == k0 + 1
        m0 = compact_measures(qc, c.reg)
        c.do("marginal", 1, 3)                                            # inside the M register: expanded into the buffer ...
        assert c.reg.marginal_stats() == (3, 1)
        c.do("sample", 3, 8)                                              # ... and the compact form is still what is scanned
        assert compact_measures(qc, c.reg) == m0 + 1 and c.reg.sample_stats()[0] >= 1
        c.do("marginal", 7, 4)
        assert c.reg.marginal_stats() == (1, 1) and compact_measures(qc, c.reg) == m0 + 2
        c.do("u1", 2, 3)
        c.do("marginal", 0, 6)
        assert c.reg.marginal_stats() == (0, 1)
        c.do("read", 12345, 4096)


def test_chain_compact_postselect_iqft_measure_marginal_two_qubit_gate(qc, ob, tmp_path, shor_20):
    with Chain(qc, ob, 15, 5, 0, tmp_path) as c:
        compact_start(c, shor_20)
        v = int(np.argmax(c.m.marginal(5, 4)))
        c.do("postselect", 5, 4, v)
        assert c.reg.collapse_stats() == (3, 1, 1)
        c.do("iqft")
        c.do("measure", 0.61)
        c.do("marginal", 3, 6)                                            # the pending basis state: no kernel
        assert c.reg.marginal_stats() == (2, 0)
        c.do("u2", 4, 17, 9)
        c.do("marginal", 3, 6)
        assert c.reg.marginal_stats() == (0, 1)
        c.do("read", 0, 1 << 14)
        c.do("total")


def test_chain_inf_window_error_keeps_state_then_finite_overwrite(qc, ob, tmp_path):
    with Chain(qc, ob, 8, 4, 0, tmp_path) as c:
        c.do("fill", 3)
        c.do("write", 700, 64, 21, "inf")
        c.do("cu1", 5, 1, 4)                                              # strict pass
        got = c.do("measure_qubits", 0, 0, 0.5)                           # the total is not finite: refused, state kept
        assert got[2] == rm.BAD_ARGUMENTS
        c.do("read", 600, 300)
        c.do("h", 7)                                                      # still strict
        c.do("write", 0, c.dim, 22, "negzero")                            # finite data over everything
        c.do("h", 0)
        c.do("postselect", 3, 2, 1)
        c.state()


def test_chain_measure_mode_switches_save_load(qc, ob, tmp_path):
    with Chain(qc, ob, 9, 5, 0, tmp_path) as c:
        c.do("fill", 8)
        c.do("measure", 0.37)
        c.do("fusion", -1)                                                # the flush writes the pending basis state
        c.do("u2", 0, 13, 5)
        c.do("fusion", 1)
        c.do("h", 6); c.do("cphase", 6, 2, 0.8); c.do("camodc", 21, 4, 9)
        c.do("save", 0)
        c.do("h", 1); c.do("u1", 3, 12); c.do("cphase", 1, 12, 2.0)
        c.do("load", 0)
        c.do("marginal", 4, 5)
        assert c.reg.marginal_stats() == (0, 1)
        c.state()


def test_chain_front_queued_behind_reset_then_postselect_is_not_basis_only(qc, ob, tmp_path):
    L, M = 9, 5
    with Chain(qc, ob, L, M, 1, tmp_path) as c:
        c.do("reset")
        for l in range(M, M + L):
            c.do("h", l)
        x = 2
        for l in range(M, M + L):
            c.do("camodc", 21, x, l)
            x = (x * x) % 21
        v = int(np.flatnonzero(c.m.marginal(0, M) > 0)[1])
        c.do("postselect", 0, M, v)
        assert c.reg.collapse_stats() == (0, 1, 1), "gates were queued: the basis-state shortcut does not apply"
        c.do("sample", 2, 17)
        assert c.reg.sample_stats()[0] >= 1
        c.do("iqft")
        c.state()


def test_chain_fill_over_a_compact_result(qc, ob, tmp_path):
    with Chain(qc, ob, 15, 5, 0, tmp_path) as c:
        k0 = compact_chains(qc, c.reg)
        qc.reset_register(c.reg); qc.quantum_computation(21, 2, c.reg)
        assert compact_chains(qc, c.reg) == k0 + 1
        c.do("fill", 4)
        c.do("marginal", 8, 3)
        assert c.reg.marginal_stats() == (0, 1)
        c.do("measure_qubits", 3, 4, 0.42)
        assert c.reg.collapse_stats() == (0, 1, 1)
        c.do("read", 99, 5000)
        c.do("total")


def test_chain_two_registers_nan_write_between_the_others_measurements(qc, ob, tmp_path):
    def run_b(with_a):
        out = []
        with Chain(qc, ob, 10, 4, 0, tmp_path, "b") as b, Chain(qc, ob, 7, 4, 1, tmp_path, "a") as a:
            b.do("fill", 5)
            b.do("h", 3)
            if with_a:
                a.do("fill", 1); a.do("h", 2)
            # (the first word of the scan's statistics counts records looked at closely, which depends on timing: it is compared
            #  across A's write, which borrows that word, and only the record count between the two runs)
            out.append(b.do("sample", 7, 17).tolist()); out.append(measure_last_stats(qc)[1])
            if with_a:
                before = measure_last_stats(qc)
                a.do("write", 100, 50, 3, "nan")
                a.do("h", 4)
                assert measure_last_stats(qc) == before, "a write into A changed the statistics of B's last scan"
            out.append(b.do("sample", 8, 8).tolist()); out.append(measure_last_stats(qc)[1])
            if with_a:
                a.do("read", 0, a.dim)
            out.append(b.do("measure", 0.77)); out.append(measure_last_stats(qc)[1])
            out.append(bits(b.state()).tolist())
            if with_a:
                a.do("cu1", 1, 5, 2)
                a.state()
        return out

    assert run_b(True) == run_b(False)


def test_chain_two_registers_device_table_scan_returns_the_borrowed_word(qc, ob, tmp_path):
    """qcx_diagonal_gate_device checks its table through the flag word that doubles as the last measurement scan's statistics: B's
    statistics survive A's call, whether the table passes or is refused, and the refusal leaves A's state alone.  B has n = 12:
    the smallest register whose scan is the parallel one (meas_min_log2), the only scan that writes those statistics -- at
    n = 10 the record count is 0"""
    import torch
    import diagonal_ref as dr
    with Chain(qc, ob, 8, 4, 0, tmp_path, "b") as b, Chain(qc, ob, 3, 4, 1, tmp_path, "a") as a:
        b.do("fill", 5)
        b.do("h", 3)
        a.do("fill", 1); a.do("h", 2)
        b.do("sample", 7, 17)
        before = measure_last_stats(qc)
        assert before[1] > 0, "B's scan must be the parallel one, which records its blocks"
        held = a.state()
        ph = np.linspace(-3.0, 3.0, 1 << 5)
        t = np.clip(np.cos(ph), -1, 1) + 1j * np.clip(np.sin(ph), -1, 1)
        dev = torch.from_numpy(t).cuda()
        torch.cuda.synchronize()
        qc.diagonal_gate(1, 5, dev, a.reg)
        assert measure_last_stats(qc) == before, "the scan of A's table changed the statistics of B's last scan"
        after = a.reg.read()
        same(after, dr.apply(held, a.n, 1, 5, t), "A behind the table that passed")
        t[9] = complex(0.5, np.nan)
        dev = torch.from_numpy(t).cuda()
        torch.cuda.synchronize()
        with pytest.raises(qc.QcxError) as e:
            qc.diagonal_gate(1, 5, dev, a.reg)
        assert e.value.status == rm.BAD_ARGUMENTS
        assert measure_last_stats(qc) == before, "the refused table's flag stayed in the statistics of B's last scan"
        assert np.array_equal(bits(a.reg.read()), bits(after)), "the refusal touched A's state"
        b.do("sample", 8, 8)                                              # B goes on from the state it had


def test_chain_circuit_queued_in_mode_1_sample_then_partial_write(qc, ob, tmp_path, shor_20):
    with Chain(qc, ob, 15, 5, 1, tmp_path) as c:
        k0, m0 = compact_chains(qc, c.reg), compact_measures(qc, c.reg)
        compact_start(c, shor_20)                                          # mode 1: everything is still queued
        assert compact_chains(qc, c.reg) == k0
        c.do("sample", 9, 4)                                              # the observer's flush keeps the result compact
        assert compact_chains(qc, c.reg) == k0 + 1 and compact_measures(qc, c.reg) == m0 + 1
        c.do("write", 4000, 128, 5, "negzero")                            # into the expanded register
        c.do("marginal", 0, 5)
        assert c.reg.marginal_stats() == (0, 1)
        c.do("h", 0)
        c.do("read", 3900, 400)


def test_chain_gates_queued_behind_a_pending_basis_state_are_seen(qc, ob, tmp_path):
    with Chain(qc, ob, 10, 0, 1, tmp_path) as c:
        c.do("reset")
        c.do("marginal", 0, 3)
        assert c.reg.marginal_stats() == (2, 0)
        c.do("h", 0); c.do("h", 9)
        c.do("marginal", 0, 3)                                            # gates are queued: not the host shortcut
        assert c.reg.marginal_stats() == (0, 1)
        c.do("measure", 0.3)
        c.do("h", 4)
        c.do("sample", 3, 9)
        assert c.reg.sample_stats()[0] >= 1
        c.do("measure", 0.9)
        c.do("postselect", 2, 4, (c.m.measure_state(0.5) >> 2) & 15)      # (the model's state is that basis state already)
        assert c.reg.collapse_stats() == (2, 0, 0)
        c.state()


def test_chain_negative_zeros_wait_for_the_first_gate(qc, ob, tmp_path):
    with Chain(qc, ob, 7, 4, 0, tmp_path) as c:
        c.do("write", 0, c.dim, 31, "negzero")
        c.do("marginal", 2, 5); c.do("sample", 1, 8); c.do("total")
        c.do("read", 0, c.dim)                                            # the -0 are still there
        c.do("save", 1)
        c.do("cphase", 10, 0, 0.4)                                        # canonicalises every amplitude, touched or not
        c.state()
        c.do("load", 1)
        c.do("fusion", 1)
        c.do("cphase", 10, 0, 0.4)
        c.do("cu2", 3, 0, 8, 2)
        c.state()


def test_chain_collapse_that_underflows_to_negative_zero_owes_the_zero_pass(qc, ob, tmp_path):
    """the collapse itself makes -0 (negative subnormals times s < 1/2) on a register whose zero pass was not owed: the next gate
    must still canonicalise every amplitude, also those it does not act on (the rotation rewrites every amplitude itself)"""
    for follow in (("cphase", 9, 10, 0.7), ("cu1", 10, 9, 6), ("cu2", 10, 9, 8, 7), ("h", 10), ("prot", 1 << 10 | 1 << 9, 1 << 9, 0.7)):
        with Chain(qc, ob, 7, 4, 0, tmp_path) as c:
            c.do("write", 0, c.dim, 77, "subnormal")
            c.do("cphase", 9, 10, 0.4)                                    # runs the pass the write owes; touches a quarter of the state
            v = int(np.argmax(c.m.marginal(0, 1)))
            p, st = c.do("postselect", 0, 1, v)
            assert st == 0 and p > 4.0
            made = (c.m.a == 0) & np.signbit(c.m.a)
            idx = np.arange(c.dim)
            alone = np.repeat((idx & 1 == v) & ((idx >> 10) & 1 == 0), 2)   # kept, and outside what the gates below act on (but H)
            assert np.count_nonzero(made & alone) > 50, "the chain must make -0 where the next gate does not act"
            c.do("read", 0, 64)                                           # the -0 are the state until a gate runs
            c.do(*follow)
            c.state()


def test_chain_pending_basis_state_through_the_flushing_observers(qc, ob, tmp_path):
    with Chain(qc, ob, 8, 4, 0, tmp_path) as c:
        c.do("fill", 2)
        c.do("measure", 0.52)
        c.do("total")
        c.do("measure", 0.1)
        c.do("norm2")
        c.do("measure", 0.99)
        c.do("save", 0)
        c.do("fill", 3)
        c.do("load", 0)
        c.do("iqft")
        c.do("measure_qubits", 4, 8, 0.35)
        c.do("qcomp", 15, 7)
        c.state()


# ---- named chains: the Pauli calls, the handed-out pointer, the caller's stream ------------------------------------------------------

def popcount(v):
    return bin(v).count("1")


def test_chain_pending_basis_state_answers_pauli_values_on_the_host(qc, ob, tmp_path):
    with Chain(qc, ob, 9, 5, 0, tmp_path) as c:
        for start in ("reset", "measure"):
            if start == "reset":
                c.do("reset")
                idx = 1
            else:
                c.do("fill", 5)
                idx = c.do("measure", 0.61)
                assert popcount(idx) >= 3, "the chain wants a basis state with several bits set"
            z = 0x2A5F
            assert c.do("expect", 0, z) == (-1.0 if popcount(idx & z) & 1 else 1.0)
            assert c.reg.expectation_stats() == (2, 0), "a Z string on a pending basis state is answered on the host"
            assert bits([c.do("expect", 0x0106, 0x0003)])[0] == 0, "a string with an X or a Y has no diagonal entry: +0"
            assert c.reg.expectation_stats() == (2, 0)
            total, values = c.do("expect_sum", 17, 6)
            assert c.reg.expectation_stats() == (2, 0) and set(np.abs(values).tolist()) <= {0.0, 1.0}
            c.do("marginal", 3, 6)
            assert c.reg.marginal_stats() == (2, 0), "the Pauli values left the basis state pending"
            c.do("prot", 0x1803, 0x0801, 1.1)                             # writes the basis state, then pairs of tiles
            c.do("expect", 0, z)
            assert c.reg.expectation_stats() == (0, 1)
            c.do("expect", 0x1803, 0x0801)
            c.state()


def test_chain_compact_result_pauli_values_keep_the_compact_form(qc, ob, tmp_path, shor_20):
    with Chain(qc, ob, 15, 5, 0, tmp_path) as c:
        k0 = compact_chains(qc, c.reg)
        compact_start(c, shor_20)
        assert compact_chains(qc, c.reg) == k0 + 1
        m0 = compact_measures(qc, c.reg)
        c.do("expect_sum", 23, 3)                                         # expanded into the register's stale buffer ...
        assert c.reg.expectation_stats() == (3, 3)
        c.do("sample", 3, 8)                                              # ... and the compact form is still what is scanned
        assert compact_measures(qc, c.reg) == m0 + 1
        c.do("marginal", 1, 3)                                            # inside the M register: borrows marg_buf after the Pauli tree did
        assert c.reg.marginal_stats() == (3, 1)
        c.do("expect", 0x81020, 0x01021)
        assert c.reg.expectation_stats() == (3, 1)
        c.do("sample", 4, 4)
        assert compact_measures(qc, c.reg) == m0 + 2
        c.do("prot", 0x40011, 0x40101, -2.3)                              # the compact form is history
        c.do("marginal", 0, 6)
        assert c.reg.marginal_stats() == (0, 1)
        c.do("expect", 0x40011, 0x40101)
        assert c.reg.expectation_stats() == (0, 1)
        c.do("read", 12345, 4096)


def test_chain_mode_1_queue_pauli_value_runs_it_rotation_flushes_uncounted(qc, ob, tmp_path):
    with Chain(qc, ob, 9, 5, 1, tmp_path) as c:
        c.do("fill", 7)
        c.do("flush")
        s0 = c.reg.fusion_stats()
        c.do("h", 3); c.do("cphase", 4, 9, 0.3); c.do("h", 13)
        assert c.reg.fusion_stats() == s0, "mode 1 queues the gates"
        c.do("expect", 0x2008, 0x0218)                                    # an observer: the queue runs first
        s1 = c.reg.fusion_stats()
        assert s1 != s0 and c.reg.expectation_stats() == (0, 1)
        c.do("h", 6); c.do("cphase", 6, 2, 0.8)
        assert c.reg.fusion_stats() == s1
        c.do("prot", 0x0040, 0x0041, 0.9)                                 # never queued: flushes the two gates ...
        s2 = c.reg.fusion_stats()
        assert s2 != s1
        c.do("prot", 0, 0x1040, -0.4)                                     # ... and nothing is counted for a rotation
        assert c.reg.fusion_stats() == s2
        total, values = c.do("expect_sum", 5, 0)                          # no terms: nothing runs
        assert bits([total])[0] == 0 and len(values) == 0 and c.reg.expectation_stats() == (0, 0)
        c.state()


@pytest.mark.parametrize("x_mask, z_mask", [(0, 0x405), (0x0C1, 0x441)], ids=["diagonal", "pairs"])
def test_chain_negative_zeros_rotation_rewrites_them_all(qc, ob, tmp_path, x_mask, z_mask):
    with Chain(qc, ob, 7, 4, 0, tmp_path) as c:
        c.do("write", 0, c.dim, 31, "negzero")
        c.do("expect", x_mask, z_mask)
        got = c.do("read", 0, c.dim)                                      # the -0 are still there
        assert np.count_nonzero((got == 0) & np.signbit(got)) > 100
        c.do("prot", x_mask, z_mask, 0.7)                                 # clears the owed zero pass without one: it writes 0 + ... everywhere
        assert not np.any((c.m.a == 0) & np.signbit(c.m.a)), "the definition leaves no -0"
        c.state()
        c.do("h", 10)                                                     # nothing is owed
        c.state()


def test_chain_non_finite_register_pauli_calls_stay_strict(qc, ob, tmp_path):
    with Chain(qc, ob, 8, 4, 0, tmp_path) as c:
        c.do("fill", 3)
        c.do("write", 700, 64, 21, "inf")
        v = c.do("expect", 0x0A3, 0x821)                                  # whatever the definition gives
        assert not np.isfinite(v)
        c.do("expect_sum", 9, 3)
        c.do("prot", 0x0A3, 0x821, 2.2)                                   # runs unchanged on a non-finite register
        c.do("read", 600, 300)
        c.do("h", 7)                                                      # still strict
        got = c.do("postselect", 0, 0, 0)                                 # the total is not finite: refused, state kept
        assert got[1] == rm.BAD_ARGUMENTS
        c.do("prot", 0, 0x003, -1.0)
        c.do("fill", 9)
        assert np.isfinite(c.do("expect", 0x0A3, 0x821))
        c.do("prot", 0x0A3, 0x821, 2.2)
        c.state()


def test_chain_handed_out_pointer_ends_the_compact_chains(qc, ob, tmp_path, shor_20):
    with Chain(qc, ob, 15, 5, 0, tmp_path) as c:
        k0 = compact_chains(qc, c.reg)
        compact_start(c, shor_20)
        assert compact_chains(qc, c.reg) == k0 + 1
        c.do("devptr", 12345, 4096)                                       # the compact result was expanded into the buffer
        k1, p1 = compact_chains(qc, c.reg), chain_stats(qc, c.reg)
        compact_start(c, shor_20)                                         # in place from now on: no compact copy, no second buffer
        assert compact_chains(qc, c.reg) == k1 and chain_stats(qc, c.reg) == p1
        c.do("read", 1 << 19, 1 << 14)
        c.do("devptr", 0, 1 << 14)
        c.do("iqft")
        assert compact_chains(qc, c.reg) == k1 and chain_stats(qc, c.reg) == p1
        c.do("devptr", 0, c.dim)                                          # (read_through_pointer: the same pointer all along)


def test_chain_handed_out_pointer_behind_a_basis_state_and_a_queue(qc, ob, tmp_path):
    with Chain(qc, ob, 9, 5, 0, tmp_path) as c:
        c.do("reset")
        c.do("devptr", 0, 64)                                             # the basis state is in the buffer
        c.do("fusion", 1)
        c.do("h", 13); c.do("h", 2); c.do("h", 7)
        c.do("devptr", 0, c.dim)
        idx = c.do("measure", 0.7)
        c.do("devptr", max(0, idx - 100), 200)
        c.do("h", 12)
        c.do("expect", 0x1000, 0)
        c.do("devptr", 0, c.dim)


def test_chain_callers_stream(qc, ob, tmp_path):
    """every kind of call on a non-blocking stream: the synchronous copies of write / read, the scan of what was written and the
    kernels before and after them must be ordered by the library, not by the null stream"""
    with Chain(qc, ob, 9, 5, 0, tmp_path) as c:
        c.do("stream", 1)
        c.do("fill", 3)
        c.do("write", 1000, 300, 6, "negzero")
        c.do("h", 3)
        c.do("read", 900, 500)
        c.do("write", 5000, 40, 8, "nan")
        c.do("cu1", 5, 1, 4)
        c.do("read", 4990, 60)
        c.do("fill", 4)
        c.do("measure", 0.37)
        c.do("fill", 5)
        c.do("sample", 5, 9)
        c.do("marginal", 2, 4)
        c.do("postselect", 2, 4, int(np.argmax(c.m.marginal(2, 4))))
        c.do("prot", 0x2011, 0x0013, 0.8)
        c.do("expect", 0x2011, 0x0013)
        c.do("iqft")
        c.do("save", 0)
        c.do("h", 1)
        c.do("load", 0)
        c.do("devptr", 8000, 500)
        c.do("fusion", 1)
        c.do("h", 4); c.do("cphase", 4, 11, 0.3)
        c.do("write", 0, 16, 9, "plain")
        c.do("total")
        c.state()
    with Chain(qc, ob, 11, 5, 0, tmp_path) as c:                          # the compact form
        c.do("stream", 1)
        k0, m0 = compact_chains(qc, c.reg), compact_measures(qc, c.reg)
        c.do("reset")
        c.do("qcomp", 21, 2)
        assert compact_chains(qc, c.reg) == k0 + 1, "reset + quantum_computation runs as a compact chain on the caller's stream too"
        c.do("sample", 2, 9)
        assert compact_measures(qc, c.reg) == m0 + 1
        c.do("stream", 0)
        c.do("h", 0)
        c.state()


def plain(v):
    """what a call returned, as something == compares bit for bit"""
    if v is None or isinstance(v, (int, np.integer)):
        return v
    if isinstance(v, tuple):
        return tuple(plain(e) for e in v)
    return bits(np.atleast_1d(v)).tolist()


def test_random_sequence_gives_the_same_on_the_callers_stream(qc, ob, tmp_path):
    """one op list of vocabulary 2, twice: on the register's own stream throughout, and with ("stream", 1) behind the first op"""
    seed = next(s for s in rm.seeds_of(2) if len(rm.Config(s).shapes) == 1 and not rm.Config(s).compact and sum(rm.Config(s).shapes[0][:2]) >= 13)
    cfg, ops = rm.generate(ob, seed)
    ops = [op for _, op in ops if op[0] != "stream"]
    (L, M, Cn, a), mode = cfg.shapes[0], cfg.mode

    def run(ops):
        out, ctx = [], {}
        with qc.Register(L, M) as reg:
            reg.set_fusion(mode)
            for i, op in enumerate(ops):
                got = apply_to_register(qc, reg, op, lambda slot: str(tmp_path / f"twice_slot{slot}.qcx"), ctx)
                if op[0] != "stream":
                    out.append((i - (1 if "stream" in ctx else 0), op[0], plain(got)))
            out.append(plain(reg.read()))
        ctx.clear()
        return out

    own = run(ops)
    callers = run(ops[:1] + [("stream", 1)] + ops[1:])
    assert len(own) == len(callers)
    for a_, b_ in zip(own, callers):
        assert a_ == b_, f"{cfg!r}: op {a_[:2]} returned something else on the caller's stream\nops = {ops!r}"


# ---- named chains: the batched Pauli sum and the reduced density matrix --------------------------------------------------------------

def test_the_model_restates_the_librarys_limits(qc):
    assert (rm.BATCH_WIDTH, rm.RDM_MAX) == (qc.pauli_batch_width(), qc.rdm_max_qubits())


def shared_mask_seed(n, k, shape=None):
    """a seed at which register_model.batch_terms(n, seed, k) draws k terms on ONE x_mask (of the given draw_masks shape)"""
    for seed in range(1, 200):
        xs = {x for _, x, _ in rm.batch_terms(n, seed, k)}
        if len(xs) == 1 and (shape is None or rm.mask_shape(min(xs)) == shape):
            return seed
    raise AssertionError("no such seed below 200")


def passes_of(qc, n, seed, k):
    return qc.pauli_batch_plan([x for _, x, _ in rm.batch_terms(n, seed, k)])[1]


def test_chain_compact_result_density_matrix_and_batch_keep_the_compact_form(qc, ob, tmp_path):
    with Chain(qc, ob, 11, 5, 0, tmp_path) as c:
        k0 = compact_chains(qc, c.reg)
        c.do("reset"); c.do("qcomp", 21, 2)
        assert compact_chains(qc, c.reg) == k0 + 1
        m0 = compact_measures(qc, c.reg)
        c.do("rdm", 2, 3)                                                 # expanded into the register's stale buffer ...
        assert c.reg.rdm_stats() == (3, 1)
        seed = shared_mask_seed(c.n, 40)
        got = c.do("expect_batch", seed, 40)
        assert got[3] == (3, 2), "more terms on one x_mask than a read serves: two reads, of the expanded compact result"
        c.do("marginal", 1, 3)                                            # inside the M register: borrows marg_buf after both did
        assert c.reg.marginal_stats() == (3, 1)
        c.do("rdm", 12, 4)                                                # the range above a unit's summed bits
        assert c.reg.rdm_stats() == (3, 1)
        got = c.do("expect_batch", 29, 6)
        assert got[3] == (3, passes_of(qc, c.n, 29, 6))
        assert compact_measures(qc, c.reg) == m0
        c.do("measure", 0.61)                                             # ... and the compact form is still what is scanned
        assert compact_measures(qc, c.reg) == m0 + 1
        c.do("rdm", 9, 4)                                                 # the pending basis state
        assert c.reg.rdm_stats() == (2, 0)
        c.state()


def test_chain_pending_basis_state_answers_density_matrix_and_batch_on_the_host(qc, ob, tmp_path):
    with Chain(qc, ob, 9, 5, 0, tmp_path) as c:
        for start in ("reset", "measure"):
            if start == "reset":
                c.do("reset")
            else:
                c.do("fill", 5)
                assert popcount(c.do("measure", 0.61)) >= 3, "the chain wants a basis state with several bits set"
            for first, num in [(0, 0), (0, 4), (3, 3), (7, 4), (10, 4), (13, 1)]:
                rho = c.do("rdm", first, num)
                assert c.reg.rdm_stats() == (2, 0), "a basis state's density matrix is answered on the host"
                assert np.count_nonzero(rho) == 1 and rho.sum() == 1.0
            for seed, k in [(shared_mask_seed(c.n, 40), 40), (17, 6), (3, 1)]:
                got = c.do("expect_batch", seed, k)
                assert got[3] == (2, 0) and set(np.abs(got[1]).tolist()) <= {0.0, 1.0}
            c.do("marginal", 3, 6)
            assert c.reg.marginal_stats() == (2, 0), "neither call wrote the basis state: it is still pending"
            c.do("sample", 4, 3)
            c.do("h", 12)
            c.do("rdm", 10, 4)
            assert c.reg.rdm_stats() == (0, 1)
            c.state()


def test_chain_mode_1_queue_is_run_by_density_matrix_and_by_batch(qc, ob, tmp_path):
    with Chain(qc, ob, 9, 5, 1, tmp_path) as c:
        c.do("fill", 7)
        c.do("flush")
        s0 = c.reg.fusion_stats()
        c.do("h", 3); c.do("cphase", 4, 9, 0.3); c.do("h", 13)
        assert c.reg.fusion_stats() == s0, "mode 1 queues the gates"
        c.do("rdm", 2, 3)                                                 # an observer: the queue runs first
        s1 = c.reg.fusion_stats()
        assert s1 != s0 and c.reg.rdm_stats() == (0, 1)
        c.do("h", 6); c.do("cphase", 6, 2, 0.8)
        assert c.reg.fusion_stats() == s1
        got = c.do("expect_batch", 11, 6)
        s2 = c.reg.fusion_stats()
        assert s2 != s1 and got[3] == (0, passes_of(qc, c.n, 11, 6))
        c.do("h", 0); c.do("camodc", 21, 4, 9)
        c.do("rdm", 11, 3)                                                # the range at and above bit 12 - num
        assert c.reg.fusion_stats() != s2
        got = c.do("expect_batch", 5, 0)                                  # no terms: nothing runs, nothing is flushed
        assert bits([got[0]])[0] == 0 and len(got[1]) == 0
        c.state()


def test_chain_owed_negative_zeros_are_still_owed_after_density_matrix_and_batch(qc, ob, tmp_path):
    with Chain(qc, ob, 7, 4, 0, tmp_path) as c:
        c.do("write", 0, c.dim, 31, "negzero")
        c.do("rdm", 4, 4)
        c.do("expect_batch", shared_mask_seed(c.n, 40), 40)
        c.do("rdm", 0, 2)
        got = c.do("read", 0, c.dim)                                      # the -0 are still there
        assert np.count_nonzero((got == 0) & np.signbit(got)) > 100
        c.do("cphase", 10, 0, 0.4)                                        # canonicalises every amplitude, touched or not
        assert not np.any((c.m.a == 0) & np.signbit(c.m.a))
        c.state()
        c.do("write", 0, c.dim, 32, "negzero")
        c.do("expect_batch", 8, 3)
        c.do("rdm", 7, 4)
        c.do("cu1", 3, 8, 2)
        c.state()


def test_chain_non_finite_register_stays_strict_through_density_matrix_and_batch(qc, ob, tmp_path):
    with Chain(qc, ob, 8, 4, 0, tmp_path) as c:
        c.do("fill", 3)
        c.do("write", 700, 64, 21, "inf")
        rho = c.do("rdm", 8, 4)                                           # whatever the definition gives
        assert not np.all(np.isfinite(rho))
        got = c.do("expect_batch", shared_mask_seed(c.n, 40), 40)
        assert not np.isfinite(got[0])
        c.do("rdm", 2, 2)
        c.do("h", 7)                                                      # still the strict gate: the oracle's products, NaN / Inf included
        c.do("read", 600, 300)
        got = c.do("postselect", 0, 0, 0)                                 # the total is not finite: refused, state kept
        assert got[1] == rm.BAD_ARGUMENTS
        c.do("cphase", 2, 11, 0.9)
        c.do("fill", 9)
        assert np.all(np.isfinite(c.do("rdm", 8, 4)))
        c.state()


def test_chain_density_matrix_and_batch_behind_the_handed_out_pointer_on_a_callers_stream(qc, ob, tmp_path):
    with Chain(qc, ob, 9, 5, 0, tmp_path) as c:
        c.do("stream", 1)
        c.do("fill", 3)
        c.do("devptr", 0, 64)                                             # in place from here on
        c.do("h", 13)
        c.do("rdm", 10, 4)
        c.do("write", 1000, 300, 6, "negzero")
        got = c.do("expect_batch", shared_mask_seed(c.n, 40, 2), 40)      # pairs of tiles
        assert got[3] == (0, 2)
        c.do("prot", 0x2011, 0x0013, 0.8)
        c.do("rdm", 0, 4)
        c.do("devptr", 900, 500)
        c.do("fusion", 1)
        c.do("h", 4); c.do("cphase", 4, 11, 0.3)
        c.do("expect_batch", 21, 6)
        c.do("stream", 0)
        c.do("h", 2)
        c.do("rdm", 8, 4)
        c.do("reset")
        c.do("rdm", 0, 1)
        assert c.reg.rdm_stats() == (2, 0)
        c.do("devptr", 0, c.dim)


def last_stats(reg):
    return {"marginal": reg.marginal_stats(), "expectation": reg.expectation_stats(), "rdm": reg.rdm_stats(), "collapse": reg.collapse_stats()}


BATCH_OF_THREE = [(0.5, 0x2011, 0x0013), (-1.25, 0x2011, 0x8100), (2.0, 0, 0x0A05)]       # two x_masks: two reads of the state
# (op, the getter it answers to): what every state below is asked, in this order
OBSERVERS = [(("marginal", 8, 3), "marginal"), (("marginal", 1, 2), "marginal"), (("expect", 0x2011, 0x0013), "expectation"),
             (("expect_batch",), "expectation"), (("rdm", 2, 2), "rdm"), (("measure_qubits", 3, 4, 0.5), "collapse")]
# (source, state reads[, state writes]) of the callee behind each of OBSERVERS, per state: read off the build before the observers'
# statistics became one struct and one getter body, not reasoned
OWN_STATS = {
    "basis":   [(2, 0), (2, 0), (2, 0), (2, 0), (2, 0), (2, 0, 0)],
    "compact": [(1, 1), (3, 1), (3, 1), (3, 2), (3, 1), (3, 1, 1)],
    "filled":  [(0, 1), (0, 1), (0, 1), (0, 2), (0, 1), (0, 1, 1)],
}


def test_chain_one_observers_last_call_statistics_are_its_own(qc, ob, tmp_path):
    """the four *_last_stats getters behind every observer call, in three states of ONE register: the callee's pair is the
    documented one, the others keep what they held -- but for measure_qubits, which runs the marginal and sets its pair too.
    M = 4 and more than 12 qubits (the tiled Pauli and density-matrix kernels); L = 12 and not 9, because a register of 13 qubits
    cannot hold a compact result: compact_chain wants L + 2 >= 14 for the four residues of C = 15 (register_model.COMPACT_SHAPES)"""
    with Chain(qc, ob, 12, 4, 0, tmp_path) as c:
        for state in ("basis", "compact", "filled"):
            if state == "basis":
                c.do("reset")
            elif state == "compact":
                k0 = compact_chains(qc, c.reg)
                c.do("reset"); c.do("qcomp", 15, 7)
                assert compact_chains(qc, c.reg) == k0 + 1
            else:
                c.do("fill", 6)
            for (op, getter), own in zip(OBSERVERS, OWN_STATS[state]):
                before = last_stats(c.reg)
                if op[0] == "expect_batch":                               # (Chain's op runs expectation_sum behind the batch)
                    got = c.reg.expectation_batch([(cf, (x, z)) for cf, x, z in BATCH_OF_THREE])
                    want = c.m.expectation_batch(BATCH_OF_THREE)
                    same([got[0]], [want[0]], "the batch's sum"); same(got[1], want[1], "the values of the batch's terms")
                else:
                    c.do(*op)
                after = last_stats(c.reg)
                assert after[getter] == own, f"{state}: {op!r} left {getter} statistics {after[getter]}"
                if getter == "collapse":                                  # (a range that begins inside the M register: one source)
                    assert after["marginal"] == own[:2], f"{state}: measure_qubits runs the marginal: {after['marginal']}"
                    before["marginal"] = after["marginal"]
                before[getter] = after[getter]
                assert after == before, f"{state}: {op!r} moved another call's statistics: {before} -> {after}"
        c.state()


# marginal, density matrix and batch all borrow one scratch area of the register (marg_buf, grown by marg_reserve): sizes that
# grow and shrink; (first, num) of a marginal go up to its 2^12 outcomes, far more than the few rows of a density matrix
INTERLEAVED = [("marginal", 0, 1), ("rdm", 0, 4), ("marginal", 0, 12), ("rdm", 5, 1), ("marginal", 3, 2), ("rdm", 9, 4),
               ("expect_batch", 7, 40), ("marginal", 2, 9), ("rdm", 0, 0), ("marginal", 0, 0), ("rdm", 10, 4), ("marginal", 1, 12),
               ("expect_batch", 9, 6), ("rdm", 3, 3), ("marginal", 8, 5), ("rdm", 8, 4)]


def test_chain_marginal_density_matrix_marginal_growing_and_shrinking_on_one_register(qc, ob, tmp_path):
    with Chain(qc, ob, 9, 5, 0, tmp_path) as c:
        c.do("fill", 12)
        for op in INTERLEAVED:
            c.do(*op)
            if op[0] == "rdm":
                assert c.reg.rdm_stats() == (0, 1)
        c.do("h", 5)
        for op in INTERLEAVED[::-1]:
            c.do(*op)
        c.state()


def test_chain_marginal_density_matrix_marginal_alternating_between_two_registers(qc, ob, tmp_path):
    small = [(k, min(f, 4), min(v, 4)) if k != "expect_batch" else (k, f, v) for k, f, v in INTERLEAVED]      # ranges that fit n = 9
    with Chain(qc, ob, 9, 5, 0, tmp_path, "a") as a, Chain(qc, ob, 9, 0, 1, tmp_path, "b") as b:
        a.do("fill", 12); b.do("fill", 13)
        b.do("h", 3); b.do("cphase", 2, 7, 0.4)                           # queued in mode 1
        for k, op in enumerate(INTERLEAVED):
            a.do(*op)
            b.do(*small[(k + 5) % len(small)])
            if k == 7:
                a.do("postselect", 2, 3, int(np.argmax(a.m.marginal(2, 3))))
                b.do("h", 8)
        a.state(); b.state()


def test_chain_forty_terms_on_one_x_mask_take_two_reads(qc, ob, tmp_path):
    for L, M, shape in ((6, 0, 1), (9, 5, 0), (9, 5, 1), (9, 5, 2)):       # a partial unit; a diagonal string, one tile, pairs of tiles
        with Chain(qc, ob, L, M, 0, tmp_path) as c:
            c.do("fill", 21 + shape)
            seed = shared_mask_seed(c.n, 40, shape)
            assert passes_of(qc, c.n, seed, 40) == 2
            got = c.do("expect_batch", seed, 40)
            assert got[3] == (0, 2), f"expectation_stats() {got[3]}"
            got = c.do("expect_batch", shared_mask_seed(c.n, 6, shape), 6)
            assert got[3] == (0, 1)
            c.state()
