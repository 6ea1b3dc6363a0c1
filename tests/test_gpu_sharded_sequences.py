"""GPU: random call sequences over the API of a SHARDED register (qcx_register_create_sharded, csrc/qcx_sharded.inc.h), and named
chains, against the host model of tests/register_model.py -- the same model as for an unsharded register: a sharded register
promises the same bits for the calls it supports.  Between calls it keeps a logical -> physical qubit layout that trades leave
swapped, a gate queue in every fusion mode, a pending basis state, a circuit front written per shard, a compact circuit on a
companion register, an owed zero pass, relays and the slice / window geometry, and every entry point settles these in its own
way; tests/test_gpu_sharded_c.py checks each feature in one scenario, this file checks chains of them: partial writes and
windows across shard boundaries, mode switches, measurements, save / load, resets and the refused calls while the layout is
swapped, gates are queued or a compact result is due.  The shards are spread over the visible GPUs (qc.spread_devices), as in
test_gpu_sharded_c.py.  tests/test_sharded_sequences_dry.py replays the same lists on a dry-run register without a GPU.

Everything a call returns is compared bit for bit with the model, except norm2 (a tree sum: within 1e-9, the model's rule).

test_tiny_registers runs the seeds whose registers have n_local < 2 k + 6 (sh_set_slices trades runs shorter than 1 KiB there;
the smallest registers the library accepts: 2 shards from n = 3, 4 from n = 6, 8 from n = 9) as a test of their own.

One seed alone:  QCX_SHSEQ_CASE=<seed> [QCX_SHSEQ_OPS=<k>] python -m pytest tests/test_gpu_sharded_sequences.py -m gpu -q -s -k "random or tiny"
(a failure prints the seed, the index of the failing op and the ops up to it as a Python literal)."""
import os

import numpy as np
import pytest

import register_model as rm
from test_gpu_api_sequences import compact_chains, compact_measures, compare, same, status_of

pytestmark = pytest.mark.gpu

ENV_KEYS = ("QCX_SHARD_SLICES_LOG2", "QCX_SHARD_OVERLAP", "QCX_SHARD_FORCE_STAGED", "QCX_SHARD_RELAYS", "QCX_SHARDS", "QCX_SHARD_SELFCHECK")
FLUSHES_NOTHING = ("reset", "fill") + rm.QUIET_SH + rm.QUEUED           # these leave a queued circuit queued, or drop it


def snapshot(qc, reg):
    """everything a refused call, a stats call or a self-check must leave as it is (the self-check: but for its own count)"""
    return dict(sharded=reg.sharded_stats(), fusion=reg.fusion_stats(), relays=reg.relay_stats(), layout=reg.sharded_layout(),
                overlap=reg.overlap_stats(), compact=(compact_chains(qc, reg), compact_measures(qc, reg)), selfchecks=reg.selfchecks)


def refused_call(qc, reg, inner):
    """a call the register must refuse, made; its status.  The rng forms: no draw may have been made"""
    j, n = inner[0], reg.num_qubits
    if j == "h": return status_of(qc, lambda: qc.hadamard_gate(inner[1], reg))
    if j == "cphase": return status_of(qc, lambda: qc.c_phase_shift_gate(inner[1], inner[2], inner[3], reg))
    if j in ("sample_rng", "measure_qubits_rng"):
        rng, twin = qc.Rng(inner[-2] if j == "sample_rng" else inner[-1]), qc.Rng(inner[-2] if j == "sample_rng" else inner[-1])
        if j == "sample_rng":
            st = status_of(qc, lambda: qc.sample_states(reg, rng, inner[2]))
        else:
            st = reg.measure_qubits(inner[1], inner[2], rng, strict=False)[2]
        assert rng.get() == twin.get(), f"{j}: the refused call drew from the generator"
        return st
    if j == "marginal": return status_of(qc, lambda: reg.marginal(inner[1], inner[2]))
    if j == "postselect": return reg.postselect(inner[1], inner[2], inner[3], strict=False)[1]
    if j == "expect": return status_of(qc, lambda: reg.expectation((inner[1], inner[2])))
    if j in ("expect_sum", "expect_batch"):
        terms = [(c, (x, z)) for c, x, z in rm.sum_terms(n, inner[1], inner[2])]
        return status_of(qc, lambda: (reg.expectation_sum if j == "expect_sum" else reg.expectation_batch)(terms))
    if j == "u1": return status_of(qc, lambda: qc.one_qubit_gate(inner[1], rm.matrix_data(2, inner[2]), reg))
    if j == "cu1": return status_of(qc, lambda: qc.c_one_qubit_gate(inner[1], inner[2], rm.matrix_data(2, inner[3]), reg))
    if j == "u2": return status_of(qc, lambda: qc.two_qubit_gate(inner[1], inner[2], rm.matrix_data(4, inner[3]), reg))
    if j == "cu2": return status_of(qc, lambda: qc.c_two_qubit_gate(inner[1], inner[2], inner[3], rm.matrix_data(4, inner[4]), reg))
    if j == "prot": return status_of(qc, lambda: qc.pauli_rotation((inner[1], inner[2]), inner[3], reg))
    if j == "set_stream": return status_of(qc, lambda: reg.set_stream(0))
    if j == "events_create": return status_of(qc, lambda: reg.events_create(inner[1]))
    if j == "devptr": return rm.UNSUPPORTED if reg.device_pointer() == 0 else rm.NO_ERROR      # (NULL stands for the refusal)
    raise ValueError(f"unknown refused op {inner!r}")


def apply_to_register(qc, reg, op, path_of, devs):
    """one op on the sharded register; returns what the call returns, in the form register_model.apply_to_model gives"""
    k = op[0]
    if k == "reset": qc.reset_register(reg)
    elif k == "fill": reg.fill_random(op[1])
    elif k == "write": reg.write(rm.window_data(reg.num_states, op[2], op[3], op[4]), op[1])
    elif k == "read": return reg.read(op[1], op[2])
    elif k == "h": qc.hadamard_gate(op[1], reg)
    elif k == "cphase": qc.c_phase_shift_gate(op[1], op[2], op[3], reg)
    elif k == "camodc": qc.c_amodc_gate(op[1], op[2], op[3], reg)
    elif k == "iqft": qc.inverse_QFT(reg)
    elif k == "qcomp": qc.quantum_computation(op[1], op[2], reg)
    elif k == "measure": return qc.measure_state(reg, float(op[1]))
    elif k == "total": return reg.total_probability()
    elif k == "norm2": return reg.norm2()
    elif k == "save": reg.save(path_of(op[1]))
    elif k == "load": reg.load(path_of(op[1]))
    elif k == "flush": reg.flush()
    elif k == "sync": reg.synchronize()
    elif k == "fusion": reg.set_fusion(op[1])
    elif k == "relays": reg.set_relays(qc.idle_devices(devs, 1) if op[1] else [])
    elif k in ("selfcheck", "stats", "refused"):
        before = snapshot(qc, reg)
        got = None
        if k == "selfcheck":
            reg.selfcheck()
            before["selfchecks"] += 1
        elif k == "refused":
            got = refused_call(qc, reg, op[1])
        after = snapshot(qc, reg)
        assert after == before, f"{k} changed the register's bookkeeping: {before} -> {after}"
        return got
    else:
        raise ValueError(f"unknown op {op!r}")
    return None


class Sharded:
    """one sharded register and its model, op by op; do() compares what the call returns and hands it back"""

    def __init__(self, qc, ob, shards, L, M, mode, tmp_path, relays=0, tag="s"):
        self.qc, self.ob, self.tmp, self.tag = qc, ob, tmp_path, tag
        self.devs = qc.spread_devices(shards)
        self.reg = qc.Register(L, M, shards=shards, devices=self.devs)
        try:
            self.reg.set_fusion(mode)
            if relays:
                self.reg.set_relays(qc.idle_devices(self.devs, relays))
        except Exception:
            self.reg.close()
            raise
        self.m = rm.RegisterModel(ob, L, M)
        self.shards, self.k = shards, shards.bit_length() - 1
        self.n, self.dim = L + M, 1 << (L + M)
        self.per = self.dim // shards                                      # amplitudes of one shard
        self.identity = list(range(self.n))
        self.done = []

    def do(self, *op):
        self.done.append(op)
        try:
            got = apply_to_register(self.qc, self.reg, op, lambda slot: str(self.tmp / f"{self.tag}_slot{slot}.qcx"), self.devs)
            compare(op, got, rm.apply_to_model(self.m, op))
        except Exception as e:
            raise AssertionError(f"op {len(self.done) - 1}: {op!r}\n{type(e).__name__}: {e}\nops = {self.done!r}") from e
        return got

    def state(self):
        return self.do("read", 0, self.dim)

    def swapped(self):
        return self.reg.sharded_layout() != self.identity

    def chains(self):
        return compact_chains(self.qc, self.reg)

    def measures(self):
        return compact_measures(self.qc, self.reg)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.reg.close()


def run_ops(qc, ob, cfg, ops, tmp_path, monkeypatch):
    """the ops on a fresh sharded register and a fresh model, everything returned compared; ends with a full read.  A compact seed:
    reset + quantum_computation must run as a compact circuit (qcx_compact_stats moves at the first call that flushes the queue --
    a sharded register queues in modes 0 and 1 alike), and a measure_state directly behind it scans the companion"""
    for key in ENV_KEYS:
        monkeypatch.delenv(key, raising=False)
    for key, value in cfg.env.items():
        monkeypatch.setenv(key, value)
    L, M, Cn, a = cfg.shape
    header = f"{cfg!r} ({len(ops)} ops)"
    mode, owed = cfg.mode, None
    with Sharded(qc, ob, cfg.shards, L, M, cfg.mode, tmp_path, relays=cfg.relays, tag=f"seed{cfg.seed}") as c:
        for i, (_, op) in enumerate(ops):
            try:
                chains, measures = c.chains(), c.measures()
                c.do(*op)
                k = op[0]
                if k == "fusion":
                    mode = op[1]
                if cfg.compact:
                    if owed is not None and k not in FLUSHES_NOTHING:
                        assert c.chains() == owed, f"the queued circuit did not run as a compact circuit ({chains} before, {c.chains()} now)"
                        if k == "measure":
                            assert c.measures() == measures + 1, "measure_state right behind a compact circuit scans the companion"
                    if owed is not None and k not in rm.QUIET_SH:
                        owed = None
                    if k == "qcomp" and i and ops[i - 1][1] == ("reset",) and mode >= 0:
                        assert c.chains() == chains, "a sharded register queues the circuit in modes 0 and 1"
                        owed = chains + 1
            except Exception as e:
                raise AssertionError(f"{header}\nop {i}: {op!r}\n{type(e).__name__}: {e}\nops = {[o for _, o in ops[:i + 1]]!r}") from e
        same(c.reg.read(), c.m.a, f"{header}: the final state")
        if not os.environ.get("QCX_SHSEQ_OPS"):
            assert c.reg.sharded_stats()[0] >= 1, f"{header}: no trade in the whole list (every list ends with an H that needs one)"


# ---- random sequences ----------------------------------------------------------------------------------------------------------

ONLY = os.environ.get("QCX_SHSEQ_CASE")


def seeds_of(tiny):
    seeds = [int(ONLY)] if ONLY else range(rm.NSEEDS_SH)
    return [s for s in seeds if (rm.ShardedConfig(s).kind == "tiny") == tiny]


def one_seed(qc, ob, seed, tmp_path, monkeypatch):
    cfg, ops = rm.generate_sharded(ob, seed)
    limit = os.environ.get("QCX_SHSEQ_OPS")
    if limit:
        ops = ops[:int(limit)]
    run_ops(qc, ob, cfg, ops, tmp_path, monkeypatch)


@pytest.mark.parametrize("seed", seeds_of(False))
def test_random_sequences_against_the_model(qc, ob, tmp_path, monkeypatch, seed):
    """the seeds with an ordinary or a compact shape"""
    one_seed(qc, ob, seed, tmp_path, monkeypatch)


@pytest.mark.parametrize("seed", seeds_of(True))
def test_tiny_registers(qc, ob, tmp_path, monkeypatch, seed):
    """the seeds whose registers have n_local < 2 k + 6: trades of runs shorter than 1 KiB (k_pack_push's small form, k_swap_bits),
    the per-shard gate kernels at n_local = 2 .. 10"""
    one_seed(qc, ob, seed, tmp_path, monkeypatch)


# ---- named chains ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(autouse=True)
def default_geometry(monkeypatch):
    for key in ENV_KEYS:
        monkeypatch.delenv(key, raising=False)


def test_chain_swapped_layout_partial_write_global_h_window_read(qc, ob, tmp_path):
    with Sharded(qc, ob, 2, 9, 0, 1, tmp_path) as c:
        c.do("fill", 3)
        c.do("h", c.n - 1)
        c.do("flush")
        assert c.swapped(), "an H on the shard-id qubit leaves the layout swapped"
        c.do("write", c.per - 100, 200, 5, "negzero")                     # by index: across the shard boundary
        assert not c.swapped()
        c.do("h", c.n - 1)
        c.do("norm2")
        assert c.swapped()
        c.do("read", c.per - 150, 300)
        c.state()


def test_chain_pending_reset_partial_write_measure(qc, ob, tmp_path):
    for r in (0.4, 0.97):
        with Sharded(qc, ob, 2, 5, 4, 1, tmp_path) as c:
            c.do("reset")                                                 # pending: nothing is written yet
            c.do("write", c.per - 3, 10, 7, "plain")                      # the basis state first, then the window over it
            c.do("measure", r)
            c.state()


def test_chain_front_queued_then_per_gate_mode(qc, ob, tmp_path):
    L, M = 5, 4
    with Sharded(qc, ob, 2, L, M, 1, tmp_path) as c:
        c.do("reset")
        for l in range(M, M + L):
            c.do("h", l)
        c.do("camodc", 15, 7, M); c.do("camodc", 15, 4, M + 1)
        fronts, ex = c.reg.fusion_stats()[0], c.reg.sharded_stats()[0]
        c.do("fusion", -1)                                                # flushes: the front goes out as one write per shard
        assert c.reg.fusion_stats()[0] == fronts + 1 and c.reg.sharded_stats()[0] == ex, "one front, no exchange"
        c.do("cphase", c.n - 1, 2, 0.6)
        c.do("total")
        c.state()


def test_chain_compact_measure_then_global_h(qc, ob, tmp_path):
    with Sharded(qc, ob, 2, 7, 4, 1, tmp_path) as c:
        k0, m0 = c.chains(), c.measures()
        c.do("reset"); c.do("qcomp", 15, 7)
        assert c.chains() == k0
        c.do("measure", 0.61)
        assert (c.chains(), c.measures()) == (k0 + 1, m0 + 1), "the measurement scans the companion's compact form"
        c.do("h", c.n - 1)
        c.do("read", c.per - 40, 80)
        c.state()


@pytest.mark.parametrize("second", ["reset", "fill"])
def test_chain_compact_circuit_dropped_before_any_observer(qc, ob, tmp_path, second):
    with Sharded(qc, ob, 2, 7, 4, 1, tmp_path) as c:
        k0 = c.chains()
        c.do("reset"); c.do("qcomp", 15, 7)
        c.do(*((second,) if second == "reset" else (second, 9)))          # the queued circuit acts on a state that is overwritten
        c.do("read", c.per - 5, 10)
        assert c.chains() == k0, "the circuit never ran"
        c.state()
        c.do("reset"); c.do("qcomp", 15, 7)                               # ... and the next one runs compact all the same
        c.do("flush")
        assert c.chains() == k0 + 1
        c.do(*((second,) if second == "reset" else (second, 10)))         # over a compact result that was expanded
        c.state()


def test_chain_compact_with_relays_then_without(qc, ob, tmp_path):
    with Sharded(qc, ob, 8, 12, 4, 1, tmp_path, relays=1) as c:
        assert c.reg.relay_stats()[0] == 1, "a trade zone of 2^10 amplitudes is striped over one relay"
        k0, m0 = c.chains(), c.measures()
        c.do("reset"); c.do("qcomp", 15, 7)
        c.do("read", c.per - 100, 200)
        assert c.chains() == k0 + 1
        c.do("relays", 0)                                                 # the companion is dropped with the relays
        assert c.reg.relay_stats()[0] == 0
        c.do("reset"); c.do("qcomp", 15, 7)
        c.do("measure", 0.37)
        assert (c.chains(), c.measures()) == (k0 + 2, m0 + 1)
        c.state()


def negative_zeros(a):
    return int(np.count_nonzero((a == 0) & np.signbit(a)))


def test_chain_zero_pass_before_a_local_phase(qc, ob, tmp_path):
    with Sharded(qc, ob, 2, 9, 0, 1, tmp_path) as c:
        c.do("write", 0, c.dim, 31, "negzero")
        assert negative_zeros(c.do("read", 0, c.dim)) > 100                # the -0 are the state until a gate runs
        c.do("cphase", 1, 4, 0.4)                                         # touches a quarter of the amplitudes, canonicalises all
        c.do("flush")
        assert negative_zeros(c.state()) == 0


def test_chain_zero_pass_before_a_trade(qc, ob, tmp_path):
    with Sharded(qc, ob, 2, 9, 0, 1, tmp_path) as c:
        c.do("write", 0, c.dim, 32, "negzero")
        c.do("h", c.n - 1)
        assert negative_zeros(c.state()) == 0


def test_chain_every_refused_call_between_queued_gates_under_a_swapped_layout(qc, ob, tmp_path):
    with Sharded(qc, ob, 4, 9, 4, 1, tmp_path) as c:
        n = c.n
        c.do("fill", 6)
        c.do("h", n - 1); c.do("flush")
        assert c.swapped()
        lay = c.reg.sharded_layout()
        refused = [("sample_rng", 5, 8), ("marginal", 2, 3), ("measure_qubits_rng", 4, 3, 11), ("postselect", 0, 2, 1), ("expect", 0x21, 0x1001),
                   ("expect_sum", 17, 3), ("expect_batch", 18, 6), ("u1", n - 1, 3), ("cu1", 0, n - 2, 4), ("u2", 1, n - 1, 5), ("cu2", 2, 3, n - 1, 6),
                   ("prot", 0x1003, 0x0801, 0.7), ("set_stream",), ("events_create", 4), ("devptr",)]
        assert [j[0] for j in refused] == list(rm.REFUSED_SH)
        far = next(q for q in range(n) if lay[q] >= n - c.k)               # a qubit that sits in the shard id now: its H needs a trade,
        for i, inner in enumerate(refused):                               # so a refused call that flushed first would show in the counts
            c.do(*[("h", i % n), ("cphase", (i + 3) % n, i % n, 0.3 + i), ("camodc", 15, 2 + i, 4 + i % 9)][i % 3])     # queued
            c.do("h", far)
            c.do("refused", inner, rm.UNSUPPORTED)
            assert c.reg.sharded_layout() == lay, "nothing ran"
        c.do("refused", ("h", n), rm.BAD_QUBIT)
        c.do("refused", ("cphase", 3, 3, 0.5), rm.BAD_QUBIT)
        c.do("read", c.per - 64, 128)
        c.state()


def test_chain_save_under_a_swapped_layout_load_with_gates_queued(qc, ob, tmp_path):
    L, M = 9, 4
    with Sharded(qc, ob, 4, L, M, 1, tmp_path) as c, qc.Register(L, M) as plain:
        c.do("fill", 2)
        c.do("h", c.n - 1); c.do("camodc", 15, 7, c.n - 2); c.do("norm2")
        assert c.swapped()
        c.do("save", 0)
        plain.load(str(tmp_path / "s_slot0.qcx"))
        same(plain.read(), c.m.a, "the unsharded register's copy of the saved state")
        qc.hadamard_gate(3, plain); qc.c_phase_shift_gate(c.n - 1, 0, 1.1, plain)
        plain.save(str(tmp_path / "s_slot1.qcx"))
        other = c.m.a.copy()
        ob.hadamard(other, c.n, 3); ob.cphase(other, c.n, c.n - 1, 0, 1.1)
        same(plain.read(), other, "the state the unsharded register saved")
        c.m.saved[1] = other
        c.do("h", c.n - 2); c.do("cphase", 1, c.n - 1, 0.2)
        c.do("load", 1)                                                   # the queued gates run first, then the file replaces it all
        c.do("h", c.n - 1)
        c.do("read", c.per - 10, 20)
        c.state()


@pytest.mark.parametrize("r", ["0.0", "nan", "1.5", "-0.25"])
def test_chain_measure_edge_draws_on_a_compact_result_and_under_a_swapped_layout(qc, ob, tmp_path, r):
    with Sharded(qc, ob, 2, 7, 4, 1, tmp_path) as c:
        k0, m0 = c.chains(), c.measures()
        c.do("reset"); c.do("qcomp", 15, 7)
        c.do("measure", r)
        assert (c.chains(), c.measures()) == (k0 + 1, m0 + 1)
        c.state()
        c.do("fill", 12)
        c.do("h", c.n - 1); c.do("flush")
        assert c.swapped()
        c.do("measure", r)
        c.state()


def test_chain_automatic_flush_behind_a_pending_basis_state(qc, ob, tmp_path):
    """more gates than the queue holds (max_queue = 8192) behind a lazily pending reset: the automatic flush writes the basis
    state, runs the 8191 phases and the first H, and the rest of the layer and the global H follow"""
    n = 9
    with Sharded(qc, ob, 2, n, 0, 1, tmp_path) as c:
        c.do("reset")
        for i in range(8191):
            c.do("cphase", i % n, (i + 1 + i // n % (n - 1)) % n, 0.001 * (i + 1))
        for q in range(n - 1):
            c.do("h", q)
        c.do("h", n - 1)
        c.state()
