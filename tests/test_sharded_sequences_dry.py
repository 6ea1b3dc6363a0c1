"""CPU: the op lists of the sharded family (register_model.generate_sharded) on a DRY-RUN sharded register (devices = [-1]) of the
same shape, shard count and environment, with the schedule it hands back replayed by tests/sharded_replay.py.

A dry-run register runs the whole host half of qcx_sharded.inc.h -- the queue, the layout, the choice of qubits to give up, the
windows, the restoration of the identity layout -- and records the steps as text instead of launching them.  Per op:

  * gate calls, reset, flush, set_fusion and synchronize go to the register;
  * calls that need amplitudes (read, write, measure_state, total_probability, norm2, fill_random, the self-check) are made and
    must return QCX_UNSUPPORTED -- the library has done its host-side settling by then -- and the test does by hand what the call
    would have done to the data: it takes the model's state (write, load, fill, the collapse of a measurement).  save and load
    would go to the file system between the settling and the refusal, so qcx_sharded_restore_identity stands in for them: it is
    the settling both of them do;
  * the calls a sharded register refuses must return QCX_UNSUPPORTED and leave no step in the trace;
  * the observing calls are made with whatever is queued: they must flush, and restore the identity layout, on their own; whether
    one met a swapped layout is read off the schedule it left (it ends with the layout steps of the restoration);
  * after every call the trace is fetched and replayed on ONE array in physical index order, and whenever nothing is queued
    the array is compared with the model bit for bit: directly when qcx_sharded_layout is the identity, through it otherwise.

What a dry run does not trace is the zero pass (k_canon_zeros before the first gate behind a write or a load): the test applies
x + 0.0 to its array where the library owes it, before the first gate step behind a write or load.  Neither does it cover
anything the kernels do: the pending basis state and the fronts, compact circuits, the copies of sh_copy, the measurement scan,
relays and the staged exchange -- tests/test_gpu_sharded_sequences.py runs the same lists on the GPU for those.

Over the 48 seeds (3274 ops): 865 observing calls, 208 of them (24 %) on a layout other than the identity; 470 trades, at
least one in every seed (test_dry_replay_of_every_seed prints these figures)."""
import numpy as np

import register_model as rm
from sharded_replay import replay

OBSERVERS = ("read", "write", "measure", "total", "save", "load")        # calls that restore the identity layout first


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def logical_view(phys, n, layout):
    """the amplitudes of `phys` (physical index order) in logical order: logical index i sits where bit layout[q] = bit q of i"""
    idx = np.arange(1 << n, dtype=np.int64)
    at = np.zeros_like(idx)
    for q in range(n):
        at |= ((idx >> q) & 1) << layout[q]
    return phys.reshape(-1, 2)[at].reshape(-1)


def status_of(qc, call):
    try:
        call()
    except qc.QcxError as e:
        return e.status
    return rm.NO_ERROR


def refused_on_dry(qc, reg, inner):
    """the refused call, made; its status"""
    j = inner[0]
    n = reg.num_qubits
    if j == "h": return status_of(qc, lambda: qc.hadamard_gate(inner[1], reg))
    if j == "cphase": return status_of(qc, lambda: qc.c_phase_shift_gate(inner[1], inner[2], inner[3], reg))
    if j == "sample_rng": return status_of(qc, lambda: qc.sample_states(reg, qc.Rng(inner[1]), inner[2]))
    if j == "marginal": return status_of(qc, lambda: reg.marginal(inner[1], inner[2]))
    if j == "measure_qubits_rng": return reg.measure_qubits(inner[1], inner[2], qc.Rng(inner[3]), strict=False)[2]
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
    if j == "devptr": return rm.UNSUPPORTED if reg.device_pointer() == 0 else rm.NO_ERROR
    raise ValueError(inner)


def run_dry(qc, ob, cfg, ops):
    """one op list on a dry-run register; returns (observing calls, of them on a swapped layout, trades)"""
    L, M, Cn, a = cfg.shape
    n, k = cfg.n, cfg.k
    ident = list(range(n))
    m = rm.RegisterModel(ob, L, M)
    phys = np.zeros(2 << n)                     # what the shards would hold, physical order
    seen = dict(observers=0, swapped=0, trades=0)
    with qc.Register(L, M, shards=cfg.shards, devices=[-1]) as reg:
        reg.set_fusion(cfg.mode)
        reg.sharded_trace()
        queued, dirty = 0, False

        def settle(what):
            """replay what the library has scheduled since the last look; with nothing queued the array must be the model's state"""
            nonlocal phys, dirty
            tr = reg.sharded_trace()
            if dirty and any(line[:2] in ("h ", "p ", "c ") for line in tr.splitlines()):
                phys = phys + 0.0               # the zero pass the library owes before the first gate behind a write / load
                dirty = False
            if "reset" in tr.split():
                dirty = False
            phys, c = replay(tr, n, k, M, phys, ob)
            seen["trades"] += c["trade"]
            if queued == 0:
                lay = reg.sharded_layout()
                got = phys if lay == ident else logical_view(phys, n, lay)
                assert np.array_equal(bits(got), bits(m.a)), f"{what}: the replayed state differs from the model under layout {lay}"
            return tr

        for i, (_, op) in enumerate(ops):
            kind = op[0]
            what = f"{cfg!r}\nop {i}: {op!r}\nops = {[o for _, o in ops[:i + 1]]!r}"
            if kind == "reset": qc.reset_register(reg); queued = 0
            elif kind == "h": qc.hadamard_gate(op[1], reg)
            elif kind == "cphase": qc.c_phase_shift_gate(op[1], op[2], op[3], reg)
            elif kind == "camodc": qc.c_amodc_gate(op[1], op[2], op[3], reg)
            elif kind == "iqft": qc.inverse_QFT(reg)
            elif kind == "qcomp": qc.quantum_computation(op[1], op[2], reg)
            elif kind == "flush": reg.flush(); queued = 0
            elif kind == "sync": reg.synchronize(); queued = 0
            elif kind == "fusion": reg.set_fusion(op[1]); queued = 0
            elif kind == "fill":
                assert status_of(qc, lambda: reg.fill_random(op[1])) == rm.UNSUPPORTED, what
                queued = 0
            elif kind == "read": assert status_of(qc, lambda: reg.read(op[1], op[2])) == rm.UNSUPPORTED, what
            elif kind == "write":
                assert status_of(qc, lambda: reg.write(rm.window_data(1 << n, op[2], op[3], op[4]), op[1])) == rm.UNSUPPORTED, what
            elif kind == "measure": assert status_of(qc, lambda: qc.measure_state(reg, float(op[1]))) == rm.UNSUPPORTED, what
            elif kind == "total": assert status_of(qc, lambda: reg.total_probability()) == rm.UNSUPPORTED, what
            elif kind == "norm2": assert status_of(qc, lambda: reg.norm2()) == rm.UNSUPPORTED, what
            elif kind in ("save", "load"): reg.sharded_restore_identity()
            elif kind == "relays": reg.set_relays([])                          # (nothing happens on a dry run)
            elif kind == "selfcheck": assert status_of(qc, reg.selfcheck) == rm.UNSUPPORTED, what
            elif kind == "stats": reg.sharded_stats(); reg.fusion_stats(); reg.overlap_stats(); reg.sharded_layout()
            elif kind == "refused":
                lay, st = reg.sharded_layout(), reg.sharded_stats()
                assert refused_on_dry(qc, reg, op[1]) == op[2], what
                assert (reg.sharded_layout(), reg.sharded_stats()) == (lay, st), what
                assert reg.sharded_trace() == "", f"{what}: a refused call scheduled something"
            else:
                raise ValueError(op)
            if kind in rm.QUEUED:
                queued += 1
            elif kind in OBSERVERS or kind == "norm2":                         # the call itself has run what was queued
                queued = 0
            if kind == "fill":                                                 # (what was queued is dropped, nothing is scheduled)
                assert reg.sharded_trace() == "" and reg.sharded_layout() == ident, what
                rm.apply_to_model(m, op)
                phys, dirty = m.a.copy(), False
                continue
            if kind in ("write", "load", "measure"):                           # by hand: what the call would have done to the data
                tr = settle(what)
                rm.apply_to_model(m, op)
                phys = m.a.copy()
                dirty = dirty or kind != "measure"
            else:
                rm.apply_to_model(m, op)
                tr = settle(what)
            if kind in OBSERVERS:
                assert reg.sharded_layout() == ident, f"{what}: the call works by index, so on the identity layout"
                # a flush ends with the gate that needed its last trade, so a schedule that ends with a layout step restored the identity
                seen["observers"] += 1
                seen["swapped"] += tr.splitlines()[-1:] != [] and tr.splitlines()[-1].split()[0] in ("trade", "permute", "pack")
            elif kind == "norm2":                                              # (observes in whatever layout the flush leaves)
                seen["observers"] += 1
                seen["swapped"] += reg.sharded_layout() != ident
        assert queued == 0 and reg.sharded_layout() == ident                   # (every list ends with a full read)
        assert reg.sharded_stats()[0] == seen["trades"], "qcx_sharded_stats counts the trades of the trace"
    return seen


def test_dry_replay_of_every_seed(qc, ob, monkeypatch):
    """every seed of the sharded family; the scheduler's bookkeeping holds under the interleaving, and the lists really meet
    swapped layouts: at least a fifth of the observing calls do, every seed trades at least once"""
    total = dict(observers=0, swapped=0, trades=0, ops=0)
    for seed in range(rm.NSEEDS_SH):
        cfg, ops = rm.generate_sharded(ob, seed)
        for key in ("QCX_SHARD_SLICES_LOG2", "QCX_SHARD_OVERLAP", "QCX_SHARD_FORCE_STAGED", "QCX_SHARD_RELAYS", "QCX_SHARDS"):
            monkeypatch.delenv(key, raising=False)
        for key, value in cfg.env.items():
            monkeypatch.setenv(key, value)
        seen = run_dry(qc, ob, cfg, ops)
        assert seen["trades"] >= 1, f"{cfg!r}: no trade in the whole list"
        for key in seen:
            total[key] += seen[key]
        total["ops"] += len(ops)
    print(f"sharded family, dry: {total['ops']} ops, {total['observers']} observing calls, {total['swapped']} of them on a layout other "
          f"than the identity ({100.0 * total['swapped'] / total['observers']:.0f} %), {total['trades']} trades")
    assert 5 * total["swapped"] >= total["observers"]


def test_dry_replay_notices_a_write_that_skips_the_identity_layout(qc, ob):
    """the check is not vacuous: data written by index into a register whose layout is swapped lands elsewhere"""
    cfg = rm.ShardedConfig(0)
    L, M, Cn, a = cfg.shape
    n = cfg.n
    with qc.Register(L, M, shards=cfg.shards, devices=[-1]) as reg:
        qc.hadamard_gate(n - 1, reg)
        reg.flush()
        lay = reg.sharded_layout()
        assert lay != list(range(n))
        want = ob.fill_random(n, 3)
        assert not np.array_equal(bits(logical_view(want, n, lay)), bits(want))
        assert status_of(qc, lambda: reg.write(want[:64], 0)) == rm.UNSUPPORTED
        assert reg.sharded_layout() == list(range(n)), "a write restores the identity layout first"
