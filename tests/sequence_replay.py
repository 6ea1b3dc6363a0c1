"""Replaying the op lists of tests/register_model.py on GPU registers: one op on a register (apply_to_register), what it returned
against what the model returned (compare), and a whole list on fresh registers (run_ops).  Shared by
tests/test_gpu_api_sequences.py, which replays one list at a time, and tests/test_gpu_concurrent_callers.py, which replays
several from threads against values the model gave beforehand (record_ops).  No test in here; imports no GPU code itself."""
import ctypes as C

import numpy as np

import register_model as rm


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(got, want, what):
    """bitwise, NaN matching NaN"""
    got, want = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(want, dtype=np.float64).reshape(-1)
    assert got.shape == want.shape, what
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f"{what}: NaN positions differ at {np.flatnonzero(gn != wn)[:6]}"
    bad = np.flatnonzero(bits(got[~gn]) != bits(want[~wn]))
    assert bad.size == 0, f"{what}: {bad.size} values differ, first at {bad[:4]}: {got[~gn][bad[:4]]} vs {want[~wn][bad[:4]]}"


def compact_measures(qc, reg):
    v = C.c_ulong(0)
    assert qc.lib().qcx_compact_measure_stats(reg._h, C.byref(v)) == 0
    return int(v.value)


def compact_chains(qc, reg):
    v = C.c_ulong(0)
    assert qc.lib().qcx_compact_stats(reg._h, C.byref(v)) == 0
    return int(v.value)


def diagonal_passes(qc, reg):
    """fused passes so far that carried merged diagonals (the tolerance mode's arithmetic; the others ran the exact interpreter)"""
    v = C.c_ulong(0)
    assert qc.lib().qcx_diag_stats(reg._h, C.byref(v)) == 0
    return int(v.value)


_hip_memcpy = None


def hip_memcpy():
    """hipMemcpy of the HIP runtime this process already holds (quantumcomputer_amd/_lib.py arranges that there is one): looked
    up in the process image, or, where the runtime was not loaded into the global scope, in the one copy that is mapped"""
    global _hip_memcpy
    if _hip_memcpy is None:
        try:
            fn = C.CDLL(None).hipMemcpy
        except AttributeError:
            with open("/proc/self/maps") as f:
                mapped = sorted({line.split()[-1] for line in f if "libamdhip64.so" in line})
            assert len(mapped) == 1, f"one HIP runtime per process, mapped are {mapped}"
            fn = C.CDLL(mapped[0]).hipMemcpy
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _hip_memcpy = fn
    return _hip_memcpy


def read_through_pointer(reg, first, count, ctx):
    """`count` amplitudes from qcx_device_pointer() + 16 * first, copied by the caller; the pointer never changes"""
    assert 0 <= first and 0 < count and first + count <= reg.num_states
    ptr = reg.device_pointer()
    assert ptr, "qcx_device_pointer returned null"
    assert ctx.setdefault("pointer", ptr) == ptr, f"the buffer that was handed out as {ctx['pointer']:#x} is now {ptr:#x}"
    reg.synchronize()
    out = np.empty(2 * count, dtype=np.float64)
    st = hip_memcpy()(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr + 16 * first), 16 * count, 2)      # hipMemcpyDeviceToHost
    assert st == 0, f"hipMemcpy: error {st}"
    return out


def set_stream(reg, on, ctx):
    """on: the register works on ONE non-blocking stream of PyTorch's, alive until the register is closed; off: on its own"""
    if on:
        if "stream" not in ctx:
            import torch
            ctx["stream"] = torch.cuda.Stream()
        reg.set_stream(ctx["stream"].cuda_stream)
    else:
        reg.set_stream(0)


def status_of(qc, call):
    try:
        call()
    except qc.QcxError as e:
        return e.status
    return rm.NO_ERROR


def batch_arrays(terms):
    """(k, x_masks, z_masks, coeffs, values) of a term list as the C ABI takes them"""
    xs = np.array([x for _, x, _ in terms], dtype=np.uint64)
    zs = np.array([z for _, _, z in terms], dtype=np.uint64)
    cs = np.array([c for c, _, _ in terms], dtype=np.float64)
    return len(terms), xs, zs, cs, np.zeros(len(terms), dtype=np.float64)


def apply_to_register(qc, reg, op, path_of, ctx):
    """one op on the GPU register; returns what the call returns, in the form register_model.apply_to_model gives.  ctx: a dict
    per register that lives until the register is closed (the handed-out pointer, the caller's stream)"""
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
    elif k == "u1": qc.one_qubit_gate(op[1], rm.matrix_data(2, op[2]), reg)
    elif k == "cu1": qc.c_one_qubit_gate(op[1], op[2], rm.matrix_data(2, op[3]), reg)
    elif k == "u2": qc.two_qubit_gate(op[1], op[2], rm.matrix_data(4, op[3]), reg)
    elif k == "cu2": qc.c_two_qubit_gate(op[1], op[2], op[3], rm.matrix_data(4, op[4]), reg)
    elif k == "measure": return qc.measure_state(reg, op[1])
    elif k == "sample": return qc.sample_states(reg, rm.sample_draws(op[1], op[2]))
    elif k == "marginal": return reg.marginal(op[1], op[2])
    elif k == "measure_qubits": return reg.measure_qubits(op[1], op[2], op[3], strict=False)
    elif k == "postselect": return reg.postselect(op[1], op[2], op[3], strict=False)
    elif k == "total": return reg.total_probability()
    elif k == "norm2": return reg.norm2()
    elif k == "save": reg.save(path_of(op[1]))
    elif k == "load": reg.load(path_of(op[1]))
    elif k == "flush": reg.flush()
    elif k == "sync": reg.synchronize()
    elif k == "fusion": reg.set_fusion(op[1])
    elif k == "stats":
        reg.fusion_stats(); reg.marginal_stats(); reg.sample_stats(); reg.collapse_stats(); compact_measures(qc, reg)
        reg.expectation_stats(); reg.rdm_stats()
    elif k == "expect": return reg.expectation((op[1], op[2]))
    elif k == "expect_sum": return reg.expectation_sum([(c, (x, z)) for c, x, z in rm.sum_terms(reg.num_qubits, op[1], op[2])])
    elif k == "expect_batch":
        terms = [(c, (x, z)) for c, x, z in rm.batch_terms(reg.num_qubits, op[1], op[2])]
        got = reg.expectation_batch(terms)
        stats = reg.expectation_stats()
        return got + (reg.expectation_sum(terms), stats)               # (the same terms one by one: the call promises its bits)
    elif k == "rdm":
        rho = reg.reduced_density_matrix(op[1], op[2])
        return np.ascontiguousarray(rho).view(np.float64).reshape(rho.shape + (2,))       # (re, im) pairs, as rdm_ref gives them
    elif k == "prot": qc.pauli_rotation((op[1], op[2]), op[3], reg)
    elif k == "prot_batch":
        terms = rm.rotation_terms(reg.num_qubits, op[1], op[2])
        qc.pauli_rotation_batch(terms, reg)
        passes = qc.pauli_rotation_batch_plan(terms, reg.num_qubits)[1]
        return reg.rotation_batch_stats(), (len(passes), sum(kind for kind, _ in passes))       # (what ran, what the plan says)
    elif k == "devptr": return read_through_pointer(reg, op[1], op[2], ctx)
    elif k == "stream": set_stream(reg, op[1], ctx)
    elif k == "refused":
        inner = op[1]
        j = inner[0]
        if j == "postselect":
            p, st = reg.postselect(inner[1], inner[2], inner[3], strict=False)
            return (p, st) if inner[3] < (1 << inner[2]) and inner[1] + inner[2] <= reg.num_qubits else st
        if j == "h": return status_of(qc, lambda: qc.hadamard_gate(inner[1], reg))
        if j == "marginal": return status_of(qc, lambda: reg.marginal(inner[1], inner[2]))
        if j == "cphase": return status_of(qc, lambda: qc.c_phase_shift_gate(inner[1], inner[2], inner[3], reg))
        if j == "u1": return status_of(qc, lambda: qc.one_qubit_gate(inner[1], rm.matrix_data(2, inner[2]), reg))
        if j == "u1x": return status_of(qc, lambda: qc.one_qubit_gate(inner[1], rm.matrix_data(2, inner[2], ulp=True), reg))
        if j == "expect":                                                  # (through the library: pauli_masks would raise first)
            v = C.c_double(0.0)
            return qc.lib().qcx_pauli_expectation(reg._h, inner[1], inner[2], C.byref(v))
        if j == "prot": return qc.lib().qcx_pauli_rotation(inner[1], inner[2], float(inner[3]), reg._h)
        if j == "u2x": return status_of(qc, lambda: qc.two_qubit_gate(inner[1], inner[2], rm.matrix_data(4, inner[3], ulp=True), reg))
        if j == "rdm":                                                     # (a buffer of the widest matrix the call serves)
            out = np.zeros(2 << (2 * rm.RDM_MAX), dtype=np.float64)
            return qc.lib().qcx_reduced_density_matrix(reg._h, inner[1], inner[2], out.ctypes.data_as(C.c_void_p))
        if j == "expect_batch":                                            # term inner[3] reaches bit n in its x or its z mask
            kk, xs, zs, cs, values = batch_arrays(rm.batch_terms(reg.num_qubits, inner[1], inner[2]))
            (xs if inner[4] == "x" else zs)[inner[3]] |= np.uint64(1 << reg.num_qubits)
            total = C.c_double(0.0)
            ptr = lambda a: a.ctypes.data_as(C.c_void_p)
            return qc.lib().qcx_pauli_expectation_batch(reg._h, kk, ptr(xs), ptr(zs), ptr(cs), ptr(values), C.byref(total))
        raise ValueError(f"unknown refused op {op!r}")
    else:
        raise ValueError(f"unknown op {op!r}")
    return None


def compare(op, got, want):
    k = op[0]
    if k in ("read", "marginal", "devptr"):
        same(got, want, k)
    elif k == "expect":
        same([got], [want], "expectation")
    elif k == "expect_sum":
        same([got[0]], [want[0]], "the terms' sum")
        same(got[1], want[1], "the values of the terms")
    elif k == "expect_batch":
        same([got[0]], [want[0]], "the batch's sum")
        same(got[1], want[1], "the values of the batch's terms")
        same([got[2][0]], [got[0]], "the batch's sum against expectation_sum on the same terms")
        same(got[2][1], got[1], "the batch's values against expectation_sum on the same terms")
        if op[2] == 0:
            assert got[3] == (0, 0), f"a batch of no terms reports {got[3]}"
    elif k == "rdm":
        nv = 1 << op[2]
        assert got.shape == (nv, nv, 2), got.shape
        same(got, want[0], "reduced density matrix")
        diag = got[np.arange(nv), np.arange(nv)]
        same(diag[:, 0], want[1], "the density matrix's diagonal against the model's marginal")
        assert not bits(diag[:, 1]).any(), "a diagonal entry's imaginary part is +0"
    elif k in ("measure",):
        assert got == want, f"index {got} != {want}"
    elif k == "sample":
        assert np.array_equal(got, want), f"indices {got.tolist()} != {want.tolist()}"
    elif k == "measure_qubits":
        assert (got[0], got[2]) == (want[0], want[2]), f"(outcome, status) {(got[0], got[2])} != {(want[0], want[2])}"
        same([got[1]], [want[1]], "probability")
    elif k == "postselect":
        assert got[1] == want[1], f"status {got[1]} != {want[1]}"
        same([got[0]], [want[0]], "probability")
    elif k == "total":
        same([got], [want], "total_probability")
    elif k == "norm2":
        if want is not None:                                               # (a tree sum: not bit-defined; skipped on a non-finite state)
            assert abs(got - want) < 1e-9, f"norm2 {got!r} vs {want!r}"
    elif k == "prot_batch":
        assert want is None and got[0] == got[1], f"rotation_batch_stats() {got[0]}, the plan's (passes, wide terms) {got[1]}"
    elif k == "refused":
        if isinstance(want, tuple):
            assert got[1] == want[1], f"status {got[1]} != {want[1]}"
            same([got[0]], [want[0]], "probability")
        else:
            assert got == want, f"status {got} != {want}"
    else:
        assert got is None and want is None


FLUSHES_NOTHING = ("reset", "fill", "stats", "refused") + rm.QUEUED      # (in mode 1: these leave a queued circuit queued, or drop it)


def record_ops(ob, shapes, ops):
    """the ops on fresh models alone: (what every op returns, the final state of every register), for run_ops(.., recorded=)"""
    models = [rm.RegisterModel(ob, L, M) for L, M, _, _ in shapes]
    wants = [rm.apply_to_model(models[which], op) for which, op in ops]
    return wants, [m.a for m in models]


def run_ops(qc, ob, shapes, modes, ops, tmp_path, header, compact=False, recorded=None):
    """the ops on fresh registers and fresh models, everything returned compared; ends with a full read of every register.
    compact: register 0 has a shape at which reset + quantum_computation must run as a compact chain (qcx_compact_stats moves:
    with the call in mode 0, with the first call that flushes the queue in mode 1).  recorded: what record_ops gave for the
    same ops, in place of models that run along (several threads replay at once; the oracle is then not called from them)"""
    regs, models, ctxs = [], [], []
    done = []
    modes = list(modes)
    owed = None                                 # the compact-chain count register 0 must show after its next flushing call
    try:
        for (L, M, Cn, a), mode in zip(shapes, modes):
            reg = qc.Register(L, M)
            reg.set_fusion(mode)
            regs.append(reg)
            ctxs.append({})
            if recorded is None:
                models.append(rm.RegisterModel(ob, L, M))
        for i, (which, op) in enumerate(ops):
            done.append((which, op))
            try:
                chains = compact_chains(qc, regs[0]) if compact and which == 0 else 0
                got = apply_to_register(qc, regs[which], op, lambda slot: str(tmp_path / f"reg{which}_slot{slot}.qcx"), ctxs[which])
                want = rm.apply_to_model(models[which], op) if recorded is None else recorded[0][i]
                compare(op, got, want)
                if op[0] == "fusion":
                    modes[which] = op[1]
                if compact and which == 0:
                    if owed is not None and op[0] not in FLUSHES_NOTHING:
                        assert compact_chains(qc, regs[0]) == owed, f"the queued circuit did not run as a compact chain ({chains} chains before, {compact_chains(qc, regs[0])} now)"
                    if owed is not None and op[0] != "stats":
                        owed = None
                    if op[0] == "qcomp" and len(done) > 1 and [o for w, o in done[:-1] if w == 0][-1:] == [("reset",)]:
                        if modes[0] == 0:
                            assert compact_chains(qc, regs[0]) == chains + 1, "reset + quantum_computation did not run as a compact chain"
                        elif modes[0] == 1:
                            owed = chains + 1
                if i + 1 == len(ops):
                    for w in range(len(regs)):
                        same(regs[w].read(), models[w].a if recorded is None else recorded[1][w], f"the final state of register {w}")
            except Exception as e:
                raise AssertionError(f"{header}\nop {i} on register {which}: {op!r}\n{type(e).__name__}: {e}\nops = {done!r}") from e
    finally:
        for reg in regs:
            reg.close()
        ctxs.clear()                                # (the callers' streams go after the registers that worked on them)
