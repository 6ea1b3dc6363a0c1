"""Host-side mirror of the reference's gate/state interface over libqcx.so.

Function names, argument order and qubit numbering follow qc_shor.c so that code
(and tests) written against the reference read the same here:

    reference (qc_shor.c)                       here
    ------------------------------------------  -------------------------------------
    Register + alloc/free (194-203, 1316-1333)  Register(L_size, M_size) / .close()
    reset_register(reg)              318-324    reset_register(reg)
    hadamard_gate(q, &reg, matrix)   442-484    hadamard_gate(q, reg, matrix=None)
    c_phase_shift_gate(c, q, th, ..) 513-565    c_phase_shift_gate(c, q, theta, reg)
    c_amodc_gate(C, atox, c, ..)     595-660    c_amodc_gate(C, atox, c, reg)
    inverse_QFT(&reg, matrix)        678-690    inverse_QFT(reg)
    quantum_computation(C, a, ..)    712-737    quantum_computation(C, a, reg)
    measure_state(reg, rng)          272-306    measure_state(reg, rng)
    swap_states(&reg)                242-249    swap_states(reg)   (no-op: in place)
    gsl_rng mt19937                  1296-1299  Rng(seed)

The `matrix` scratch argument of the reference is accepted and ignored: no gate
matrix is ever built.  Everything executes in the HIP library; a missing library
or GPU raises (see _lib.py).
"""
import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import check, lib


class Rng:
    """gsl_rng_mt19937 equivalent (qc_shor.c:1296-1299)."""

    def __init__(self, seed=0):
        self._h = lib().qcx_rng_alloc()
        if not self._h:
            raise MemoryError("qcx_rng_alloc")
        lib().qcx_rng_set(self._h, seed & 0xFFFFFFFF)

    def set(self, seed):
        lib().qcx_rng_set(self._h, seed & 0xFFFFFFFF)

    def get(self):
        return int(lib().qcx_rng_get(self._h))

    def uniform(self):
        return float(lib().qcx_rng_uniform(self._h))

    def close(self):
        if self._h:
            lib().qcx_rng_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Register:
    """The qubit register (qc_shor.c:194-203): L_size, M_size, num_qubits, num_states and the
    state vector, which lives in HBM as 2^n interleaved (re, im) doubles, updated in place."""

    def __init__(self, L_size, M_size, shards=1, devices=None):
        """shards > 1: the register is sharded over that many GPUs by this process (qcx_register_create_sharded);
        devices = HIP device of each shard (default: spread over the visible GPUs, see spread_devices; entries may
        repeat; [-1] = dry run: the schedule only, see sharded_trace)"""
        h = C.c_void_p()
        if shards == 1 and devices is None:
            check(lib().qcx_register_create(int(L_size), int(M_size), C.byref(h)), "qcx_register_create")
        else:
            dv = None
            if devices is not None:
                devices = list(devices) + [devices[-1]] * max(0, int(shards) - len(devices))
                dv = (C.c_int * len(devices))(*devices)
            check(lib().qcx_register_create_sharded(int(L_size), int(M_size), int(shards), dv, C.byref(h)), "qcx_register_create_sharded")
        self._h = h
        self.L_size = int(L_size)
        self.M_size = int(M_size)
        self.num_qubits = int(lib().qcx_num_qubits(h))
        self.num_states = int(lib().qcx_num_states(h))

    # -- lifecycle -------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            lib().qcx_register_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- state access (gsl_vector_complex_get/set uses; testing_and_debug.c:7-37) ------------
    def read(self, first=0, count=None):
        """Amplitudes [first, first+count) as a float64 array of 2*count (re, im) values."""
        if count is None:
            count = self.num_states - first
        out = np.empty(2 * count, dtype=np.float64)
        check(lib().qcx_state_read(self._h, first, count, out.ctypes.data_as(C.c_void_p)), "qcx_state_read")
        return out

    def write(self, amps, first=0):
        a = np.ascontiguousarray(amps, dtype=np.float64)
        if a.size % 2:
            raise ValueError("amplitudes are (re, im) pairs")
        check(lib().qcx_state_write(self._h, first, a.size // 2, a.ctypes.data_as(C.c_void_p)), "qcx_state_write")

    def save(self, path):
        """state file: 64-byte header + interleaved binary64 amplitudes (qcx_state_save); see load_state_file()"""
        check(lib().qcx_state_save(self._h, str(path).encode()), "qcx_state_save")

    def load(self, path):
        check(lib().qcx_state_load(self._h, str(path).encode()), "qcx_state_load")

    def fill_random(self, seed):
        """synthetic dense state generated on the device (include/qcx.h: qcx_state_fill_random)"""
        check(lib().qcx_state_fill_random(self._h, int(seed)), "qcx_state_fill_random")

    def norm2(self):
        """Total probability (testing_and_debug.c:28-37), tree-summed on the GPU."""
        out = C.c_double(0.0)
        check(lib().qcx_norm2(self._h, C.byref(out)), "qcx_norm2")
        return out.value

    @property
    def shards(self):
        return int(lib().qcx_register_shards(self._h))

    def sharded_stats(self):
        """(exchanges, pack passes) a sharded register has performed"""
        e, p = C.c_ulong(0), C.c_ulong(0)
        check(lib().qcx_sharded_stats(self._h, C.byref(e), C.byref(p)), "qcx_sharded_stats")
        return e.value, p.value

    def selfcheck(self):
        """the pre-flight exchange check on demand (runs by itself at creation when the shards sit on several GPUs)"""
        check(lib().qcx_sharded_selfcheck(self._h), "qcx_sharded_selfcheck")

    @property
    def selfchecks(self):
        return int(lib().qcx_sharded_selfchecks(self._h))

    def set_relays(self, devices):
        """multi-path striping: GPUs without a shard relay a share of every trade ([] = off)"""
        dv = (C.c_int * max(len(devices), 1))(*devices)
        check(lib().qcx_sharded_set_relays(self._h, len(devices), dv), "qcx_sharded_set_relays")

    def relay_stats(self):
        n, b = C.c_uint(0), C.c_ulong(0)
        check(lib().qcx_sharded_relay_stats(self._h, C.byref(n), C.byref(b)), "qcx_sharded_relay_stats")
        return n.value, b.value

    def overlap_stats(self):
        """(log2 of the slices a trade is cut into, gates that ran inside exchange windows so far)"""
        sg, g = C.c_uint(0), C.c_ulong(0)
        check(lib().qcx_sharded_overlap_stats(self._h, C.byref(sg), C.byref(g)), "qcx_sharded_overlap_stats")
        return sg.value, g.value

    def sharded_trace(self):
        """diagnostics: the steps a dry-run sharded register has scheduled since the last call, as text"""
        need = C.c_size_t(0)
        lib().qcx_sharded_trace(self._h, None, 0, C.byref(need))
        buf = C.create_string_buffer(need.value)
        check(lib().qcx_sharded_trace(self._h, buf, need.value, C.byref(need)), "qcx_sharded_trace")
        return buf.value.decode()

    def sharded_restore_identity(self):
        check(lib().qcx_sharded_restore_identity(self._h), "qcx_sharded_restore_identity")

    def sharded_layout(self):
        """logical qubit -> physical index bit of a sharded register"""
        perm = (C.c_uint * self.num_qubits)()
        check(lib().qcx_sharded_layout(self._h, perm, self.num_qubits), "qcx_sharded_layout")
        return list(perm)

    def total_probability(self):
        """Total probability summed in the reference's order (testing_and_debug.c:28-37: index-ascending, one addition
        per amplitude) -- the exact scan of the measurement run to the end."""
        out = C.c_double(0.0)
        check(lib().qcx_total_probability(self._h, C.byref(out)), "qcx_total_probability")
        return out.value

    def sample_stats(self):
        """(whole-state scans launched, shots answered by a per-shot scan) of the last sample_states call on this register"""
        scans, fb = C.c_ulong(0), C.c_ulong(0)
        check(lib().qcx_sample_last_stats(self._h, C.byref(scans), C.byref(fb)), "qcx_sample_last_stats")
        return scans.value, fb.value

    def marginal(self, first, num):
        """The exact outcome distribution of qubits [first, first + num), the others summed out: a float64 array of 2^num
        (include/qcx.h: qcx_marginal_probabilities; one pinned pairwise summation order, tests/marginal_ref.py)."""
        first, num = int(first), int(num)
        if first < 0 or num < 0:
            raise ValueError("marginal: first and num must be >= 0")
        out = np.empty(1 << num if num <= 30 else 1, dtype=np.float64)      # (num > 30: the call refuses, QCX_UNSUPPORTED)
        check(lib().qcx_marginal_probabilities(self._h, first, num, out.ctypes.data_as(C.c_void_p)), "qcx_marginal_probabilities")
        return out

    def marginal_stats(self):
        """(source, state reads) of the last marginal call on this register: source 0 = the register, 1 = the compact form in
        place, 2 = a pending basis state (no kernel), 3 = the compact form expanded first"""
        src, reads = C.c_uint(0), C.c_ulong(0)
        check(lib().qcx_marginal_last_stats(self._h, C.byref(src), C.byref(reads)), "qcx_marginal_last_stats")
        return src.value, reads.value

    def measure_qubits(self, first, num, rng_or_r, strict=True):
        """Measure the qubits [first, first + num), keep the others and collapse the state (include/qcx.h: qcx_measure_qubits).
        `rng_or_r` is an Rng (one uniform draw is made) or a float r.  Returns (outcome, probability of that outcome).  An
        outcome the state cannot be collapsed onto (probability not a finite number > 0) raises QcxError, which then carries
        .outcome and .probability; strict=False returns (outcome, probability, status) instead and raises nothing for it."""
        first, num = int(first), int(num)
        if first < 0 or num < 0:
            raise ValueError("measure_qubits: first and num must be >= 0")
        out, p = C.c_ulong(0), C.c_double(float("nan"))
        if isinstance(rng_or_r, Rng):
            st = lib().qcx_measure_qubits(self._h, rng_or_r._h, first, num, C.byref(out), C.byref(p))
        else:
            st = lib().qcx_measure_qubits_r(self._h, first, num, float(rng_or_r), C.byref(out), C.byref(p))
        return _collapse_result(st, "measure_qubits", strict, int(out.value), p.value, True)

    def postselect(self, first, num, outcome, strict=True):
        """Collapse the state onto `outcome` of the qubits [first, first + num) (include/qcx.h: qcx_postselect_qubits).  Returns
        the probability the outcome had.  Errors as in measure_qubits; strict=False returns (probability, status)."""
        first, num, outcome = int(first), int(num), int(outcome)
        if first < 0 or num < 0 or outcome < 0:
            raise ValueError("postselect: first, num and outcome must be >= 0")
        p = C.c_double(float("nan"))
        st = lib().qcx_postselect_qubits(self._h, first, num, outcome, C.byref(p))
        return _collapse_result(st, "postselect_qubits", strict, outcome, p.value, False)

    def collapse_stats(self):
        """(source, state reads, state writes) of the last measure_qubits / postselect call on this register: source 0 = the
        register, 2 = a pending basis state (no kernel), 3 = a compact circuit result expanded first"""
        src, reads, writes = C.c_uint(0), C.c_ulong(0), C.c_ulong(0)
        check(lib().qcx_collapse_last_stats(self._h, C.byref(src), C.byref(reads), C.byref(writes)), "qcx_collapse_last_stats")
        return src.value, reads.value, writes.value

    def expectation(self, pauli):
        """<psi|P|psi> of a Pauli string, exactly, from one read of the state, which stays as it was (include/qcx.h:
        qcx_pauli_expectation; the pinned arithmetic is restated in tests/pauli_ref.py).  `pauli`: a str such as "XIZY"
        (character k = qubit k), a dict {qubit: 'X' | 'Y' | 'Z' | 'I'}, or an (x_mask, z_mask) pair (pauli_masks)."""
        x, z = _lib.pauli_masks(pauli, self.num_qubits)
        out = C.c_double(float("nan"))
        check(lib().qcx_pauli_expectation(self._h, x, z, C.byref(out)), "qcx_pauli_expectation")
        return out.value

    def _expectation_terms(self, terms, entry):
        terms = list(terms)
        k = len(terms)
        masks = [_lib.pauli_masks(p, self.num_qubits) for _, p in terms]
        xs = np.array([m[0] for m in masks], dtype=np.uint64)
        zs = np.array([m[1] for m in masks], dtype=np.uint64)
        cs = np.array([float(c) for c, _ in terms], dtype=np.float64)
        values = np.zeros(k, dtype=np.float64)
        total = C.c_double(float("nan"))
        ptr = (lambda a: a.ctypes.data_as(C.c_void_p)) if k else (lambda a: None)
        check(getattr(lib(), entry)(self._h, k, ptr(xs), ptr(zs), ptr(cs), ptr(values), C.byref(total)), entry)
        return total.value, values

    def expectation_sum(self, terms):
        """terms = [(coeff, pauli), ...]: (total, values) with values[k] = expectation(pauli_k), one pass over the state per
        term, and total = the terms' coeff * value added up in order (include/qcx.h: qcx_pauli_expectation_sum)."""
        return self._expectation_terms(terms, "qcx_pauli_expectation_sum")

    def expectation_batch(self, terms):
        """expectation_sum(terms), bit for bit, with the terms that share an x_mask served by one read of the state, up to
        pauli_batch_width() of them a read (include/qcx.h: qcx_pauli_expectation_batch; pauli_batch_plan gives the passes)."""
        return self._expectation_terms(terms, "qcx_pauli_expectation_batch")

    def expectation_stats(self):
        """(source, state reads) of the last expectation / expectation_sum / expectation_batch call on this register: source 0 =
        the register, 2 = a pending basis state (no kernel), 3 = a compact circuit result expanded first; one state read per
        term, or per pass of expectation_batch"""
        src, reads = C.c_uint(0), C.c_ulong(0)
        check(lib().qcx_expectation_last_stats(self._h, C.byref(src), C.byref(reads)), "qcx_expectation_last_stats")
        return src.value, reads.value

    def reduced_density_matrix(self, first, num):
        """The reduced density matrix of qubits [first, first + num), the others traced out: complex128[2^num, 2^num], exactly,
        from one read of the state, which stays as it was (include/qcx.h: qcx_reduced_density_matrix; the pinned arithmetic is
        restated in tests/rdm_ref.py).  Qubit `first` is bit 0 of the row and column index; num <= rdm_max_qubits()."""
        first, num = int(first), int(num)
        if first < 0 or num < 0:
            raise ValueError("reduced_density_matrix: first and num must be >= 0")
        dim = 1 << num if num <= _lib.rdm_max_qubits() else 1          # (a wider range: the call refuses, QCX_UNSUPPORTED)
        out = np.empty((dim, dim), dtype=np.complex128)
        check(lib().qcx_reduced_density_matrix(self._h, first, num, out.ctypes.data_as(C.c_void_p)), "qcx_reduced_density_matrix")
        return out

    def rdm_stats(self):
        """(source, state reads) of the last reduced_density_matrix call on this register: source 0 = the register, 2 = a pending
        basis state (no kernel), 3 = a compact circuit result expanded first; state reads: 1, or 0 for a basis state"""
        src, reads = C.c_uint(0), C.c_ulong(0)
        check(lib().qcx_rdm_last_stats(self._h, C.byref(src), C.byref(reads)), "qcx_rdm_last_stats")
        return src.value, reads.value

    def rotation_batch_stats(self):
        """(passes, wide terms) of the last pauli_rotation_batch call on this register: the passes over the state it ran (the
        plan's: pauli_rotation_batch_plan), and those of them that were one wide term on its own"""
        passes, wide = C.c_ulong(0), C.c_ulong(0)
        check(lib().qcx_rotation_batch_last_stats(self._h, C.byref(passes), C.byref(wide)), "qcx_rotation_batch_last_stats")
        return passes.value, wide.value

    def diagonal_stats(self):
        """(form, table entries) of the last diagonal_gate call on this register: the form of its launch (diagonal_plan's:
        DIAG_TILE, DIAG_GROUP or DIAG_LANE) and the 2^num entries of its table"""
        form, entries = C.c_uint(0), C.c_ulong(0)
        check(lib().qcx_diagonal_last_stats(self._h, C.byref(form), C.byref(entries)), "qcx_diagonal_last_stats")
        return form.value, entries.value

    def permutation_stats(self):
        """(form, moved) of the last permutation_gate call on this register: the form of its plan (permutation_plan's: PERM_LINES
        or PERM_SHARED) and the number of table entries with perm[k] != k (0: the identity, which launches no kernel on a
        register of finite amplitudes)"""
        form, moved = C.c_uint(0), C.c_ulong(0)
        check(lib().qcx_permutation_last_stats(self._h, C.byref(form), C.byref(moved)), "qcx_permutation_last_stats")
        return form.value, moved.value

    def multi_qubit_stats(self):
        """(form, num_targets) of the last multi_qubit_gate call on this register that passed its checks: the form of its plan
        (multi_gate_plan's; always PERM_LINES) and the number of its targets"""
        form, k = C.c_uint(0), C.c_uint(0)
        check(lib().qcx_multi_qubit_last_stats(self._h, C.byref(form), C.byref(k)), "qcx_multi_qubit_last_stats")
        return form.value, k.value

    def gate_batch_stats(self):
        """(passes, low-target gates) of the last gate_batch call on this register: the passes over the state it ran (the plan's:
        gate_batch_plan; the number of gates on a register flagged non-finite), and the gates in them with a target on qubits 0-7,
        which exchange between threads"""
        passes, lds = C.c_ulong(0), C.c_ulong(0)
        check(lib().qcx_gate_batch_last_stats(self._h, C.byref(passes), C.byref(lds)), "qcx_gate_batch_last_stats")
        return passes.value, lds.value

    def expectation_matrix(self, first, O):
        """Tr(rho O) as a Python complex, for any 2^num x 2^num matrix O on the qubits [first, first + num) (qubit `first` = bit 0
        of O's index): <psi|O|psi> of an observable that need not be a Pauli string.  rho is reduced_density_matrix(first, num),
        pinned bit for bit; the product over it is ordinary numpy on the host and is NOT pinned."""
        O = np.asarray(O, dtype=np.complex128)
        dim = O.shape[0] if O.ndim == 2 else 0
        if O.ndim != 2 or O.shape[1] != dim or dim < 1 or dim & (dim - 1):
            raise ValueError("expectation_matrix: O must be a 2^num x 2^num matrix")
        rho = self.reduced_density_matrix(first, dim.bit_length() - 1)
        return complex(np.sum(rho * O.T))

    def set_fusion(self, enable=True):
        """Fused LDS-tile passes (bit-identical results).  True/1: every gate call is queued; False/0 (default): only
        the whole-circuit calls (inverse_QFT, quantum_computation) run as fused passes; -1: strictly one kernel launch
        per gate, inside the whole-circuit calls too; 2 (FUSION_TOLERANCE): opt-in tolerance mode -- runs of controlled
        phases sharing a qubit are merged into one diagonal, NOT bit-exact (rounding-level differences, include/qcx.h)."""
        if enable is True or enable is False:
            mode = int(enable)
        else:
            mode = -1 if int(enable) < 0 else min(int(enable), 2)
        check(lib().qcx_set_fusion(self._h, mode), "qcx_set_fusion")

    def flush(self):
        check(lib().qcx_flush(self._h), "qcx_flush")

    def fusion_stats(self):
        p, g = C.c_ulong(0), C.c_ulong(0)
        check(lib().qcx_fusion_stats(self._h, C.byref(p), C.byref(g)), "qcx_fusion_stats")
        return p.value, g.value

    def synchronize(self):
        check(lib().qcx_synchronize(self._h), "qcx_synchronize")
        self._diag_keep = []                        # (the stream has passed every diagonal_gate call: their device tables are free)

    def set_stream(self, hip_stream_ptr):
        check(lib().qcx_register_set_stream(self._h, C.c_void_p(hip_stream_ptr)), "qcx_register_set_stream")

    def device_pointer(self):
        return int(lib().qcx_device_pointer(self._h) or 0)

    def events_create(self, count):
        check(lib().qcx_events_create(self._h, count), "qcx_events_create")

    def event_record(self, slot):
        check(lib().qcx_event_record(self._h, slot), "qcx_event_record")

    def event_elapsed(self, a, b):
        ms = C.c_double(0.0)
        check(lib().qcx_event_elapsed(self._h, a, b, C.byref(ms)), "qcx_event_elapsed")
        return ms.value

    def timer_start(self):
        check(lib().qcx_timer_start(self._h), "qcx_timer_start")

    def timer_stop(self):
        ms = C.c_double(0.0)
        check(lib().qcx_timer_stop(self._h, C.byref(ms)), "qcx_timer_stop")
        return ms.value


def _collapse_result(status, where, strict, outcome, probability, with_outcome):
    if strict and status != _lib.NO_ERROR:
        err = _lib.QcxError(status, where)
        err.outcome, err.probability = outcome, probability        # (set by the library before it refused the collapse)
        raise err
    res = (outcome, probability) if with_outcome else (probability,)
    if not strict:
        return res + (status,)
    return res if with_outcome else probability


# ---- the reference's free functions ----------------------------------------------------------
def reset_register(reg):
    check(lib().qcx_reset_register(reg._h), "reset_register")


def hadamard_gate(qubit_num, reg, matrix=None):
    check(lib().qcx_hadamard_gate(qubit_num, reg._h), "hadamard_gate")


def c_phase_shift_gate(c_qubit_num, qubit_num, theta, reg, matrix=None):
    check(lib().qcx_c_phase_shift_gate(c_qubit_num, qubit_num, float(theta), reg._h), "c_phase_shift_gate")


def c_amodc_gate(C_, atox, c_qubit_num, reg, matrix=None):
    check(lib().qcx_c_amodc_gate(C_, int(atox), c_qubit_num, reg._h), "c_amodc_gate")


def _matrix8(U):
    """U as the 8 doubles qcx_one_qubit_gate takes: row-major (re, im)"""
    m = np.asarray(U, dtype=complex)
    if m.shape != (2, 2):
        raise ValueError(f"a one-qubit gate is a 2x2 matrix, not shape {m.shape}")
    return np.ascontiguousarray(m.reshape(4)).view(np.float64)


def one_qubit_gate(qubit_num, U, reg):
    """Apply the 2x2 matrix U (anything numpy.asarray(U, complex) turns into shape (2, 2)) to qubit `qubit_num`, with the
    reference's mat-vec arithmetic (include/qcx.h: qcx_one_qubit_gate).  U is applied as given, not checked for unitarity."""
    u = _matrix8(U)
    check(lib().qcx_one_qubit_gate(int(qubit_num), u.ctypes.data_as(C.c_void_p), reg._h), "one_qubit_gate")


def c_one_qubit_gate(c_qubit_num, qubit_num, U, reg):
    """one_qubit_gate on the amplitudes whose qubit `c_qubit_num` reads 1 (include/qcx.h: qcx_c_one_qubit_gate)"""
    u = _matrix8(U)
    check(lib().qcx_c_one_qubit_gate(int(c_qubit_num), int(qubit_num), u.ctypes.data_as(C.c_void_p), reg._h), "c_one_qubit_gate")


def _matrix32(U):
    """U as the 32 doubles qcx_two_qubit_gate takes: row-major (re, im); U is a 4x4 matrix or those 32 doubles themselves"""
    m = np.asarray(U)
    if m.shape == (32,) and not np.iscomplexobj(m):
        return np.ascontiguousarray(m, dtype=np.float64)
    m = np.asarray(U, dtype=complex)
    if m.shape != (4, 4):
        raise ValueError(f"a two-qubit gate is a 4x4 matrix, not shape {m.shape}")
    return np.ascontiguousarray(m.reshape(16)).view(np.float64)


def two_qubit_gate(qubit0, qubit1, U, reg):
    """Apply the 4x4 matrix U (anything numpy.asarray(U, complex) turns into shape (4, 4), or the 32 doubles) to two qubits, with
    the reference's mat-vec arithmetic (include/qcx.h: qcx_two_qubit_gate).  Matrix index = bit(qubit0) + 2 * bit(qubit1): "A on
    qubit0, B on qubit1" is numpy.kron(B, A).  U is applied as given, not checked for unitarity."""
    u = _matrix32(U)
    check(lib().qcx_two_qubit_gate(int(qubit0), int(qubit1), u.ctypes.data_as(C.c_void_p), reg._h), "two_qubit_gate")


def c_two_qubit_gate(c_qubit_num, qubit0, qubit1, U, reg):
    """two_qubit_gate on the amplitudes whose qubit `c_qubit_num` reads 1 (include/qcx.h: qcx_c_two_qubit_gate)"""
    u = _matrix32(U)
    check(lib().qcx_c_two_qubit_gate(int(c_qubit_num), int(qubit0), int(qubit1), u.ctypes.data_as(C.c_void_p), reg._h), "c_two_qubit_gate")


def _control_masks(controls, values):
    """(ctrl_mask, ctrl_values) of the mc gates: controls = an iterable of qubit numbers or an int mask; values = None (all
    positive), an int mask, or a {qubit: 0 | 1} dict"""
    def qubit(q):
        if isinstance(q, bool) or not isinstance(q, (int, np.integer)) or not 0 <= int(q) < 64:
            raise ValueError(f"{q!r} is not a qubit")
        return int(q)
    if isinstance(controls, (int, np.integer)) and not isinstance(controls, bool):
        mask = int(controls)
        if not 0 <= mask < 2 ** 64:
            raise ValueError(f"a control mask is a 64-bit set of qubits, not {controls!r}")
    else:
        try:
            mask = 0
            for q in controls:
                mask |= 1 << qubit(q)
        except TypeError:
            raise ValueError(f"controls are an iterable of qubits or an int mask, not {controls!r}") from None
    if values is None:
        return mask, mask
    if isinstance(values, dict):
        vals = mask
        for q, v in values.items():
            if not (mask >> qubit(q)) & 1:
                raise ValueError(f"values names qubit {q}, which is no control")
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v not in (0, 1):
                raise ValueError(f"a control's value is 0 or 1, not {v!r}")
            if not v:
                vals &= ~(1 << int(q))
        return mask, vals
    if isinstance(values, (int, np.integer)) and not isinstance(values, bool):
        vals = int(values)
        if vals < 0 or vals & ~mask:
            raise ValueError(f"values {vals:#x} has bits outside the controls {mask:#x}")
        return mask, vals
    raise ValueError(f"values is None, an int mask or a {{qubit: 0 | 1}} dict, not {values!r}")


def mc_one_qubit_gate(controls, qubit_num, U, reg, values=None):
    """one_qubit_gate on the amplitudes whose control qubits read their `values` (include/qcx.h: qcx_mc_one_qubit_gate): any
    number of controls, positive or negative.  controls: an iterable of qubit numbers or an int mask; values: None = all
    positive, an int mask (a subset of the controls: set = fires on 1), or a {qubit: 0 | 1} dict for the controls that differ
    from 1.  mc_one_qubit_gate({c0, c1}, t, GATES["X"], reg) is a Toffoli."""
    mask, vals = _control_masks(controls, values)
    u = _matrix8(U)
    check(lib().qcx_mc_one_qubit_gate(mask, vals, int(qubit_num), u.ctypes.data_as(C.c_void_p), reg._h), "mc_one_qubit_gate")


def mc_two_qubit_gate(controls, qubit0, qubit1, U, reg, values=None):
    """two_qubit_gate on the amplitudes whose control qubits read their `values` (include/qcx.h: qcx_mc_two_qubit_gate);
    controls and values as for mc_one_qubit_gate.  mc_two_qubit_gate({c}, a, b, GATES2["SWAP"], reg) is a Fredkin."""
    mask, vals = _control_masks(controls, values)
    u = _matrix32(U)
    check(lib().qcx_mc_two_qubit_gate(mask, vals, int(qubit0), int(qubit1), u.ctypes.data_as(C.c_void_p), reg._h), "mc_two_qubit_gate")


def gate_batch(gates, reg):
    """Apply gates = [(U, targets) or (U, targets, control), ...] in order -- a circuit layer -- in as few passes over the state as
    locality allows: bit for bit the state that one_qubit_gate / c_one_qubit_gate / two_qubit_gate / c_two_qubit_gate gate by
    gate leave (include/qcx.h: qcx_gate_batch).  `targets` is a qubit or a 1- or 2-tuple (qubit0, qubit1); U is 2x2 for one target
    and 4x4 (or the 32 doubles) for two, as those calls take it.  gate_batch_plan(gates, n) gives the passes and
    reg.gate_batch_stats() what the last call ran."""
    gates = list(gates)
    recs = (_lib.Gate * max(len(gates), 1))()
    for rec, g in zip(recs, gates):
        t, c = _lib.gate_targets(g)
        for q in t + (() if c is None else (c,)):
            if not 0 <= q < 2 ** 31:
                raise ValueError(f"{q} is not a qubit")
        u = _matrix8(g[0]) if len(t) == 1 else _matrix32(g[0])
        rec.ntargets, rec.control, rec.qubit0, rec.qubit1 = len(t), (-1 if c is None else c), t[0], (t[1] if len(t) == 2 else 0)
        rec.u[:u.size] = u.tolist()
    check(lib().qcx_gate_batch(reg._h, len(gates), C.cast(recs, C.c_void_p) if gates else None), "gate_batch")


def pauli_rotation(pauli, theta, reg):
    """Apply exp(-i theta/2 P) for the Pauli string P in one pass over the state, for any string (include/qcx.h:
    qcx_pauli_rotation; the pinned arithmetic is restated in tests/pauli_rotation_ref.py).  `pauli`: what Register.expectation
    takes -- a str such as "XIZY" (character k = qubit k), a dict {qubit: 'X' | 'Y' | 'Z' | 'I'}, or an (x_mask, z_mask) pair."""
    x, z = _lib.pauli_masks(pauli, reg.num_qubits)
    check(lib().qcx_pauli_rotation(x, z, float(theta), reg._h), "pauli_rotation")


def pauli_rotation_batch(terms, reg):
    """Apply the rotations terms = [(pauli, theta), ...] in order -- a Trotter step -- in as few passes over the state as locality
    allows: bit for bit the state that pauli_rotation(pauli, theta, reg) term by term leaves (include/qcx.h:
    qcx_pauli_rotation_batch).  `pauli` as for pauli_rotation; pauli_rotation_batch_plan(terms, n) gives the passes and
    reg.rotation_batch_stats() what the last call ran."""
    terms = list(terms)
    k = len(terms)
    masks = [_lib.pauli_masks(p, reg.num_qubits) for p, _ in terms]
    xs = np.array([m[0] for m in masks], dtype=np.uint64)
    zs = np.array([m[1] for m in masks], dtype=np.uint64)
    th = np.array([float(t) for _, t in terms], dtype=np.float64)
    ptr = (lambda a: a.ctypes.data_as(C.c_void_p)) if k else (lambda a: None)
    check(lib().qcx_pauli_rotation_batch(reg._h, k, ptr(xs), ptr(zs), ptr(th)), "pauli_rotation_batch")


def diagonal_gate(first, num, d, reg):
    """Multiply every amplitude by the entry of the table d that its bits first .. first+num-1 select, qubit `first` being bit 0
    of the entry's number, in one pass over the state (include/qcx.h: qcx_diagonal_gate; the pinned arithmetic is restated in
    tests/diagonal_ref.py).  d is either
      - anything numpy.asarray(d, complex) turns into 2^num values: the host form, copied before the call returns
        (num <= diagonal_host_max_qubits()), or
      - a table in the memory of the register's GPU, for any num <= n: an integer device address of 2^num complex128 values, or
        an object with data_ptr() such as a torch tensor -- complex128, contiguous, 2^num elements, on a GPU.  The table must be
        complete when the call is made: the stream that produced it must have been synchronised (torch.cuda.synchronize()).
        It must stay unchanged until reg.synchronize(); the register keeps a reference to the object until then.
    Every component must be finite with |.| <= 1; the table is applied as given, not checked for unit modulus."""
    first, num = int(first), int(num)
    if hasattr(d, "data_ptr") or isinstance(d, (int, np.integer)):
        if hasattr(d, "data_ptr"):
            if "complex128" not in str(getattr(d, "dtype", "")):
                raise TypeError(f"a device table holds complex128 values, not {getattr(d, 'dtype', None)}")
            if not d.is_contiguous():
                raise ValueError("a device table must be contiguous")
            if num < 0 or int(d.numel()) != 1 << num:
                raise ValueError(f"a diagonal over {num} qubits has {1 << max(num, 0)} entries, not {int(d.numel())}")
            if not getattr(d, "is_cuda", False):
                raise ValueError("a table with data_ptr() must lie on a GPU; pass host values as an array")
            address = int(d.data_ptr())
        else:
            address = int(d)
        check(lib().qcx_diagonal_gate_device(first, num, C.c_void_p(address), reg._h), "diagonal_gate")
        if not hasattr(reg, "_diag_keep"):
            reg._diag_keep = []
        reg._diag_keep.append(d)
        return
    t = np.ascontiguousarray(np.asarray(d, dtype=complex).reshape(-1))
    if num < 0 or t.size != 1 << num:
        raise ValueError(f"a diagonal over {num} qubits has {1 << max(num, 0)} entries, not {t.size}")
    check(lib().qcx_diagonal_gate(first, num, t.view(np.float64).ctypes.data_as(C.c_void_p), reg._h), "diagonal_gate")


def phase_table(angles):
    """e^{i angle} for every angle, each through qcx_polar (one sincos, the factor c_phase_shift_gate uses): a complex128 array
    for diagonal_gate, so that the table (1, 1, 1, e^{i theta}) on two qubits gives c_phase_shift_gate's bits"""
    th = np.ascontiguousarray(np.asarray(angles, dtype=np.float64).reshape(-1))
    out = np.empty(2 * th.size, dtype=np.float64)
    if th.size:
        lib().qcx_polar_array(th.size, th.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    return out.view(np.complex128)


def diagonal_phase(first, num, angles, reg):
    """diagonal_gate with the table phase_table(angles): amplitude i takes the phase e^{i angles[k(i)]} -- a QAOA cost layer is
    diagonal_phase(0, n, -gamma * C, reg)"""
    diagonal_gate(first, num, phase_table(angles), reg)


def permutation_gate(first, num, perm, reg, controls=None, values=None):
    """A classical reversible function on the qubits first .. first+num-1: basis state |k> of the range goes to |perm[k]>, qubit
    `first` being bit 0 of k, on the amplitudes whose control qubits read their `values`, in one pass over those amplitudes
    (include/qcx.h: qcx_permutation_gate; tests/permutation_ref.py restates it).  perm is anything numpy.asarray turns into
    2^num integers that form a bijection of [0, 2^num), num <= permutation_max_qubits(); controls and values as for
    mc_one_qubit_gate (None: no control).  The table is copied before the call returns.  modmul_table, modadd_table,
    xor_oracle_table and qubit_permutation_table build common tables."""
    first, num = int(first), int(num)
    t = np.asarray(perm)
    if t.dtype.kind not in "iu" or num < 0 or t.size != 1 << num:
        raise ValueError(f"a permutation of {num} qubits is a table of {1 << max(num, 0)} integers")
    t = t.reshape(-1)
    if t.size and (int(t.min()) < 0 or int(t.max()) > 0xFFFFFFFF):
        raise ValueError("a permutation table holds values in [0, 2^num)")
    t = np.ascontiguousarray(t, dtype=np.uint32)
    mask, vals = _control_masks(() if controls is None else controls, values)
    check(lib().qcx_permutation_gate(mask, vals, first, num, t.ctypes.data_as(C.c_void_p), reg._h), "permutation_gate")


def modmul_table(a, C_, num):
    """k -> a k mod C_ for k < C_ and k -> k above: the table of a modular multiply on num qubits (under a control above them,
    c_amodc_gate).  gcd(a, C_) must be 1 and C_ <= 2^num."""
    a, C_, num = int(a), int(C_), int(num)
    if C_ < 1 or C_ > 1 << num or math.gcd(a, C_) != 1:
        raise ValueError(f"modmul_table: k -> {a} k mod {C_} is no permutation of {num} qubits' basis states")
    k = np.arange(1 << num, dtype=np.int64)
    return np.where(k < C_, (a % C_) * k % C_, k).astype(np.uint32)


def modadd_table(c, num, modulus=None):
    """k -> k + c mod 2^num, or with a modulus <= 2^num: k -> k + c mod modulus below it and k -> k above"""
    c, num = int(c), int(num)
    m = 1 << num if modulus is None else int(modulus)
    if m < 1 or m > 1 << num:
        raise ValueError(f"modadd_table: a modulus of {m} does not fit {num} qubits")
    k = np.arange(1 << num, dtype=np.int64)
    return np.where(k < m, (k + c % m) % m, k).astype(np.uint32)


def xor_oracle_table(f_values, nx, ny):
    """|x>|y> -> |x>|y xor f(x)> on nx + ny qubits, x in the low nx bits of the table's index and y in the ny above them;
    f_values = f(0), ..., f(2^nx - 1), each below 2^ny"""
    nx, ny = int(nx), int(ny)
    f = np.asarray(f_values).reshape(-1)
    if f.dtype.kind not in "iu" or f.size != 1 << nx or (f.size and (int(f.min()) < 0 or int(f.max()) >= 1 << ny)):
        raise ValueError(f"xor_oracle_table: f is {1 << nx} integers below 2^{ny}")
    k = np.arange(1 << (nx + ny), dtype=np.int64)
    x, y = k & ((1 << nx) - 1), k >> nx
    return (x | ((y ^ f.astype(np.int64)[x]) << nx)).astype(np.uint32)


def qubit_permutation_table(order):
    """bit j of k moves to bit order[j]: a re-ordering of the range's qubits.  qubit_permutation_table(range(num)[::-1]) is the
    bit reversal a QFT owes."""
    order = [int(q) for q in order]
    num = len(order)
    if sorted(order) != list(range(num)):
        raise ValueError(f"qubit_permutation_table: {order!r} is no re-ordering of {num} qubits")
    k = np.arange(1 << num, dtype=np.int64)
    out = np.zeros_like(k)
    for j, q in enumerate(order):
        out |= ((k >> j) & 1) << q
    return out.astype(np.uint32)


def _matrix_multi(U, k):
    """U as the 2 * 4^k doubles qcx_mc_multi_qubit_gate takes: row-major (re, im); U is a 2^k x 2^k matrix or those doubles"""
    d = 1 << k
    m = np.asarray(U)
    if m.shape == (2 * d * d,) and not np.iscomplexobj(m):
        return np.ascontiguousarray(m, dtype=np.float64)
    m = np.asarray(U, dtype=complex)
    if m.shape != (d, d):
        raise ValueError(f"a gate on {k} qubits is a {d}x{d} matrix, not shape {m.shape}")
    return np.ascontiguousarray(m.reshape(d * d)).view(np.float64)


def multi_qubit_gate(targets, U, reg, controls=None, values=None):
    """Apply the dense 2^k x 2^k matrix U to the k = 1 .. 5 distinct qubits `targets`, on the amplitudes whose control qubits
    read their `values`, in one pass over those amplitudes, with the reference's mat-vec arithmetic (include/qcx.h:
    qcx_mc_multi_qubit_gate; tests/multi_qubit_ref.py restates it).  targets[j] is bit j of the matrix index, two_qubit_gate's
    convention: "A on targets[0], B on targets[1], C on targets[2]" is numpy.kron(C, numpy.kron(B, A)).  U is anything
    numpy.asarray(U, complex) turns into shape (2^k, 2^k), or the 2 * 4^k doubles; it is applied as given, not checked for
    unitarity, and copied before the call returns.  controls and values as for mc_one_qubit_gate (None: no control).
    fused_matrix turns a list of one- and two-qubit gates into such a block."""
    t = [int(q) for q in (targets if np.ndim(targets) else (targets,))]
    if any(not 0 <= q < 2 ** 31 for q in t):
        raise ValueError(f"{targets!r} are not qubits")
    if not 1 <= len(t) <= _lib.multi_qubit_max_targets():
        raise ValueError(f"a matrix acts on 1 to {_lib.multi_qubit_max_targets()} qubits, not {len(t)}")
    u = _matrix_multi(U, len(t))
    mask, vals = _control_masks(() if controls is None else controls, values)
    arr = (C.c_uint * len(t))(*t)
    check(lib().qcx_mc_multi_qubit_gate(mask, vals, len(t), C.cast(arr, C.c_void_p), u.ctypes.data_as(C.c_void_p), reg._h), "multi_qubit_gate")


def fused_matrix(gates, targets):
    """The product of gates = [(U, targets) or (U, targets, control), ...] (gate_batch's form, applied in order) as ONE
    2^k x 2^k matrix on the k qubits `targets`, in multi_qubit_gate's index convention (targets[j] is bit j), in plain numpy:
    multi_qubit_gate(targets, fused_matrix(layer, targets), reg) is the layer as one block.  Every qubit a gate names, its
    control included, must lie in `targets`.  The product is rounded as numpy rounds a matrix product, so the block equals
    the gate-by-gate calls to rounding error, not bit for bit."""
    tq = [int(q) for q in targets]
    if len(set(tq)) != len(tq):
        raise ValueError(f"fused_matrix: the targets {targets!r} are not distinct")
    k = len(tq)
    where = {q: j for j, q in enumerate(tq)}
    idx = np.arange(1 << k)
    out = np.eye(1 << k, dtype=complex)
    for g in gates:
        t, c = _lib.gate_targets(g)
        for q in t + (() if c is None else (c,)):
            if q not in where:
                raise ValueError(f"fused_matrix: qubit {q} of a gate is not among the targets {tq}")
        d = 1 << len(t)
        u = np.asarray(g[0])
        u = u.astype(np.float64).view(np.complex128).reshape(d, d) if u.shape == (2 * d * d,) and not np.iscomplexobj(u) else np.asarray(g[0], dtype=complex)
        if u.shape != (d, d):
            raise ValueError(f"fused_matrix: a gate on {len(t)} qubits is a {d}x{d} matrix, not shape {u.shape}")
        local = sum(((idx >> where[q]) & 1) << l for l, q in enumerate(t))      # the gate's own index of every block index
        tmask = sum(1 << where[q] for q in t)
        fires = np.ones(1 << k, dtype=bool) if c is None else ((idx >> where[c]) & 1).astype(bool)
        G = np.zeros((1 << k, 1 << k), dtype=complex)
        for r in idx:
            if not fires[r]:
                G[r, r] = 1.0
                continue
            for col in range(d):
                G[r, (r & ~tmask) | sum(((col >> l) & 1) << where[q] for l, q in enumerate(t))] = u[local[r], col]
        out = G @ out
    return out


def controlled(U2):
    """the 4x4 matrix "U2 on qubit1 where qubit0 reads 1": the identity with U2 in rows and columns {1, 3}, so that
    c_two_qubit_gate(c, a, b, controlled(X)) is a Toffoli with controls c and a"""
    m = np.asarray(U2, dtype=complex)
    if m.shape != (2, 2):
        raise ValueError(f"controlled() takes a 2x2 matrix, not shape {m.shape}")
    out = np.eye(4, dtype=complex)
    out[np.ix_([1, 3], [1, 3])] = m
    return out


def phase(theta):
    """diag(1, e^{i theta}) with the factor c_phase_shift_gate uses (qcx_polar)"""
    c, s = _lib.polar(theta)
    return np.array([[1.0, 0.0], [0.0, complex(c, s)]], dtype=complex)


def rz(theta):
    """diag(e^{-i theta/2}, e^{+i theta/2}), both factors from qcx_polar"""
    cm, sm = _lib.polar(-0.5 * float(theta))
    cp, sp = _lib.polar(0.5 * float(theta))
    return np.array([[complex(cm, sm), 0.0], [0.0, complex(cp, sp)]], dtype=complex)


def __getattr__(name):
    """GATES: the exact matrices X, Y, Z, S, T, H.  Built on first use (PEP 562), because T's factor is the library's
    qcx_polar(pi/4) and importing the package must not load the library."""
    if name == "GATES2":
        # the exact two-qubit matrices, matrix index = bit(qubit0) + 2 * bit(qubit1); CNOT: control qubit0, target qubit1
        gates2 = {
            "SWAP": np.array([[1, 0, 0, 0], [0, 0, 1, 0], [0, 1, 0, 0], [0, 0, 0, 1]], dtype=complex),
            "ISWAP": np.array([[1, 0, 0, 0], [0, 0, 1j, 0], [0, 1j, 0, 0], [0, 0, 0, 1]], dtype=complex),
            "CNOT": np.array([[1, 0, 0, 0], [0, 0, 0, 1], [0, 0, 1, 0], [0, 1, 0, 0]], dtype=complex),
            "CZ": np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, -1]], dtype=complex),
        }
        globals()["GATES2"] = gates2
        return gates2
    if name != "GATES":
        raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
    s = 0.70710678118654752440          # M_SQRT1_2 (qc_shor.c:210-213): hadamard_gate's entry
    gates = {
        "X": np.array([[0, 1], [1, 0]], dtype=complex),
        "Y": np.array([[0, -1j], [1j, 0]], dtype=complex),
        "Z": np.array([[1, 0], [0, -1]], dtype=complex),
        "S": np.array([[1, 0], [0, 1j]], dtype=complex),
        "T": phase(np.pi / 4),
        "H": np.array([[s, s], [s, -s]], dtype=complex),
    }
    globals()["GATES"] = gates
    return gates


def swap_states(reg):
    check(lib().qcx_swap_states(reg._h), "swap_states")


def inverse_QFT(reg, matrix=None):
    check(lib().qcx_inverse_QFT(reg._h), "inverse_QFT")


def quantum_computation(C_, a, reg, matrix=None, ref_intpow=False):
    """ref_intpow=True reproduces the reference's 32-bit INT_POW(a, x) (qc_shor.c:158-159, 729)."""
    check(lib().qcx_quantum_computation(C_, a, int(bool(ref_intpow)), reg._h), "quantum_computation")


def measure_state(reg, rng):
    """Collapse the register; returns the measured basis-state index (qc_shor.c:272-306).
    `rng` is an Rng, or a float r in [0,1) to inject the uniform draw directly."""
    out = C.c_ulong(0)
    if isinstance(rng, Rng):
        check(lib().qcx_measure_state(reg._h, rng._h, C.byref(out)), "measure_state")
    else:
        check(lib().qcx_measure_state_r(reg._h, float(rng), C.byref(out)), "measure_state")
    return int(out.value)


def sample_states(reg, rng_or_rs, shots=None):
    """Many measurement shots from the current state WITHOUT collapsing it, from one read of the state (include/qcx.h:
    qcx_sample_states).  `rng_or_rs` is an Rng -- `shots` draws are made, shot i gets the i-th: the indices K rounds of
    reset + circuit + measure_state would give with the same Rng --, or a sequence of draws r (any order, repeats allowed).
    Returns a numpy.uint64 array; the register's state is left exactly as it was."""
    if isinstance(rng_or_rs, Rng):
        if shots is None:
            raise ValueError("sample_states: an Rng needs the number of shots")
        k = int(shots)
        out = np.zeros(k, dtype=np.uint64)
        check(lib().qcx_sample_states(reg._h, rng_or_rs._h, k, out.ctypes.data_as(C.c_void_p)), "sample_states")
        return out
    rs = np.ascontiguousarray(np.asarray(rng_or_rs, dtype=np.float64).reshape(-1))
    if shots is not None and int(shots) != rs.size:
        raise ValueError(f"sample_states: {rs.size} draws given for {shots} shots")
    out = np.zeros(rs.size, dtype=np.uint64)
    check(lib().qcx_sample_states_r(reg._h, rs.ctypes.data_as(C.c_void_p), rs.size, out.ctypes.data_as(C.c_void_p)),
          "sample_states")
    return out


def measure_qubits(reg, first, num, rng_or_r, strict=True):
    """Measure the qubits [first, first + num) of `reg` and collapse it: (outcome, probability) (Register.measure_qubits).
    `rng_or_r` is an Rng or a float r, as for measure_state."""
    return reg.measure_qubits(first, num, rng_or_r, strict=strict)


def postselect_qubits(reg, first, num, outcome, strict=True):
    """Collapse `reg` onto `outcome` of the qubits [first, first + num): the probability it had (Register.postselect)."""
    return reg.postselect(first, num, outcome, strict=strict)


def purity(rho):
    """Re Tr rho^2 of a matrix Register.reduced_density_matrix returned: 1 for a pure reduced state, 2^-num for the maximally
    mixed one (ordinary numpy, not pinned)"""
    rho = np.asarray(rho, dtype=np.complex128)
    return float(np.real(np.sum(rho * rho.T)))


def von_neumann_entropy(rho, base=2):
    """-Tr rho log rho of a matrix Register.reduced_density_matrix returned, in units of log `base` (bits by default), from
    numpy.linalg.eigvalsh; eigenvalues <= 0 are dropped (ordinary numpy, not pinned)"""
    ev = np.linalg.eigvalsh(np.asarray(rho, dtype=np.complex128))
    ev = ev[ev > 0]
    return float(-np.sum(ev * np.log(ev)) / np.log(base))


def omega_distribution(reg):
    """P[x~] for x~ = 0 .. 2^L - 1: the exact probability that measuring the register gives x~ (the L register read in
    reversed bit order, as read_omega reads it), from one marginal of the L register (Register.marginal)."""
    L, M = reg.L_size, reg.M_size
    probs = reg.marginal(M, L)
    v = np.arange(1 << L, dtype=np.uint64)
    xt = np.zeros_like(v)
    for p in range(L):
        xt |= ((v >> np.uint64(L - 1 - p)) & np.uint64(1)) << np.uint64(p)
    out = np.empty_like(probs)
    out[xt] = probs
    return out


def read_omega(state_num, reg):
    """x~/2^L with the L register read in reversed bit order (qc_shor.c:868-883)."""
    x = 0
    for p in range(reg.L_size):
        x |= ((state_num >> (reg.L_size + reg.M_size - 1 - p)) & 1) << p
    return x / float(1 << reg.L_size)


def display_state(reg, file=None, limit=None):
    """testing_and_debug.c:7-26: one line per basis state with non-zero amplitude, qubits MSB first,
    followed by |amplitude| with two decimals.  Reads the whole state to the host (debug tool)."""
    import sys
    out = file or sys.stdout
    v = reg.read().reshape(-1, 2)
    mag = np.hypot(v[:, 0], v[:, 1])
    shown = 0
    for i in np.nonzero(mag)[0]:
        print("|" + format(int(i), "0%db" % reg.num_qubits) + "> %.2f" % mag[i], file=out)
        shown += 1
        if limit is not None and shown >= limit:
            break
    return shown


def check_normalisation(reg, file=None):
    """testing_and_debug.c:28-37: prints the total probability with 16 decimals and returns it"""
    import sys
    total = reg.total_probability()
    print("Total Probability: %.16f" % total, file=file or sys.stdout)
    return total


def load_state_file(path):
    """Read a state file written by Register.save / qcx_state_save on the host: returns (L, M, amplitudes as an
    interleaved float64 array, memory-mapped).  Verifies magic and version; the checksum is checked by Register.load."""
    import struct
    with open(path, "rb") as f:
        hdr = f.read(64)
    magic, version, bpa, L, M, dim, checksum = struct.unpack("<8sIIiiQQ", hdr[:40])
    if magic != b"QCXSTATE" or version != 1 or bpa != 16 or dim != 1 << (L + M):
        raise ValueError(f"{path}: not a qcx state file")
    return L, M, np.memmap(path, dtype="<f8", mode="r", offset=64, shape=(2 * dim,))
