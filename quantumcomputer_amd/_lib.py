"""ctypes loader for libqcx.so (include/qcx.h).

The HIP library is the product: if it is missing this module raises -- there is
no CPU fallback anywhere in quantumcomputer_amd.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("QCX_LIB", os.path.join(_HERE, "libqcx.so"))      # (override: sanitizer builds of the host code, test rigs)

# status codes (include/qcx.h; 0..4 are the reference's ErrorCode, qc_shor.c:164-170)
NO_ERROR, INSUFFICIENT_MEMORY, BAD_ARGUMENTS, PERIOD_NOT_FOUND, UNKNOWN_ERROR = range(5)
HIP_ERROR, BAD_QUBIT, UNSUPPORTED = 5, 6, 7


class QcxError(RuntimeError):
    def __init__(self, status, where=""):
        self.status = status
        msg = lib().qcx_status_string(status).decode()
        detail = lib().qcx_last_error().decode()
        super().__init__(f"{where}: {msg} ({status})" + (f" [{detail}]" if detail else ""))


# every symbol include/qcx.h declares, with its ctypes signature
_u, _ul, _ull, _i, _d, _p = C.c_uint, C.c_ulong, C.c_ulonglong, C.c_int, C.c_double, C.c_void_p
_u64, _i64 = C.c_uint64, C.c_int64
SIGNATURES = {
    "qcx_version": (C.c_char_p, []),
    "qcx_status_string": (C.c_char_p, [_i]),
    "qcx_last_error": (C.c_char_p, []),
    "qcx_device_count": (_i, [C.POINTER(_i)]),
    "qcx_set_device": (_i, [_i]),
    "qcx_register_create": (_i, [_i, _i, C.POINTER(_p)]),
    "qcx_register_destroy": (_i, [_p]),
    "qcx_register_create_sharded": (_i, [_i, _i, _u, C.POINTER(_i), C.POINTER(_p)]),
    "qcx_spread_devices": (_i, [_u, _i, C.POINTER(_i)]),
    "qcx_sharded_selfcheck": (_i, [_p]),
    "qcx_sharded_selfchecks": (_ul, [_p]),
    "qcx_register_shards": (_u, [_p]),
    "qcx_sharded_stats": (_i, [_p, C.POINTER(_ul), C.POINTER(_ul)]),
    "qcx_sharded_set_relays": (_i, [_p, _u, C.POINTER(_i)]),
    "qcx_num_qubits": (_u, [_p]),
    "qcx_num_states": (_ul, [_p]),
    "qcx_L_size": (_i, [_p]),
    "qcx_M_size": (_i, [_p]),
    "qcx_register_set_stream": (_i, [_p, _p]),
    "qcx_synchronize": (_i, [_p]),
    "qcx_reset_register": (_i, [_p]),
    "qcx_hadamard_gate": (_i, [_u, _p]),
    "qcx_c_phase_shift_gate": (_i, [_u, _u, _d, _p]),
    "qcx_c_amodc_gate": (_i, [_u, _ull, _u, _p]),
    "qcx_one_qubit_gate": (_i, [_u, _p, _p]),
    "qcx_c_one_qubit_gate": (_i, [_u, _u, _p, _p]),
    "qcx_two_qubit_gate": (_i, [_u, _u, _p, _p]),
    "qcx_c_two_qubit_gate": (_i, [_u, _u, _u, _p, _p]),
    "qcx_mc_one_qubit_gate": (_i, [_u64, _u64, _u, _p, _p]),
    "qcx_mc_two_qubit_gate": (_i, [_u64, _u64, _u, _u, _p, _p]),
    "qcx_pauli_rotation": (_i, [_u64, _u64, _d, _p]),
    "qcx_pauli_rotation_batch": (_i, [_p, _ul, _p, _p, _p]),
    "qcx_pauli_rotation_batch_width": (_u, []),
    "qcx_rotation_batch_last_stats": (_i, [_p, C.POINTER(_ul), C.POINTER(_ul)]),
    "qcx_pauli_rotation_batch_plan": (_i, [_u, _ul, _p, _u, _p, C.POINTER(_ul), _p, _p]),
    "qcx_gate_batch": (_i, [_p, _ul, _p]),
    "qcx_gate_batch_width": (_u, []),
    "qcx_gate_batch_last_stats": (_i, [_p, C.POINTER(_ul), C.POINTER(_ul)]),
    "qcx_gate_batch_plan": (_i, [_u, _ul, _p, _p, _u, _p, C.POINTER(_ul), _p]),
    "qcx_diagonal_gate": (_i, [_u, _u, _p, _p]),
    "qcx_diagonal_gate_device": (_i, [_u, _u, _p, _p]),
    "qcx_diagonal_host_max_qubits": (_u, []),
    "qcx_diagonal_last_stats": (_i, [_p, C.POINTER(_u), C.POINTER(_ul)]),
    "qcx_diagonal_plan": (_i, [_u, _u, _u, _p]),
    "qcx_polar_array": (None, [_ul, _p, _p]),
    "qcx_permutation_gate": (_i, [_u64, _u64, _u, _u, _p, _p]),
    "qcx_permutation_max_qubits": (_u, []),
    "qcx_permutation_last_stats": (_i, [_p, C.POINTER(_u), C.POINTER(_ul)]),
    "qcx_permutation_plan": (_i, [_u, _u64, _u64, _u, _u, _p]),
    "qcx_mc_multi_qubit_gate": (_i, [_u64, _u64, _u, _p, _p, _p]),
    "qcx_multi_qubit_max_targets": (_u, []),
    "qcx_multi_qubit_last_stats": (_i, [_p, C.POINTER(_u), C.POINTER(_u)]),
    "qcx_multi_gate_plan": (_i, [_u, _u64, _u64, _u, _p, _p]),
    "qcx_swap_states": (_i, [_p]),
    "qcx_inverse_QFT": (_i, [_p]),
    "qcx_quantum_computation": (_i, [_u, _u, _i, _p]),
    "qcx_ref_int_pow": (_u, [_d, _d]),
    "qcx_polar": (None, [_d, C.POINTER(_d), C.POINTER(_d)]),
    "qcx_set_fusion": (_i, [_p, _i]),
    "qcx_flush": (_i, [_p]),
    "qcx_fusion_stats": (_i, [_p, C.POINTER(_ul), C.POINTER(_ul)]),
    "qcx_measure_state": (_i, [_p, _p, C.POINTER(_ul)]),
    "qcx_measure_state_r": (_i, [_p, _d, C.POINTER(_ul)]),
    "qcx_sample_states": (_i, [_p, _p, _ul, _p]),
    "qcx_sample_states_r": (_i, [_p, _p, _ul, _p]),
    "qcx_sample_last_stats": (_i, [_p, C.POINTER(_ul), C.POINTER(_ul)]),
    "qcx_marginal_probabilities": (_i, [_p, _u, _u, _p]),
    "qcx_marginal_last_stats": (_i, [_p, C.POINTER(_u), C.POINTER(_ul)]),
    "qcx_measure_qubits_r": (_i, [_p, _u, _u, _d, C.POINTER(_ul), C.POINTER(_d)]),
    "qcx_measure_qubits": (_i, [_p, _p, _u, _u, C.POINTER(_ul), C.POINTER(_d)]),
    "qcx_postselect_qubits": (_i, [_p, _u, _u, _ul, C.POINTER(_d)]),
    "qcx_collapse_last_stats": (_i, [_p, C.POINTER(_u), C.POINTER(_ul), C.POINTER(_ul)]),
    "qcx_pauli_expectation": (_i, [_p, _u64, _u64, C.POINTER(_d)]),
    "qcx_pauli_expectation_sum": (_i, [_p, _ul, _p, _p, _p, _p, C.POINTER(_d)]),
    "qcx_pauli_expectation_batch": (_i, [_p, _ul, _p, _p, _p, _p, C.POINTER(_d)]),
    "qcx_pauli_batch_width": (_u, []),
    "qcx_pauli_batch_plan": (_i, [_ul, _p, _u, _p, C.POINTER(_ul)]),
    "qcx_expectation_last_stats": (_i, [_p, C.POINTER(_u), C.POINTER(_ul)]),
    "qcx_reduced_density_matrix": (_i, [_p, _u, _u, _p]),
    "qcx_rdm_max_qubits": (_u, []),
    "qcx_rdm_last_stats": (_i, [_p, C.POINTER(_u), C.POINTER(_ul)]),
    "qcx_rdm_plan": (_i, [_u, _u, _u, _p, _p, C.POINTER(_u)]),
    "qcx_mc_gate_plan": (_i, [_u, _u64, _u64, _u, _u, _u, _p]),
    "qcx_marginal_plan": (_i, [_u, _u, _u, _p, C.POINTER(_u)]),
    "qcx_marginal_plan_compact": (_i, [_u, _u, _u, _u, _p, C.POINTER(_u)]),
    "qcx_state_read": (_i, [_p, _ul, _ul, _p]),
    "qcx_state_write": (_i, [_p, _ul, _ul, _p]),
    "qcx_norm2": (_i, [_p, C.POINTER(_d)]),
    "qcx_total_probability": (_i, [_p, C.POINTER(_d)]),
    "qcx_device_pointer": (_p, [_p]),
    "qcx_state_fill_random": (_i, [_p, _u64]),
    "qcx_shard_fill_random": (_i, [_p, _u, _u64, _u64, _d, _p]),
    "qcx_timer_start": (_i, [_p]),
    "qcx_timer_stop": (_i, [_p, C.POINTER(_d)]),
    "qcx_events_create": (_i, [_p, _u]),
    "qcx_event_record": (_i, [_p, _u]),
    "qcx_event_elapsed": (_i, [_p, _u, _u, C.POINTER(_d)]),
    "qcx_rng_alloc": (_p, []),
    "qcx_rng_set": (None, [_p, _ul]),
    "qcx_rng_get": (_ul, [_p]),
    "qcx_rng_uniform": (_d, [_p]),
    "qcx_rng_free": (None, [_p]),
    "qcx_shard_reset": (_i, [_p, _u, _i, _p]),
    "qcx_shard_hadamard": (_i, [_p, _u, _u, _p]),
    "qcx_shard_one_qubit": (_i, [_p, _u, _u, _i, _p, _p]),
    "qcx_shard_two_qubit": (_i, [_p, _u, _u, _u, _i, _p, _p]),
    "qcx_shard_pauli_rotation": (_i, [_p, _u, _u64, _u64, _d, _d, _p]),
    "qcx_shard_pauli_rotation_run": (_i, [_p, _u, _u64, _u, _p, _p, _p, _p, _p]),
    "qcx_shard_gate_run": (_i, [_p, _u, _u64, _u, _p, _p]),
    "qcx_shard_diagonal": (_i, [_p, _u, _u, _u, _p, _p]),
    "qcx_shard_phase": (_i, [_p, _u, _u64, _d, _d, _p]),
    "qcx_shard_camodc": (_i, [_p, _u, _u, _u, _u, _i, _p]),
    "qcx_shard_swap_bits": (_i, [_p, _p, _u, _u, C.POINTER(_u), C.POINTER(_u), _p]),
    "qcx_shard_norm2": (_i, [_p, _u, C.POINTER(_d), _p]),
    "qcx_shard_run_fused": (_i, [_p, _u, _u, _u, _p, _p]),
    "qcx_shard_run_fused_mode": (_i, [_i, _p, _u, _u, _u, _p, _p]),
    "qcx_shard_release_stream": (_i, [_p]),
    "qcx_shard_basis_front": (_i, [_p, _u, _u64, _u, _u, _u64, _u, _p, C.POINTER(_u), _p]),
    "qcx_compact_plan": (_i, [_u, _u, _u64, _u, _p, C.POINTER(_u), C.POINTER(_u), C.POINTER(_u), C.POINTER(C.c_uint16)]),
    "qcx_shard_compact_front": (_i, [_p, _u, _u64, _u, _u, _u64, _u, _p, _u, _u, C.POINTER(C.c_uint16), _p]),
    "qcx_shard_expand_compact": (_i, [_p, _p, _u, _u, _u, _u, C.POINTER(C.c_uint16), _p]),
    "qcx_state_save": (_i, [_p, C.c_char_p]),
    "qcx_state_load": (_i, [_p, C.c_char_p]),
    "qcx_fusion_plan": (_i, [_u, _u, _u, _p, _p, _u, C.POINTER(_u), _p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "qcx_fusion_plan_mode": (_i, [_i, _u, _u, _u, _p, _p, _u, C.POINTER(_u), _p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "qcx_pass_launch_plan": (_i, [_p, _p]),
    "qcx_shard_measure_scan": (_i, [_p, _u, _u64, _u64, _d, _d, C.POINTER(_i), C.POINTER(_u64), C.POINTER(_d), _p]),
    "qcx_shard_collapse": (_i, [_p, _u, _i64, _p]),
    "qcx_shard_canon_zeros": (_i, [_p, _u, _p]),
}
# not in the public header: diagnostics / tuning hooks
_EXTRA = {
    "qcx_tune_set": (_i, [C.c_char_p, C.c_long]),
    "qcx_tune_get": (C.c_long, [C.c_char_p]),
    "qcx_measure_last_stats": (_i, [C.POINTER(_u), C.POINTER(_u)]),
    "qcx_sharded_trace": (_i, [_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "qcx_sharded_restore_identity": (_i, [_p]),
    "qcx_sharded_relay_stats": (_i, [_p, C.POINTER(_u), C.POINTER(_ul)]),
    "qcx_sharded_overlap_stats": (_i, [_p, C.POINTER(_u), C.POINTER(_ul)]),
    "qcx_sharded_layout": (_i, [_p, C.POINTER(_u), _u]),
    "qcx_front_plan": (_i, [_u, _u, _u64, _u, _p, C.POINTER(_u), _p, C.c_size_t]),
    "qcx_chain_stats": (_i, [_p, C.POINTER(_ul)]),
    "qcx_diag_stats": (_i, [_p, C.POINTER(_ul)]),
    "qcx_gen_stats": (_i, [_p, C.POINTER(_ul)]),
    "qcx_gen_cols_stats": (_i, [_p, C.POINTER(_ul)]),
    "qcx_compact_stats": (_i, [_p, C.POINTER(_ul)]),
    "qcx_compact_measure_stats": (_i, [_p, C.POINTER(_ul)]),
    "qcx_expanding_store_stats": (_i, [_p, C.POINTER(_ul)]),
    "qcx_plan_cache_stats": (_i, [_p, C.POINTER(_ul)]),
    "qcx_collapse_pass": (_i, [_p, _u, _u, _ul, _d]),
    "qcx_expand_store_plan": (_i, [_u, _p, _p, _u, _u, _p, _p, _p, C.POINTER(_i)]),
}


class BasisFront(C.Structure):
    """struct BasisFront (csrc/qcx_kernels.h): the parameters of k_basis_front"""
    _fields_ = [("first", C.c_uint64), ("basis", C.c_uint64), ("hmask", C.c_uint64), ("fixed_mask", C.c_uint64), ("sign_mask", C.c_uint64),
                ("v", C.c_double), ("M", C.c_uint), ("ncam", C.c_uint), ("C", C.c_uint32 * 64), ("A", C.c_uint32 * 64),
                ("ctl", C.c_uint8 * 64)]


def front_plan(n_local, M, basis, descs):
    """host half of the basis-state front (no GPU): (gates consumed, BasisFront)"""
    arr = (GateDesc * max(len(descs), 1))()
    for i, d in enumerate(descs):
        arr[i].type, arr[i].q, arr[i].mask, arr[i].c, arr[i].s, arr[i].C, arr[i].A = d
    used, B = C.c_uint(0), BasisFront()
    check(lib().qcx_front_plan(n_local, M, basis, len(descs), C.cast(arr, C.c_void_p), C.byref(used), C.byref(B), C.sizeof(B)), "qcx_front_plan")
    return used.value, B

class GateDesc(C.Structure):
    """qcx_gate_desc (include/qcx.h)"""
    _fields_ = [("type", C.c_uint32), ("q", C.c_uint32), ("mask", C.c_uint64), ("c", C.c_double), ("s", C.c_double),
                ("C", C.c_uint32), ("A", C.c_uint32)]


class FuseRecord(C.Structure):
    """qcx_fuse_record (include/qcx.h): one 32-byte record of a fused pass"""
    _fields_ = [("type", C.c_uint32), ("a", C.c_uint32), ("mask", C.c_uint64), ("c", C.c_double), ("s", C.c_double)]


class PlanAction(C.Structure):
    """qcx_plan_action (include/qcx.h)"""
    _fields_ = [("fused", C.c_int), ("first_gate", C.c_uint), ("ngates", C.c_uint), ("T", C.c_uint), ("c", C.c_uint),
                ("nh", C.c_uint), ("hbit", C.c_ubyte * 16), ("nopipe", C.c_uint), ("rounds_form", C.c_uint),
                ("rec_off", C.c_size_t), ("rec_cnt", C.c_size_t), ("nops", C.c_uint), ("table_bytes", C.c_uint),
                ("table_rec_off", C.c_uint), ("diag_cnt", C.c_uint), ("diag_rec_off", C.c_uint),
                ("chained", C.c_uint), ("tl", C.c_ubyte * 16), ("in_pos", C.c_ubyte * 16), ("st_loc", C.c_ubyte * 16),
                ("st_pos", C.c_ubyte * 16), ("nseg_in", C.c_ubyte), ("nseg_out", C.c_ubyte), ("nseg_lg", C.c_ubyte), ("pad_", C.c_ubyte),
                ("seg_in", C.c_ubyte * 64), ("seg_out", C.c_ubyte * 64), ("seg_lg", C.c_ubyte * 64),      # segments: (src, dst, len, pad) x 16
                ("kernel", C.c_char * 64), ("grid", C.c_uint), ("block", C.c_uint), ("lds_bytes", C.c_uint)]     # the launch (qcx_pass_launch_plan)


class PassLaunchIn(C.Structure):
    """qcx_pass_launch_in (include/qcx_plan.h): what the launch of a fused pass depends on"""
    _fields_ = [(k, C.c_uint) for k in ("n", "M", "T", "rounds_form", "table_bytes", "has_cam", "xm_cnt", "dg_cnt", "dg_slim", "chained", "gen",
                                        "gen_tab_bytes", "zpad", "zskip", "xp_on", "tables_cover", "buffers_differ")]


class PassLaunchOut(C.Structure):
    """qcx_pass_launch_out (include/qcx_plan.h)"""
    _fields_ = [("kernel", C.c_char * 64)] + [(k, C.c_uint) for k in ("grid", "block", "lds_bytes", "waves", "xm_off", "dg_lds_off", "gen_lds_off",
                                                                      "table_lds_off", "dbg", "expanding_store_ok")]


def pass_launch_plan(**fields):
    """How one fused pass would be launched under the knobs of the moment (host code, no GPU needed): (status, PassLaunchOut,
    the refusal's text or "")."""
    I, O = PassLaunchIn(**fields), PassLaunchOut()
    st = lib().qcx_pass_launch_plan(C.byref(I), C.byref(O))
    return st, O, (lib().qcx_last_error().decode() if st else "")


MARGINAL_MAX_STAGES = 8     # QCX_MARGINAL_MAX_STAGES (include/qcx_plan.h)


class MarginalStage(C.Structure):
    """qcx_marginal_stage (include/qcx_plan.h): one stage of a marginal's plan"""
    _fields_ = [("kind", _u), ("in_bits", _u), ("T", _u), ("c", _u), ("tile_mask", _u64), ("sum_mask", _u64),
                ("qubits", _u64), ("out_bits", _u), ("final_stage", _u), ("out_offset", _u64)]


def marginal_plan(n, first, num, M=None):
    """The stage plan of qcx_marginal_probabilities (host code, no GPU needed): a list of MarginalStage.  M: the plan for a
    compact circuit result with that M register (first >= M)."""
    arr = (MarginalStage * MARGINAL_MAX_STAGES)()
    ns = C.c_uint(0)
    if M is None:
        st = lib().qcx_marginal_plan(n, first, num, C.cast(arr, C.c_void_p), C.byref(ns))
    else:
        st = lib().qcx_marginal_plan_compact(n, M, first, num, C.cast(arr, C.c_void_p), C.byref(ns))
    check(st, "qcx_marginal_plan")
    return [arr[i] for i in range(ns.value)]


class RdmStage0(C.Structure):
    """qcx_rdm_stage0 (include/qcx_plan.h): the first stage of a reduced density matrix's plan"""
    _fields_ = [("sum_mask", _u64), ("sum_bits", _u), ("group_bits", _u), ("rest_bits", _u), ("rows", _u), ("row_stride", _u64), ("scratch", _u64)]


def rdm_max_qubits():
    """the widest range Register.reduced_density_matrix serves (qcx_rdm_max_qubits)"""
    return int(lib().qcx_rdm_max_qubits())


def rdm_plan(n, first, num):
    """The stage plan of qcx_reduced_density_matrix (host code, no GPU needed): (RdmStage0, the list of MarginalStage behind it)."""
    s0 = RdmStage0()
    arr = (MarginalStage * MARGINAL_MAX_STAGES)()
    ns = C.c_uint(0)
    check(lib().qcx_rdm_plan(n, first, num, C.byref(s0), C.cast(arr, C.c_void_p), C.byref(ns)), "qcx_rdm_plan")
    return s0, [arr[i] for i in range(ns.value)]


MC_MAX_RUNS = 17            # QCX_MC_MAX_RUNS (include/qcx_plan.h)
MC_PAIR, MC_LINE_PAIR, MC_LINE_SHFL, MC_QUAD, MC_LINES2 = range(5)


class McPlan(C.Structure):
    """qcx_mc_plan (include/qcx_plan.h): the launch of a gate under a control mask"""
    _fields_ = [("form", _u), ("ns", _u), ("count", _u64), ("nruns", _u), ("run_pos", C.c_ubyte * MC_MAX_RUNS),
                ("run_len", C.c_ubyte * MC_MAX_RUNS), ("or_const", _u64), ("low_mask", _u), ("low_values", _u), ("store_all", _u),
                ("shfl_lo", _u), ("shfl_hi", _u), ("nt", _u), ("grid", _u), ("block", _u), ("items_per_thread", _u),
                ("glog", _u), ("slog", _u), ("kernel", C.c_char * 48)]


def mc_gate_plan(n, ctrl_mask, ctrl_values, targets):
    """What mc_one_qubit_gate / mc_two_qubit_gate would launch on n qubits under the knobs of the moment (host code, no GPU
    needed; include/qcx_plan.h: qcx_mc_gate_plan): (status, McPlan).  targets: a 1- or 2-tuple (qubit0[, qubit1])."""
    t = tuple(int(q) for q in targets)
    pl = McPlan()
    st = lib().qcx_mc_gate_plan(int(n), int(ctrl_mask), int(ctrl_values), len(t), t[0], t[1] if len(t) > 1 else 0, C.byref(pl))
    return st, pl


DIAG_TILE, DIAG_GROUP, DIAG_LANE = range(3)        # QCX_DIAG_* (include/qcx_plan.h)


class DiagPlan(C.Structure):
    """qcx_diag_plan (include/qcx_plan.h): the launch of a diagonal on a qubit range"""
    _fields_ = [("form", _u), ("full", _u), ("lds", _u), ("T", _u), ("first", _u), ("num", _u), ("kmask", _u64), ("units", _u64),
                ("elems", _u), ("slice_entries", _u64), ("grid", _u), ("block", _u), ("lds_bytes", _u), ("kernel", C.c_char * 48)]


def diagonal_plan(n, first, num):
    """What diagonal_gate(first, num, ...) would launch on n qubits under the knobs of the moment (host code, no GPU needed;
    include/qcx_plan.h: qcx_diagonal_plan): (status, DiagPlan)."""
    pl = DiagPlan()
    st = lib().qcx_diagonal_plan(int(n), int(first), int(num), C.byref(pl))
    return st, pl


def diagonal_host_max_qubits():
    """the widest range diagonal_gate takes a host table for (qcx_diagonal_host_max_qubits); wider tables go in device memory"""
    return int(lib().qcx_diagonal_host_max_qubits())


PERM_LINES, PERM_SHARED = range(2)                 # QCX_PERM_* (include/qcx_plan.h)


class TileGeom(C.Structure):
    """qcx_tile_geom (include/qcx_plan.h): the tile geometry PermPlan and MultiPlan embed; its fields read as theirs"""
    _fields_ = [("form", _u), ("T", _u), ("tile_bits", C.c_ubyte * 12), ("tile_mask", _u64), ("unit_mask", _u64),
                ("squeezed", _u64), ("or_const", _u64), ("nruns", _u), ("run_pos", C.c_ubyte * 20), ("run_len", C.c_ubyte * 20),
                ("elem_mask", _u), ("elem_values", _u), ("unit_mask_low", _u), ("unit_values_low", _u), ("units", _u64)]


class PermPlan(C.Structure):
    """qcx_perm_plan (include/qcx_plan.h): the launch of a permutation of a qubit range's basis states"""
    _anonymous_ = ("geom",)
    _fields_ = [("geom", TileGeom), ("first", _u), ("num", _u), ("range_pos", _u), ("grid", _u), ("block", _u), ("lds_bytes", _u),
                ("store_all", _u), ("nt", _u), ("kernel", C.c_char * 48)]


def permutation_plan(n, ctrl_mask, ctrl_values, first, num):
    """What permutation_gate(first, num, ...) under these controls would launch on n qubits that hold finite amplitudes, under
    the knobs of the moment (host code, no GPU needed; include/qcx_plan.h: qcx_permutation_plan): (status, PermPlan)."""
    pl = PermPlan()
    st = lib().qcx_permutation_plan(int(n), int(ctrl_mask), int(ctrl_values), int(first), int(num), C.byref(pl))
    return st, pl


def permutation_max_qubits():
    """the widest range permutation_gate takes a table for (qcx_permutation_max_qubits)"""
    return int(lib().qcx_permutation_max_qubits())


class MultiPlan(C.Structure):
    """qcx_multi_plan (include/qcx_plan.h): the launch of a dense matrix on 1 .. 5 target qubits"""
    _anonymous_ = ("geom",)
    _fields_ = [("geom", TileGeom), ("num_targets", _u), ("targets", C.c_ubyte * 5), ("target_pos", C.c_ubyte * 5),
                ("grid", _u), ("block", _u), ("lds_bytes", _u), ("rows_per_item", _u), ("store_all", _u), ("nt", _u),
                ("kernel", C.c_char * 48)]


def multi_gate_plan(n, ctrl_mask, ctrl_values, targets):
    """What multi_qubit_gate(targets, ...) under these controls would launch on n qubits that hold finite amplitudes, under the
    knobs of the moment (host code, no GPU needed; include/qcx_plan.h: qcx_multi_gate_plan): (status, MultiPlan).  targets =
    None passes a NULL pointer (the plan refuses it)."""
    pl = MultiPlan()
    if targets is None:
        return lib().qcx_multi_gate_plan(int(n), int(ctrl_mask), int(ctrl_values), 0, None, C.byref(pl)), pl
    t = [int(q) for q in targets]
    arr = (C.c_uint * max(len(t), 1))(*t)
    st = lib().qcx_multi_gate_plan(int(n), int(ctrl_mask), int(ctrl_values), len(t), C.cast(arr, C.c_void_p), C.byref(pl))
    return st, pl


def multi_qubit_max_targets():
    """the most targets multi_qubit_gate takes a matrix for (qcx_multi_qubit_max_targets)"""
    return int(lib().qcx_multi_qubit_max_targets())


def pauli_batch_width():
    """W: the most terms one read of the state serves in Register.expectation_batch (qcx_pauli_batch_width)"""
    return int(lib().qcx_pauli_batch_width())


def pauli_batch_plan(x_masks, width=None):
    """The passes of Register.expectation_batch (host code, no GPU needed; include/qcx_plan.h: qcx_pauli_batch_plan):
    (pass_of_term, npasses) for the terms' x_masks in order; width=None: the library's W."""
    import numpy as np
    xs = np.array([int(x) for x in x_masks], dtype=np.uint64)
    out = np.zeros(xs.size, dtype=np.uint64)
    np_ = C.c_ulong(0)
    ptr = (lambda a: a.ctypes.data_as(C.c_void_p)) if xs.size else (lambda a: None)
    check(lib().qcx_pauli_batch_plan(xs.size, ptr(xs), pauli_batch_width() if width is None else int(width), ptr(out), C.byref(np_)),
          "qcx_pauli_batch_plan")
    return [int(v) for v in out], int(np_.value)


def pauli_rotation_batch_width():
    """W: the most terms one pass of pauli_rotation_batch applies (qcx_pauli_rotation_batch_width)"""
    return int(lib().qcx_pauli_rotation_batch_width())


def pauli_rotation_batch_plan(terms, n, width=None):
    """The passes of pauli_rotation_batch over n qubits (host code, no GPU needed; include/qcx_plan.h:
    qcx_pauli_rotation_batch_plan): (pass_of_term, passes) for terms = [(pauli, theta), ...] in order, passes = [(kind, hot_mask),
    ...] -- kind 0: a run of terms over the tile of qubits 0-7 and hot_mask, kind 1: one wide term on its own; width=None: the
    library's W."""
    import numpy as np
    n = int(n)
    xs = np.array([pauli_masks(p, n)[0] for p, _ in terms], dtype=np.uint64)
    pass_of, kind, hot = np.zeros(xs.size, dtype=np.uint64), np.zeros(xs.size, dtype=np.uint32), np.zeros(xs.size, dtype=np.uint64)
    np_ = C.c_ulong(0)
    ptr = (lambda a: a.ctypes.data_as(C.c_void_p)) if xs.size else (lambda a: None)
    check(lib().qcx_pauli_rotation_batch_plan(n, xs.size, ptr(xs), pauli_rotation_batch_width() if width is None else int(width),
                                              ptr(pass_of), C.byref(np_), ptr(kind), ptr(hot)), "qcx_pauli_rotation_batch_plan")
    return [int(v) for v in pass_of], [(int(kind[p]), int(hot[p])) for p in range(np_.value)]


class Gate(C.Structure):
    """qcx_gate (include/qcx.h): one record of qcx_gate_batch"""
    _fields_ = [("ntargets", _u), ("control", _i), ("qubit0", _u), ("qubit1", _u), ("u", _d * 32)]


def gate_targets(entry):
    """(targets, control) of one gate_batch entry (U, targets) or (U, targets, control): targets as a 1- or 2-tuple of ints,
    control an int or None"""
    if len(entry) not in (2, 3):
        raise ValueError(f"a gate is (U, targets) or (U, targets, control), not {len(entry)} items")
    t = entry[1]
    t = (int(t),) if not hasattr(t, "__len__") else tuple(int(q) for q in t)
    if len(t) not in (1, 2):
        raise ValueError(f"a gate has one or two targets, not {len(t)}")
    c = entry[2] if len(entry) == 3 else None
    return t, (None if c is None else int(c))


def gate_batch_width():
    """W: the units one pass of gate_batch holds -- 1 per one-target gate, 4 per two-target gate (qcx_gate_batch_width)"""
    return int(lib().qcx_gate_batch_width())


def gate_batch_plan(gates, n, width=None):
    """The passes of gate_batch over n qubits (host code, no GPU needed; include/qcx_plan.h: qcx_gate_batch_plan):
    (pass_of_gate, hot_masks) for gates = [(U, targets) or (U, targets, control), ...] in order (U is not looked at) -- pass p is a
    run of gates over the tile of qubits 0-7 and hot_masks[p]; width=None: the library's W."""
    import numpy as np
    n = int(n)
    ts = [gate_targets(g)[0] for g in gates]
    for t in ts:
        if min(t) < 0 or max(t) >= 64:
            raise ValueError(f"targets {t} are not qubits")
    masks = np.array([sum(1 << q for q in set(t)) for t in ts], dtype=np.uint64)
    units = np.array([1 if len(t) == 1 else 4 for t in ts], dtype=np.uint32)
    pass_of, hot = np.zeros(masks.size, dtype=np.uint64), np.zeros(masks.size, dtype=np.uint64)
    np_ = C.c_ulong(0)
    ptr = (lambda a: a.ctypes.data_as(C.c_void_p)) if masks.size else (lambda a: None)
    check(lib().qcx_gate_batch_plan(n, masks.size, ptr(masks), ptr(units), gate_batch_width() if width is None else int(width),
                                    ptr(pass_of), C.byref(np_), ptr(hot)), "qcx_gate_batch_plan")
    return [int(v) for v in pass_of], [int(hot[p]) for p in range(np_.value)]


def fusion_plan(n_local, M, descs, mode=1):
    """The pass planner alone (host code, no GPU needed).  descs: (type, q, mask, c, s, C, A) tuples as for
    qcx_shard_run_fused.  Returns (actions, records): a list of PlanAction and a ctypes array of FuseRecord.
    mode 1: the bit-exact plan; 2: the tolerance mode's plan (merged diagonals); | 4: with chained passes (PlanAction.chained)."""
    arr = (GateDesc * max(len(descs), 1))()
    for i, d in enumerate(descs):
        arr[i].type, arr[i].q, arr[i].mask, arr[i].c, arr[i].s, arr[i].C, arr[i].A = d
    na, nr = C.c_uint(0), C.c_size_t(0)
    cap_a, cap_r = len(descs) + 4, 4 * len(descs) + 64
    while True:
        acts = (PlanAction * cap_a)()
        recs = (FuseRecord * cap_r)()
        st = lib().qcx_fusion_plan_mode(mode, n_local, M, len(descs), C.cast(arr, C.c_void_p), C.cast(acts, C.c_void_p), cap_a, C.byref(na),
                                   C.cast(recs, C.c_void_p), cap_r, C.byref(nr))
        if st == 1 and (na.value > cap_a or nr.value > cap_r):        # QCX_INSUFFICIENT_MEMORY: grow and retry
            cap_a, cap_r = max(cap_a, na.value), max(cap_r, nr.value)
            continue
        check(st, "qcx_fusion_plan_mode")
        return [acts[k] for k in range(na.value)], recs, nr.value


_lib = None


def _share_hip_runtime_with_torch():
    """One HIP runtime per process.  The torch wheel bundles its own libamdhip64.so (same SONAME as
    /opt/rocm's, different file); if libqcx.so pulled in the system copy first and torch its bundled
    copy later, the process would hold two HSA runtimes and the second to initialise sees no device.
    Loading torch's copy first (without importing torch) makes both resolve to that one file."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return                      # torch already loaded its runtime; libqcx.so resolves to it by SONAME
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec and spec.submodule_search_locations:
        cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
        if os.path.exists(cand):
            try:
                C.CDLL(cand, mode=C.RTLD_GLOBAL)
            except OSError:
                pass


def lib():
    """Load libqcx.so once; raise loudly if the HIP extension has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} not found: build it with `make -C quantumcomputer_amd/csrc` "
                "(or __graft_entry__.build()); quantumcomputer_amd has no CPU fallback")
        _share_hip_runtime_with_torch()
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in {**SIGNATURES, **_EXTRA}.items():
            fn = getattr(L, name)          # AttributeError here = header/library mismatch
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(status, where=""):
    if status != NO_ERROR:
        raise QcxError(status, where)


def spread_devices(shards, visible=None):
    """HIP device of each shard, as qcx_register_create_sharded(devices=NULL) places them: over the largest
    power-of-two number of devices <= min(shards, visible), neighbouring shards together; one visible GPU gives
    [0] * shards (the virtual shards of the one-GPU tests).  visible=None asks HIP (needs a GPU); an explicit count is
    pure arithmetic."""
    out = (C.c_int * int(shards))()
    check(lib().qcx_spread_devices(int(shards), 0 if visible is None else int(visible), out), "qcx_spread_devices")
    return list(out)


def idle_devices(shard_devices, count, visible=None):
    """`count` relay GPUs for multi-path striping: devices that hold no shard first, then (when there are not enough
    idle ones, e.g. on a one-GPU box) the shard devices again"""
    if visible is None:
        n = C.c_int(0)
        check(lib().qcx_device_count(C.byref(n)), "qcx_device_count")
        visible = n.value
    idle = [d for d in range(visible) if d not in set(shard_devices)]
    pool = idle + sorted(set(shard_devices))
    return [pool[i % len(pool)] for i in range(count)]


def pauli_masks(spec, n):
    """(x_mask, z_mask) of a Pauli string over n qubits (include/qcx.h: qcx_pauli_expectation): x_mask = the qubits that carry X
    or Y, z_mask = those that carry Z or Y.  spec: a str such as "XIZY" (character k = qubit k; at most n characters, the rest
    I), a dict {qubit: 'X' | 'Y' | 'Z' | 'I'}, or an (x_mask, z_mask) pair, which is only checked.  Host arithmetic only."""
    n = int(n)
    if isinstance(spec, str):
        if len(spec) > n:
            raise ValueError(f"a Pauli string of {len(spec)} characters on {n} qubits")
        items = list(enumerate(spec))
    elif isinstance(spec, dict):
        items = list(spec.items())
    else:
        x, z = (int(v) for v in spec)
        if x < 0 or z < 0 or (x | z) >> n:
            raise ValueError(f"masks ({x:#x}, {z:#x}) do not fit {n} qubits")
        return x, z
    x = z = 0
    for q, p in items:
        if isinstance(q, bool) or int(q) != q or not 0 <= int(q) < n:
            raise ValueError(f"qubit {q!r} is not one of the {n} qubits")
        p = p.upper() if isinstance(p, str) else p
        if p not in ("I", "X", "Y", "Z"):
            raise ValueError(f"{p!r} is not one of I, X, Y, Z")
        if p in ("X", "Y"):
            x |= 1 << int(q)
        if p in ("Z", "Y"):
            z |= 1 << int(q)
    return x, z


def polar(theta):
    """(cos, sin) of theta exactly as the gate path computes them (glibc sincos, include/qcx.h: qcx_polar)"""
    c, s = C.c_double(0.0), C.c_double(0.0)
    lib().qcx_polar(float(theta), C.byref(c), C.byref(s))
    return c.value, s.value


def tune(**kv):
    for k, v in kv.items():
        check(lib().qcx_tune_set(k.encode(), int(v)), f"tune {k}")
