"""quantumcomputer_amd -- MI355X-native gate engine for the qc_shor.c hot path.

Only what the path needs: csrc/ (HIP kernels + the C ABI, built into libqcx.so),
the ctypes loader and the host-side mirror of the reference's gate interface.
"""
from ._lib import DIAG_GROUP, DIAG_LANE, DIAG_TILE, LIB_PATH, PERM_LINES, PERM_SHARED, QcxError, diagonal_host_max_qubits, diagonal_plan, front_plan, fusion_plan, gate_batch_plan, gate_batch_width, idle_devices, lib, marginal_plan, mc_gate_plan, multi_gate_plan, multi_qubit_max_targets, pauli_batch_plan, pauli_batch_width, pauli_masks, pauli_rotation_batch_plan, pauli_rotation_batch_width, permutation_max_qubits, permutation_plan, polar, rdm_max_qubits, rdm_plan, spread_devices, tune  # noqa: F401
from .register import (Register, Rng, load_state_file, c_amodc_gate, c_one_qubit_gate, c_phase_shift_gate,  # noqa: F401
                       c_two_qubit_gate, check_normalisation, controlled, diagonal_gate, diagonal_phase, display_state, fused_matrix, gate_batch, hadamard_gate,
                       inverse_QFT, mc_one_qubit_gate, mc_two_qubit_gate, measure_qubits, measure_state, modadd_table, modmul_table, multi_qubit_gate, omega_distribution, one_qubit_gate, pauli_rotation, pauli_rotation_batch, permutation_gate, phase, phase_table, postselect_qubits, purity, qubit_permutation_table,
                       quantum_computation, read_omega, reset_register, rz, sample_states, swap_states, two_qubit_gate, von_neumann_entropy, xor_oracle_table)

FUSION_TOLERANCE = 2      # qcx_set_fusion(reg, 2): the opt-in tolerance mode (include/qcx.h)


def __getattr__(name):
    if name == "GATES":       # register.GATES: X, Y, Z, S, T, H (built on first use: T's factor comes from the library)
        from . import register
        return register.GATES
    if name == "GATES2":      # register.GATES2: SWAP, ISWAP, CNOT, CZ
        from . import register
        return register.GATES2
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


__all__ = ["FUSION_TOLERANCE", "Register", "Rng", "reset_register", "hadamard_gate", "c_phase_shift_gate", "c_amodc_gate",
           "one_qubit_gate", "c_one_qubit_gate", "GATES", "rz", "phase",
           "two_qubit_gate", "c_two_qubit_gate", "mc_one_qubit_gate", "mc_two_qubit_gate", "mc_gate_plan", "GATES2", "controlled", "gate_batch", "gate_batch_plan", "gate_batch_width", "pauli_rotation", "pauli_rotation_batch", "pauli_rotation_batch_plan", "pauli_rotation_batch_width",
           "diagonal_gate", "diagonal_phase", "phase_table", "diagonal_plan", "diagonal_host_max_qubits", "DIAG_TILE", "DIAG_GROUP", "DIAG_LANE",
           "permutation_gate", "permutation_plan", "permutation_max_qubits", "PERM_LINES", "PERM_SHARED", "modmul_table", "modadd_table", "xor_oracle_table", "qubit_permutation_table",
           "multi_qubit_gate", "multi_gate_plan", "multi_qubit_max_targets", "fused_matrix",
           "swap_states", "inverse_QFT", "quantum_computation", "measure_state", "measure_qubits", "postselect_qubits", "sample_states", "omega_distribution", "read_omega",
           "display_state", "check_normalisation", "lib", "tune", "polar", "pauli_masks", "pauli_batch_width", "pauli_batch_plan", "rdm_max_qubits", "purity", "von_neumann_entropy", "QcxError", "LIB_PATH", "spread_devices", "idle_devices"]
