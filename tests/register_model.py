"""The host model of an unsharded register, and the generator of random call sequences over the whole register API
(tests/test_register_model.py pins both on the CPU, tests/test_gpu_api_sequences.py runs them against the GPU).

The model holds the state as interleaved float64 and has one method per public call; every method does what the project already
defines for that call -- the oracle (oracle/binding.py) for reset, fill, the reference's gates, the circuits and measure_state,
tests/one_qubit_ref.py / two_qubit_ref.py for the matrix gates, tests/marginal_ref.py / collapse_ref.py for the marginal and the
range collapse, tests/pauli_ref.py / pauli_rotation_ref.py for the Pauli calls -- so a sequence of calls on the model is the
bit-for-bit expectation for the same calls on the GPU, whatever lazy form (queue, pending basis state, compact result, owed zero
pass, strict mode, a handed-out buffer pointer, a caller's stream) the library keeps the state in between them.

The generator has three vocabularies.  Seeds below NSEEDS_V1 draw from the calls up to the matrix gates; their op lists are frozen
(tests/golden/sequence_digests.json: whatever is added here must leave them as they are).  The seeds NSEEDS_V1 .. NSEEDS - 1 add
expect / expect_sum / prot (the Pauli calls), devptr (a read through qcx_device_pointer, after which the register works in
place for the rest of its life) and stream (qcx_register_set_stream: a caller's non-blocking stream, or the own one again).

A third vocabulary (seeds NSEEDS .. NSEEDS_V3 - 1) adds the two newest observers: expect_batch (qcx_pauli_expectation_batch, the
terms that share an x_mask in one read of the state) and rdm (qcx_reduced_density_matrix).  Its seeds also draw the launch knobs
of the fused engine (KNOBS_FUSED), so that every call of the vocabulary meets a state that just left a chained pass, a generated
front or a compact chain under other than the default knobs.

A further family, generate_sharded (seeds 0 .. NSEEDS_SH - 1 of its own, at the end of this file), draws sequences for a SHARDED
register (qcx_register_create_sharded): the same model -- a sharded register promises the same bits for the calls it supports --
with the calls it refuses (QCX_UNSUPPORTED, nothing touched) as refused ops, and relays / selfcheck / stats ops the model does
nothing for.  tests/test_sharded_sequences_dry.py replays them on a dry-run register, tests/test_gpu_sharded_sequences.py on the GPU.

One op no generator above draws: prot_batch (qcx_pauli_rotation_batch, terms from rotation_terms), which the model applies as the
loop of the single rotation; tests/tolerance_twin.py deals it out behind the tolerance mode.

An op is a tuple of a name and plain numbers / strings, so that a failing sequence prints as a Python literal and replays:
written data and matrices are regenerated from the seed inside the op (window_data, matrix_data).  Host only."""
import numpy as np

import one_qubit_ref
import pauli_ref
import pauli_rotation_ref
import two_qubit_ref
from collapse_ref import collapse_ref, measure_ref
from marginal_ref import marginal_ref
from rdm_ref import rdm_ref

NO_ERROR, BAD_ARGUMENTS, BAD_QUBIT, UNSUPPORTED = 0, 2, 6, 7
THREADS = 8


# ---- data an op names by seed -----------------------------------------------------------------------------------------------

def window_data(dim, count, seed, flavour):
    """`count` amplitudes a write op stores: components U(-0.5, 0.5) at the scale of a normalised state of `dim` amplitudes;
    "negzero": a quarter of the components are zeros of either sign; "inf" / "nan": one component is not finite; "subnormal": four
    times the scale (a whole state of norm^2 about 16) with a quarter of the components the smallest subnormal of either sign -- a
    collapse onto an outcome of probability > 4 scales by s < 1/2, and the negative ones underflow to -0"""
    rs = np.random.RandomState(seed)
    a = rs.uniform(-0.5, 0.5, 2 * count) * np.sqrt(6.0 / dim)
    if flavour == "subnormal":
        a *= 4.0
        k = max(2, (2 * count) // 4)
        a[rs.randint(0, 2 * count, k)] = -5e-324
        a[rs.randint(0, 2 * count, k // 3)] = 5e-324
        return a
    if flavour == "negzero":
        k = max(2, (2 * count) // 4)
        a[rs.randint(0, 2 * count, k)] = -0.0
        a[rs.randint(0, 2 * count, k // 2)] = 0.0
        a[int(rs.randint(0, 2 * count))] = -0.0
    elif flavour in ("inf", "nan"):
        a[int(rs.randint(0, 2 * count))] = {"inf": [np.inf, -np.inf][int(rs.randint(0, 2))], "nan": np.nan}[flavour]
    else:
        assert flavour == "plain", flavour
    return a


_S = 0.70710678118654752440
_NAMED2 = [np.array(m, dtype=complex) for m in (
    [[_S, _S], [_S, -_S]], [[0, 1], [1, 0]], [[0, -1j], [1j, 0]], [[1, 0], [0, -1]], [[1, 0], [0, 1j]])]
_NAMED4 = [np.array(m, dtype=complex) for m in (
    [[1, 0, 0, 0], [0, 0, 1, 0], [0, 1, 0, 0], [0, 0, 0, 1]], [[1, 0, 0, 0], [0, 0, 1j, 0], [0, 1j, 0, 0], [0, 0, 0, 1]],
    [[1, 0, 0, 0], [0, 0, 0, 1], [0, 0, 1, 0], [0, 1, 0, 0]], [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, -1]])]


def matrix_data(k, seed, ulp=False):
    """the k x k complex matrix a gate op applies (k = 2, 4): one of the exact named gates or a random unitary, every component
    within [-1, 1]; ulp: one component is 1 + 1 ulp, which the library must refuse"""
    rs = np.random.RandomState(seed)
    if rs.randint(0, 3) == 0:
        named = _NAMED2 if k == 2 else _NAMED4
        m = named[int(rs.randint(0, len(named)))].copy()
    else:
        m, _ = np.linalg.qr(rs.standard_normal((k, k)) + 1j * rs.standard_normal((k, k)))
    d = np.ascontiguousarray(m.reshape(-1)).view(np.float64).copy()
    d /= max(1.0, float(np.max(np.abs(d))))
    if ulp:
        d[int(rs.randint(0, d.size))] = np.nextafter(1.0, 2.0) * [1.0, -1.0][int(rs.randint(0, 2))]
    return d.view(np.complex128).reshape(k, k)


def sample_draws(seed, shots):
    """the draws of a sample op: uniform, with the reference's edge values mixed in"""
    rs = np.random.RandomState(seed)
    r = rs.uniform(0.0, 1.0, shots)
    if shots > 2 and rs.randint(0, 2):
        r[int(rs.randint(0, shots))] = float(rs.choice([0.0, 1.0, 1.5, -0.25, 1e-300]))
    return r


def draw_masks(rs, n):
    """(x_mask, z_mask) of a Pauli string over n qubits, drawn over the three unit shapes of k_pauli_leaves / k_pauli_rot with
    equal weight: x_mask = 0 (a diagonal string), x_mask != 0 inside the low min(n, 12) bits (the partner amplitude sits in the
    same tile and goes through LDS), x_mask with a bit >= 12 (pairs of tiles; n >= 13 -- a smaller register draws the second
    shape in its place).  z_mask is random; one draw in four has z_mask = x_mask: every letter a Y"""
    c = int(rs.randint(0, 3))
    if c == 2 and n < 13:
        c = 1
    if c == 0:
        x = 0
    elif c == 1:
        x = int(rs.randint(1, 1 << min(n, 12)))
    else:
        x = int(rs.randint(0, 1 << n)) | (1 << int(rs.randint(12, n)))
    z = x if rs.randint(0, 4) == 0 else int(rs.randint(0, 1 << n))
    return x, z


def mask_shape(x_mask):
    """0, 1, 2: which of draw_masks' three unit shapes x_mask has"""
    return 0 if x_mask == 0 else 1 if x_mask < (1 << 12) else 2


def sum_terms(n, seed, k):
    """the k terms (coeff, x_mask, z_mask) of an expect_sum op: coefficients U(-2, 2), one of them exactly 0.0 when k >= 3"""
    rs = np.random.RandomState(seed)
    terms = []
    for _ in range(k):
        c = float(rs.uniform(-2.0, 2.0))
        terms.append((c,) + draw_masks(rs, n))
    if k >= 3:
        j = int(rs.randint(0, k))
        terms[j] = (0.0,) + terms[j][1:]
    return terms


BATCH_WIDTH = 32                          # qcx_pauli_batch_width(): the most terms one read of the state serves
RDM_MAX = 4                               # qcx_rdm_max_qubits() (tests/test_gpu_api_sequences.py checks both against the library)


def batch_terms(n, seed, k):
    """the k terms (coeff, x_mask, z_mask) of an expect_batch op.  One seed in two draws them as sum_terms does (every term its
    own x_mask, some of them equal by chance); the others share ONE x_mask -- of any of draw_masks' three shapes -- with
    z_masks of their own, two of them equal when k >= 2: k = 40 of those are more than BATCH_WIDTH and take a second read"""
    rs = np.random.RandomState(seed)
    if rs.randint(0, 2):
        return sum_terms(n, int(rs.randint(1, 1 << 30)), k)
    x, _ = draw_masks(rs, n)
    terms = [(float(rs.uniform(-2.0, 2.0)), x, x if rs.randint(0, 4) == 0 else int(rs.randint(0, 1 << n))) for _ in range(k)]
    if k >= 2:
        terms[-1] = (terms[-1][0],) + terms[0][1:]
    if k >= 3:
        j = int(rs.randint(0, k))
        terms[j] = (0.0,) + terms[j][1:]
    return terms


ROTATION_THETAS = [0.0, float(np.pi), -0.7, 7.5, 0.3]     # tests/test_gpu_pauli_rotation_batch.THETAS (tests/test_tolerance_twin.py holds them equal)


def rotation_terms(n, seed, k):
    """the k terms ((x_mask, z_mask), theta) of a prot_batch op, in the order the call applies them: masks as draw_masks gives
    them (all three unit shapes, so that a list of 40 closes passes by the width, by a fifth hot bit and by a wide term), thetas
    the ones the direct test of qcx_pauli_rotation_batch cycles through, from a start the seed picks"""
    rs = np.random.RandomState(seed)
    shift = int(rs.randint(0, len(ROTATION_THETAS)))
    return [(draw_masks(rs, n), ROTATION_THETAS[(j + shift) % len(ROTATION_THETAS)]) for j in range(k)]


def rdm_shape(n, first, num):
    """0, 1, 2: which kernel form a reduced density matrix takes: k_rdm_small (n < 12), k_rdm_leaves with the range beginning
    below the 12 - num summed bits of a unit, k_rdm_leaves with the range at or above them"""
    return 0 if n < 12 else 1 if first < 12 - num else 2


# ---- the model --------------------------------------------------------------------------------------------------------------

class RegisterModel:
    def __init__(self, ob, L, M):
        self.ob, self.L, self.M, self.n = ob, L, M, L + M
        self.dim = 1 << self.n
        self.a = np.zeros(2 * self.dim)
        self.saved = {}

    def holds_nonfinite(self):
        return not bool(np.all(np.isfinite(self.a)))

    # state access
    def reset_register(self):
        self.a = np.zeros(2 * self.dim)
        self.ob.reset(self.a, self.n)

    def fill_random(self, seed):
        self.a = self.ob.fill_random(self.n, seed)

    def write(self, amps, first=0):
        amps = np.ascontiguousarray(amps, dtype=np.float64)
        self.a[2 * first:2 * first + amps.size] = amps                   # (a -0 stays until a gate canonicalises it)

    def read(self, first=0, count=None):
        count = self.dim - first if count is None else count
        return self.a[2 * first:2 * (first + count)].copy()

    def save(self, key):
        self.saved[key] = self.a.copy()

    def load(self, key):
        self.a = self.saved[key].copy()

    def flush(self): pass
    def synchronize(self): pass
    def set_fusion(self, mode): pass

    # the reference's gates and circuits
    def hadamard_gate(self, q): self.ob.hadamard(self.a, self.n, q, THREADS)
    def c_phase_shift_gate(self, c, t, theta): self.ob.cphase(self.a, self.n, c, t, theta, THREADS)
    def c_amodc_gate(self, Cn, atox, ctl): self.ob.camodc(self.a, self.n, self.M, Cn, atox, ctl, THREADS)
    def inverse_QFT(self): self.ob.iqft(self.a, self.n, self.M, THREADS)
    def quantum_computation(self, Cn, a): self.ob.quantum_computation(self.a, self.n, self.M, Cn, a, threads=THREADS)

    # the matrix gates
    def one_qubit_gate(self, q, U): self.a = one_qubit_ref.apply(self.a, self.n, q, U)
    def c_one_qubit_gate(self, c, q, U): self.a = one_qubit_ref.apply(self.a, self.n, q, U, control=c)
    def two_qubit_gate(self, q0, q1, U): self.a = two_qubit_ref.apply(self.a, self.n, q0, q1, U)
    def c_two_qubit_gate(self, c, q0, q1, U): self.a = two_qubit_ref.apply(self.a, self.n, q0, q1, U, control=c)

    # observers and collapses
    def measure_state(self, r):
        return self.ob.measure(self.a, self.n, float(r))                  # (collapses self.a)

    def sample_states(self, rs):
        return np.array([self.ob.measure(self.a.copy(), self.n, float(r)) for r in rs], dtype=np.uint64)

    def marginal(self, first, num):
        return marginal_ref(self.a, self.n, first, num)

    def measure_qubits(self, first, num, r):
        """(outcome, probability, status); BAD_ARGUMENTS leaves the state as it was"""
        v, p, out = measure_ref(self.a, self.n, first, num, r)
        if out is None:
            return v, p, BAD_ARGUMENTS
        self.a = out
        return v, p, NO_ERROR

    def postselect(self, first, num, outcome):
        p, out = collapse_ref(self.a, self.n, first, num, outcome)
        if out is None:
            return p, BAD_ARGUMENTS
        self.a = out
        return p, NO_ERROR

    def expectation(self, x_mask, z_mask):
        return pauli_ref.pauli_ref(self.a, self.n, x_mask, z_mask)

    def expectation_sum(self, terms):
        """terms: (coeff, x_mask, z_mask); (total, values)"""
        total, values = pauli_ref.pauli_sum_ref(self.a, self.n, terms)
        return total, np.array(values, dtype=np.float64)

    def expectation_batch(self, terms):
        """the same definition as expectation_sum: how the terms share reads of the state changes no bit"""
        return self.expectation_sum(terms)

    def reduced_density_matrix(self, first, num):
        """float64[2^num, 2^num, 2]: (re, im)"""
        return rdm_ref(self.a, self.n, first, num)

    def pauli_rotation(self, x_mask, z_mask, theta):
        self.a = pauli_rotation_ref.apply(self.a, self.n, x_mask, z_mask, theta)

    def total_probability(self):
        with np.errstate(over="ignore", invalid="ignore"):
            return self.ob.norm2(self.a, self.n)                          # the sequential sum (testing_and_debug.c:28-37)

    def norm2(self):
        """not bit-defined (the GPU sums a tree): compare within 1e-9, and not at all on a non-finite state"""
        return self.ob.norm2(self.a, self.n)


# ---- ops ---------------------------------------------------------------------------------------------------------------------

FOLLOWING = ("reset", "fill", "write", "read", "h", "cphase", "camodc", "iqft", "qcomp", "u1", "cu1", "u2", "cu2", "measure",
             "sample", "marginal", "measure_qubits", "postselect", "total", "norm2", "save", "load", "flush", "sync", "fusion")
# the second vocabulary (seeds NSEEDS_V1 .. NSEEDS - 1): the Pauli calls, the handed-out buffer pointer, the caller's stream
FOLLOWING_V2 = FOLLOWING + ("expect", "expect_sum", "prot", "devptr", "stream")
# the third vocabulary (seeds NSEEDS .. NSEEDS_V3 - 1): the batched Pauli sum and the reduced density matrix
FOLLOWING_V3 = FOLLOWING_V2 + ("expect_batch", "rdm")
SETTING = ("reset", "measure_state", "fill", "write_full_negzero", "write_partial", "write_nonfinite", "collapse", "compact",
           "queued_mode1", "queued_behind_basis", "load")
QUEUED = ("h", "cphase", "camodc", "iqft", "qcomp")
# calls that leave a lazily pending basis state pending (answered from the basis index, or refused before anything runs)
QUIET_FOR_PENDING = ("sample", "marginal", "stats", "measure_qubits", "postselect", "refused", "expect", "expect_sum", "expect_batch", "rdm")


def apply_to_model(m, op):
    """one op on the model; returns what the call returns, in the form apply_to_register (test_gpu_api_sequences.py) gives"""
    k = op[0]
    if k == "reset": m.reset_register()
    elif k == "fill": m.fill_random(op[1])
    elif k == "write": m.write(window_data(m.dim, op[2], op[3], op[4]), op[1])
    elif k == "read": return m.read(op[1], op[2])
    elif k == "h": m.hadamard_gate(op[1])
    elif k == "cphase": m.c_phase_shift_gate(op[1], op[2], op[3])
    elif k == "camodc": m.c_amodc_gate(op[1], op[2], op[3])
    elif k == "iqft": m.inverse_QFT()
    elif k == "qcomp": m.quantum_computation(op[1], op[2])
    elif k == "u1": m.one_qubit_gate(op[1], matrix_data(2, op[2]))
    elif k == "cu1": m.c_one_qubit_gate(op[1], op[2], matrix_data(2, op[3]))
    elif k == "u2": m.two_qubit_gate(op[1], op[2], matrix_data(4, op[3]))
    elif k == "cu2": m.c_two_qubit_gate(op[1], op[2], op[3], matrix_data(4, op[4]))
    elif k == "measure": return m.measure_state(op[1])
    elif k == "sample": return m.sample_states(sample_draws(op[1], op[2]))
    elif k == "marginal": return m.marginal(op[1], op[2])
    elif k == "measure_qubits": return m.measure_qubits(op[1], op[2], op[3])
    elif k == "postselect": return m.postselect(op[1], op[2], op[3])
    elif k == "total": return m.total_probability()
    elif k == "norm2": return None if m.holds_nonfinite() else m.norm2()
    elif k == "save": m.save(op[1])
    elif k == "load": m.load(op[1])
    elif k == "flush": m.flush()
    elif k == "sync": m.synchronize()
    elif k == "fusion": m.set_fusion(op[1])
    elif k == "stats": pass
    elif k == "expect": return m.expectation(op[1], op[2])
    elif k == "expect_sum": return m.expectation_sum(sum_terms(m.n, op[1], op[2]))
    elif k == "expect_batch": return m.expectation_batch(batch_terms(m.n, op[1], op[2]))
    elif k == "rdm": return (m.reduced_density_matrix(op[1], op[2]), m.marginal(op[1], op[2]))
    elif k == "prot": m.pauli_rotation(op[1], op[2], op[3])
    elif k == "prot_batch":                                                 # (qcx_pauli_rotation_batch promises the bits of the loop)
        for (x, z), theta in rotation_terms(m.n, op[1], op[2]):
            m.pauli_rotation(x, z, theta)
    elif k == "devptr": return m.read(op[1], op[2])
    elif k == "stream": pass
    elif k in ("relays", "selfcheck"): pass                                 # (a sharded register's; no amplitude changes)
    elif k == "refused":
        inner, status = op[1], op[2]
        if status == UNSUPPORTED:                                           # (a sharded register refuses the call before it looks at it)
            return status
        if inner[0] == "postselect" and inner[3] < (1 << inner[2]) and inner[1] + inner[2] <= m.n:
            p, out = collapse_ref(m.a, m.n, inner[1], inner[2], inner[3])
            assert out is None, ("the generator drew an outcome the state CAN be collapsed onto", op)
            return (p, status)
        return status                                                       # the state stays as it was
    else:
        raise ValueError(f"unknown op {op!r}")
    return None


# ---- the generator -----------------------------------------------------------------------------------------------------------

NSEEDS_V1, NSEEDS = 64, 128              # seeds < NSEEDS_V1: vocabulary 1, frozen (tests/golden/sequence_digests.json); the others: 2
NSEEDS_V3 = NSEEDS + 64                   # seeds NSEEDS .. NSEEDS_V3 - 1: vocabulary 3, frozen like the others
SMALL_V1 = 24                             # the same for the small sequences of generate(.., small=True): 24 of every vocabulary
# (L, M, C, a); n = 6 .. 14, M = 0 and n < 9 (partial tiles in several kernels) included
SHAPES = [(8, 4, 15, 7), (9, 5, 21, 2), (8, 5, 21, 2), (6, 0, 1, 1), (10, 0, 1, 1), (2, 4, 15, 7), (3, 4, 15, 7), (4, 4, 15, 7),
          (5, 5, 21, 2), (13, 0, 1, 1), (7, 6, 35, 2), (10, 4, 15, 7), (4, 5, 21, 2), (8, 0, 1, 1)]
# compact_chain (csrc/qcx_fuse.inc.h) runs a circuit on the compact copy when L + cb >= 14 with cb = the orbit's column bits
# (2 for the four residues of C = 15, 3 for the six of C = 21): the smallest registers that reach it have n = 16
COMPACT_SHAPES = [(11, 5, 21, 2), (12, 4, 15, 7)]
SMALL_SHAPES = [(2, 2, 3, 2), (3, 3, 7, 3), (2, 4, 15, 7), (5, 0, 1, 1), (6, 0, 1, 1), (3, 0, 1, 1), (1, 4, 15, 7), (3, 2, 3, 2)]
# launch knobs: values the forced-form tests of K1 / K2 / K12 / K13 use (registers of n >= 9 only), and K11's
KNOBS_N9 = [dict(h_variant=1, h_ppt=2, h_streams_log2=3), dict(h_variant=2, h_wave_r=4, h_nt=0, h_streams_log2=0), dict(ph_lines=0),
            dict(ph_lines=0, ph_nt=0, ph_streams_log2=0), dict(u2_variant=1), dict(u2_streams_log2=3), dict(u2_variant=1, u2_nt=0)]
KNOBS_ANY = [dict(collapse_upt=8), dict(collapse_perm=0), dict(collapse_grid_cap=1), dict(collapse_grid_cap=3, collapse_upt=8)]
# vocabulary 2 adds K15's grid cap, at values that do not divide the number of units a rotation walks
KNOBS_V2 = [dict(prot_grid_cap=1), dict(prot_grid_cap=3)]
# vocabulary 3 adds the launch knobs of the fused engine, at the values tests/test_gpu_fuzz.py draws: chained passes from n = 13
# on (the default begins at n = 20), the walk on 8 amplitudes per thread from one tile on or not at all, smaller and larger
# tiles, no generated front, no column form of it, a compact result that is expanded at once, k_expand_compact in place of the
# expanding store, no plan cache, the record scan of the measurement from 2^10 amplitudes on.  Drawn only for registers of
# n >= max(M + 6, 10), the range the fuzz test uses
KNOBS_FUSED = [dict(fuse_chain_min_n=13), dict(fuse_chain_min_n=13, fuse_chain_dir=0), dict(fuse_chain_min_n=13, fuse_chain_dir=1),
               dict(fuse_x8_min_tiles_log2=0), dict(fuse_x8=0), dict(fuse_T=10), dict(fuse_T=12, fuse_c=3), dict(fuse_gen=0),
               dict(fuse_gen_cols=0), dict(fuse_compact_lazy=0), dict(fuse_expand_fused=0), dict(fuse_plan_cache=0),
               dict(meas_min_log2=10, meas_block_log=8), dict(meas_min_log2=10, meas_fast=0)]
# without these two no flush runs as a compact chain (compact_chain_plan, csrc/qcx_fuse.inc.h), which run_ops asserts on the
# compact seeds
ENDS_COMPACT_CHAINS = ("fuse_gen", "fuse_gen_cols")


class Config:
    def __init__(self, seed, small=False):
        rs = np.random.RandomState(7919 * seed + 13)
        self.seed, self.small = seed, small
        v1, v2 = (SMALL_V1, 2 * SMALL_V1) if small else (NSEEDS_V1, NSEEDS)
        self.vocab = 1 if seed < v1 else 2 if seed < v2 else 3
        self.compact = (not small) and seed % 8 == 5
        if small:
            shapes = [SMALL_SHAPES[seed % len(SMALL_SHAPES)]]
        elif self.compact:
            shapes = [COMPACT_SHAPES[(seed // 8) % 2]]
        else:
            shapes = [SHAPES[seed % len(SHAPES)]]
            if seed % 4 == 2:                                              # two registers of different sizes, interleaved
                shapes.append(SHAPES[(seed + 5) % len(SHAPES)])
        self.shapes = shapes
        self.mode = int(rs.choice([-1, 0, 1]))
        self.modes = [self.mode] + [int(rs.choice([-1, 0, 1])) for _ in shapes[1:]]      # the start mode of every register
        self.knobs = {}
        if not small and seed % 3 == 1:
            pool = KNOBS_ANY + (KNOBS_V2 if self.vocab >= 2 else []) + (KNOBS_N9 if min(s[0] + s[1] for s in shapes) >= 9 else [])
            for i in rs.choice(len(pool), 3, replace=False):
                self.knobs.update(pool[int(i)])
        # vocabulary 3, two seeds in three: the fused engine's knobs (seed % 3 == 1: one dict on top of the per-gate knobs;
        # seed % 3 == 2: two of them); seed % 3 == 0 runs under the defaults
        if self.vocab == 3 and not small and seed % 3 and all(L + M >= max(M + 6, 10) for L, M, _, _ in shapes):
            pool = [d for d in KNOBS_FUSED if not (self.compact and any(k in ENDS_COMPACT_CHAINS for k in d))]
            for i in rs.choice(len(pool), seed % 3, replace=False):
                self.knobs.update(pool[int(i)])

    def __repr__(self):
        return f"seed {self.seed}: vocabulary {self.vocab} shapes (L, M, C, a) {self.shapes} start mode {self.mode} knobs {self.knobs}"


def pair_is_legal(s, f, shape, compact):
    L, M, Cn, a = shape
    if (s == "compact") != compact:
        return False
    if f in ("camodc", "qcomp") and M == 0:
        return False
    if s == "write_nonfinite" and f == "norm2":                            # (norm2 is not compared on a non-finite state)
        return False
    if f == "devptr" and compact:          # (the pointer ends compact chains for that register, and run_ops asserts them)
        return False
    return True


def seeds_of(vocab):
    return range(NSEEDS_V1) if vocab == 1 else range(NSEEDS_V1, NSEEDS) if vocab == 2 else range(NSEEDS, NSEEDS_V3)


def following_of(vocab):
    return FOLLOWING if vocab == 1 else FOLLOWING_V2 if vocab == 2 else FOLLOWING_V3


def _schedule(vocab):
    """every legal (state-setting kind, following kind) pair of one vocabulary three times, dealt round-robin to those of its
    seeds whose register allows it; the list of seed k is out[k - the vocabulary's first seed]"""
    seeds = seeds_of(vocab)
    cfgs = [Config(s) for s in seeds]
    out = [[] for _ in seeds]
    at, ns = 0, len(seeds)
    for _ in range(3):
        for s in SETTING:
            for f in following_of(vocab):
                for k in range(ns):
                    c = cfgs[(at + k) % ns]
                    if pair_is_legal(s, f, c.shapes[0], c.compact):
                        out[c.seed - seeds[0]].append((s, f))
                        at = (at + k + 1) % ns
                        break
    return out


_SCHEDULE = {}


class _Gen:
    """the ops of ONE register: scheduled (setting, following) probes with random parameters, random ops between them"""

    def __init__(self, ob, shape, mode, rs, allow_nonfinite=True, tag=0, vocab=1, devptr=True):
        self.ob, self.rs, self.tag = ob, rs, tag
        self.vocab, self.following, self.devptr = vocab, following_of(vocab), devptr
        self.L, self.M, self.Cn, self.a0 = shape
        self.n = self.L + self.M
        self.dim = 1 << self.n
        self.m = RegisterModel(ob, self.L, self.M)
        self.mode = mode
        self.pending = False                    # the library would hold a lazily pending basis state
        self.strict = False                     # ... would run strict passes (a non-finite write since the last reset / fill / measurement)
        self.slots = {}                         # saved slot -> the state in it was finite
        self.allow_nonfinite = allow_nonfinite
        self.ops = []
        self.emit(("reset",) if rs.randint(0, 2) else ("fill", int(rs.randint(1, 1 << 20))))

    # bookkeeping -----------------------------------------------------------------------------------------------------------
    def emit(self, op):
        self.ops.append(op)
        apply_to_model(self.m, op)
        k = op[0]
        if k == "fusion":
            self.mode = op[1]
        if k in ("reset", "measure"):
            self.pending = self.mode >= 0
        elif k in QUIET_FOR_PENDING or (k in QUEUED and self.mode == 1):
            pass
        else:
            self.pending = False
        if k == "write" and op[4] in ("inf", "nan"):
            self.strict = True
        elif k in ("reset", "measure", "fill"):
            self.strict = False
        if k == "save":
            self.slots[op[1]] = not self.m.holds_nonfinite()

    def r(self):
        rs = self.rs
        return float(rs.uniform(0, 1)) if rs.randint(0, 5) else float(rs.choice([0.0, 1.0, 1e-9, 0.999999999]))

    def seed(self):
        return int(self.rs.randint(1, 1 << 30))

    def qubits(self, k):
        return [int(v) for v in self.rs.choice(self.n, k, replace=False)]

    def a_range(self, lo=0):
        first = int(self.rs.randint(lo, self.n + 1))
        num = int(self.rs.randint(0, min(self.n - first, 6) + 1))
        if self.rs.randint(0, 4) == 0 and first < self.n:
            num = max(num, 1)
        return first, num

    def cleanse(self):
        """a finite state again (any way the API offers)"""
        if self.m.holds_nonfinite():
            c = int(self.rs.randint(0, 4))
            self.emit([("reset",), ("fill", self.seed()), ("measure", self.r()), ("write", 0, self.dim, self.seed(), "plain")][c])

    def dense(self):
        """a state with more than a few populated amplitudes (a collapse of a basis state says little)"""
        if np.count_nonzero(self.m.a) < 8 and self.rs.randint(0, 4):
            if self.rs.randint(0, 2):
                self.emit(("fill", self.seed()))
            else:
                for q in self.qubits(min(self.n, 4)):
                    self.emit(("h", q))

    def gate(self):
        rs = self.rs
        k = int(rs.randint(0, 3)) if self.M else int(rs.randint(0, 2))
        if k == 0 or self.n < 2:
            return ("h", int(rs.randint(0, self.n)))
        if k == 1:
            c, t = self.qubits(2)
            th = float(rs.uniform(-3.2, 3.2)) if rs.randint(0, 2) else float(np.pi / (1 << int(rs.randint(1, 12))))
            return ("cphase", c, t, th)
        return ("camodc", self.Cn, int(rs.randint(1, 4 * self.Cn)), int(rs.randint(0, self.n)))

    def good_outcome(self, first, num):
        P = self.m.marginal(first, num)
        ok = [v for v in range(P.size) if np.isfinite(P[v]) and P[v] > 0 and np.isfinite(1.0 / np.sqrt(P[v]))]
        return int(ok[int(self.rs.randint(0, len(ok)))]) if ok else None

    # ops by following kind ---------------------------------------------------------------------------------------------------
    def op_of(self, f):
        rs, n = self.rs, self.n
        if f == "reset": return ("reset",)
        if f == "fill": return ("fill", self.seed())
        if f == "write":
            finite = ("plain", "negzero")
            fl = str(rs.choice(finite + (("inf", "nan") if self.allow_nonfinite and rs.randint(0, 4) == 0 else ())))
            if rs.randint(0, 3) == 0:
                return ("write", 0, self.dim, self.seed(), fl)
            first = int(rs.randint(0, self.dim))
            return ("write", first, int(rs.randint(1, min(self.dim - first, 600) + 1)), self.seed(), fl)
        if f == "read":
            if rs.randint(0, 3) == 0:
                return ("read", 0, self.dim)
            first = int(rs.randint(0, self.dim))
            return ("read", first, int(rs.randint(1, min(self.dim - first, 2000) + 1)))
        if f in ("h", "cphase", "camodc"):
            while True:
                g = self.gate()
                if g[0] == f or (f == "cphase" and n < 2):
                    return g
        if f == "iqft": return ("iqft",)
        if f == "qcomp": return ("qcomp", self.Cn, self.a0)
        if f == "u1": return ("u1", int(rs.randint(0, n)), self.seed())
        if f == "cu1" and n >= 2: return ("cu1", *self.qubits(2), self.seed())
        if f == "u2" and n >= 2: return ("u2", *self.qubits(2), self.seed())
        if f == "cu2" and n >= 3: return ("cu2", *self.qubits(3), self.seed())
        if f in ("cu1", "u2", "cu2"): return ("u1", int(rs.randint(0, n)), self.seed())
        if f == "measure": return ("measure", self.r())
        if f == "sample": return ("sample", self.seed(), int(rs.choice([1, 3, 8, 17])))
        if f == "marginal": return ("marginal", *self.a_range())
        if f == "measure_qubits": return ("measure_qubits", *self.a_range(), self.r())
        if f == "postselect":
            first, num = self.a_range()
            v = self.good_outcome(first, num)
            return ("postselect", first, num, v if v is not None else int(rs.randint(0, 1 << num)))
        if f in ("total", "norm2", "flush", "sync"): return (f,)
        if f == "save": return ("save", int(rs.randint(0, 2)))
        if f == "load":
            if not self.slots:
                return ("save", 0)
            return ("load", int(rs.choice(sorted(self.slots))))
        if f == "fusion": return ("fusion", int(rs.choice([-1, 0, 1])))
        if f == "expect": return ("expect", *draw_masks(rs, n))
        if f == "expect_sum": return ("expect_sum", self.seed(), int(rs.choice([0, 1, 3, 6])))
        if f == "prot": return ("prot", *draw_masks(rs, n), self.theta())
        if f == "expect_batch": return ("expect_batch", self.seed(), int(rs.choice([0, 1, 3, 6, 6, 40])))
        if f == "rdm": return ("rdm", *self.rdm_range())
        if f == "devptr":
            if rs.randint(0, 3) == 0:
                return ("devptr", 0, self.dim)
            first = int(rs.randint(0, self.dim))
            return ("devptr", first, int(rs.randint(1, min(self.dim - first, 2000) + 1)))
        if f == "stream": return ("stream", int(rs.randint(0, 2)))
        raise ValueError(f)

    def rdm_range(self):
        """(first, num) with num = 0 .. RDM_MAX; on a register of n >= 12 one draw in two begins below bit 12 - num and the other
        at or above it (rdm_shape: the two forms of k_rdm_leaves)"""
        rs, n = self.rs, self.n
        num = int(rs.randint(0, min(RDM_MAX, n) + 1))
        if n < 12:
            return int(rs.randint(0, n - num + 1)), num
        if rs.randint(0, 2):
            return int(rs.randint(0, 12 - num)), num
        return int(rs.randint(12 - num, n - num + 1)), num

    def theta(self):
        """uniform in (-7, 7); one draw in six is 0.0, pi, 2 pi or -0.0 (the two zeros leave the state's bits as they are)"""
        rs = self.rs
        if rs.randint(0, 6) == 0:
            return float([0.0, np.pi, 2.0 * np.pi, -0.0][int(rs.randint(0, 4))])
        return float(rs.uniform(-7.0, 7.0))

    def pauli(self):
        """a burst of Pauli calls with nothing between them: value, two rotations, then the value of the same string again or a sum"""
        x, z = draw_masks(self.rs, self.n)
        self.emit(("expect", x, z))
        self.emit(("prot", *draw_masks(self.rs, self.n), self.theta()))
        self.emit(("prot", x, z, self.theta()))
        self.emit(("expect", x, z) if self.rs.randint(0, 2) else ("expect_sum", self.seed(), int(self.rs.choice([1, 3, 6]))))
        if self.vocab == 3:                     # the same state through the batched sum and the density matrix, either first
            tail = [("expect_batch", self.seed(), int(self.rs.choice([3, 6, 40]))), ("rdm", *self.rdm_range())]
            for op in tail[::-1] if self.rs.randint(0, 2) else tail:
                self.emit(op)

    def quiet(self):
        """a call that leaves every lazy form as it is (the issue's "non-flushing" calls)"""
        c = int(self.rs.randint(0, {1: 3, 2: 4, 3: 6}[self.vocab]))
        if c == 0: return ("sample", self.seed(), int(self.rs.choice([1, 4, 9])))
        if c == 1: return ("marginal", *self.a_range(self.M))
        if c == 3: return ("expect", *draw_masks(self.rs, self.n))
        if c == 4: return ("expect_batch", self.seed(), int(self.rs.choice([1, 3, 6])))
        if c == 5: return ("rdm", *self.rdm_range())
        return ("stats",)

    def refused(self):
        """a call the library must refuse with the state untouched: (inner op, status)"""
        rs, n = self.rs, self.n
        c = int(rs.randint(0, {1: 4, 2: 6, 3: 8}[self.vocab]))
        if c == 6:                                                           # a density matrix past the register, or wider than the call serves
            if n > RDM_MAX and rs.randint(0, 2):
                return ("rdm", int(rs.randint(0, n - RDM_MAX)), RDM_MAX + 1), UNSUPPORTED
            num = int(rs.randint(1, RDM_MAX + 3))                            # (past the register is looked at first: RDM_MAX + 1 and + 2 too)
            return ("rdm", int(rs.randint(max(0, n - num + 1), n + 2)), num), BAD_QUBIT
        if c == 7:                                                           # a batch with ONE mask that reaches bit n: nothing runs
            k = int(rs.choice([1, 3, 6, 40]))
            return ("expect_batch", self.seed(), k, int(rs.randint(0, k)), str(rs.choice(["x", "z"]))), BAD_QUBIT
        if c >= 4:                                                           # the Pauli calls: a mask that reaches bit n, an angle that is not finite
            x, z = draw_masks(rs, n)
            k = int(rs.randint(0, 3))
            if k == 2:
                return ("prot", x, z, str(rs.choice(["inf", "-inf", "nan"]))), BAD_ARGUMENTS
            if rs.randint(0, 2):
                x |= 1 << n
            else:
                z |= 1 << n
            return (("expect", x, z) if k == 0 else ("prot", x, z, self.theta())), BAD_QUBIT
        if c == 0:                                                           # bad qubit
            k = int(rs.randint(0, 4))
            if k == 0: return ("h", n), BAD_QUBIT
            if k == 1: return ("marginal", n - 1, 2), BAD_QUBIT
            if k == 2: return ("u1", n + 3, self.seed()), BAD_QUBIT
            q = int(rs.randint(0, n))
            return ("cphase", q, q, 0.5), BAD_QUBIT
        if c == 1:                                                           # a matrix component of 1 + 1 ulp
            if n >= 2 and rs.randint(0, 2):
                return ("u2x", *self.qubits(2), self.seed()), BAD_ARGUMENTS
            return ("u1x", int(rs.randint(0, n)), self.seed()), BAD_ARGUMENTS
        first, num = self.a_range()
        if c == 2:                                                           # an outcome that does not fit
            return ("postselect", first, num, 1 << num), BAD_ARGUMENTS
        for first, num in [self.a_range() for _ in range(6)]:                # an outcome of probability +0
            P = self.m.marginal(first, num)
            zero = np.flatnonzero((P == 0) & ~np.signbit(P))
            if zero.size:
                return ("postselect", first, num, int(zero[int(rs.randint(0, zero.size))])), BAD_ARGUMENTS
        return ("postselect", first, num, 1 << num), BAD_ARGUMENTS

    # state-setting kinds -----------------------------------------------------------------------------------------------------
    def finite_slot(self):
        good = [k for k, fin in self.slots.items() if fin]
        if not good:
            self.cleanse()
            self.emit(("save", int(self.rs.randint(0, 2))))
            good = [k for k, fin in self.slots.items() if fin]
        return int(self.rs.choice(good))

    def want_mode(self, modes):
        if self.mode not in modes:
            self.emit(("fusion", int(self.rs.choice(modes))))

    def setting(self, s, f):
        rs = self.rs
        if f == "load" and not self.slots:
            self.emit(("save", int(rs.randint(0, 2))))
        if s == "reset": self.emit(("reset",))
        elif s == "measure_state": self.emit(("measure", self.r()))
        elif s == "fill": self.emit(("fill", self.seed()))
        elif s == "write_full_negzero": self.emit(("write", 0, self.dim, self.seed(), "negzero"))
        elif s == "write_partial":
            self.cleanse()
            first = int(rs.randint(0, self.dim - 1))
            self.emit(("write", first, int(rs.randint(1, min(self.dim - first, 600, self.dim - 1) + 1)), self.seed(), str(rs.choice(["plain", "negzero"]))))
        elif s == "write_nonfinite":
            first = int(rs.randint(0, self.dim)) if rs.randint(0, 4) else 0
            count = self.dim - first if rs.randint(0, 4) == 0 else int(rs.randint(1, min(self.dim - first, 600) + 1))
            self.emit(("write", first, count, self.seed(), str(rs.choice(["inf", "nan"]))))
        elif s == "collapse":
            self.cleanse()
            self.dense()
            first, num = self.a_range()
            v = self.good_outcome(first, num)
            if v is None or rs.randint(0, 2):
                self.emit(("measure_qubits", first, num, float(rs.uniform(0.02, 0.98))))
            else:
                self.emit(("postselect", first, num, v))
        elif s == "compact":
            self.want_mode([0, 1])
            self.emit(("reset",))
            self.emit(("qcomp", self.Cn, self.a0))
        elif s == "queued_mode1":
            self.want_mode([1])
            self.cleanse()
            if self.strict:                                                  # (strict passes are not queued)
                self.emit(("fill", self.seed()))
            if self.pending:
                self.emit(("fill", self.seed()) if rs.randint(0, 2) else ("flush",))
            for _ in range(int(rs.randint(1, 6))):
                self.emit(self.gate())
        elif s == "queued_behind_basis":
            self.want_mode([1])
            self.emit(("reset",) if rs.randint(0, 2) else ("measure", self.r()))
            if self.M and rs.randint(0, 2):                                  # a circuit front: the H layer, then part of the multiply ladder
                for l in range(self.M, self.n):
                    self.emit(("h", l))
                x = self.a0 % self.Cn
                for l in range(self.M, self.M + int(rs.randint(0, min(self.L, 3) + 1))):
                    self.emit(("camodc", self.Cn, x, l))
                    x = (x * x) % self.Cn
                if rs.randint(0, 2):
                    self.emit(self.gate())
            else:
                for _ in range(int(rs.randint(1, 5))):
                    self.emit(self.gate())
        elif s == "load":
            slot = self.finite_slot()
            if rs.randint(0, 2):
                self.emit(self.op_of(str(rs.choice(["h", "fill", "reset", "u1"]))))   # (so that the load changes something)
            self.emit(("load", slot))
        else:
            raise ValueError(s)

    def probe(self, s, f):
        self.setting(s, f)
        for _ in range(int(self.rs.choice([0, 0, 1, 2]))):
            self.emit(self.quiet())
        if f == "norm2" and self.m.holds_nonfinite():
            f = "total"
        self.emit(self.op_of(f))

    def refuse(self):
        """a refused call, then a window that shows the state untouched"""
        inner, status = self.refused()
        self.emit(("refused", inner, status))
        first = int(self.rs.randint(0, self.dim))
        self.emit(("read", first, int(self.rs.randint(1, min(self.dim - first, 2000) + 1))))

    def underflow(self):
        """a collapse that itself makes -0 out of negative subnormals, on a state whose zero pass was NOT owed before it; then a
        gate that leaves most amplitudes alone (the reference turns their -0 into +0 all the same) and a read"""
        rs = self.rs
        self.emit(("write", 0, self.dim, self.seed(), "subnormal"))
        c, t = self.qubits(2)
        self.emit(("cphase", c, t, float(rs.uniform(-3, 3))))               # runs the pass the write owes
        if self.mode == 1:
            self.emit(("flush",))
        first = int(rs.randint(0, self.n))
        self.emit(("postselect", first, 1, int(np.argmax(self.m.marginal(first, 1)))))
        if rs.randint(0, 2) or self.n < 3:
            self.emit(("cphase", c, t, float(rs.uniform(-3, 3))))
        else:
            self.emit(("cu2", *self.qubits(3), self.seed()))
        self.emit(("read", 0, self.dim))

    def extra(self):
        rs = self.rs
        if rs.randint(0, 7) == 0:
            self.refuse()
            return
        if rs.randint(0, 12) == 0:
            self.underflow()
            return
        if self.vocab >= 2 and rs.randint(0, 8) == 0:
            self.pauli()
            return
        f = self.following[int(rs.randint(0, len(self.following)))]
        if (f in ("camodc", "qcomp") and self.M == 0) or (f == "norm2" and self.m.holds_nonfinite()) or (f == "devptr" and not self.devptr):
            f = "h"
        if f == "write" and not self.allow_nonfinite:
            self.cleanse()
        self.emit(self.op_of(f))


def generate(ob, seed, small=False, length=None):
    """(Config, ops) of one seed; an op of the list is (register number, op tuple).  small: registers of n <= 6, no non-finite
    values, `length` ops (the sequences test_register_model.py replays in long double)"""
    cfg = Config(seed, small)
    rs = np.random.RandomState(104729 * seed + 71)
    g = _Gen(ob, cfg.shapes[0], cfg.mode, rs, allow_nonfinite=not small, vocab=cfg.vocab, devptr=not cfg.compact)
    following = following_of(cfg.vocab)
    if small:
        while len(g.ops) < length:
            s, f = SETTING[int(rs.randint(0, len(SETTING)))], following[int(rs.randint(0, len(following)))]
            if pair_is_legal(s, f, cfg.shapes[0], False) and s != "write_nonfinite" and rs.randint(0, 2):
                g.probe(s, f)
            else:
                g.extra()
        return cfg, [(0, op) for op in g.ops[:length]]
    if cfg.vocab not in _SCHEDULE:
        _SCHEDULE[cfg.vocab] = _schedule(cfg.vocab)
    probes = list(_SCHEDULE[cfg.vocab][seed - seeds_of(cfg.vocab)[0]])
    rs.shuffle(probes)
    for s, f in probes:
        g.probe(s, f)
        if rs.randint(0, 6) == 0:
            g.emit(("read", 0, g.dim))
        if rs.randint(0, 5) == 0:                                            # about one op in twenty is a refused call
            g.refuse()
        if rs.randint(0, 10) < 2:
            g.extra()
        if cfg.vocab >= 2 and rs.randint(0, 10) < (5 if g.m.holds_nonfinite() else 1):    # (often where the state is not finite:
            g.pauli()                                                                       #  the strict register's Pauli calls)
    while len(g.ops) < 40:
        g.extra()
    g.emit(("read", 0, g.dim))
    ops = [(0, op) for op in g.ops]
    if len(cfg.shapes) > 1:                                                  # the second register: random ops, dealt in between
        h = _Gen(ob, cfg.shapes[1], cfg.modes[1], rs, tag=1, vocab=cfg.vocab)
        while len(h.ops) < max(12, len(g.ops) // 3):
            h.extra()
        h.emit(("read", 0, h.dim))
        where = np.sort(rs.randint(0, len(ops) + 1, len(h.ops)))
        for k in range(len(h.ops) - 1, -1, -1):
            ops.insert(int(where[k]), (1, h.ops[k]))
    return cfg, ops


# ---- what a list of ops reaches (judged on the list alone) ---------------------------------------------------------------------

def is_quiet(op, M, vocab=1):
    return (op[0] in ("sample", "stats") or (op[0] == "marginal" and op[1] >= M) or (vocab in (2, 3) and op[0] == "expect")
            or (vocab == 3 and op[0] in ("expect_batch", "rdm")))


def compact_shape(shape):
    L, M, Cn, a = shape
    cb = {15: 2, 21: 3}.get(Cn)
    return M in (4, 5) and L >= 8 and L + M >= 12 and cb is not None and L + cb >= 14


def pairs_reached(shape, start_mode, ops, vocab=1):
    """{(setting kind, following kind): count} over the ops of one register: a pair counts when nothing but quiet calls stand
    between the two"""
    L, M, Cn, a = shape
    dim = 1 << (L + M)
    mode, pending, strict = start_mode, False, False
    kinds = []
    for i, op in enumerate(ops):
        k, s = op[0], None
        if k == "reset": s = "reset"
        elif k == "measure": s = "measure_state"
        elif k == "fill": s = "fill"
        elif k == "load": s = "load"
        elif k == "write":
            if op[4] in ("inf", "nan"): s = "write_nonfinite"
            elif op[2] < dim: s = "write_partial"
            elif op[4] == "negzero": s = "write_full_negzero"
        elif k in ("measure_qubits", "postselect"): s = "collapse"
        elif k == "qcomp" and i and ops[i - 1][0] == "reset" and mode in (0, 1) and compact_shape(shape): s = "compact"
        elif k in QUEUED and mode == 1 and not strict:
            s = "queued_behind_basis" if pending else "queued_mode1"
        kinds.append(s)
        if k == "fusion": mode = op[1]
        if k in ("reset", "measure"): pending = mode >= 0
        elif k in QUIET_FOR_PENDING or (k in QUEUED and mode == 1 and not strict): pass
        else: pending = False
        if k == "write" and op[4] in ("inf", "nan"): strict = True
        elif k in ("reset", "measure", "fill"): strict = False
    out = {}
    for i, s in enumerate(kinds):
        if s is None:
            continue
        for op in ops[i + 1:]:
            if op[0] in following_of(vocab):
                out[(s, op[0])] = out.get((s, op[0]), 0) + 1
            if not is_quiet(op, M, vocab):
                break
    return out


# ---- the sharded family ------------------------------------------------------------------------------------------------------------
# Sequences for a register of 2, 4 or 8 shards.  Between calls such a register keeps a logical -> physical qubit layout that
# trades leave swapped, a gate queue (in EVERY fusion mode: mode 0 behaves as 1, mode -1 only launches gate by gate), a pending
# basis state (reset in a mode >= 0; measure_state collapses at once), a circuit front written per shard, a compact circuit on a
# companion register, an owed zero pass, relays and the slice / window geometry.  The model is RegisterModel, unchanged.

NSEEDS_SH = 48
FOLLOWING_SH = ("reset", "fill", "write", "read", "h", "cphase", "camodc", "iqft", "qcomp", "measure", "total", "norm2", "save",
                "load", "flush", "sync", "fusion", "relays", "selfcheck", "stats", "refused")
SETTING_SH = ("reset", "measure_state", "fill", "write_full_negzero", "write_partial", "load", "swapped_layout", "queued",
              "queued_behind_basis", "compact")
QUIET_SH = ("stats", "selfcheck", "refused")          # calls that leave every lazy form of a sharded register as it is
RESTORES_IDENTITY = ("reset", "fill", "write", "read", "measure", "total", "save", "load")      # (relays too, but not on a dry run)
# (L, M, C, a) by shard count.  ordinary: n_local = n - k >= 2 k + 6; tiny: n_local < 2 k + 6, where sh_set_slices lets runs
# shorter than 1 KiB be traded (min_evict = M): the smallest registers qcx_register_create_sharded accepts are among them;
# compact: the smallest shapes per shard count at which reset + quantum_computation runs on the companion register (sh_compact:
# 4 <= M <= 12 and n_local >= M + 6; the companion of L + cb qubits is accepted whenever the register itself is); on 8 shards
# that is (11, 4) of the ordinary list, and the list holds the smallest whose trade zone is large enough for a relay as well.  Shapes of the other two lists that meet the condition -- (9, 4) and
# (8, 5) on 4 shards, (11, 4) and the tiny (9, 4) on 8 -- are compact shapes as well (ShardedConfig.compact) and asserted as such
SH_SHAPES = {
    "ordinary": {2: [(9, 0, 1, 1), (5, 4, 15, 7), (6, 5, 21, 2)], 4: [(12, 0, 1, 1), (9, 4, 15, 7), (8, 5, 21, 2)], 8: [(15, 0, 1, 1), (11, 4, 15, 7)]},
    "tiny": {2: [(3, 0, 1, 1), (4, 0, 1, 1), (6, 0, 1, 1), (3, 4, 15, 7), (3, 5, 21, 2)], 4: [(6, 0, 1, 1), (8, 0, 1, 1), (6, 4, 15, 7), (6, 5, 21, 2)],
             8: [(9, 0, 1, 1), (12, 0, 1, 1), (9, 4, 15, 7)]},
    "compact": {2: [(7, 4, 15, 7)], 4: [(8, 4, 15, 7)], 8: [(12, 4, 15, 7)]},
}
MEASURE_EDGES = ("nan", "1.5", "-0.25")                # draws outside [0, 1): ops carry them as strings (a NaN does not replay from its repr)
# every entry point include/qcx.h lists as QCX_UNSUPPORTED on a sharded register
REFUSED_SH = ("sample_rng", "marginal", "measure_qubits_rng", "postselect", "expect", "expect_sum", "expect_batch", "u1", "cu1", "u2",
              "cu2", "prot", "set_stream", "events_create", "devptr")


class ShardedConfig:
    """shards, shape list, shape, start mode and the environment at creation of one seed of the sharded family"""

    def __init__(self, seed):
        rs = np.random.RandomState(6007 * seed + 29)
        self.seed = seed
        self.shards = (2, 4, 8)[(seed // 3) % 3]
        self.kind = ("ordinary", "tiny", "compact" if (seed // 3) % 2 == 0 else ("ordinary", "tiny")[(seed // 6) % 2])[seed % 3]
        shapes = SH_SHAPES[self.kind][self.shards]
        self.shape = shapes[(seed // 9) % len(shapes)]
        self.k = self.shards.bit_length() - 1
        self.n = self.shape[0] + self.shape[1]
        self.n_local = self.n - self.k
        self.compact = 4 <= self.shape[1] <= 12 and self.n_local >= self.shape[1] + 6      # sh_compact's condition
        self.mode = int(rs.choice([-1, 0, 1]))
        self.env = {}
        sl, ov = int(rs.randint(0, 4)), int(rs.randint(0, 3))
        if sl: self.env["QCX_SHARD_SLICES_LOG2"] = str((0, 0, 2, 3)[sl])
        if ov: self.env["QCX_SHARD_OVERLAP"] = str(ov - 1)
        if (seed + seed // 6) % 6 == 4: self.env["QCX_SHARD_FORCE_STAGED"] = "1"     # (staggered: seeds of every shape list)
        # one relay set right after creation for one seed in six, over the three shape lists: 0, 18, 36 ordinary, 13, 31 tiny,
        # 8, 26, 44 compact on 8 shards (where the relay is really set up: smaller trade zones are not striped); five seeds of
        # the compact list start without
        self.relays = int(seed % 6 == (0, 2, 1)[(seed // 6) % 3])

    def __repr__(self):
        return (f"sharded seed {self.seed}: {self.shards} shards, {self.kind} shape (L, M, C, a) {self.shape} start mode {self.mode} "
                f"environment {self.env} relays {self.relays}")


def sh_pair_is_legal(s, f, cfg):
    if s == "compact" and not cfg.compact:
        return False
    if f in ("camodc", "qcomp") and cfg.shape[1] == 0:
        return False
    return True


def _sh_schedule():
    """every legal (state-setting kind, following kind) pair of the sharded family three times, dealt round-robin to the seeds
    whose register allows it, evenly"""
    cfgs = [ShardedConfig(s) for s in range(NSEEDS_SH)]
    out = [[] for _ in cfgs]
    at = 0
    for _ in range(3):
        for s in SETTING_SH:
            for f in FOLLOWING_SH:
                legal = [c.seed for c in cfgs if sh_pair_is_legal(s, f, c)]
                seed = min(legal, key=lambda k: (len(out[k]), (k - at) % NSEEDS_SH))        # the seed with the fewest probes so far
                out[seed].append((s, f))
                at = (seed + 1) % NSEEDS_SH
    return out


class _ShGen(_Gen):
    """the ops of one sharded register"""

    def __init__(self, ob, cfg, rs):
        self.cfg, self.k, self.n_local = cfg, cfg.k, cfg.n_local
        self.refused_next = 7 * cfg.seed                # (where this seed starts in REFUSED_SH)
        super().__init__(ob, cfg.shape, cfg.mode, rs, allow_nonfinite=False, vocab="sharded", devptr=False)
        self.following = FOLLOWING_SH

    def emit(self, op):
        self.ops.append(op)
        apply_to_model(self.m, op)
        k = op[0]
        if k == "fusion":
            self.mode = op[1]
        if k == "reset":
            self.pending = self.mode >= 0
        elif k in QUIET_SH or k in QUEUED:              # (a sharded register queues in every mode)
            pass
        else:
            self.pending = False
        if k == "save":
            self.slots[op[1]] = True

    def r(self):
        if self.rs.randint(0, 8) == 0:
            return str(self.rs.choice(MEASURE_EDGES))
        return super().r()

    def cleanse(self): pass                             # (no non-finite values in this family)

    def window(self, cap):
        """(first, count) of a partial window; two in three straddle a multiple of 2^n_local (a shard boundary)"""
        rs, per = self.rs, 1 << self.n_local
        if rs.randint(0, 3):
            b = int(rs.randint(1, self.cfg.shards)) * per
            first = b - int(rs.randint(1, min(b, cap // 2) + 1))
            hi = min(self.dim - first, cap, self.dim - 1)
            return first, int(rs.randint(b - first + 1, hi + 1))
        first = int(rs.randint(0, self.dim - 1))
        return first, int(rs.randint(1, min(self.dim - first, cap, self.dim - 1) + 1))

    def gate(self):
        rs = self.rs
        k = int(rs.randint(0, 3)) if self.M else int(rs.randint(0, 2))
        if k == 0:                                      # two Hadamards in five on one of the top k + 1 qubits
            top = self.n - 1 - int(rs.randint(0, self.k + 1))
            return ("h", top if rs.randint(0, 5) < 2 else int(rs.randint(0, self.n)))
        if k == 1:
            c, t = self.qubits(2)
            th = float(rs.uniform(-3.2, 3.2)) if rs.randint(0, 2) else float(np.pi / (1 << int(rs.randint(1, 12))))
            return ("cphase", c, t, th)
        return ("camodc", self.Cn, int(rs.randint(1, 4 * self.Cn)), int(rs.randint(self.M, self.n)))

    def op_of(self, f):
        rs = self.rs
        if f == "write":
            fl = str(rs.choice(("plain", "negzero")))
            if rs.randint(0, 4) == 0:
                return ("write", 0, self.dim, self.seed(), fl)
            return ("write", *self.window(600), self.seed(), fl)
        if f == "read":
            if rs.randint(0, 4) == 0:
                return ("read", 0, self.dim)
            return ("read", *self.window(2000))
        if f == "relays": return ("relays", int(rs.randint(0, 2)))
        if f in ("selfcheck", "stats"): return (f,)
        if f == "refused": return ("refused", *self.refused())
        return super().op_of(f)

    def quiet(self):
        c = int(self.rs.randint(0, 4))
        return ("stats",) if c < 2 else ("selfcheck",) if c == 2 else ("refused", *self.refused())

    def refused(self):
        """(inner op, status): one of the calls a sharded register refuses (dealt in turn, so that every one occurs), arguments
        the unsharded register would accept; one draw in eight is the BAD_QUBIT kind instead"""
        rs, n = self.rs, self.n
        if rs.randint(0, 8) == 0:
            if rs.randint(0, 2) or n < 2:
                return ("h", n), BAD_QUBIT
            q = int(rs.randint(0, n))
            return ("cphase", q, q, 0.5), BAD_QUBIT
        j = REFUSED_SH[self.refused_next % len(REFUSED_SH)]
        self.refused_next += 1
        if j in ("cu1", "u2") and n < 2: j = "u1"
        if j == "cu2" and n < 3: j = "u1"
        if j == "sample_rng": inner = (j, self.seed(), int(rs.choice([1, 3, 8])))
        elif j == "marginal": inner = (j, *self.a_range())
        elif j == "measure_qubits_rng": inner = (j, *self.a_range(), self.seed())
        elif j == "postselect":
            first, num = self.a_range()
            inner = (j, first, num, int(rs.randint(0, 1 << num)))
        elif j == "expect": inner = (j, *draw_masks(rs, n))
        elif j in ("expect_sum", "expect_batch"): inner = (j, self.seed(), int(rs.choice([1, 3, 6])))
        elif j == "u1": inner = (j, int(rs.randint(0, n)), self.seed())
        elif j in ("cu1", "u2"): inner = (j, *self.qubits(2), self.seed())
        elif j == "cu2": inner = (j, *self.qubits(3), self.seed())
        elif j == "prot": inner = (j, *draw_masks(rs, n), self.theta())
        elif j == "events_create": inner = (j, int(rs.randint(1, 9)))
        else: inner = (j,)
        return inner, UNSUPPORTED

    def setting(self, s, f):
        rs = self.rs
        if f == "load" and not self.slots:
            self.emit(("save", int(rs.randint(0, 2))))
        if s == "reset": self.emit(("reset",))
        elif s == "measure_state": self.emit(("measure", self.r()))
        elif s == "fill": self.emit(("fill", self.seed()))
        elif s == "write_full_negzero": self.emit(("write", 0, self.dim, self.seed(), "negzero"))
        elif s == "write_partial": self.emit(("write", *self.window(600), self.seed(), str(rs.choice(["plain", "negzero"]))))
        elif s == "load":
            if not self.slots:
                self.emit(("save", int(rs.randint(0, 2))))
            slot = int(rs.choice(sorted(self.slots)))
            if rs.randint(0, 2):
                self.emit(self.op_of(str(rs.choice(["h", "fill", "reset"]))))
            self.emit(("load", slot))
        elif s == "swapped_layout":                     # from the identity layout with nothing pending: the H needs a trade
            if self.ops[-1][0] not in RESTORES_IDENTITY or self.pending:
                self.emit(("fill", self.seed()) if rs.randint(0, 2) else ("total",))
            self.emit(("h", self.n - 1 - int(rs.randint(0, self.k))))
            self.emit(("flush",))
        elif s == "queued":
            if self.pending:
                self.emit(("fill", self.seed()) if rs.randint(0, 2) else ("flush",))
            for _ in range(int(rs.randint(1, 6))):
                self.emit(self.gate())
        elif s == "queued_behind_basis":
            if self.mode < 0:
                self.emit(("fusion", int(rs.choice([0, 1]))))
            self.emit(("reset",))
            if rs.randint(0, 2):                        # the front form: the H layer, then part of the multiply ladder
                for l in range(self.M, self.n):
                    self.emit(("h", l))
                x = self.a0 % self.Cn
                for l in range(self.M, self.M + (int(rs.randint(0, min(self.L, 3) + 1)) if self.M else 0)):
                    self.emit(("camodc", self.Cn, x, l))
                    x = (x * x) % self.Cn
                if rs.randint(0, 2):
                    self.emit(self.gate())
            else:                                       # the other form: the basis state is written, then the gates run
                g = self.gate()
                while g[0] == "h":                      # (an H first would be a front of one gate)
                    g = self.gate()
                self.emit(g)
                for _ in range(int(rs.randint(0, 4))):
                    self.emit(self.gate())
        elif s == "compact":
            if self.mode < 0:
                self.emit(("fusion", int(rs.choice([0, 1]))))
            self.emit(("reset",))
            self.emit(("qcomp", self.Cn, self.a0))
        else:
            raise ValueError(s)

    def probe(self, s, f):
        self.setting(s, f)
        for _ in range(int(self.rs.choice([0, 0, 1, 2]))):
            self.emit(self.quiet())
        self.emit(self.op_of(f))

    def refuse(self):
        self.emit(("refused", *self.refused()))
        self.emit(("read", *self.window(2000)))

    def extra(self):
        rs = self.rs
        if rs.randint(0, 6) == 0:
            self.refuse()
            return
        f = self.following[int(rs.randint(0, len(self.following)))]
        if f in ("camodc", "qcomp") and self.M == 0:
            f = "h"
        self.emit(self.op_of(f))


def generate_sharded(ob, seed):
    """(ShardedConfig, ops) of one seed of the sharded family; an op of the list is (0, op tuple), as generate() gives them"""
    cfg = ShardedConfig(seed)
    rs = np.random.RandomState(15485863 * seed + 101)
    g = _ShGen(ob, cfg, rs)
    if "sharded" not in _SCHEDULE:
        _SCHEDULE["sharded"] = _sh_schedule()
    probes = list(_SCHEDULE["sharded"][seed])
    rs.shuffle(probes)
    for s, f in probes:
        g.probe(s, f)
        if rs.randint(0, 8) == 0:
            g.emit(("read", 0, g.dim))
        if rs.randint(0, 6) == 0:
            g.refuse()
        if rs.randint(0, 10) < 2:
            g.extra()
    while len(g.ops) < 40:
        g.extra()
    g.probe("swapped_layout", "read")                    # every list trades at least once and reads under a swapped layout
    g.emit(("read", 0, g.dim))
    return cfg, [(0, op) for op in g.ops]


def sh_pairs_reached(cfg, ops):
    """pairs_reached for one sharded register, judged on the op list alone: {(setting kind, following kind): count}, a pair
    counting when nothing but quiet calls (QUIET_SH) stand between the two.  swapped_layout: a flush right behind an H on a
    shard-id qubit that was queued in the identity layout with no basis state pending (that H cannot run without a trade)"""
    L, M, Cn, a = cfg.shape
    n, dim = L + M, 1 << (L + M)
    mode, pending, identity = cfg.mode, False, True         # identity: the layout is known to be the identity
    was_identity = True                                     # ... and was before the previous op
    kinds = []
    for i, op in enumerate(ops):
        k, s = op[0], None
        if k == "reset": s = "reset"
        elif k == "measure": s = "measure_state"
        elif k == "fill": s = "fill"
        elif k == "load": s = "load"
        elif k == "write":
            if op[2] < dim: s = "write_partial"
            elif op[4] == "negzero": s = "write_full_negzero"
        elif k == "flush" and i and ops[i - 1][0] == "h" and ops[i - 1][1] >= n - cfg.k and was_identity and not pending:
            s = "swapped_layout"
        elif k == "qcomp" and i and ops[i - 1][0] == "reset" and mode >= 0 and cfg.compact: s = "compact"
        elif k in QUEUED:
            s = "queued_behind_basis" if pending else "queued"
        kinds.append(s)
        if k == "fusion": mode = op[1]
        if k == "reset": pending = mode >= 0
        elif k in QUIET_SH or k in QUEUED: pass
        else: pending = False
        was_identity = identity
        if k in RESTORES_IDENTITY: identity = True
        elif k in QUEUED: identity = False                  # (a queued gate may cost a trade when it runs)
    out = {}
    for i, s in enumerate(kinds):
        if s is None:
            continue
        for op in ops[i + 1:]:
            if op[0] in FOLLOWING_SH:
                out[(s, op[0])] = out.get((s, op[0]), 0) + 1
            if op[0] not in QUIET_SH:
                break
    return out
