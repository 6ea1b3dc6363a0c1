/*
 * qcx.h -- C ABI of libqcx.so: the MI355X (gfx950) state-vector gate engine that
 * replaces the gate-application path of adamalderton/QuantumComputer's
 * qc_shor.c (cited as Q:line).  Plain C, plain pointers and sizes; no GSL, no
 * torch types.  The library is HIP only: every entry point that computes
 * returns QCX_HIP_ERROR when no gfx950 device is usable -- there is no CPU
 * fallback.
 *
 * The reference has no library interface (every function is `static`, only
 * `main` is exported, Q:242-1284); the seam this ABI fills is the set of
 * gate/state functions the circuit builders call (Q:683, Q:687, Q:721, Q:729,
 * Q:922-923, Q:928) plus the allocation block in main (Q:1316-1333).
 * include/qcx_compat.h re-creates the reference's own names and signatures on
 * top of this header so that the bodies of inverse_QFT / quantum_computation
 * compile unchanged.
 *
 * Conventions kept from the reference
 *   - qubit b is bit b of the state index (LSB = qubit 0, GET_BIT Q:150-151);
 *     the M register is bits [0,M), the L register bits [M,M+L) (Q:620-652).
 *   - amplitudes are interleaved (re, im) binary64, index ascending (Q:405-406).
 *   - status values 0..4 are the reference's ErrorCode (Q:164-170).
 * Differences
 *   - gates return int status instead of void (a bad qubit index is an error
 *     here; the reference silently computes garbage);
 *   - the `gsl_spmatrix_complex *matrix` scratch argument is gone (no matrix is
 *     ever built); qcx_compat.h accepts and ignores it;
 *   - one state buffer, updated in place; swap_states is a no-op.
 * All gate calls are asynchronous on the register's HIP stream; read-back,
 * measurement and qcx_synchronize() wait.
 * Threads: distinct registers may be used from distinct threads at the same time (the per-device scratch is locked);
 *   one register is used by one thread at a time -- the caller serialises calls on the same handle;
 *   the launch knobs (qcx_tune_set) are process-wide: do not change them while another thread is inside the library.
 */
#ifndef QCX_H
#define QCX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Q:164-170 ErrorCode, extended */
enum {
    QCX_NO_ERROR            = 0,
    QCX_INSUFFICIENT_MEMORY = 1,
    QCX_BAD_ARGUMENTS       = 2,
    QCX_PERIOD_NOT_FOUND    = 3,
    QCX_UNKNOWN_ERROR       = 4,
    QCX_HIP_ERROR           = 5,   /* HIP runtime / no device */
    QCX_BAD_QUBIT           = 6,   /* qubit index >= num_qubits, or control == target */
    QCX_UNSUPPORTED         = 7    /* valid request this build cannot serve */
};

typedef struct qcx_register qcx_register;   /* replaces Register, Q:194-203 */
typedef struct qcx_rng      qcx_rng;        /* replaces gsl_rng (mt19937), Q:1296-1299 */

const char *qcx_version(void);
const char *qcx_status_string(int status);
const char *qcx_last_error(void);      /* detail of the calling thread's last failure (HIP error string, file name ...) */
int  qcx_device_count(int *count);
int  qcx_set_device(int device);

/* ---- register lifecycle: replaces Q:1316-1324 / Q:1330-1332 -------------- */
int  qcx_register_create(int L_size, int M_size, qcx_register **out);
int  qcx_register_destroy(qcx_register *reg);
unsigned      qcx_num_qubits(const qcx_register *reg);   /* Register.num_qubits */
unsigned long qcx_num_states(const qcx_register *reg);   /* Register.num_states */
int  qcx_L_size(const qcx_register *reg);
int  qcx_M_size(const qcx_register *reg);
/* The same register sharded over `nshards` = 2, 4, 8 or 16 GPUs by THIS process (shard = top log2(nshards)
 * index bits).  The handle is an ordinary qcx_register: every function of this header works on it, so the reference's
 * circuit builders and main (Q:678-737, Q:1284-1347) run unchanged on the 8 GPUs of a node.  A Hadamard on a qubit held
 * in the shard id costs one exchange: each GPU's pack pass stores straight into its peers' buffers over xGMI.
 * devices[r] = HIP device of shard r (entries may repeat: several shards on one GPU).  NULL: the shards are spread over
 * the visible devices (qcx_spread_devices: 8 shards on 8 GPUs = shard r on device r, on 4 GPUs two neighbours per GPU,
 * on one GPU all on device 0).
 * Setting QCX_SHARDS=N in the environment makes qcx_register_create do this by itself (QCX_SHARD_DEVICES="0,1,..").
 * Pre-flight check: when the shards sit on more than one device, creation first trades a small register there and back
 * on the same devices and compares every amplitude, bit for bit, with what the layout says it must be; on a mismatch
 * creation fails with QCX_HIP_ERROR and qcx_last_error() names the shard (QCX_SHARD_SELFCHECK=0 skips, =1 forces the
 * check; qcx_sharded_set_relays runs it again through the relays).
 * M_size > 12 works like on one GPU (the modular multiply then runs in place through a per-device staging buffer instead of
 * LDS tiles; M_size <= 26).  Not available on a sharded register: qcx_register_set_stream, qcx_device_pointer (NULL),
 * the event pool, qcx_one_qubit_gate / qcx_c_one_qubit_gate, qcx_two_qubit_gate / qcx_c_two_qubit_gate,
 * qcx_mc_one_qubit_gate / qcx_mc_two_qubit_gate, qcx_pauli_rotation, qcx_pauli_rotation_batch, qcx_gate_batch (QCX_UNSUPPORTED). */
int  qcx_register_create_sharded(int L_size, int M_size, unsigned nshards, const int *devices, qcx_register **out);
int  qcx_spread_devices(unsigned nshards, int visible_devices /* <= 0: ask HIP */, int *devices_out /* [nshards] */);
int  qcx_sharded_selfcheck(qcx_register *reg);             /* the pre-flight exchange check on demand */
unsigned long qcx_sharded_selfchecks(const qcx_register *reg);   /* checks this register has passed */
unsigned qcx_register_shards(const qcx_register *reg);      /* 1 for an unsharded register */
int  qcx_sharded_stats(qcx_register *reg, unsigned long *exchanges, unsigned long *pack_passes);
/* Multi-path striping for fewer shards than GPUs on the node: the listed GPUs (which hold no shard)
 * relay a share of every chunk of every trade, so that a pair of shards exchanges over several xGMI links instead of its
 * one direct link.  nrelays = 0 turns it off (default; QCX_SHARD_RELAYS="4,5,6,7" sets it at creation).  Results are
 * the same bits either way. */
int  qcx_sharded_set_relays(qcx_register *reg, unsigned nrelays, const int *devices);
/* launch on a caller-owned hipStream_t (NULL = the register's own stream) */
int  qcx_register_set_stream(qcx_register *reg, void *hip_stream);
int  qcx_synchronize(qcx_register *reg);

/* ---- gate layer ----------------------------------------------------------- */
int  qcx_reset_register(qcx_register *reg);                                        /* Q:318-324 */
int  qcx_hadamard_gate(unsigned qubit_num, qcx_register *reg);                     /* Q:442-484 */
int  qcx_c_phase_shift_gate(unsigned c_qubit_num, unsigned qubit_num, double theta,
                            qcx_register *reg);                                    /* Q:513-565 */
int  qcx_c_amodc_gate(unsigned C, unsigned long long atox, unsigned c_qubit_num,
                      qcx_register *reg);                                          /* Q:595-660 */
/* Any one-qubit gate, plain or controlled by qubit c_qubit_num (no reference counterpart; the construction of hadamard_gate
 * and c_phase_shift_gate, Q:456-481 / Q:529-562, with four free complex entries, applied as the reference's mat-vec applies
 * every gate, Q:393-413; tests/one_qubit_ref.py restates it in numpy).
 *   u = 8 doubles, row-major: u00r, u00i, u01r, u01i, u10r, u10i, u11r, u11i.  For every index pair (i0, i1 = i0 | 2^qubit_num)
 *   with bit qubit_num of i0 clear, a = amp[i0], b = amp[i1], every fl() one binary64 rounding, no FMA, the triplets in column
 *   order (Q:396-413):
 *     lo.re = fl( fl(0.0 + fl(fl(u00r*a.re) - fl(u00i*a.im))) + fl(fl(u01r*b.re) - fl(u01i*b.im)) )
 *     lo.im = fl( fl(0.0 + fl(fl(u00r*a.im) + fl(u00i*a.re))) + fl(fl(u01r*b.im) + fl(u01i*b.re)) )
 *     hi.*  = the same with u10 for u00 and u11 for u01;   amp[i0] = lo, amp[i1] = hi.
 *   All four entries count as stored triplets, entries that are exactly zero included (0 * Inf = NaN, as in the reference).
 *   The controlled form does this to the pairs whose bit c_qubit_num is set; every other amplitude takes the reference's
 *   identity row (fl(0.0 + fl(fl(1*x) - fl(0*y))), fl(0.0 + fl(fl(1*y) + fl(0*x)))) -- on a finite state without -0 the value
 *   unchanged, so those amplitudes are not touched; a register flagged non-finite has them rewritten by a strict pass (K9).
 *   With H's entries (M_SQRT1_2) the plain gate gives qcx_hadamard_gate's bits, controlled with diag(1, qcx_polar(theta))
 *   qcx_c_phase_shift_gate's.
 * The matrix is applied as given and NOT checked for unitarity; each of the 8 components must be finite with absolute value
 * <= 1, which every unitary satisfies (else QCX_BAD_ARGUMENTS).  The 2^500 bound behind the non-finite flag (qcx_state_write)
 * covers any sane sequence of such gates; a caller who keeps applying norm-growing matrices is outside the overflow guarantee.
 * Asynchronous like the other gates.  In every fusion mode the call flushes what is pending (queued gates, a pending basis
 * state, a circuit's compact result) and launches its own kernel: it never enters the queue, qcx_fusion_stats does not count
 * it (the statistics move by what qcx_flush alone would have counted there: the queued gates' passes, a front, the deferred
 * last pass of a circuit's compact chain), and in mode 2 the gate itself stays exact.
 * NULL reg or u: QCX_BAD_ARGUMENTS; a qubit >= n or c_qubit_num == qubit_num: QCX_BAD_QUBIT; a sharded register:
 * QCX_UNSUPPORTED, nothing touched. */
int  qcx_one_qubit_gate(unsigned qubit_num, const double *u, qcx_register *reg);
int  qcx_c_one_qubit_gate(unsigned c_qubit_num, unsigned qubit_num, const double *u, qcx_register *reg);
/* Any two-qubit gate, plain or controlled by qubit c_qubit_num (no reference counterpart; a general 4x4 complex matrix applied
 * as the reference's mat-vec applies every gate, Q:393-413; tests/two_qubit_ref.py restates it in numpy and IS the definition).
 *   u = 32 doubles, a 4x4 complex matrix, row-major, (re, im) per entry.  The matrix index is k = bit(qubit0) + 2 * bit(qubit1):
 *   qubit0 is bit 0 of the matrix index (the LSB convention of this library); "A on qubit0, B on qubit1" is kron(B, A).
 *   The reference accumulates a row's triplets in ascending state index, so with lo = min(qubit0, qubit1), hi = max(...):
 *   if qubit0 > qubit1 the matrix is first permuted to m = P u P (P = the index swap 1 <-> 2), else m = u.  For every i with
 *   bits lo and hi clear, x0 = amp[i], x1 = amp[i | 2^lo], x2 = amp[i | 2^hi], x3 = amp[i | 2^lo | 2^hi], and with every fl()
 *   one binary64 rounding, no FMA, for each row r = 0 .. 3:
 *     out_r.re = fl(fl(fl(fl(0.0 + P(r,0).re) + P(r,1).re) + P(r,2).re) + P(r,3).re),   out_r.im the same with .im,
 *     P(r,k).re = fl(fl(m[r][k].re * x_k.re) - fl(m[r][k].im * x_k.im))                                        (Q:409)
 *     P(r,k).im = fl(fl(m[r][k].re * x_k.im) + fl(m[r][k].im * x_k.re))                                        (Q:412)
 *   then x_r = out_r.  All 16 entries count as stored triplets, exact zeros included (0 * Inf = NaN, as in the reference); no
 *   special case for permutation, diagonal or tensor-product matrices.  A result is never -0.
 *   The controlled form does this to the quads whose bit c_qubit_num is set; every other amplitude takes the reference's
 *   identity row, exactly as for qcx_c_one_qubit_gate -- on a finite state without -0 the value unchanged, so those amplitudes
 *   are not touched; a register flagged non-finite has them rewritten by a strict pass.  Two controls: a Toffoli is the
 *   controlled CNOT matrix, a Fredkin the controlled SWAP.
 *   On finite states without -0: kron(I, U) gives qcx_one_qubit_gate(qubit0, U)'s bits, kron(U, I) those of qubit1,
 *   diag(1, 1, 1, e^{i theta}) qcx_c_phase_shift_gate's, and (qubit0, qubit1, V) the bits of (qubit1, qubit0, P V P).
 * The matrix is applied as given and NOT checked for unitarity; each of the 32 components must be finite with absolute value
 * <= 1 (else QCX_BAD_ARGUMENTS, the message names the component).  Asynchronous; flushes what is pending in every fusion mode
 * and launches its own kernel, never enters the queue, is not counted by qcx_fusion_stats, stays exact in mode 2 -- all as
 * qcx_one_qubit_gate.
 * NULL reg or u: QCX_BAD_ARGUMENTS; a qubit >= n or two of the qubits equal: QCX_BAD_QUBIT (so also every register too small to
 * name distinct qubits); a sharded register: QCX_UNSUPPORTED, nothing touched. */
int  qcx_two_qubit_gate(unsigned qubit0, unsigned qubit1, const double *u, qcx_register *reg);
int  qcx_c_two_qubit_gate(unsigned c_qubit_num, unsigned qubit0, unsigned qubit1, const double *u, qcx_register *reg);
/* A one- or two-qubit gate under any set of control qubits, of either polarity (no reference counterpart; tests/mc_gate_ref.py
 * restates it in numpy and IS the definition; K17, DESIGN s4.5m).
 *   ctrl_mask = the set of control qubits, ctrl_values (a subset of ctrl_mask) = the value each control must have: a set bit is
 *   an ordinary control, a clear bit a negative one (the gate fires where that qubit reads 0).
 *   The gate acts on the pairs (quads) whose index satisfies (i & ctrl_mask) == ctrl_values, and there it is, operation for
 *   operation, qcx_one_qubit_gate's (qcx_two_qubit_gate's) arithmetic: the same u layout, the same P u P rule for
 *   qubit0 > qubit1, every fl() one binary64 rounding, no FMA, exact zeros multiplied out.  Every other amplitude takes the
 *   reference's identity row, exactly as for qcx_c_one_qubit_gate -- on a finite state without -0 the value unchanged, so those
 *   amplitudes are not touched (with k controls at bit >= 3 only 2^-k of the state is read); a register flagged non-finite has
 *   them rewritten by a strict pass.  A Toffoli is X under two controls, a Fredkin SWAP under one, a Grover oracle Z under n - 1.
 *   So, bit for bit: ctrl_mask == 0 gives the plain gates; a mask of one bit, set in ctrl_values, gives qcx_c_one_qubit_gate /
 *   qcx_c_two_qubit_gate; diag(1, qcx_polar(theta)) under one positive control gives qcx_c_phase_shift_gate; and
 *   (ctrl_mask, qubit0, qubit1, V) gives the bits of (ctrl_mask, qubit1, qubit0, P V P).
 * Everything else is qcx_one_qubit_gate's contract: the matrix is applied as given; asynchronous, on the register's stream; in
 * every fusion mode the call flushes what is pending and launches its own kernel, never enters the queue, is not counted by
 * qcx_fusion_stats, stays exact in mode 2; a -0 the caller wrote is canonicalised first.  ctrl_mask == 0 and one positive
 * control ARE the calls above (the same kernels and launches) unless the knob mc_generic is 1.  qcx_mc_gate_plan in qcx_plan.h
 * is the launch rule on its own.
 * Checked in this order, before anything runs and with nothing touched: NULL reg or u: QCX_BAD_ARGUMENTS; a matrix component
 * that is not finite or above 1 in absolute value: QCX_BAD_ARGUMENTS (the message names it); ctrl_values & ~ctrl_mask != 0:
 * QCX_BAD_ARGUMENTS; a target >= n, two targets equal, a mask bit at or above n or on a target: QCX_BAD_QUBIT; a sharded
 * register: QCX_UNSUPPORTED. */
int  qcx_mc_one_qubit_gate(uint64_t ctrl_mask, uint64_t ctrl_values, unsigned qubit_num, const double *u, qcx_register *reg);
int  qcx_mc_two_qubit_gate(uint64_t ctrl_mask, uint64_t ctrl_values, unsigned qubit0, unsigned qubit1, const double *u, qcx_register *reg);
/* The rotation about a Pauli string, exp(-i theta/2 P) = cos(theta/2) I - i sin(theta/2) P, in ONE read and one write of the
 * state for any string (no reference counterpart; the matrix applied as the reference's mat-vec applies every gate, Q:393-413;
 * tests/pauli_rotation_ref.py restates it in numpy and IS the definition).  The string is qcx_pauli_expectation's pair of masks:
 * x_mask = the qubits that carry X or Y, z_mask = those that carry Z or Y, <i|P|j> = i^g (-1)^popcount(j & z_mask) for
 * j = i ^ x_mask, g = popcount(x_mask & z_mask) mod 4.
 *   (c, s) = qcx_polar(fl(theta / 2)) -- one sincos, as qcx_c_phase_shift_gate obtains its factor.
 *   (er, ei) = -i * i^g * s = (+0, -s), (s, +0), (+0, s), (-s, +0) for g = 0, 1, 2, 3; the entry of row i at column j is (er, ei)
 *   with its ONE non-zero component negated when popcount(j & z_mask) is odd; the zero component stays +0.
 *   Triplets are taken in ascending column order, products as Q:409 / Q:412, every fl() one binary64 rounding, no FMA, zero
 *   components multiplied out (0 * Inf = NaN, as in the reference):
 *     P(m, x).re = fl(fl(m.re*x.re) - fl(m.im*x.im)),   P(m, x).im = fl(fl(m.re*x.im) + fl(m.im*x.re))
 *   x_mask != 0: D = P((c, +0), amp[i]), O = P(entry, amp[j]);  new[i] = fl(fl(0.0 + D) + O) if i < j, else fl(fl(0.0 + O) + D),
 *   component-wise.  x_mask == 0: the one triplet m = (c, -s) where popcount(i & z_mask) is even, (c, s) where it is odd;
 *   new[i] = fl(0.0 + P(m, amp[i])).  The empty string is the global phase e^{-i theta/2} and still runs.
 *   Every amplitude is rewritten: a result is never -0, and an Inf or NaN reaches rows i and i ^ x_mask only, so a register
 *   flagged non-finite keeps its flag and runs the same kernel.
 *   On finite states: one letter on qubit q gives qcx_one_qubit_gate(q, .)'s bits with [[c, -is], [-is, c]] (X), [[c, -s], [s, c]]
 *   (Y), diag(c - is, c + is) (Z); two letters give qcx_two_qubit_gate's with c I - i s P built component by component, in either
 *   qubit order.
 * Asynchronous; flushes what is pending in every fusion mode and launches its own kernel, never enters the queue, is not counted
 * by qcx_fusion_stats, stays exact in mode 2 -- all as qcx_one_qubit_gate.
 * NULL reg or a theta that is not finite: QCX_BAD_ARGUMENTS; a mask bit at or above n: QCX_BAD_QUBIT; a sharded register:
 * QCX_UNSUPPORTED, nothing touched. */
int  qcx_pauli_rotation(uint64_t x_mask, uint64_t z_mask, double theta, qcx_register *reg);
/* A list of rotations -- a Trotter step -- in as few passes over the state as locality allows (K15b, DESIGN s4.5k).  The state
 * afterwards is, bit for bit, what the loop  for k: qcx_pauli_rotation(x_masks[k], z_masks[k], thetas[k], reg)  leaves, for any
 * list in any order, on finite and non-finite registers: each term has its own (c, s) = qcx_polar(fl(theta / 2)) and
 * qcx_pauli_rotation's arithmetic; theta = 0 still runs; no term is merged, reordered or skipped.  The terms need not commute.
 * The passes: a run of consecutive terms whose partners i ^ x_mask all stay inside one tile of 2^12 amplitudes -- index bits
 * 0-7 plus four more bits chosen from the strings themselves -- is applied in order while the tile sits in registers, one read
 * and one write of the state for up to W = qcx_pauli_rotation_batch_width() terms; Z letters never constrain a pass.  A term
 * with more than four X or Y letters on qubits 8 and up is a pass of its own, qcx_pauli_rotation's.
 * qcx_pauli_rotation_batch_plan in qcx_plan.h is the rule on its own; qcx_rotation_batch_last_stats reports the last call's
 * passes and how many of them were such single wide terms.
 * Everything else is qcx_pauli_rotation's contract: asynchronous, never queued, flushes what is pending in every fusion mode,
 * not counted by qcx_fusion_stats, exact in mode 2; a register flagged non-finite keeps its flag and runs the same kernels.
 * Checked in this order, before anything runs: NULL reg, or a NULL array with nterms > 0: QCX_BAD_ARGUMENTS; a theta that is not
 * finite: QCX_BAD_ARGUMENTS, qcx_last_error() names the term; a mask bit at or above n: QCX_BAD_QUBIT; a sharded register:
 * QCX_UNSUPPORTED -- nothing touched in any of these cases.  nterms = 0: QCX_NO_ERROR, nothing is launched and queued gates stay
 * queued. */
int  qcx_pauli_rotation_batch(qcx_register *reg, unsigned long nterms, const uint64_t *x_masks, const uint64_t *z_masks,
                              const double *thetas);
unsigned qcx_pauli_rotation_batch_width(void);   /* W: the most terms one pass applies; a build constant, 8 <= W <= 64 */
/* the last qcx_pauli_rotation_batch call on this register that passed its checks: passes = the plan's npasses (kernel launches:
 * reads and writes of the state), wide_terms = those of them that are one wide term */
int  qcx_rotation_batch_last_stats(qcx_register *reg, unsigned long *passes, unsigned long *wide_terms);
/* A list of one- and two-qubit gates -- a circuit layer -- in as few passes over the state as locality allows (K12b / K13b, DESIGN
 * s4.5l).  Gate k is qcx_one_qubit_gate(qubit0, u) (ntargets = 1, control < 0), qcx_c_one_qubit_gate(control, qubit0, u),
 * qcx_two_qubit_gate(qubit0, qubit1, u) (ntargets = 2) or qcx_c_two_qubit_gate(control, qubit0, qubit1, u), and the state
 * afterwards is, bit for bit, what the loop of those calls leaves: for any list in any order, on finite and non-finite registers,
 * zero signs included.  No gate is merged, reordered, skipped or special-cased; exact zeros in a matrix are multiplied out; with
 * qubit0 > qubit1 the matrix is taken as P u P exactly as qcx_two_qubit_gate takes it.
 * The passes: a run of consecutive gates whose targets all lie inside one tile of 2^12 amplitudes -- index bits 0-7 plus four more
 * bits chosen from the gates' targets -- is applied in order while the tile sits in registers, one read and one write of the
 * state.  A one-target gate costs 1 unit of a pass's W = qcx_gate_batch_width(), a two-target gate 4; controls never constrain a
 * pass.  qcx_gate_batch_plan in qcx_plan.h is the rule on its own; qcx_gate_batch_last_stats reports what the last call ran.
 * Everything else is qcx_one_qubit_gate's contract: asynchronous, never queued, flushes what is pending in every fusion mode, not
 * counted by qcx_fusion_stats, exact in mode 2; a -0 the caller wrote is canonicalised before the first launch.  A register
 * flagged non-finite keeps its flag and runs the list gate by gate through those calls' own paths (passes = ngates).
 * Checked in this order, before anything runs: NULL reg, or NULL gates with ngates > 0: QCX_BAD_ARGUMENTS; an ntargets that is
 * not 1 or 2: QCX_BAD_ARGUMENTS, qcx_last_error() names the gate; a matrix component (the first 8, or all 32) that is not finite
 * or above 1 in absolute value: QCX_BAD_ARGUMENTS, the message names gate and component; a qubit or control at or above n, or two
 * of a gate's qubits equal: QCX_BAD_QUBIT, the message names the gate; a sharded register: QCX_UNSUPPORTED -- nothing touched in
 * any of these cases.  ngates = 0: QCX_NO_ERROR, nothing is launched and queued gates stay queued. */
typedef struct qcx_gate {
    unsigned ntargets;        /* 1: u holds 8 doubles (qcx_one_qubit_gate's layout); 2: 32 doubles (qcx_two_qubit_gate's) */
    int      control;         /* < 0: none */
    unsigned qubit0, qubit1;  /* qubit1 ignored when ntargets == 1 */
    double   u[32];
} qcx_gate;
int  qcx_gate_batch(qcx_register *reg, unsigned long ngates, const qcx_gate *gates);
unsigned qcx_gate_batch_width(void);             /* W, in units: a build constant */
/* the last qcx_gate_batch call on this register that passed its checks: passes = kernel launches (reads and writes of the state;
 * the plan's npasses, or ngates on a register flagged non-finite), lds_gates = the gates of those passes with a target on
 * qubits 0-7, which exchange between threads -- through LDS, or inside the wave (the others never leave the thread's registers) */
int  qcx_gate_batch_last_stats(qcx_register *reg, unsigned long *passes, unsigned long *lds_gates);
/* A diagonal operator on the qubit range [first_qubit, first_qubit + num_qubits) from a table, in ONE read and one write of the
 * state (no reference counterpart; the matrix applied as the reference's mat-vec applies every gate, Q:393-413;
 * tests/diagonal_ref.py restates it in numpy and IS the definition; K18, DESIGN s4.5n).  d holds 2^num_qubits entries as
 * (re, im) pairs; entry k belongs to the amplitudes whose bits first_qubit .. first_qubit + num_qubits - 1 read k, qubit
 * first_qubit being bit 0 of k.  For every index i, with m = d[k(i)] and x = amp[i], every fl() one binary64 rounding, no FMA:
 *     new.re = fl(0.0 + fl(fl(m.re*x.re) - fl(m.im*x.im))),   new.im = fl(0.0 + fl(fl(m.re*x.im) + fl(m.im*x.re)))
 *   Zero components are multiplied out (0 * Inf = NaN, as in the reference).  Every amplitude is rewritten: a result is never
 *   -0, and an Inf or NaN stays in its own row, so a register flagged non-finite keeps its flag and runs the same kernel.
 *   num_qubits = 0 is the global factor d[0] and still runs.
 *   So, bit for bit: the table (c - is, c + is, ...) by parity gives qcx_pauli_rotation of a Z string; on finite states
 *   diag(u00, u11) gives qcx_one_qubit_gate, a 4-entry table qcx_two_qubit_gate with that diagonal, (1, qcx_polar(theta)) at
 *   entry 3 of a 2-qubit table qcx_c_phase_shift_gate, and -1 at the last entry of an n-qubit table Z under n - 1 controls.
 * qcx_diagonal_gate takes the table from host memory: it is copied into the library's scratch before the call returns, so the
 * caller may reuse d at once; num_qubits <= qcx_diagonal_host_max_qubits().  qcx_diagonal_gate_device takes 2^num_qubits complex
 * doubles in memory of the register's device, for any num_qubits <= n (a full-register diagonal): the range must lie in device
 * memory of that device and must not overlap the register's buffer (hipPointerGetAttributes and the address ranges), and the
 * library scans it on the device for the rule below before use -- one read of the table, a 4-byte copy and a sync of the
 * register's stream.  The caller guarantees that the table is complete when the call is made and stays unchanged until the
 * register's stream has passed the call.
 * Both are qcx_pauli_rotation's sequence: asynchronous, on the register's stream; flush queued gates, a pending basis state and
 * a compact circuit result in every fusion mode; never enter the queue, are not counted by qcx_fusion_stats, stay exact in
 * mode 2.  qcx_diagonal_plan in qcx_plan.h is the launch rule on its own; qcx_diagonal_last_stats reports the last call's form
 * (QCX_DIAG_* of qcx_plan.h) and its table's entries.
 * Checked in this order, before anything runs and with nothing touched: NULL reg or table: QCX_BAD_ARGUMENTS;
 * first_qubit + num_qubits > n: QCX_BAD_QUBIT; host form: num_qubits above the maximum: QCX_BAD_ARGUMENTS (the message points
 * to the device form); a component that is not finite or above 1 in absolute value: QCX_BAD_ARGUMENTS (host form: the message
 * names entry and component); device form: a range that is not device memory of the register's device, or that overlaps the
 * register: QCX_BAD_ARGUMENTS; a sharded register: QCX_UNSUPPORTED (the device form then checks the kind of memory only). */
int  qcx_diagonal_gate(unsigned first_qubit, unsigned num_qubits, const double *d, qcx_register *reg);
int  qcx_diagonal_gate_device(unsigned first_qubit, unsigned num_qubits, const void *d_device, qcx_register *reg);
unsigned qcx_diagonal_host_max_qubits(void);     /* a build constant: 20 (a 16-MiB table) */
/* the last qcx_diagonal_gate(_device) call on this register that passed its checks: form = the plan's, table_entries = 2^num_qubits */
int  qcx_diagonal_last_stats(qcx_register *reg, unsigned *form, unsigned long *table_entries);
/* A classical reversible function on the qubit range [first_qubit, first_qubit + num_qubits), |k> -> |perm[k]>, under any set
 * of controls of either polarity, in ONE pass over the amplitudes that fire (the general form of qcx_c_amodc_gate; the matrix
 * applied as the reference's mat-vec applies every gate, Q:393-413; tests/permutation_ref.py restates it in numpy and IS the
 * definition; K19, DESIGN s4.5o).  perm holds 2^num_qubits entries, a bijection of [0, 2^num_qubits); qubit first_qubit is bit 0
 * of k.  Index i fires when (i & ctrl_mask) == ctrl_values; the operator is the permutation matrix that sends a firing i to i
 * with its range bits k replaced by perm[k], and the identity on every other index.  Every row holds the one triplet (1, 0):
 * with x = old[source of the row], every fl() one binary64 rounding, no FMA,
 *     new.re = fl(0.0 + fl(fl(1.0*x.re) - fl(0.0*x.im))),   new.im = fl(0.0 + fl(fl(1.0*x.im) + fl(0.0*x.re)))
 *   On a finite state that is pure movement with -0 turned into +0: a register that holds finite amplitudes (its zeros are
 *   made +0 first, as for every exact gate) has the firing amplitudes moved by one kernel and nothing else touched.  A register
 *   flagged non-finite takes one strict pass that rewrites EVERY amplitude by the formula (an Inf or NaN poisons the other
 *   component of its amplitude, as under qcx_mc_one_qubit_gate) and keeps its flag.  The identity table (num_qubits = 0 is one)
 *   on a finite register launches no kernel.
 *   So, bit for bit on finite states: (1, 0) on one qubit is X, under controls CNOT and Toffoli; (0, 2, 1, 3) is SWAP, under
 *   a control Fredkin; k -> a k mod C below C on the low M bits under a control above them is qcx_c_amodc_gate.
 * The table is inverted on the host and copied into the library's scratch before the call returns, so the caller may reuse
 * perm at once.  qcx_pauli_rotation's sequence: asynchronous, on the register's stream; flushes queued gates, a pending basis
 * state and a compact circuit result in every fusion mode; never enters the queue, is not counted by qcx_fusion_stats, stays
 * exact in mode 2.  qcx_permutation_plan in qcx_plan.h is the launch rule on its own.
 * Checked in this order, before anything runs and with nothing touched: NULL reg or perm: QCX_BAD_ARGUMENTS; ctrl_values with
 * bits outside ctrl_mask: QCX_BAD_ARGUMENTS; first_qubit + num_qubits > n: QCX_BAD_QUBIT; a mask bit at or above n or inside
 * the range: QCX_BAD_QUBIT; num_qubits above qcx_permutation_max_qubits(): QCX_BAD_ARGUMENTS (the message states the maximum);
 * an entry >= 2^num_qubits or a value that occurs twice: QCX_BAD_ARGUMENTS (the message names the first such entry and its
 * value); a sharded register: QCX_UNSUPPORTED. */
int  qcx_permutation_gate(uint64_t ctrl_mask, uint64_t ctrl_values, unsigned first_qubit, unsigned num_qubits,
                          const uint32_t *perm, qcx_register *reg);
unsigned qcx_permutation_max_qubits(void);       /* a build constant: 12 (a tile of 2^12 amplitudes holds the range) */
/* the last qcx_permutation_gate call on this register that passed its checks: form = the plan's (QCX_PERM_* of qcx_plan.h),
 * moved = the number of k with perm[k] != k */
int  qcx_permutation_last_stats(qcx_register *reg, unsigned *form, unsigned long *moved);
/* A dense 2^k x 2^k matrix on the k = num_targets = 1 .. 5 distinct qubits targets[0 .. k), under any set of controls of either
 * polarity, in ONE pass over the amplitudes that fire: a circuit block fused into one operator costs one trip through memory
 * however many gates were multiplied into it (the matrix applied as the reference's mat-vec applies every gate, Q:393-413;
 * tests/multi_qubit_ref.py restates it in numpy and IS the definition; K20, DESIGN s4.5p).  u holds 2 * 4^k doubles, row-major,
 * (re, im) per entry; targets[j] is bit j of the matrix index (qcx_two_qubit_gate's convention).  The matrix is first permuted
 * to m = P u P, so that row and column c of m stand for the c-th amplitude of a group in ascending state index (for k = 2 the
 * index swap 1 <-> 2 where qubit0 lies above qubit1).  Index i fires when (i & ctrl_mask) == ctrl_values.  For every firing
 * group (the 2^k indices that differ in the target bits alone), with x_c its amplitudes in ascending index, every fl() one
 * binary64 rounding, no FMA, the sums started at 0.0 and taken over c ascending, exact zeros multiplied out:
 *     new_r.re = fl(... fl(fl(0.0 + fl(fl(m_r0.re*x_0.re) - fl(m_r0.im*x_0.im))) + fl(fl(m_r1.re*x_1.re) - fl(m_r1.im*x_1.im))) ...)
 *     new_r.im = fl(... fl(fl(0.0 + fl(fl(m_r0.re*x_0.im) + fl(m_r0.im*x_0.re))) + fl(fl(m_r1.re*x_1.im) + fl(m_r1.im*x_1.re))) ...)
 *   Every other amplitude takes the identity row (1, 0): on a register of finite amplitudes (its zeros are made +0 first, as
 *   for every exact gate) it is not touched; a register flagged non-finite takes one strict pass that rewrites EVERY amplitude
 *   by the formula and keeps its flag.  So, bit for bit on finite states: k = 1 and 2 are qcx_mc_one_qubit_gate and
 *   qcx_mc_two_qubit_gate (and ARE those calls, the same kernels and launches, unless the knob multi_generic is set);
 *   kron(I2, U4) on (t0, t1, t2) is qcx_two_qubit_gate(t0, t1, U4), and the 8x8 controlled(U4) is that gate under a control on
 *   t2.  The matrix is applied as given: it is not checked for unitarity; every component must be finite with |.| <= 1.
 * The matrix is permuted on the host and copied into the library's scratch before the call returns, so the caller may reuse
 * u at once.  qcx_mc_two_qubit_gate's sequence: asynchronous, on the register's stream; flushes queued gates, a pending basis
 * state and a compact circuit result in every fusion mode; never enters the queue, is not counted by qcx_fusion_stats, stays
 * exact in mode 2.  qcx_multi_gate_plan in qcx_plan.h is the launch rule on its own.
 * Checked in this order, before anything runs and with nothing touched: NULL reg, u or targets: QCX_BAD_ARGUMENTS; num_targets
 * 0 or above qcx_multi_qubit_max_targets(): QCX_BAD_ARGUMENTS (the message states the maximum); a component that is not finite
 * or exceeds 1 in absolute value: QCX_BAD_ARGUMENTS (the message names it); ctrl_values with bits outside ctrl_mask:
 * QCX_BAD_ARGUMENTS; a target >= n, two targets equal, or a mask bit at or above n or on a target: QCX_BAD_QUBIT; a sharded
 * register: QCX_UNSUPPORTED. */
int  qcx_mc_multi_qubit_gate(uint64_t ctrl_mask, uint64_t ctrl_values, unsigned num_targets, const unsigned *targets, const double *u,
                             qcx_register *reg);
unsigned qcx_multi_qubit_max_targets(void);      /* a build constant: 5 */
/* the last qcx_mc_multi_qubit_gate call on this register that passed its checks: form = the plan's (always QCX_PERM_LINES of
 * qcx_plan.h), num_targets = its k */
int  qcx_multi_qubit_last_stats(qcx_register *reg, unsigned *form, unsigned *num_targets);
int  qcx_swap_states(qcx_register *reg);                                           /* Q:242-249: no-op */
/* host-side gate schedules */
int  qcx_inverse_QFT(qcx_register *reg);                                           /* Q:678-690 */
/* atox per control qubit: intpow_mode 0 = exact a^(2^k) mod C, 1 = the
 * reference's 32-bit INT_POW(a, x) including its wrap (Q:158-159, Q:729) */
int  qcx_quantum_computation(unsigned C, unsigned a, int intpow_mode, qcx_register *reg); /* Q:712-737 */

/* e^{i theta} as the reference's gsl_complex_polar(1.0, theta) yields it under gcc -O2 + glibc: one sincos()
 * call (Q:526).  Hosts that compute the phase factor themselves (qcx_shard_phase) must use this. */
void qcx_polar(double theta, double *cos_out, double *sin_out);
/* qcx_polar per element: out_re_im[2k], out_re_im[2k + 1] = cos, sin of thetas[k] -- a phase table for qcx_diagonal_gate */
void qcx_polar_array(unsigned long count, const double *thetas, double *out_re_im);

/* the reference's INT_POW macro (Q:158-159) exactly as x86-64 gcc evaluates it, 32-bit wrap included */
unsigned qcx_ref_int_pow(double base, double power);

/* ---- gate fusion (no reference counterpart) ------------
 * Queued gates are executed as fused passes (one HBM round trip applies many gates to LDS-resident
 * tiles); in modes -1, 0 and 1 results are bit-identical to the per-gate kernels.  Every call that observes the state
 * flushes the queue; qcx_flush does so explicitly.  Behind reset_register + the front of quantum_computation (Hadamard layer,
 * multiply ladder) a flush may run on a COMPACT copy of the state -- only the M-register values of the ladder's orbit can hold
 * anything but +0 -- and a whole-circuit entry point may leave its result in that form: qcx_measure_state reads it there,
 * every other observer (qcx_flush included) first expands it into the register.  Same bits either way.
 *   enable =  0 (default): a gate call launches its own kernel; the whole-circuit entry points
 *                (qcx_inverse_QFT, qcx_quantum_computation) hand their complete gate list to the pass scheduler
 *   enable =  1: every gate call is queued
 *   enable = -1: strictly one kernel launch per gate, inside the whole-circuit entry points too
 *   enable =  2: TOLERANCE MODE, opt-in, NOT bit-exact: like 1, and every run of consecutive controlled phases that
 *                share a qubit (Q:682-689: all phases after H(l) share l) is merged into one diagonal -- one complex
 *                multiply per amplitude by the product of the factors of its set target bits, FMA allowed.  Amplitudes
 *                differ from the bit-exact modes by rounding only: |delta| <= 1e-14 * |amplitude| per merged diagonal
 *                (tests bound the whole n <= 16 circuits at 1e-12; north_star asks 1e-10); zero signs are not
 *                canonicalised.  On a sharded register (qcx_register_create_sharded) every shard's passes run in this mode. */
int  qcx_set_fusion(qcx_register *reg, int enable);
int  qcx_flush(qcx_register *reg);
/* passes_launched: fused passes plus circuit fronts executed (a front = the lazily pending basis state written together with
 * the closed-form prefix of the queue; also one that was generated inside its first pass); gates_fused: gates that went into
 * either.  Sharded register: passes_launched counts the fronts only (see qcx_sharded_stats), gates_fused is 0. */
int  qcx_fusion_stats(qcx_register *reg, unsigned long *passes_launched, unsigned long *gates_fused);

/* ---- measurement: Q:272-306 ----------------------------------------------- */
int  qcx_measure_state(qcx_register *reg, qcx_rng *rng, unsigned long *state_num);
int  qcx_measure_state_r(qcx_register *reg, double r, unsigned long *state_num);   /* r supplied */
/* K shots from the current state, NOT collapsed (no reference counterpart: Q:298-300 notes that the collapse could be left out to
 * measure one state repeatedly).  state_nums[i] is the index qcx_measure_state_r(reg, r_i) would return on this state, with r_i
 * the i-th draw qcx_rng_uniform(rng) makes (the _r form takes the r_i from the caller, in any order, repeats allowed): the
 * first index in 0 .. dim-2 whose sequential running sum fl(cum + |a|^2) reaches r_i, else dim-1; r_i <= 0 gives 0, NaN and
 * r_i above the total give dim-1.  So K shots of one state give, in order, the indices of K rounds of reset + circuit +
 * qcx_measure_state with the same rng.  The state is read once for all shots (DESIGN s4.5c).
 * The state, and every lazy form of it, is left exactly as it was: a pending basis state stays pending, a circuit's compact
 * result stays compact (a call that scanned it counts in qcx_compact_measure_stats, as a measurement does), a register written
 * with non-finite amplitudes keeps its strict gates.  Queued gates are flushed first.  shots = 0 does nothing (no draw);
 * NULL state_nums with shots > 0: QCX_BAD_ARGUMENTS; a sharded register: QCX_UNSUPPORTED, and no draw is made. */
int  qcx_sample_states(qcx_register *reg, qcx_rng *rng, unsigned long shots, unsigned long *state_nums);
int  qcx_sample_states_r(qcx_register *reg, const double *r, unsigned long shots, unsigned long *state_nums);
/* the last sample call on this register: whole-state scans launched (1 on the fast path, plus one per fallback shot; 0 for a
 * pending basis state), and shots a per-shot scan answered (shots the fast path could not vouch for, or every shot of a
 * register holding non-finite amplitudes) */
int  qcx_sample_last_stats(qcx_register *reg, unsigned long *state_scans, unsigned long *fallback_shots);
/* The exact outcome distribution of the qubits [first_qubit, first_qubit + num_qubits), the others summed out (no reference
 * counterpart; Table I of the reference's report estimates it from 100 shots).  probs[v], v < 2^num_qubits, is the sum of
 * p_i = fl(fl(re_i*re_i) + fl(im_i*im_i)) (Q:286, no FMA) over the indices i whose bits [first_qubit, first_qubit + num_qubits)
 * equal v, summed as ONE PAIRWISE TREE over the summed bits s_0 < s_1 < ...: level h adds the pairs of partial sums that differ
 * only in bit s_(h-1), lower bits reduced completely before higher ones (tests/marginal_ref.py restates it in numpy).  Inf and
 * NaN propagate by IEEE rules; +-0 give +0.  The state is read once (K10, DESIGN s4.5d; stage plan: qcx_plan.h).
 * The state, and every lazy form of it, is left as it was: a pending basis state with no gate queued is answered on the host
 * (no kernel); a circuit's compact result stays compact -- a range above the M register is read there in place (the call
 * counts in qcx_compact_measure_stats), a range that reaches into it is read from the expanded state.  Queued gates are flushed
 * first.  first_qubit + num_qubits > n: QCX_BAD_QUBIT; num_qubits > 30: QCX_UNSUPPORTED; NULL probs: QCX_BAD_ARGUMENTS; a
 * sharded register: QCX_UNSUPPORTED, nothing touched. */
int  qcx_marginal_probabilities(qcx_register *reg, unsigned first_qubit, unsigned num_qubits, double *probs);
/* the last marginal call on this register: source 0 = the register, 1 = the compact form in place, 2 = a pending basis state
 * (no kernel), 3 = the compact form expanded first; state_reads = the passes that read amplitudes (0 for a basis state) */
int  qcx_marginal_last_stats(qcx_register *reg, unsigned *source, unsigned long *state_reads);
/* Measure the qubits [first_qubit, first_qubit + num_qubits), keep the others, and collapse the state (no reference counterpart:
 * Q:272-306 measures the whole register).  Two passes over the state: the marginal above, then one collapse pass (DESIGN s4.5e;
 * tests/collapse_ref.py restates all of it in numpy).
 *   P[v], v < 2^num_qubits, is exactly what qcx_marginal_probabilities(reg, first_qubit, num_qubits, P) returns on this state.
 *   The outcome is the scan of Q:283-292 on P: cum = 0; for v = 0 .. 2^num_qubits - 2 in order cum = fl(cum + P[v]), the first
 *   v with cum >= r wins, none: 2^num_qubits - 1.  So r <= 0 gives 0, NaN and an r above the total give the last value;
 *   num_qubits = 0 has the single outcome 0.  qcx_measure_qubits takes r from one qcx_rng_uniform(rng) draw;
 *   qcx_postselect_qubits takes the outcome from the caller (outcome >= 2^num_qubits: QCX_BAD_ARGUMENTS).
 *   *probability (may be NULL) receives P[outcome], bit for bit, whether or not the collapse then happens.
 *   Collapse: with s = fl(1 / fl(sqrt(P[outcome]))) (binary64, on the host) every amplitude whose bits [first_qubit,
 *   first_qubit + num_qubits) equal the outcome becomes (fl(re * s), fl(im * s)) -- two separately rounded products, no FMA,
 *   IEEE signs: a -0 stays -0 -- and every other amplitude (+0, +0); those are written without being read.  If P[outcome] is
 *   not a finite number > 0 (or s is not finite) nothing is written, the state and its lazy forms stay as they were, and the call
 *   returns QCX_BAD_ARGUMENTS with a qcx_last_error() that names the outcome and its probability; *outcome and *probability are
 *   still set.
 * Queued gates are flushed first.  A pending basis state with no gate queued is answered on the host (P = 1 at its range value,
 * s = 1: it stays pending, no kernel; any other post-selected value is the P = 0 error).  A circuit's compact result is read by
 * the marginal as described there, then expanded into the register and collapsed there.  A register flagged non-finite keeps its
 * flag.  Afterwards the state is an ordinary one in the register's buffer, and every following call behaves as if it had been
 * written with qcx_state_write (it may hold -0: the next gate canonicalises it as it does caller data).
 * first_qubit + num_qubits > n: QCX_BAD_QUBIT; num_qubits > 30: QCX_UNSUPPORTED; NULL reg, outcome (measure forms) or rng:
 * QCX_BAD_ARGUMENTS; a sharded register: QCX_UNSUPPORTED, nothing touched, no draw made. */
int  qcx_measure_qubits_r(qcx_register *reg, unsigned first_qubit, unsigned num_qubits, double r,
                          unsigned long *outcome, double *probability);
int  qcx_measure_qubits(qcx_register *reg, qcx_rng *rng, unsigned first_qubit, unsigned num_qubits,
                        unsigned long *outcome, double *probability);
int  qcx_postselect_qubits(qcx_register *reg, unsigned first_qubit, unsigned num_qubits, unsigned long outcome,
                           double *probability);
/* the last measure_qubits / postselect_qubits call on this register: source 0 = the register, 2 = a pending basis state (no
 * kernel), 3 = a compact result expanded first; state_reads = the passes that read amplitudes for the probabilities (the
 * marginal's count); state_writes = collapse passes launched (0 or 1) */
int  qcx_collapse_last_stats(qcx_register *reg, unsigned *source, unsigned long *state_reads, unsigned long *state_writes);
/* <psi|P|psi> for a Pauli string P, exactly, from one read of the state (no reference counterpart).  The string is two masks
 * over the n qubits: x_mask = the qubits that carry X or Y, z_mask = those that carry Z or Y (Y sits on x_mask & z_mask).  With
 * g = popcount(x_mask & z_mask) mod 4, a = amp[i], b = amp[i ^ x_mask] and every fl() one binary64 rounding (no FMA),
 *   t      = g even ? fl(fl(a.re*b.re) + fl(a.im*b.im)) : fl(fl(a.im*b.re) - fl(a.re*b.im))
 *   leaf_i = fl(0.0 + (odd ? -t : t)),  odd = (popcount((i ^ x_mask) & z_mask) + (g >> 1)) & 1
 * and *value is the marginal's ONE PAIRWISE TREE over all n index bits, lowest first, on these leaves (tests/pauli_ref.py
 * restates it in numpy; with both masks 0 it is qcx_marginal_probabilities(reg, 0, 0, ..) bit for bit).  Inf and NaN propagate
 * by IEEE rules; a result is never -0.  The state is read once, every amplitude once, whatever the string (K14, DESIGN s4.5h).
 * The state, and every lazy form of it, is left exactly as it was: a pending basis state k with no gate queued is answered on
 * the host (no kernel): x_mask == 0 gives +-1.0 by the parity of popcount(k & z_mask), any other string +0.0; a circuit's
 * compact result stays compact and is read from the expanded state (the register's buffer gets it first).  Queued gates are
 * flushed first.  Nothing is written to the state, so a register flagged non-finite keeps its flag and needs nothing special.
 * qcx_pauli_expectation_sum: one pass per term, in order; values[k] (values may be NULL) is term k's value and
 *   *total = acc after  acc = 0.0; for k in order: acc = fl(acc + fl(coeffs[k] * values[k])).  nterms = 0 gives +0.0 and launches
 *   nothing (queued gates stay queued).
 * NULL reg, value or total, or a NULL x_masks / z_masks / coeffs with nterms > 0: QCX_BAD_ARGUMENTS; a mask bit at or above n
 * (in any term: checked before anything runs): QCX_BAD_QUBIT; a sharded register: QCX_UNSUPPORTED, nothing touched. */
int  qcx_pauli_expectation(qcx_register *reg, uint64_t x_mask, uint64_t z_mask, double *value);
int  qcx_pauli_expectation_sum(qcx_register *reg, unsigned long nterms, const uint64_t *x_masks, const uint64_t *z_masks,
                               const double *coeffs, double *values /* [nterms], may be NULL */, double *total);
/* qcx_pauli_expectation_sum with the terms that SHARE an x_mask served by one read of the state (K14b, DESIGN s4.5h): what a
 * term's leaf takes from the amplitudes depends on x_mask alone, z_mask only picks one of two sums and a sign, and each term
 * keeps its own tree.  values[k] and *total are, bit for bit, what qcx_pauli_expectation_sum gives for the same arguments on
 * the same state, and everything it documents holds here -- checks, NULLs, nterms = 0, the lazy forms (a compact result is
 * expanded once per call), errors.  The passes: walk the terms in order; term k joins the open pass of its x_mask while that
 * holds fewer than W = qcx_pauli_batch_width() terms, otherwise it opens a new pass; passes run in the order they were opened,
 * each one read of the state (qcx_pauli_batch_plan in qcx_plan.h is this rule on its own).  The all-Z strings of an Ising or
 * Heisenberg model share x_mask = 0.  qcx_expectation_last_stats reports the reads of this call: one per pass. */
int  qcx_pauli_expectation_batch(qcx_register *reg, unsigned long nterms, const uint64_t *x_masks, const uint64_t *z_masks,
                                 const double *coeffs, double *values /* [nterms], may be NULL */, double *total);
unsigned qcx_pauli_batch_width(void);   /* W: the most terms one read of the state serves; a build constant, 8 <= W <= 64 */
/* the last pauli_expectation / pauli_expectation_sum / pauli_expectation_batch call on this register: source 0 = the register,
 * 2 = a pending basis state (no kernel), 3 = a compact result expanded first; state_reads = the passes that read amplitudes:
 * one per term, or per pass of the batch call (0 for a basis state) */
int  qcx_expectation_last_stats(qcx_register *reg, unsigned *source, unsigned long *state_reads);
/* The reduced density matrix of the qubits [first_qubit, first_qubit + num_qubits), the others traced out, exactly, from one read
 * of the state (no reference counterpart; tests/rdm_ref.py restates it in numpy and IS the definition).  rho holds
 * 2 * 4^num_qubits doubles, row-major, (re, im) per entry, row v and column w in 0 .. 2^num_qubits - 1:
 *   rho[v][w] = sum over r of amp[r, v] * conj(amp[r, w]),
 * r running over the values of the n - num_qubits qubits outside the range, amp[r, v] the amplitude whose range bits are v and
 * whose other bits are r.  first_qubit is bit 0 of v (the LSB convention of this library, as qcx_two_qubit_gate's kron(B, A)).
 * The leaves are qcx_pauli_expectation's arithmetic: for v < w, a = amp[r, v], b = amp[r, w], every fl() one binary64 rounding,
 * no FMA,
 *   re-leaf = fl(0.0 + fl(fl(a.re*b.re) + fl(a.im*b.im))),   im-leaf = fl(0.0 + fl(fl(a.im*b.re) - fl(a.re*b.im)));
 * for v = w the re-leaf is the same expression -- qcx_marginal_probabilities' p_i -- and the imaginary part of a diagonal entry is
 * +0.0 by contract, not computed.  Each computed component (re or im) is the marginal's ONE PAIRWISE TREE over its leaves, over
 * the summed bits s_0 < s_1 < ... (every bit outside the range), lowest first: tests/marginal_ref.py's tree for the same
 * (first_qubit, num_qubits).  The lower triangle is the conjugate of the upper one: rho[w][v].re = rho[v][w].re,
 * rho[w][v].im = fl(0.0 - rho[v][w].im), so that a zero stays +0.  Inf and NaN propagate by IEEE rules in the computed
 * components; a result is never -0; num_qubits = 0 gives the 1 x 1 matrix (norm^2, +0).  Hence rho[v][v].re is
 * qcx_marginal_probabilities(reg, first_qubit, num_qubits)[v] bit for bit, and for one qubit q on a finite state 2 rho[0][1].re
 * and -2 rho[0][1].im are qcx_pauli_expectation's values of X_q and Y_q (up to the sign of a zero).
 * The state is read once, every amplitude once, wherever the range lies (K16, DESIGN s4.5j; stage plan: qcx_plan.h).
 * The state, and every lazy form of it, is left exactly as it was, and nothing is written to the state: queued gates are flushed
 * first; a pending basis state k with no gate queued is answered on the host (no kernel): (1, +0) at [v_k][v_k], v_k the range
 * value of k, +0 everywhere else; a circuit's compact result stays compact and is read from the expanded state (the register's
 * buffer gets it first); a register flagged non-finite keeps its flag and needs nothing special.
 * Checked in this order, before anything runs: NULL reg or rho: QCX_BAD_ARGUMENTS; a sharded register: QCX_UNSUPPORTED, nothing
 * touched; first_qubit + num_qubits > n: QCX_BAD_QUBIT; num_qubits > qcx_rdm_max_qubits(): QCX_UNSUPPORTED. */
int  qcx_reduced_density_matrix(qcx_register *reg, unsigned first_qubit, unsigned num_qubits, double *rho);
unsigned qcx_rdm_max_qubits(void);   /* the widest range one call serves; a build constant, >= 4 */
/* the last qcx_reduced_density_matrix call on this register: source 0 = the register, 2 = a pending basis state (no kernel),
 * 3 = a compact result expanded first; state_reads = the passes that read amplitudes: 1, or 0 for a basis state */
int  qcx_rdm_last_stats(qcx_register *reg, unsigned *source, unsigned long *state_reads);

/* ---- state access (replaces gsl_vector_complex_get/set uses, T:7-37) ------- */
int  qcx_state_read(qcx_register *reg, unsigned long first, unsigned long count, double *out_re_im);
int  qcx_state_write(qcx_register *reg, unsigned long first, unsigned long count, const double *in_re_im);
int  qcx_norm2(qcx_register *reg, double *total_probability);                      /* T:28-37, summed as a tree (fast) */
/* the same total with the reference's own summation order (index-ascending, one addition per amplitude): the bits
 * check_normalisation prints (T:28-37) */
int  qcx_total_probability(qcx_register *reg, double *total_probability);
/* State files (golden vectors, debugging, checkpoint): a 64-byte header ("QCXSTATE", version,
 * L, M, 2^n, FNV-1a 64 checksum) followed by the amplitudes as interleaved little-endian binary64 (re, im).  Streamed
 * in 64 MiB pieces.  Load requires a register of the same L and M and verifies the checksum. */
int  qcx_state_save(qcx_register *reg, const char *path);
int  qcx_state_load(qcx_register *reg, const char *path);
/* The amplitude buffer in HBM (for interop).  Flushes first.  Its contents are the register's state only after qcx_flush,
 * qcx_synchronize or a fresh call of this function: reset_register and the collapse of measure_state are lazy, and fused
 * passes may alternate between two buffers.  Calling it pins the state to the returned buffer from then on (the register
 * stops chaining passes through its second buffer), so the pointer stays valid until the register is destroyed.  NULL for a
 * sharded register. */
void *qcx_device_pointer(qcx_register *reg);
/* synthetic input for benches and full-size tests: component k (k = 2*index + {0 re, 1 im}) is
 * ((splitmix64(seed + k) >> 11) * 2^-53 - 0.5) * sqrt(6 / 2^n); generated on the device */
int  qcx_state_fill_random(qcx_register *reg, uint64_t seed);

/* ---- HIP-event timing on the register's stream (bench / roofline) ---------- */
int  qcx_timer_start(qcx_register *reg);
int  qcx_timer_stop(qcx_register *reg, double *milliseconds);    /* waits for the stop event */
/* a pool of events: record between gates inside a timed region, read the differences afterwards */
int  qcx_events_create(qcx_register *reg, unsigned count);
int  qcx_event_record(qcx_register *reg, unsigned slot);
int  qcx_event_elapsed(qcx_register *reg, unsigned from_slot, unsigned to_slot, double *milliseconds);

/* ---- MT19937 with gsl_rng_mt19937 semantics (Q:1296-1299, Q:281) ----------- */
qcx_rng      *qcx_rng_alloc(void);
void          qcx_rng_set(qcx_rng *rng, unsigned long seed);    /* seed 0 -> 4357 like GSL */
unsigned long qcx_rng_get(qcx_rng *rng);
double        qcx_rng_uniform(qcx_rng *rng);                    /* get / 2^32 */
void          qcx_rng_free(qcx_rng *rng);

/* ---- beyond the boundary ---------------------------------------------------
 * Two further interfaces of the same library live in headers of their own and are included here for convenience:
 *   qcx_shard.h   the per-rank (shard-level) entry points on caller-owned device memory: what a one-process-per-GPU host
 *                 calls between its exchanges (quantumcomputer_amd/sharded.py), plus the compact-circuit helpers;
 *   qcx_plan.h    the fused-pass planner alone, on the host: a test and tooling interface (tests/fuse_emulator.py).
 * A program that replaces the reference's gate path needs neither. */
#ifdef __cplusplus
}
#endif
#include "qcx_shard.h"
#include "qcx_plan.h"
#endif /* QCX_H */
