/*
 * qcx_plan.h -- the fused-pass PLANNER of libqcx.so on its own, host code only (no GPU needed).  A test and tooling
 * interface: the CPU-only suite plans gate lists, interprets the returned records with a numpy restatement of the pass
 * kernels (tests/fuse_emulator.py) and compares with the oracle; tools/plan_cost.py prices plans.  Every pass comes with
 * the launch it would get -- kernel instantiation, grid, block, LDS bytes -- and qcx_pass_launch_plan answers that question
 * for one pass on its own (tests/test_pass_launch_plan.py).  Nothing a user of the gate engine needs.
 */
#ifndef QCX_PLAN_H
#define QCX_PLAN_H

#include <stddef.h>
#include <stdint.h>
#include "qcx_shard.h"          /* qcx_gate_desc */

#ifdef __cplusplus
extern "C" {
#endif

/* The pass planner alone, on the host (no GPU needed; test and tooling interface).  Cuts a gate list into actions --
 * fused passes over LDS tiles, or single gates that run as their stand-alone kernel -- and returns the records the
 * pass kernels interpret, 32 bytes each, all passes back to back.  Record formats: csrc/qcx_kernels.h (FuseOp and
 * the ROUNDS form); tests/fuse_emulator.py interprets them on the CPU and compares with the oracle.
 * Returns QCX_INSUFFICIENT_MEMORY (with the needed counts in n_actions / n_records) when an array is too small. */
typedef struct {
    uint32_t type, a;
    uint64_t mask;
    double   c, s;
} qcx_fuse_record;
typedef struct {
    int      fused;                 /* 0: the single gate first_gate, stand-alone kernel; 1: one fused pass */
    unsigned first_gate, ngates;    /* the gates of the list this action covers (in order, no gaps between actions) */
    unsigned T, c, nh;              /* tile = 2^T amplitudes: the c lowest index bits + nh higher bits hbit[0..nh) */
    unsigned char hbit[16];
    unsigned nopipe;                /* 1: phase-dominated pass, planned on the smaller tile (fuse_T_phase) */
    unsigned rounds_form;           /* 1: records in ROUNDS form (rounds / items / runs), 0: plain gate list */
    size_t   rec_off, rec_cnt;      /* this pass's records (tables included) inside `records` */
    unsigned nops;                  /* records the kernel walks (the rest, if any, are tables) */
    unsigned table_bytes, table_rec_off;    /* folded modular-multiply tables: size, and offset in records from rec_off */
    unsigned diag_cnt, diag_rec_off;        /* tolerance mode: merged diagonals of the pass, record offset of their table area */
    /* tile addressing (round 4).  tl[j] = the qubit that is tile-local bit j in the records.  A CHAINED pass (chained = 1) reads
     * the register's current buffer under one logical -> physical layout and writes the other buffer under another one: tile-local
     * bit j is input index bit in_pos[j]; the j-th lowest output position of the tile's bits is output index bit st_pos[j] and
     * belongs to tile-local bit st_loc[j]; bits [src, src + len) of the tile number go to index bits [dst, dst + len) of the
     * input / output / logical index (seg_in / seg_out / seg_lg).  In place (chained = 0): out = in = logical, seg_in only. */
    unsigned chained;
    unsigned char tl[16], in_pos[16], st_loc[16], st_pos[16];
    unsigned char nseg_in, nseg_out, nseg_lg, pad_;
    struct { unsigned char src, dst, len, pad; } seg_in[16], seg_out[16], seg_lg[16];
    /* how the pass would be launched (qcx_pass_launch_plan below, under the knobs of the moment, in place or chained as planned):
     * the kernel instantiation as a kernel trace spells it, e.g. "k_fused_x8<512, 12, false, false>", its grid and block, and
     * the dynamic LDS of a workgroup.  kernel = "" when the launch would be refused. */
    char     kernel[64];
    unsigned grid, block, lds_bytes;
} qcx_plan_action;
int  qcx_fusion_plan(unsigned n_local, unsigned M, unsigned count, const qcx_gate_desc *gates,
                     qcx_plan_action *actions, unsigned max_actions, unsigned *n_actions,
                     qcx_fuse_record *records, size_t max_records, size_t *n_records);
/* the same for a fusion mode: 1 = the bit-exact plan (what qcx_fusion_plan returns), 2 = the tolerance mode's plan;
 * | 4: as a register with a second buffer plans (runs of passes chained through it, see qcx_plan_action) */
int  qcx_fusion_plan_mode(int mode, unsigned n_local, unsigned M, unsigned count, const qcx_gate_desc *gates,
                          qcx_plan_action *actions, unsigned max_actions, unsigned *n_actions,
                          qcx_fuse_record *records, size_t max_records, size_t *n_records);

/* The launch of one fused pass, decided on the host: which kernel instantiation interprets the pass's records, with which grid,
 * block and dynamic LDS layout.  qcx_pass_launch_in is everything that decision reads: the fields below of the pass as planned
 * (FusePass, csrc/qcx_kernels.h) -- a flush adds gen, zskip, zpad, gen_tab_bytes and xp_on to what the planner sets -- the
 * register's shape, and what the launch knows about its buffers; plus the knobs of the moment (qcx_tune_set). */
typedef struct {
    unsigned n, M;                  /* the register: n index bits, the low M of them the M register */
    unsigned T;                     /* tile = 2^T amplitudes */
    unsigned rounds_form;           /* records in ROUNDS form */
    unsigned table_bytes;           /* folded modular-multiply tables behind the records */
    unsigned has_cam;               /* the pass holds modular multiplies */
    unsigned xm_cnt;                /* records whose outside-tile masks go to LDS */
    unsigned dg_cnt, dg_slim;       /* merged diagonals; 1: fast rounds only, 2: radix-8 fast rounds, 3: the exact walk on 8 amplitudes */
    unsigned chained;               /* reads one buffer, writes the other */
    unsigned gen;                   /* 1: tiles generated, 2 / 3: by columns (3: of a compact chain) */
    unsigned gen_tab_bytes, zpad;   /* by columns: the residue -> column table, the padded column count */
    unsigned zskip;
    unsigned xp_on;                 /* the expanding store of a compact chain's last pass */
    unsigned tables_cover;          /* the addressing tables deposit all n - T bits of the tile number */
    unsigned buffers_differ;        /* the launch got two different buffers */
} qcx_pass_launch_in;
typedef struct {
    char     kernel[64];            /* as in qcx_plan_action */
    unsigned grid, block, lds_bytes;
    unsigned waves;                 /* k_gen_cols: waves per workgroup (else 0) */
    unsigned xm_off, dg_lds_off, gen_lds_off, table_lds_off, dbg;   /* the FusePass fields the launch fills in (table_lds_off: cam_ctl_local[3]) */
    unsigned expanding_store_ok;    /* could this pass take the expanding store (asked of the pass with xp_on = 0, in place)? */
} qcx_pass_launch_out;
/* QCX_NO_ERROR and *out, or the status of the refusal with its text in qcx_last_error() (out->expanding_store_ok is set either way) */
int  qcx_pass_launch_plan(const qcx_pass_launch_in *in, qcx_pass_launch_out *out);

/* The stage plan of qcx_marginal_probabilities (include/qcx.h; K10, DESIGN s4.5d), on the host.  The marginal sums the bits
 * outside [first, first + num) as one pairwise tree, lowest summed bit first; each stage reduces the lowest summed bits that
 * are left, inside tiles of 2^T elements of its input: the c lowest index bits (whole 128-B runs: 8 amplitudes, 16 partials),
 * then summed bits above them, then -- once no summed bit is left outside the tile -- the lowest other bits, up to 2^12
 * elements (2^8 compact blocks).  A stage's output is indexed by its input's bits that it does not sum, in ascending order,
 * so the last stage's output is the marginal itself.  Non-final outputs lie back to back in the call's device scratch: at
 * most 1/512 of the state's bytes.  stages[] must hold QCX_MARGINAL_MAX_STAGES entries.  first + num > n: QCX_BAD_QUBIT;
 * num > 30: QCX_UNSUPPORTED. */
#define QCX_MARGINAL_MAX_STAGES 8
typedef struct {
    unsigned kind;              /* 0: reads the amplitudes; 1: reads the partials of the stage before; 2: reads a circuit's compact
                                 * result in place, one element per L-register block (its 2^M leaves summed first) */
    unsigned in_bits;           /* the input holds 2^in_bits elements */
    unsigned T, c;              /* a tile: 2^T elements, input index bits 0 .. c-1 among them */
    uint64_t tile_mask;         /* the input index bits of a tile */
    uint64_t sum_mask;          /* the input index bits this stage sums out (inside tile_mask) */
    uint64_t qubits;            /* the same bits as qubit numbers (kind 2: the M register's bits as well) */
    unsigned out_bits;          /* the output: 2^out_bits doubles */
    unsigned final_stage;       /* 1: the output is the marginal */
    uint64_t out_offset;        /* a non-final stage's output in the scratch, in doubles from its start */
} qcx_marginal_stage;
int  qcx_marginal_plan(unsigned n, unsigned first, unsigned num, qcx_marginal_stage *stages, unsigned *n_stages);
/* the same for a compact circuit result (M-register bits = the orbit residues, include/qcx.h): needs first >= M */
int  qcx_marginal_plan_compact(unsigned n, unsigned M, unsigned first, unsigned num, qcx_marginal_stage *stages, unsigned *n_stages);

/* The passes of qcx_pauli_expectation_batch (include/qcx.h), on the host: walk the terms in order; term k joins the open pass of
 * its x_mask while that holds fewer than `width` terms, otherwise it opens a new pass (a full pass is closed).  Passes are
 * numbered in the order they are opened; pass_of_term[k] is term k's.  The library calls it with width =
 * qcx_pauli_batch_width().  width = 0, a NULL npasses, or NULL arrays with nterms > 0: QCX_BAD_ARGUMENTS. */
int  qcx_pauli_batch_plan(unsigned long nterms, const uint64_t *x_masks, unsigned width,
                          unsigned long *pass_of_term /* [nterms] */, unsigned long *npasses);

/* The passes of qcx_pauli_rotation_batch (include/qcx.h; K15b, DESIGN s4.5k) over n qubits, on the host.  For term k let hx_k be
 * the bits of x_masks[k] at positions >= 8; the term is WIDE when popcount(hx_k) > 4.  Walk the terms in order; at most one pass
 * is open, with a hot set H and a term count:
 *   a wide term closes the open pass and is a pass of its own (kind 1: the qcx_pauli_rotation launch, hot mask 0);
 *   any other term joins the open pass if count < width and popcount(H | hx_k) <= 4, otherwise the open pass closes and the term
 *   opens a new one with H = hx_k (kind 0);
 *   on closing, H is padded with the lowest qubits of [8, n) not yet in it, up to min(4, max(n, 8) - 8) bits.
 * A kind-0 pass's tile is qubits 0-7 plus H: the whole register for n <= 12 (no term is wide, only `width` splits passes), and
 * for n >= 13 one tile per value of the other n - 12 bits.  pass_of_term[k] is term k's pass (non-decreasing), *npasses their
 * number, pass_kind[p] and pass_hot[p] pass p's kind and hot mask (all three arrays hold nterms entries).  The library calls it
 * with width = qcx_pauli_rotation_batch_width().  width = 0, n = 0 or n > 40, a NULL npasses, or a NULL array with nterms > 0:
 * QCX_BAD_ARGUMENTS; an x_mask bit at or above n: QCX_BAD_QUBIT. */
int  qcx_pauli_rotation_batch_plan(unsigned n, unsigned long nterms, const uint64_t *x_masks, unsigned width,
                                   unsigned long *pass_of_term /* [nterms] */, unsigned long *npasses,
                                   unsigned *pass_kind /* [nterms] */, uint64_t *pass_hot /* [nterms] */);

/* The passes of qcx_gate_batch (include/qcx.h; K12b / K13b, DESIGN s4.5l) over n qubits, on the host: qcx_pauli_rotation_batch_plan's
 * walk.  Gate k has its target qubits as the bits of target_masks[k] (controls do not count) and costs units[k]: 1 with one target,
 * 4 with two, the size of its record.  hx_k is target_masks[k]'s bits at positions >= 8 (at most two).  Walk the gates in order;
 * at most one pass is open, with a hot set H and the units used:
 *   a gate joins the open pass if used + units[k] <= width and popcount(H | hx_k) <= 4, otherwise the open pass closes and the
 *   gate opens a new one with H = hx_k.  A gate always fits an empty pass, whatever `width` is (width = 1 places a two-target gate
 *   in a pass of its own);
 *   on closing, H is padded with the lowest qubits of [8, n) not yet in it, up to min(4, max(n, 8) - 8) bits.
 * A pass's tile is qubits 0-7 plus H: the whole register for n <= 12 (only `width` splits passes), and for n >= 13 one tile per
 * value of the other n - 12 bits.  pass_of_gate[k] is gate k's pass (non-decreasing), *npasses their number, pass_hot[p] pass p's
 * hot mask (both arrays hold ngates entries).  The library calls it with width = qcx_gate_batch_width().  width = 0, n = 0 or
 * n > 40, a NULL npasses, a NULL array with ngates > 0, or a units[k] other than 1 or 4: QCX_BAD_ARGUMENTS; a target bit at or
 * above n, or a number of target bits that is not 1 for 1 unit and 2 for 4: QCX_BAD_QUBIT. */
int  qcx_gate_batch_plan(unsigned n, unsigned long ngates, const uint64_t *target_masks, const unsigned *units, unsigned width,
                         unsigned long *pass_of_gate /* [ngates] */, unsigned long *npasses, uint64_t *pass_hot /* [ngates] */);

/* The stage plan of qcx_reduced_density_matrix (include/qcx.h; K16, DESIGN s4.5j), on the host.  The 4^num computed components
 * (row v * 2^num + w, v <= w: Re rho[v][w]; row w * 2^num + v, v < w: Im rho[v][w]) are each the marginal's pairwise tree over
 * the bits outside [first, first + num).  Stage 0 reads the state once and sums, for every row, the sum_bits lowest summed
 * qubits (sum_mask, as qubit numbers: all of them below 12 qubits, else the 12 - num that share a unit of 2^12 amplitudes with the
 * range plus group_bits = min(n - 21, 4) more from 22 qubits on, a workgroup adding the roots of 2^group_bits units); its output is rows x row_stride doubles,
 * row-major, the column = the rest_bits summed qubits left, in ascending order.  stages[0 .. *n_stages) are the stages behind it:
 * ordinary marginal stages (kind 1) over that array as one input of rest_bits + 2 num index bits with the row number as the kept
 * high bits, so that all rows go through each launch together; *n_stages = 0 when stage 0 leaves nothing to sum.  Non-final
 * outputs lie back to back in the call's device scratch, stage 0's first (out_offset counts from the scratch's start):
 * `scratch` doubles in all, at most (1 + 2^-11) 2^(n + 2 num - 12 - group_bits) -- from 25 qubits on 2^(2 num - 17) (1 + 2^-11)
 * of the state's doubles, 32 MiB for four qubits of 30 --, and none for n <= 12.  stages[] must hold QCX_MARGINAL_MAX_STAGES entries.  first + num > n: QCX_BAD_QUBIT; num >
 * qcx_rdm_max_qubits(): QCX_UNSUPPORTED. */
typedef struct {
    uint64_t sum_mask;          /* the qubits stage 0 sums */
    unsigned sum_bits;          /* ... their number */
    unsigned group_bits;        /* ... of which a workgroup sums this many across consecutive units of 2^12 amplitudes */
    unsigned rest_bits;         /* summed qubits left behind stage 0 */
    unsigned rows;              /* 4^num */
    uint64_t row_stride;        /* 2^rest_bits: stage 0 writes component k of unit u to [k * row_stride + u] */
    uint64_t scratch;           /* doubles of all non-final outputs */
} qcx_rdm_stage0;
int  qcx_rdm_plan(unsigned n, unsigned first, unsigned num, qcx_rdm_stage0 *stage0, qcx_marginal_stage *stages, unsigned *n_stages);

/* The launch of qcx_mc_one_qubit_gate / qcx_mc_two_qubit_gate (include/qcx.h; K17, DESIGN s4.5m) on a register of n qubits, on the
 * host, under the knobs of the moment; the library launches from this very function.  ntargets = 1 (qubit1 ignored) or 2.
 * Work item p of `count` stands for the index
 *     i(p) = deposit(p) | or_const,
 * deposit = p's bits moved, in order, into the positions outside the squeezed runs [run_pos[k], run_pos[k] + run_len[k]),
 * k < nruns, ascending; squeezed are the controls at bit >= 3 (or_const = those of them that are positive) and the targets
 * that live in registers, so count = 2^(n - squeezed positions).  A lane acts when (i & low_mask) == low_values (controls below
 * bit 3); with store_all the lanes that do not act store the bits they read (whole lines go back).  Forms:
 *   QCX_MC_PAIR       one target, squeezed; a lane owns the pair (i, i | 2^q).  Target >= 3 and no control below 3
 *   QCX_MC_LINE_PAIR  the same with a predicate: a control below 3, target >= 3
 *   QCX_MC_LINE_SHFL  one target below 3, not squeezed: a lane owns i, the partner comes by xor-shuffle
 *   QCX_MC_QUAD       two targets, both squeezed; a lane owns the quad
 *   QCX_MC_LINES2     lo or a control below 3: ns = 2, 1 or 0 of the targets sit below bit 6 of the lane numbering and are
 *                     shuffled (xor masks shfl_lo, shfl_hi), the others are squeezed; ns = 0 is the quad with a predicate
 * The shuffle forms need whole waves: with count < 64, n < 9, or the knob ph_lines = 0 (two targets: also u2_variant = 1) the
 * call takes QCX_MC_PAIR / QCX_MC_QUAD with EVERY control squeezed (low_mask = 0), which is correct for any bit positions.
 * One work item per thread, block = 64 (one wave), grid = ceil(count / 64) capped where HIP caps it (the kernels stride);
 * glog / slog: the stream-interleaved tile order.  nt: nontemporal accesses -- no squeezed position below 3 and the knob on:
 * ph_nt for one target, u2_nt for two, the knobs K12 and K13 read.
 * NULL out, ntargets not 1 or 2, n = 0 or n > 40, ctrl_values outside ctrl_mask: QCX_BAD_ARGUMENTS; a target >= n, equal targets,
 * a mask bit at or above n or on a target: QCX_BAD_QUBIT; more than QCX_MC_MAX_RUNS runs (n > 34 only): QCX_UNSUPPORTED. */
#define QCX_MC_MAX_RUNS 17
enum { QCX_MC_PAIR = 0, QCX_MC_LINE_PAIR = 1, QCX_MC_LINE_SHFL = 2, QCX_MC_QUAD = 3, QCX_MC_LINES2 = 4 };
typedef struct {
    unsigned form, ns;              /* ns: QCX_MC_LINES2 only */
    uint64_t count;
    unsigned nruns;
    unsigned char run_pos[QCX_MC_MAX_RUNS], run_len[QCX_MC_MAX_RUNS];
    uint64_t or_const;
    unsigned low_mask, low_values, store_all;
    unsigned shfl_lo, shfl_hi;
    unsigned nt;
    unsigned grid, block, items_per_thread;
    unsigned glog, slog;
    char     kernel[48];            /* the instantiation as a kernel trace spells it, e.g. "k_mcu2_lines<1, true>" */
} qcx_mc_plan;
int  qcx_mc_gate_plan(unsigned n, uint64_t ctrl_mask, uint64_t ctrl_values, unsigned ntargets, unsigned qubit0, unsigned qubit1,
                      qcx_mc_plan *out);

/* The launch of qcx_diagonal_gate / qcx_diagonal_gate_device (include/qcx.h; K18, DESIGN s4.5n) for the range [first, first + num)
 * of a register of n qubits, on the host, under the knobs of the moment; the library launches from this very function.
 * A unit of work is a tile of the T = min(n, 12) lowest index bits, `units` = 2^(n - T) of them; workgroup b of `grid` takes the
 * units b, b + grid, ...  Thread tid of the 256 owns the tile-local elements e = tid + 256 j, j < elems, that exist: e < 2^T
 * (n < 12 is the one partial tile, full = 0).  The amplitude is i = (u << T) | e and its entry
 *     k(i) = (i >> first) & kmask,   kmask = 2^num - 1,
 * in 64 bits.  The forms say where a thread gets the entry from:
 *   QCX_DIAG_TILE   num = 0 or first >= T: k depends on u alone -- one entry per tile, read once per tile
 *   QCX_DIAG_GROUP  8 <= first < T: k depends on u and j, not on the lane -- at most 16 entries per tile, uniform reads
 *   QCX_DIAG_LANE   first < 8: an entry per lane, out of a slice of the table of slice_entries = 2^(min(first + num, T) - first)
 *                   entries per tile.  lds = 1: the slice is the same for every tile (first + num <= 12), the knob diag_lds is
 *                   on, and the workgroup copies the 2^num entries into lds_bytes of LDS once; lds = 0: each lane reads its entry
 *                   from memory.
 * grid = min(units, the knob diag_grid_cap (0: no cap)), within what HIP takes; block = 256.
 * NULL out, n = 0 or n > 40: QCX_BAD_ARGUMENTS; first + num > n: QCX_BAD_QUBIT. */
enum { QCX_DIAG_TILE = 0, QCX_DIAG_GROUP = 1, QCX_DIAG_LANE = 2 };
typedef struct {
    unsigned form, full, lds;
    unsigned T, first, num;
    uint64_t kmask;
    uint64_t units;
    unsigned elems;                 /* 2^(T - 8), or 1 for T <= 8 */
    uint64_t slice_entries;         /* table entries one tile reads (QCX_DIAG_TILE: 1) */
    unsigned grid, block, lds_bytes;
    char     kernel[48];            /* the instantiation as a kernel trace spells it, e.g. "k_diagonal<2, true, false>" */
} qcx_diag_plan;
int  qcx_diagonal_plan(unsigned n, unsigned first, unsigned num, qcx_diag_plan *out);

/* The tile geometry qcx_permutation_plan and qcx_multi_gate_plan share (one function of the library fills it), for an operator
 * on `num` index bits -- the range [first, first + num), or the target set -- of a register of n qubits under the controls
 * (ctrl_mask, ctrl_values), and a tile of at most 2^want amplitudes.
 * Controls at bit >= 3 are squeezed out of the work numbering, qcx_mc_gate_plan's rule: `squeezed` is their mask, its ascending
 * runs are [run_pos[k], run_pos[k] + run_len[k]), k < nruns, and or_const holds the positive ones.  With unsqueezed = n - the
 * squeezed positions, a tile is 2^T amplitudes, T = min(12, unsqueezed, want): tile_mask = the operator's bits and the lowest
 * T - num of the other unsqueezed bits (tile_bits[0 .. T) lists them ascending), so every tile is closed under any operator on
 * those bits.  unit_mask = the unsqueezed bits outside the tile; `units` = 2^(unsqueezed - T) tiles, and workgroup b of the
 * plan's `grid` takes the units b, b + grid, ...  Unit u, tile element e is the amplitude
 *     i = deposit(u, unit_mask) | deposit(e, tile_mask) | or_const,
 * deposit(v, mask) = v's bits moved, in order, into the set positions of mask.
 * A control below bit 3 is a predicate: elem_mask / elem_values where its bit lies in the tile (tested on i), unit_mask_low /
 * unit_values_low where it does not (tested on deposit(u, unit_mask); a unit that misses is skipped, nothing of it is read).
 * form: QCX_PERM_LINES when the tile holds index bits 0-2 (all of them that exist), so that it is made of whole 128-B lines;
 * QCX_PERM_SHARED when it does not: lines are shared between tiles. */
#define QCX_PERM_MAX_QUBITS 12
#define QCX_PERM_MAX_RUNS 20
enum { QCX_PERM_LINES = 0, QCX_PERM_SHARED = 1 };
typedef struct {
    unsigned form, T;
    unsigned char tile_bits[QCX_PERM_MAX_QUBITS];
    uint64_t tile_mask, unit_mask;
    uint64_t squeezed, or_const;
    unsigned nruns;
    unsigned char run_pos[QCX_PERM_MAX_RUNS], run_len[QCX_PERM_MAX_RUNS];
    unsigned elem_mask, elem_values, unit_mask_low, unit_values_low;
    uint64_t units;
} qcx_tile_geom;

/* The launch of qcx_permutation_gate (include/qcx.h; K19, DESIGN s4.5o) for the range [first, first + num) of a register of n
 * qubits under the controls (ctrl_mask, ctrl_values), on a register that holds finite amplitudes, on the host, under the knobs
 * of the moment; the library launches from this very function.
 * geom: the geometry above for the range, with want = max(num + 3, the knob perm_tile_log2) -- the range and three more bits, no
 * less than the knob asks for (12, so T = min(12, unsqueezed) for every range); QCX_PERM_SHARED occurs for num >= 10 with
 * first > 0.  Thread tid of `block` owns the tile elements e = tid + block j while e < 2^T.  The range field of e sits at bit
 * range_pos of e: the element stores tile[e with (e >> range_pos) & (2^num - 1) replaced by the inverse table's entry] to i.
 * The predicates are tested per element and per unit.  store_all: under a predicate the elements that do not act are stored
 * back as read, so that whole lines leave (the knob perm_store_all, on by measurement; 0: they are left alone).
 * block = 1024 for T = 12, else 256; grid = min(units, the knob perm_grid_cap (0: no cap)), within what HIP takes; lds_bytes =
 * 16 * 2^T for the tile + 2 * 2^num (rounded up to 16) for the inverse table: at most 64 KiB + 8 KiB.  nt: the knob perm_nt,
 * nontemporal stores.
 * NULL out, n = 0 or n > 40: QCX_BAD_ARGUMENTS; then qcx_permutation_gate's refusals, in its order: ctrl_values outside
 * ctrl_mask: QCX_BAD_ARGUMENTS; first + num > n: QCX_BAD_QUBIT; a mask bit at or above n or inside the range: QCX_BAD_QUBIT;
 * num > qcx_permutation_max_qubits(): QCX_BAD_ARGUMENTS. */
typedef struct {
    qcx_tile_geom geom;
    unsigned first, num;
    unsigned range_pos;             /* the tile bits below `first` */
    unsigned grid, block, lds_bytes;
    unsigned store_all, nt;
    char     kernel[48];            /* the instantiation as a kernel trace spells it, e.g. "k_perm_tile<false, false>" */
} qcx_perm_plan;
int  qcx_permutation_plan(unsigned n, uint64_t ctrl_mask, uint64_t ctrl_values, unsigned first, unsigned num, qcx_perm_plan *out);

/* The launch of qcx_mc_multi_qubit_gate (include/qcx.h; K20, DESIGN s4.5p) for a dense matrix on the num_targets = 3 .. 5 qubits
 * targets[] (1 and 2 as well: what the knob multi_generic = 1 launches for them) of a register of n qubits under the controls
 * (ctrl_mask, ctrl_values), on a register that holds finite amplitudes, on the host, under the knobs of the moment; the library
 * launches from this very function.
 * geom: the geometry above for the target set, with want = 12.  target_pos[j] = the bit of e that stands for targets[j] (j as
 * given, not sorted).  A group is the 2^num_targets elements that differ in those bits alone, so every tile is closed under the
 * operator; member c of a group in ascending index has the ascending target_pos bits set as c's bits are.  A work item is one
 * group and rows_per_item of its rows (4; 2 for one target); thread tid of `block` = min(1024, max(64, 2^T / rows_per_item))
 * takes the items tid, tid + block, ...: item = chunk * 2^(T - num_targets) + group number, the group number deposited into the
 * element bits that are no target.
 * A tile holds the lowest 12 - num_targets >= 7 other bits, so bits 0-2 always lie inside it: the predicate is elem_mask /
 * elem_values, tested per group on i; geom.unit_mask_low / unit_values_low are always 0 and geom.form is always QCX_PERM_LINES
 * for num_targets <= 5.  store_all: the groups that do not fire are stored back as read (the knob multi_store_all), so that
 * whole lines leave.  lds_bytes = 16 * 2^T, at most 64 KiB (the matrix is not kept in LDS).  nt: the knob multi_nt.
 * NULL out or targets, n = 0 or n > 40: QCX_BAD_ARGUMENTS; then qcx_mc_multi_qubit_gate's refusals, in its order: num_targets 0
 * or above QCX_MULTI_MAX_TARGETS: QCX_BAD_ARGUMENTS; ctrl_values outside ctrl_mask: QCX_BAD_ARGUMENTS; a target >= n, two targets
 * equal, a mask bit at or above n or on a target: QCX_BAD_QUBIT. */
#define QCX_MULTI_MAX_TARGETS 5
typedef struct {
    qcx_tile_geom geom;
    unsigned num_targets;
    unsigned char targets[QCX_MULTI_MAX_TARGETS], target_pos[QCX_MULTI_MAX_TARGETS];
    unsigned grid, block, lds_bytes, rows_per_item;
    unsigned store_all, nt;
    char     kernel[48];            /* the instantiation as a kernel trace spells it, e.g. "k_multi_tile<5, false>" */
} qcx_multi_plan;
int  qcx_multi_gate_plan(unsigned n, uint64_t ctrl_mask, uint64_t ctrl_values, unsigned num_targets, const unsigned *targets,
                         qcx_multi_plan *out);
#ifdef __cplusplus
}
#endif
#endif /* QCX_PLAN_H */
