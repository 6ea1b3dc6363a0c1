// qcx_api.hip -- the C ABI of libqcx.so (include/qcx.h) on top of the gfx950
// kernels in qcx_kernels.h.  Host side of the drop-in boundary: argument checks,
// launch geometry, the two gate schedules (Q:678-690, Q:712-737), MT19937 and
// measurement bookkeeping.  HIP only -- nothing here computes on the CPU.
#include "../../include/qcx.h"
#include "qcx_kernels.h"

#include <hip/hip_runtime.h>

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <map>
#include <mutex>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

using namespace qcx;

// ---------------------------------------------------------------------------
// error plumbing
// ---------------------------------------------------------------------------
static thread_local char g_last_error[256] = "";

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) {                                                                \
            snprintf(g_last_error, sizeof g_last_error, "%s: %s", #expr, hipGetErrorString(e_)); \
            return (e_ == hipErrorOutOfMemory) ? QCX_INSUFFICIENT_MEMORY : QCX_HIP_ERROR;      \
        }                                                                                      \
    } while (0)

#define set_error(...) snprintf(g_last_error, sizeof g_last_error, __VA_ARGS__)

#define QCX_TRY(expr)                     \
    do {                                  \
        int s_ = (expr);                  \
        if (s_ != QCX_NO_ERROR) return s_; \
    } while (0)

extern "C" const char *qcx_last_error(void) { return g_last_error; }

extern "C" const char *qcx_version(void) { return "qcx 0.1.0 (gfx950)"; }

extern "C" const char *qcx_status_string(int s)
{
    switch (s) {
    case QCX_NO_ERROR: return "NO_ERROR";
    case QCX_INSUFFICIENT_MEMORY: return "INSUFFICIENT_MEMORY";
    case QCX_BAD_ARGUMENTS: return "BAD_ARGUMENTS";
    case QCX_PERIOD_NOT_FOUND: return "PERIOD_NOT_FOUND";
    case QCX_UNKNOWN_ERROR: return "UNKNOWN_ERROR";
    case QCX_HIP_ERROR: return "HIP_ERROR";
    case QCX_BAD_QUBIT: return "BAD_QUBIT";
    case QCX_UNSUPPORTED: return "UNSUPPORTED";
    default: return "?";
    }
}

extern "C" int qcx_device_count(int *count)
{
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) { *count = 0; snprintf(g_last_error, sizeof g_last_error, "hipGetDeviceCount: %s", hipGetErrorString(e)); return QCX_HIP_ERROR; }
    *count = c;
    return QCX_NO_ERROR;
}

extern "C" int qcx_set_device(int device) { HIP_TRY(hipSetDevice(device)); return QCX_NO_ERROR; }

// ---------------------------------------------------------------------------
// launch configuration (tunable at run time so one build can be swept on the GPU)
// ---------------------------------------------------------------------------
// the knobs, once: X(name, default) and what the knob does.  The struct, qcx_tune_set and qcx_tune_get are generated from this list
#define QCX_TUNABLES(X) \
    X(h_variant, 0)               /* 0: auto, 1: always pair form, 2: wave-tile form where it applies */ \
    X(h_ppt, 1)                   /* pairs per thread, pair form */ \
    X(h_nt, 3)                    /* nontemporal: bit 0 loads, bit 1 stores (pair form, q >= 3) */ \
    X(h_wave_nt, 3)               /* same for the wave-tile form in auto mode */ \
    X(h_wc, 0)                    /* pair form: per-wave-contiguous load order */ \
    X(h_block, 64)                /* pair form: threads per block (64/128/256/512) */ \
    X(h_streams_log2, 0)          /* pair form: deal tiles as 2^k interleaved streams (3 = one per XCD) */ \
    X(h_skew, 0)                  /* pair form: stream j is rotated by j * skew tiles inside its segment */ \
    X(h_grid_cap, 0)              /* 0: one tile per block (no cap) */ \
    X(h_wave_r, 4)                /* registers per lane, wave-tile form (2, 4 or 8) */ \
    X(h_wave_block, 256)          /* wave-tile form: threads per block (64 or 256) */ \
    X(h_wave_maxq, 7)             /* auto: use the wave-tile form for q <= this */ \
    X(ph_apt, 1)                  /* measured (tools/experiments/tune_phase.py): one amplitude per lane, one wave per block, */ \
    X(ph_grid_cap, 0)             /* nontemporal, 2 or 4 interleaved streams: 6.4-6.9 TB/s on the touched quarter */ \
    X(ph_block, 64) \
    X(ph_nt, 1) \
    X(ph_streams_log2, -1)        /* -1: auto (1 when the lowest mask bit >= 8, else 2) */ \
    X(ph_lines, 1)                /* masks with a bit below 3: the whole-line kernel k_phase_lines (0: k_phase for every mask) */ \
    X(cam_grid_cap, 0)            /* (round 3: one tile per workgroup, 2.80-2.89 ms per gate at n = 30 against 2.85-3.0 with 4096 workgroups) */ \
                                  /* (measured n = 30, C = 21, M = 5: whole tiles 2.9-3.4 ms = 17.2 GB at 5.0-5.9 TB/s, partial 2.8-2.9 ms = 14.5 GB at 5.0-5.2) */ \
    X(cam_logT, 8)                /* modular multiply: tile = 2^this amplitudes, at least the 2^M block (n = 30, C = 21, M = 5: 2^11 2.65 ms, 2^10 2.50, 2^9 2.3-2.6, 2^8 2.3; 2^12 4.2) */ \
    X(cam_skip, 1)                /* modular multiply: the 128-B lines of a 2^M block above row C are neither sources nor destinations: not read */ \
    X(cam_nt_lines, 0)            /* modular multiply: completely rewritten lines leave as nontemporal stores (the partly rewritten one through L2) */ \
    X(fuse_T, 11)                 /* fused passes: tile = 2^T amplitudes in LDS (8..12) */ \
    X(fuse_c, 4)                  /* fused passes: contiguous low bits of a tile (runs of 16 * 2^c bytes) */ \
    X(fuse_grid_cap, 65536)       /* (round 4, chained passes: 65536 beats 24576 by 1-2 %, one per tile loses 15 % on the n = 30 exact Shor circuit) */ \
                                  /* workgroups of the one-tile-per-workgroup form (each walks several tiles: the table fill at kernel start is amortised) */ \
    X(fuse_qround, 1)             /* tolerance mode: rounds of the shape H D H D run as straight-line code (FUSE_QROUND) */ \
    X(fuse_q3_cap, 65536)         /* workgroups of k_fused_q3 with tables (round 3, in place: 3072 best; round 4, chained: n = 28 inverse QFT 6.12 ms with 3072, 5.85 with 65536; */ \
                                  /* n = 30 Shor circuit 18.7 with 65536, 20.5 with one per tile) */ \
    X(fuse_q3_cap_exact, 0)       /* all-Hadamard radix-8 passes (no tables to stage): one workgroup per tile (round 4, chained passes: n = 30 sweep 20.2 ms with 8192, 19.2 with one per tile) */ \
    X(fuse_q3, 1)                 /* tolerance mode: radix-8 fast rounds on 2^12 tiles when they save a pass (k_fused_q3) */ \
    X(fuse_x8, 1)                 /* bit-exact phase-dominated passes: the walk on 8 amplitudes per thread (k_fused_x8, round 5) */ \
    X(fuse_x8_T, 12)              /* ... on tiles of 2^this amplitudes (10 .. 12) with */ \
    X(fuse_x8_c, 4)               /* ... this many contiguous low bits */ \
    X(fuse_streams_log2, -1)      /* which tile a workgroup of k_fused_q3 / k_fused_x8 / k_fused_rounds takes (fuse_stream_tile): the 2^this low bits of its slot number ... */ \
    X(fuse_streams_pos, -1)       /* ... go to this bit of the tile number (+ 1; 0 = on top).  -1: by the kind of pass (launch_pass) */ \
    X(fuse_x8t, 1)                /* tolerance mode: radix-8 fast rounds run on the k_fused_x8 shell (hand-written round, K6x-t) instead of k_fused_q3 */ \
    X(fuse_x8_min_tiles_log2, 2)  /* ... on registers of at least 2^this tiles */ \
    X(fuse_x8_ratio, 1)           /* ... for passes without multiplies that hold at least this many phases per Hadamard */ \
    X(fuse_x8_map, 1)             /* ... the wave number rides on the tile bits most gates of a round test (0: plain ascending order) */ \
    X(fuse_x8_cap, 65536)         /* ... workgroups */ \
    X(fuse_gen, 1)                /* a pending reset / collapse + circuit front is GENERATED inside the first fused pass behind it (no write pass, no read) */ \
    X(fuse_chain_dir, -1)         /* chained passes: 0 = a pass stores gathered so that the NEXT tile is contiguous (reads whole tiles); 1 = stores its own tile contiguously, the next pass gathers; -1 = by the kind of chain */ \
    X(cam_block, 0)               /* threads per workgroup of k_camodc (0: 256; 1024 for tiles of 2^12 amplitudes) */ \
    X(cam_stage_mb, 1024)         /* M > 12: staging buffer of the in-place modular multiply (MiB; at least one 2^M-block) */ \
    X(fuse_compact, 1)            /* behind a circuit front whose M register stays on a small orbit: the flush runs on a compact copy of the state (compact_chain) */ \
    X(fuse_compact_lazy, 1)       /* ... and stays compact behind a whole-circuit entry point until something other than measure_state looks at the state */ \
    X(fuse_plan_cache, 1)         /* a flush whose inputs (shape, mode, knobs, front, gate list) are bit for bit those of the last one reuses its plan and, when nothing was uploaded since, its records on the device */ \
    X(fuse_expand_fused, 1)       /* the last pass of a compact chain stores the real register itself (k_fused_x8's expanding store) instead of k_expand_compact */ \
    X(fuse_cols_tol, 1)           /* tolerance mode: the by-columns pass of a compact chain keeps its merged diagonals (fast rounds inside k_gen_cols) */ \
    X(fuse_cols_cap, 12288)       /* workgroups of a k_gen_cols launch (a workgroup's prologue is long; n = 30 Shor circuit 11.06-11.09 ms with 12288-24576, 11.14-11.3 with 65536, 12.07 with 1536; tolerance 7.4-7.8 against 8.1) */ \
    X(fuse_cols_waves, 0)         /* waves per workgroup of k_gen_cols (4 ... 8; the first four generate and store the tile); 0: 8 for launches of at most 1024 tiles, else 4 */ \
    X(fuse_expand_direct, 1)      /* k_expand_compact: 1 = gather the compact sources straight from memory (8 per thread in flight) instead of staging 64 blocks in LDS */ \
    X(fuse_gen_cols, 1)           /* the generated first pass by COLUMNS of the four lowest M-register bits (K6g, k_gen_cols) */ \
    X(fuse_zskip, 1)              /* passes behind a circuit front: waves whose share of the tile is all +0 skip the rounds (FusePass::zskip) */ \
    X(fuse_zskip_maxw, 2)         /* ... on tiles of at most 2^(8 + this) amplitudes */ \
    X(fuse_lowtile, 1)            /* a pass whose hot bits lie below bit 12 takes the whole low end of the index as its (contiguous) tile */ \
    X(fuse_q3_c3, 1)              /* tolerance mode: radix-8 passes with 2^3-amplitude runs (9 hot bits) when that saves a pass */ \
    X(fuse_front, 1)              /* a pending reset / collapse is written together with the closed-form front of the queue (K0b) */ \
    X(fuse_tol_T, 10)             /* tolerance mode: tile bits of diagonal passes when that costs no extra pass (0: same as the rest) */ \
    X(fuse_tol_occ, 6)            /* tolerance-mode passes (merged diagonals): waves per SIMD the kernel is built for (6 or 8) */ \
    X(fuse_rounds_occ, 7)         /* rounds-form passes: k_fused_rounds built for this many waves per SIMD (6 or 7; 0 = the general kernel) */ \
    X(fuse_T_phase, 10)           /* tile bits of phase-dominated passes (one tile per workgroup, not pipelined); 0 = same as the rest */ \
    X(fuse_c_phase, 4) \
    X(fuse_phase_ratio, 6)        /* a pass is phase-dominated when it holds at least this many phases per H (and nothing else) */ \
    X(fuse_camruns, 1)            /* rounds form: fold runs of permutation-type modular multiplies into one gather */ \
    X(fuse_hsweep_T, 12)          /* tile geometry of an all-Hadamard tail when it saves passes (0: never) */ \
    X(fuse_hsweep_c, 3) \
    X(fuse_dbg, 0)                /* diagnostics (tools/experiments/probe_pass.py): bit 0 skip the gates, bit 1 skip the stores, bit 2 skip the fill of a rounds pass */ \
    X(fuse_rounds, 1)             /* fused passes: rounds form (4 amplitudes per thread in registers, radix-4 H steps) */ \
    X(fuse_ldsdma, 1)             /* fused passes: fill the tile with global_load_lds (LDS-DMA) */ \
    X(fuse_max_queue, 4096) \
    X(fuse_chain, 1)              /* runs of consecutive rounds-form passes go through the register's second buffer: every pass but the first reads */ \
                                  /* contiguous tiles, only its stores are gathered, the last one stores the identity layout again (FusePass) */ \
    X(fuse_chain_min_n, 20)       /* ... for registers of at least 2^this amplitudes */ \
    X(meas_block_log, 0)          /* parallel measurement: 2^this amplitudes per block (8..13); 0 = from the shard size */ \
    X(meas_parallel, 1)           /* 0: always the single-wave sequential scan */ \
    X(meas_min_log2, 12)          /* shards below 2^this amplitudes use the single-wave scan (tools/experiments/probe_shots.py) */ \
    X(meas_dbg, 0)                /* K4c diagnostics: bit 0 = no look-back (every binade guess from cum_in alone: times the pass without it); bit 1 = k_meas_fast hands over to the walk at its third candidate */ \
    X(meas_host_out, 1)           /* the scan's result is written straight into pinned host memory (no copy back on the stream) */ \
    X(meas_fast, 1)               /* K4c: the scan's events by k_meas_fast (list of candidate records, 8 waves) with k_meas_walk as the fallback; 0: the walk alone */ \
    X(meas_spin_limit, 4000000)   /* K4c: polls a look-back may spend on one window before it gives up (the block is then scanned exactly) */ \
    X(collapse_grid_cap, 65536)   /* K11 (k_collapse_range): workgroups, each walks 16-KiB steps */ \
    X(collapse_upt, 4)            /* K11: amplitudes per lane and step (4 or 8) */ \
    X(collapse_perm, 1)           /* K11: ranges starting at qubit 3 .. 5 take the wave-uniform index map (0: the plain map, divergent there) */ \
    X(u2_variant, 0)              /* K13 (two-qubit gate): 0 = the plan (line forms from n = 9 when lo or the control is below bit 3), 1 = quad form for every qubit pair */ \
    X(u2_nt, 1)                   /* K13: nontemporal accesses (only where a wave instruction covers whole 128-B lines, as in K12) */ \
    X(u2_streams_log2, -1)        /* K13: -1 = plain gate: the Hadamard plan's streams for hi; controlled: the phase gate's rule.  Both are guesses taken */ \
                                  /* over from kernels with two address streams, not four; tools/time_two_qubit_gate.py is there to measure them */ \
    X(prot_grid_cap, 2048)        /* K15 (k_pauli_rot): workgroups, each walks its units (tiles, or pairs of tiles) with this stride; 0 = one unit each */ \
    X(diag_grid_cap, 2048)        /* K18 (k_diagonal): workgroups, each walks its tiles with this stride; 0 = one tile each */ \
    X(diag_lds, 0)                /* K18: 1 = the per-lane form (first < 8) copies a table of first + num <= 12 into LDS once per workgroup; 0 = every lane reads its entry from memory (DESIGN s4.5n has both times) */ \
    X(perm_grid_cap, 2048)        /* K19 (k_perm_tile): workgroups, each walks its tiles with this stride; 0 = one tile each */ \
    X(perm_tile_log2, 12)         /* K19: a tile is 2^this amplitudes or the range and three more bits, whichever is more, at most 2^12 (DESIGN s4.5o has the times of 8, 10 and 12) */ \
    X(perm_store_all, 1)          /* K19: 1 = under a control below bit 3 the elements that do not fire are stored back as read (whole lines leave: 6.19 against 6.45 ms at n = 30) */ \
    X(perm_nt, 0)                 /* K19: 1 = nontemporal stores */ \
    X(multi_grid_cap, 2048)       /* K20 (k_multi_tile): workgroups, each walks its tiles with this stride; 0 = one tile each */ \
    X(multi_store_all, 1)         /* K20: 1 = under a control below bit 3 the groups that do not fire are stored back as read (whole lines leave; K19's measurement) */ \
    X(multi_nt, 0)                /* K20: 1 = nontemporal stores */ \
    X(multi_generic, 0)           /* K20 (qcx_mc_multi_qubit_gate): 1 = one and two targets run K20's kernel too (0: mc_gate()'s launches; the tests compare the two bit for bit) */ \
    X(mc_generic, 0)              /* K17 (gates under a control mask): 1 = no control and one positive control run K17's kernels too (0: K12's / K13's launches; the tests compare the two bit for bit) */
struct Tune {
#define X(name, value) long name = value;
    QCX_TUNABLES(X)
#undef X
};
static Tune g_tune;
static std::mutex g_tune_mutex;
// every entry point works on ONE consistent snapshot of the tunables (qcx_tune_set may run on another thread)
static Tune tune_now() { std::lock_guard<std::mutex> lock(g_tune_mutex); return g_tune; }

extern "C" int qcx_tune_set(const char *key, long value)
{
#define X(name, dflt) if (!strcmp(key, #name)) { std::lock_guard<std::mutex> lock(g_tune_mutex); g_tune.name = value; return QCX_NO_ERROR; }
    QCX_TUNABLES(X)
#undef X
    return QCX_BAD_ARGUMENTS;
}

extern "C" long qcx_tune_get(const char *key)
{
#define X(name, dflt) if (!strcmp(key, #name)) { std::lock_guard<std::mutex> lock(g_tune_mutex); return g_tune.name; }
    QCX_TUNABLES(X)
#undef X
    return -1;
}

static inline unsigned grid_for(uint64_t work_items, uint64_t per_block, long cap, unsigned block_threads = 1024)
{
    uint64_t g = (work_items + per_block - 1) / per_block;
    if (g == 0) g = 1;
    if (cap > 0 && g > (uint64_t)cap) g = (uint64_t)cap;
    // kernels grid-stride, so any cap is valid; HIP wants grid * block < 2^32 threads (n = 33, 34 registers get there)
    const uint64_t hard = std::min<uint64_t>(0x7fffffffULL, 0xffffffffULL / block_threads);
    if (g > hard) g = hard;
    return (unsigned)g;
}

// ---------------------------------------------------------------------------
// per-device scratch for the shard-level entry points
// ---------------------------------------------------------------------------
struct Workspace {
    double     *partials = nullptr;     // NORM_BLOCKS doubles + 1
    MeasureOut *mout = nullptr;
    MeasureOut *h_mout = nullptr;       // pinned
    size_t      meas_slots_pending = 0;
    size_t      meas_clean_slots = 0;   // ... and this many look-back slots from the start of meas_look are known to read "not published"
    bool        meas_clean = false;     // the last parallel scan completed: its walk kernel left ticket and candidate count at zero
    double     *h_scalar = nullptr;     // pinned
    uint32_t   *tab = nullptr;          // camodc CSR table (off + srcs)
    size_t      tab_cap = 0;
    amp_t      *cam_stage = nullptr;    // staging buffer of the M > 12 modular multiply (K3b)
    size_t      cam_stage_cap = 0;
    MeasBlock  *meas_blocks = nullptr;
    unsigned    meas_cap = 0;
    unsigned   *meas_stats = nullptr, *h_meas_stats = nullptr; // [slow-path blocks, blocks] of the last scan
    MeasCands  *meas_cands = nullptr;                           // k_meas_fast: the candidate records of the scan in flight ...
    MeasResume *meas_resume = nullptr;                          // ... and what it leaves for k_meas_walk
    meas_slot_t *meas_look = nullptr;   // K4c: look-back area (one allocation): agg, incl per workgroup, gincl per group (filled with ones), then
                                        // gsum, gcount per group and the ticket (zeroed)
    MeasBlock  *meas_up = nullptr;      // K4c: the levels above the records (sums of 64, 64^2, ... records), back to back
    double     *samp_ends = nullptr;    // K4d (sampling): the exact running sum at the end of every record
    SampCarry  *samp_aux = nullptr;     // K4d: chunk totals, chunk prefixes, then the `bad` word
    uint64_t    samp_cap = 0;           // records samp_ends / samp_aux are sized for
    double     *samp_r = nullptr;       // K4d: one batch of draws ...
    uint64_t   *samp_out = nullptr;     // ... and their answers
    size_t      samp_shot_cap = 0;
    uint64_t samp_nch_cap() const { return (samp_cap + QCX_SAMP_CHUNK - 1) / QCX_SAMP_CHUNK; }
};
static const unsigned NORM_BLOCKS = 2048;
static std::mutex g_ws_mutex;
static std::mutex g_ws_use[64];       // one user of a device's scratch (norm / measurement) at a time
static Workspace g_ws[64];

static int workspace(Workspace **out)
{
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64) return QCX_HIP_ERROR;
    std::lock_guard<std::mutex> lock(g_ws_mutex);
    Workspace &w = g_ws[dev];
    if (!w.partials) {
        HIP_TRY(hipMalloc(&w.partials, (NORM_BLOCKS + 1) * sizeof(double)));
        HIP_TRY(hipMalloc(&w.mout, sizeof(MeasureOut)));
        HIP_TRY(hipHostMalloc(&w.h_mout, sizeof(MeasureOut)));
        HIP_TRY(hipHostMalloc(&w.h_scalar, sizeof(double)));
        HIP_TRY(hipMalloc(&w.meas_stats, 2 * sizeof(unsigned)));
        HIP_TRY(hipMalloc(&w.meas_cands, sizeof(MeasCands)));
        HIP_TRY(hipMalloc(&w.meas_resume, sizeof(MeasResume)));
        HIP_TRY(hipHostMalloc(&w.h_meas_stats, 2 * sizeof(unsigned)));
        w.h_meas_stats[0] = w.h_meas_stats[1] = 0;
    }
    *out = &w;
    return QCX_NO_ERROR;
}

// ---------------------------------------------------------------------------
// shard-level launches
// ---------------------------------------------------------------------------
extern "C" int qcx_shard_reset(void *amp, unsigned n_local, int holds_index_one, void *stream)
{
    if (!amp || n_local > 40) return QCX_BAD_ARGUMENTS;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(amp, 0, (size_t)16 << n_local, st));
    if (holds_index_one) {
        if (n_local == 0) return QCX_BAD_ARGUMENTS;          // a 1-amplitude shard has no index 1
        hipLaunchKernelGGL(k_set_one, dim3(1), dim3(64), 0, st, (amp_t *)amp, (uint64_t)1);
        HIP_TRY(hipGetLastError());
    }
    return QCX_NO_ERROR;
}

extern "C" int qcx_shard_collapse(void *amp, unsigned n_local, int64_t local_index, void *stream)
{
    if (!amp || n_local > 40) return QCX_BAD_ARGUMENTS;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(amp, 0, (size_t)16 << n_local, st));
    if (local_index >= 0) {
        if ((uint64_t)local_index >= ((uint64_t)1 << n_local)) return QCX_BAD_ARGUMENTS;
        hipLaunchKernelGGL(k_set_one, dim3(1), dim3(64), 0, st, (amp_t *)amp, (uint64_t)local_index);
        HIP_TRY(hipGetLastError());
    }
    return QCX_NO_ERROR;
}

// -0 components become +0 (what the reference's mat-vec does to every amplitude at every gate, Q:393-413): for a state the
// caller wrote, before the first gate runs on it (k_canon_zeros)
extern "C" int qcx_shard_canon_zeros(void *amp, unsigned n_local, void *stream)
{
    if (!amp || n_local > 40) return QCX_BAD_ARGUMENTS;
    const uint64_t count = (uint64_t)1 << n_local;
    hipLaunchKernelGGL(k_canon_zeros, dim3(grid_for(count, 256 * 4, 0, 256)), dim3(256), 0, (hipStream_t)stream, (amp_t *)amp, count);
    HIP_TRY(hipGetLastError());
    return QCX_NO_ERROR;
}

extern "C" int qcx_shard_fill_random(void *amp, unsigned n_local, uint64_t first_global, uint64_t seed, double scale, void *stream)
{
    if (!amp || n_local > 40) return QCX_BAD_ARGUMENTS;
    const uint64_t count = (uint64_t)1 << n_local;
    hipLaunchKernelGGL(k_fill_random, dim3(grid_for(count, 256 * 4, 0, 256)), dim3(256), 0, (hipStream_t)stream,
                       (amp_t *)amp, count, first_global, seed, scale);
    HIP_TRY(hipGetLastError());
    return QCX_NO_ERROR;
}

template <int PPT, bool NTL, bool NTS, bool WC, int BLOCK>
static void launch_h_pair(const Tune &t, amp_t *a, unsigned q, uint64_t npairs, hipStream_t st)
{
    const unsigned grid = grid_for(npairs, BLOCK * PPT, t.h_grid_cap, BLOCK);
    // stream-interleaved tile order only for an uncapped power-of-two grid that divides evenly
    unsigned glog = 0, slog = 0;
    if ((grid & (grid - 1)) == 0 && (uint64_t)grid * (BLOCK * PPT) == npairs) {
        glog = 31u - (unsigned)__builtin_clz(grid);
        if (t.h_streams_log2 > 0 && (unsigned)t.h_streams_log2 <= glog) slog = (unsigned)t.h_streams_log2;
    }
    if (slog && t.h_skew > 0) slog |= (unsigned)t.h_skew << 8;
    hipLaunchKernelGGL((k_h_pair<PPT, NTL, NTS, WC, BLOCK>), dim3(grid), dim3(BLOCK), 0, st, a, q, npairs, glog, slog);
}

template <int PPT, int BLOCK>
static void launch_h_pair_flags(const Tune &t, amp_t *a, unsigned q, uint64_t npairs, hipStream_t st, long nt, bool wc)
{
    const int f = (int)(nt & 3) | (wc ? 4 : 0);
    switch (f) {
    case 0: launch_h_pair<PPT, false, false, false, BLOCK>(t, a, q, npairs, st); break;
    case 3: launch_h_pair<PPT, true, true, false, BLOCK>(t, a, q, npairs, st); break;
    case 4: launch_h_pair<PPT, false, false, true, BLOCK>(t, a, q, npairs, st); break;
    case 7: launch_h_pair<PPT, true, true, true, BLOCK>(t, a, q, npairs, st); break;
    case 1: case 5: launch_h_pair<PPT, true, false, false, BLOCK>(t, a, q, npairs, st); break;
    default: launch_h_pair<PPT, false, true, false, BLOCK>(t, a, q, npairs, st); break;
    }
}

template <int PPT>
static void launch_h_pair_block(const Tune &t, amp_t *a, unsigned q, uint64_t npairs, hipStream_t st, long nt, bool wc)
{
    switch (t.h_block) {
    case 64:  launch_h_pair_flags<PPT, 64>(t, a, q, npairs, st, nt, wc); break;
    case 128: launch_h_pair_flags<PPT, 128>(t, a, q, npairs, st, nt, wc); break;
    case 512: launch_h_pair_flags<PPT, 512>(t, a, q, npairs, st, nt, wc); break;
    default:  launch_h_pair_flags<PPT, 256>(t, a, q, npairs, st, nt, wc); break;
    }
}

static void stream_map(unsigned grid, uint64_t covered, uint64_t total, long want_slog, unsigned *glog, unsigned *slog)
{
    *glog = 0; *slog = 0;
    if ((grid & (grid - 1)) == 0 && covered == total) {       // uncapped power-of-two grid that divides evenly
        *glog = 31u - (unsigned)__builtin_clz(grid);
        if (want_slog > 0 && (unsigned)want_slog <= *glog) *slog = (unsigned)want_slog;
    }
}

template <int Q, int R, bool NTL, bool NTS>
static void launch_h_wave_q(const Tune &t, amp_t *a, uint64_t namps, hipStream_t st)
{
    const uint64_t ntiles = namps / (64 * R);
    unsigned glog, slog;
    if (t.h_wave_block == 64) {
        const unsigned grid = grid_for(ntiles, 1, t.h_grid_cap, 64);
        stream_map(grid, grid, ntiles, t.h_streams_log2, &glog, &slog);
        hipLaunchKernelGGL((k_h_wave<Q, R, NTL, NTS, 64>), dim3(grid), dim3(64), 0, st, a, ntiles, glog, slog);
    } else {
        const unsigned grid = grid_for(ntiles, 4 /* waves per 256-thread block */, t.h_grid_cap, 256);
        stream_map(grid, (uint64_t)grid * 4, ntiles, t.h_streams_log2, &glog, &slog);
        hipLaunchKernelGGL((k_h_wave<Q, R, NTL, NTS, 256>), dim3(grid), dim3(256), 0, st, a, ntiles, glog, slog);
    }
}

template <int R, bool NTL, bool NTS>
static bool launch_h_wave(const Tune &t, amp_t *a, unsigned q, uint64_t namps, hipStream_t st)
{
    switch (q) {
    case 0: launch_h_wave_q<0, R, NTL, NTS>(t, a, namps, st); return true;
    case 1: launch_h_wave_q<1, R, NTL, NTS>(t, a, namps, st); return true;
    case 2: launch_h_wave_q<2, R, NTL, NTS>(t, a, namps, st); return true;
    case 3: launch_h_wave_q<3, R, NTL, NTS>(t, a, namps, st); return true;
    case 4: launch_h_wave_q<4, R, NTL, NTS>(t, a, namps, st); return true;
    case 5: launch_h_wave_q<5, R, NTL, NTS>(t, a, namps, st); return true;
    case 6: launch_h_wave_q<6, R, NTL, NTS>(t, a, namps, st); return true;
    case 7: if constexpr (R >= 4) { launch_h_wave_q<7, R, NTL, NTS>(t, a, namps, st); return true; } return false;
    case 8: if constexpr (R >= 8) { launch_h_wave_q<8, R, NTL, NTS>(t, a, namps, st); return true; } return false;
    default: return false;
    }
}

template <int R>
static bool launch_h_wave_flags(const Tune &t, amp_t *a, unsigned q, uint64_t namps, hipStream_t st, long nt)
{
    if ((nt & 3) == 3) return launch_h_wave<R, true, true>(t, a, q, namps, st);
    return launch_h_wave<R, false, false>(t, a, q, namps, st);
}

// Launch plan per target qubit, measured on MI355X (tools/experiments/tune_h.py, profiles/r01_tune_h_*.json).
// What matters is the ABSOLUTE pair distance 2^q * 16 B (the same q behaves the same at n = 26, 28
// and 30), i.e. how the two streams of a wave fall onto HBM channels and banks:
//   - the smallest work item wins everywhere: one wave, 2 x 16 B per lane (2 KiB in flight per wave);
//   - below q = 3 a pair shares a 128-B line, so the wave-tile (shuffle) form with whole-line
//     nontemporal accesses is used; from q = 3 the pair form with nontemporal loads and stores;
//   - dealing the tiles as 2^s interleaved streams (s = 1..3) moves the concurrently active windows
//     apart; the best s depends on q (q = 20..23 are the hard distances, s = 3 and 2 pairs/thread).
struct HPlan { int wave_form; int ppt; int block; int slog; };
static HPlan h_plan(unsigned q)
{
    if (q <= 2)  return {1, 0, 256, 2};
    if (q <= 6)  return {0, 1, 64, 2};
    if (q <= 17) return {0, 1, 64, 1};
    if (q <= 19) return {0, 1, 64, 0};
    if (q == 20) return {0, 1, 64, 1};
    if (q <= 23) return {0, 2, 64, 3};
    if (q == 24 || q == 26 || q == 27) return {0, 1, 64, 1};
    return {0, 1, 64, 0};
}

extern "C" int qcx_shard_hadamard(void *amp, unsigned n_local, unsigned q, void *stream)
{
    if (!amp || n_local == 0 || n_local > 40) return QCX_BAD_ARGUMENTS;
    if (q >= n_local) return QCX_BAD_QUBIT;
    hipStream_t st = (hipStream_t)stream;
    amp_t *a = (amp_t *)amp;
    const uint64_t namps = (uint64_t)1 << n_local, npairs = namps >> 1;

    Tune t = tune_now();                             // local copy: the entry point is re-entrant
    if (t.h_variant == 0) {                          // auto: the measured plan
        const HPlan pl = h_plan(q);
        t.h_variant = pl.wave_form ? 2 : 1;
        t.h_wave_r = 2; t.h_wave_block = pl.block;
        t.h_ppt = pl.ppt; t.h_block = pl.block;
        t.h_streams_log2 = pl.slog; t.h_nt = 3; t.h_wc = 0; t.h_grid_cap = 0;
    }
    int status = QCX_NO_ERROR;
    bool launched = false;
    // wave-tile form: needs whole 64*R tiles and the partner inside the tile
    const int R = (t.h_wave_r >= 8) ? 8 : (t.h_wave_r >= 4 ? 4 : 2);
    const unsigned tile_bits = (R == 8) ? 9 : (R == 4 ? 8 : 7);
    if (t.h_variant == 2 && q < tile_bits && n_local >= tile_bits + 2) {
        launched = (R == 8) ? launch_h_wave_flags<8>(t, a, q, namps, st, t.h_nt)
                 : (R == 4) ? launch_h_wave_flags<4>(t, a, q, namps, st, t.h_nt)
                            : launch_h_wave_flags<2>(t, a, q, namps, st, t.h_nt);
    }
    if (!launched) {
        long ppt = t.h_ppt;
        while (ppt > 1 && npairs < (uint64_t)512 * (uint64_t)ppt) ppt >>= 1;
        // nontemporal accesses only pay when a wave-instruction covers whole 128-B lines (q >= 3)
        const long nt = (q >= 3) ? t.h_nt : 0;
        const bool wc = t.h_wc != 0;
        switch (ppt) {
        case 8: launch_h_pair_block<8>(t, a, q, npairs, st, nt, wc); break;
        case 4: launch_h_pair_block<4>(t, a, q, npairs, st, nt, wc); break;
        case 2: launch_h_pair_block<2>(t, a, q, npairs, st, nt, wc); break;
        default: launch_h_pair_block<1>(t, a, q, npairs, st, nt, wc); break;
        }
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { snprintf(g_last_error, sizeof g_last_error, "hadamard launch: %s", hipGetErrorString(e)); status = QCX_HIP_ERROR; }
    return status;
}

template <int NB, int APT, bool NT, int BLOCK>
static void launch_phase_cfg(const Tune &t, amp_t *a, unsigned b0, unsigned b1, double c, double s, uint64_t count, hipStream_t st)
{
    const unsigned grid = grid_for(count, (uint64_t)BLOCK * APT, t.ph_grid_cap, BLOCK);
    unsigned glog, slog;
    long want = t.ph_streams_log2;
    if (want < 0) want = (NB == 0 || b0 >= 8) ? 1 : 2;
    stream_map(grid, (uint64_t)grid * BLOCK * APT, count, want, &glog, &slog);
    hipLaunchKernelGGL((k_phase<NB, APT, NT, BLOCK>), dim3(grid), dim3(BLOCK), 0, st, a, b0, b1, c, s, count, glog, slog);
}

template <int NB, int APT, bool NT>
static void launch_phase_blk(const Tune &t, amp_t *a, unsigned b0, unsigned b1, double c, double s, uint64_t count, hipStream_t st)
{
    if (t.ph_block == 64) launch_phase_cfg<NB, APT, NT, 64>(t, a, b0, b1, c, s, count, st);
    else launch_phase_cfg<NB, APT, NT, 256>(t, a, b0, b1, c, s, count, st);
}

template <int NB>
static void launch_phase(const Tune &t, amp_t *a, unsigned b0, unsigned b1, double c, double s, uint64_t count, hipStream_t st)
{
    long apt = t.ph_apt;
    while (apt > 1 && count < (uint64_t)256 * (uint64_t)apt) apt >>= 1;
    // nontemporal only when the touched runs are whole 128-B lines (lowest mask bit >= 3, or no mask)
    const bool nt = t.ph_nt != 0 && (NB == 0 || b0 >= 3);
    if (apt >= 4)      { if (nt) launch_phase_blk<NB, 4, true>(t, a, b0, b1, c, s, count, st); else launch_phase_blk<NB, 4, false>(t, a, b0, b1, c, s, count, st); }
    else if (apt == 2) { if (nt) launch_phase_blk<NB, 2, true>(t, a, b0, b1, c, s, count, st); else launch_phase_blk<NB, 2, false>(t, a, b0, b1, c, s, count, st); }
    else               { if (nt) launch_phase_blk<NB, 1, true>(t, a, b0, b1, c, s, count, st); else launch_phase_blk<NB, 1, false>(t, a, b0, b1, c, s, count, st); }
}

extern "C" int qcx_shard_phase(void *amp, unsigned n_local, uint64_t mask, double cos_t, double sin_t, void *stream)
{
    if (!amp || n_local > 40) return QCX_BAD_ARGUMENTS;
    if (n_local < 64 && (mask >> n_local) != 0) return QCX_BAD_QUBIT;
    const int nb = __builtin_popcountll(mask);
    if (nb > 2) return QCX_BAD_ARGUMENTS;
    hipStream_t st = (hipStream_t)stream;
    amp_t *a = (amp_t *)amp;
    unsigned b0 = 0, b1 = 0;
    if (nb >= 1) b0 = (unsigned)__builtin_ctzll(mask);
    if (nb == 2) b1 = 63u - (unsigned)__builtin_clzll(mask);
    const uint64_t count = ((uint64_t)1 << n_local) >> nb;
    const Tune t = tune_now();
    if (nb >= 1 && b0 < 3 && t.ph_lines && n_local >= 9) {
        // a mask bit inside a 128-B line: one lane per amplitude of every touched line (k_phase_lines)
        unsigned lowmask = 0, hb[2] = {0, 0}, nh = 0;
        const unsigned mbits[2] = {b0, b1};                          // ascending
        for (int k = 0; k < nb; k++) { if (mbits[k] < 3) lowmask |= 1u << mbits[k]; else hb[nh++] = mbits[k]; }
        const uint64_t lines_amps = ((uint64_t)1 << n_local) >> nh;
        const int store_all = (lowmask & 3u) ? 1 : 0;               // 16- or 32-B granularity: write whole lines back (measured: masked 32-B stores 4.0 ms vs 2.6)
        const unsigned grid = grid_for(lines_amps, 64, 0, 64);
        unsigned glog, slog;
        stream_map(grid, (uint64_t)grid * 64, lines_amps, 2, &glog, &slog);
        if (nh == 0) hipLaunchKernelGGL((k_phase_lines<0, 64>), dim3(grid), dim3(64), 0, st, a, 0u, 0u, lowmask, store_all, cos_t, sin_t, lines_amps, glog, slog);
        else if (nh == 1) hipLaunchKernelGGL((k_phase_lines<1, 64>), dim3(grid), dim3(64), 0, st, a, hb[0], 0u, lowmask, store_all, cos_t, sin_t, lines_amps, glog, slog);
        else hipLaunchKernelGGL((k_phase_lines<2, 64>), dim3(grid), dim3(64), 0, st, a, hb[0], hb[1], lowmask, store_all, cos_t, sin_t, lines_amps, glog, slog);
        HIP_TRY(hipGetLastError());
        return QCX_NO_ERROR;
    }
    if (nb == 0) launch_phase<0>(t, a, 0, 0, cos_t, sin_t, count, st);
    else if (nb == 1) launch_phase<1>(t, a, b0, 0, cos_t, sin_t, count, st);
    else launch_phase<2>(t, a, b0, b1, cos_t, sin_t, count, st);
    HIP_TRY(hipGetLastError());
    return QCX_NO_ERROR;
}

// ---- K12: any one-qubit gate, plain or controlled --------------------------------------------------------------------------
template <int PPT, bool NT, bool CTL>
static void launch_u_pair(amp_t *a, unsigned q, unsigned c, const UMat &U, uint64_t npairs, long want_slog, hipStream_t st)
{
    constexpr int BLOCK = 64;                            // the smallest work item wins everywhere (h_plan)
    const unsigned grid = grid_for(npairs, BLOCK * PPT, 0, BLOCK);
    unsigned glog, slog;
    stream_map(grid, (uint64_t)grid * (BLOCK * PPT), npairs, want_slog, &glog, &slog);
    hipLaunchKernelGGL((k_u_pair<PPT, NT, CTL, BLOCK>), dim3(grid), dim3(BLOCK), 0, st, a, q, c, U, npairs, glog, slog);
}

template <int Q, int R, bool NT>
static void launch_u_wave_q(amp_t *a, const UMat &U, uint64_t namps, long want_slog, hipStream_t st)
{
    const uint64_t ntiles = namps / (64 * R);
    const unsigned grid = grid_for(ntiles, 4 /* waves per 256-thread block */, 0, 256);
    unsigned glog, slog;
    stream_map(grid, (uint64_t)grid * 4, ntiles, want_slog, &glog, &slog);
    hipLaunchKernelGGL((k_u_wave<Q, R, NT, 256>), dim3(grid), dim3(256), 0, st, a, U, ntiles, glog, slog);
}

template <int R, bool NT>
static bool launch_u_wave(amp_t *a, unsigned q, const UMat &U, uint64_t namps, long want_slog, hipStream_t st)
{
    switch (q) {
    case 0: launch_u_wave_q<0, R, NT>(a, U, namps, want_slog, st); return true;
    case 1: launch_u_wave_q<1, R, NT>(a, U, namps, want_slog, st); return true;
    case 2: launch_u_wave_q<2, R, NT>(a, U, namps, want_slog, st); return true;
    case 3: launch_u_wave_q<3, R, NT>(a, U, namps, want_slog, st); return true;
    case 4: launch_u_wave_q<4, R, NT>(a, U, namps, want_slog, st); return true;
    case 5: launch_u_wave_q<5, R, NT>(a, U, namps, want_slog, st); return true;
    case 6: launch_u_wave_q<6, R, NT>(a, U, namps, want_slog, st); return true;
    case 7: if constexpr (R >= 4) { launch_u_wave_q<7, R, NT>(a, U, namps, want_slog, st); return true; } return false;
    case 8: if constexpr (R >= 8) { launch_u_wave_q<8, R, NT>(a, U, namps, want_slog, st); return true; } return false;
    default: return false;
    }
}

// The plain gate moves the bytes the Hadamard moves, so it takes the Hadamard's measured plan (h_plan) and listens to its knobs:
// h_variant (0 = the plan, 1 = pair form for every q, 2 = wave-tile form for q < 6 + log2 h_wave_r), h_wave_r, h_ppt (1 or 2),
// h_streams_log2, h_nt (pair form only).  The controlled gate touches the control-set half: the pair form with the control as a second
// squeezed-out bit (streams as for a phase: ph_streams_log2, ph_nt), or, with the control or the target inside a 128-B line
// and n_local >= 9, the whole-line form (ph_lines = 0: the pair form for every pair of qubits).
static int launch_status(const char *what)      // did the launch go out?  (the epilogue of the general gates' shard-level entry points)
{
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { snprintf(g_last_error, sizeof g_last_error, "%s launch: %s", what, hipGetErrorString(e)); return QCX_HIP_ERROR; }
    return QCX_NO_ERROR;
}

extern "C" int qcx_shard_one_qubit(void *amp, unsigned n_local, unsigned q, int ctl, const double *u, void *stream)
{
    if (!amp || !u || n_local == 0 || n_local > 40) return QCX_BAD_ARGUMENTS;
    if (q >= n_local || (ctl >= 0 && ((unsigned)ctl >= n_local || (unsigned)ctl == q))) return QCX_BAD_QUBIT;
    hipStream_t st = (hipStream_t)stream;
    amp_t *a = (amp_t *)amp;
    const UMat U = {u[0], u[1], u[2], u[3], u[4], u[5], u[6], u[7]};
    const uint64_t namps = (uint64_t)1 << n_local;
    const Tune t = tune_now();
    if (ctl < 0) {
        const HPlan pl = h_plan(q);
        const bool autop = t.h_variant == 0;
        const bool wave = autop ? pl.wave_form != 0 : t.h_variant == 2;
        const int R = autop ? 2 : (t.h_wave_r >= 8 ? 8 : (t.h_wave_r >= 4 ? 4 : 2));
        const unsigned tile_bits = (R == 8) ? 9 : (R == 4 ? 8 : 7);
        const long slog = autop ? pl.slog : t.h_streams_log2;
        const bool nt = autop || (t.h_nt & 3) == 3;
        bool launched = false;
        if (wave && q < tile_bits && n_local >= tile_bits + 2) {      // whole 64*R tiles and the partner inside the tile
            // (whole-line accesses: always nontemporal, as in the Hadamard's plan)
            launched = (R == 8) ? launch_u_wave<8, true>(a, q, U, namps, slog, st) : (R == 4) ? launch_u_wave<4, true>(a, q, U, namps, slog, st) : launch_u_wave<2, true>(a, q, U, namps, slog, st);
        }
        if (!launched) {
            const uint64_t npairs = namps >> 1;
            long ppt = autop ? pl.ppt : t.h_ppt;
            if (ppt > 1 && npairs < 1024) ppt = 1;
            const bool ntp = nt && q >= 3;                            // nontemporal only where a wave instruction covers whole 128-B lines
            if (ppt >= 2) { if (ntp) launch_u_pair<2, true, false>(a, q, 0, U, npairs, slog, st); else launch_u_pair<2, false, false>(a, q, 0, U, npairs, slog, st); }
            else          { if (ntp) launch_u_pair<1, true, false>(a, q, 0, U, npairs, slog, st); else launch_u_pair<1, false, false>(a, q, 0, U, npairs, slog, st); }
        }
    } else {
        const unsigned c = (unsigned)ctl, lowest = c < q ? c : q;
        if (lowest < 3 && t.ph_lines && n_local >= 9) {
            const bool lowq = q < 3;
            const uint64_t count = (lowq && c < 3) ? namps : namps >> 1;
            const int store_all = c < 2 ? 1 : 0;
            const unsigned grid = grid_for(count, 64, 0, 64);
            unsigned glog, slog;
            stream_map(grid, (uint64_t)grid * 64, count, 2, &glog, &slog);
            if (lowq) hipLaunchKernelGGL((k_cu_lines<true>), dim3(grid), dim3(64), 0, st, a, q, c, store_all, U, count, glog, slog);
            else      hipLaunchKernelGGL((k_cu_lines<false>), dim3(grid), dim3(64), 0, st, a, q, c, store_all, U, count, glog, slog);
        } else {
            long slog = t.ph_streams_log2;
            if (slog < 0) slog = lowest >= 8 ? 1 : 2;
            if (t.ph_nt != 0 && lowest >= 3) launch_u_pair<1, true, true>(a, q, c, U, namps >> 2, slog, st);
            else                             launch_u_pair<1, false, true>(a, q, c, U, namps >> 2, slog, st);
        }
    }
    return launch_status("one-qubit gate");
}

// A runtime flag, and a number of targets, as a template argument -- pauli_dispatch's pattern (below): launch(tag), a generic
// lambda that reads decltype(tag)::value.
template <class Launch> static void flag_dispatch(bool flag, Launch launch) { if (flag) launch(std::true_type()); else launch(std::false_type()); }
template <unsigned K = 1, class Launch> static void targets_dispatch(unsigned k, Launch launch)         // k = 1 .. 5 (above: as 5)
{
    if constexpr (K < QCX_MULTI_MAX_TARGETS) { if (k != K) return targets_dispatch<K + 1>(k, launch); }
    launch(std::integral_constant<unsigned, K>());
}

// ---- K13: any two-qubit gate, plain or controlled --------------------------------------------------------------------------
template <bool NT, bool CTL>
static void launch_u2_quad(amp_t *a, unsigned lo, unsigned hi, unsigned c, const U4Mat &U, uint64_t count, long want_slog, hipStream_t st)
{
    constexpr int BLOCK = 64;
    unsigned s[3] = {lo, hi, c};                           // the squeezed-out bits, ascending (lo < hi already)
    if (CTL) { if (s[2] < s[1]) std::swap(s[1], s[2]); if (s[1] < s[0]) std::swap(s[0], s[1]); }
    const unsigned grid = grid_for(count, BLOCK, 0, BLOCK);
    unsigned glog, slog;
    stream_map(grid, (uint64_t)grid * BLOCK, count, want_slog, &glog, &slog);
    hipLaunchKernelGGL((k_u2_quad<NT, CTL, BLOCK>), dim3(grid), dim3(BLOCK), 0, st, a, lo, hi, c, s[0], s[1], s[2], U, count, glog, slog);
}

// The reference sums a row's triplets in ascending state index: with qubit0 above qubit1 the matrix is taken as P u P (P = the
// index swap 1 <-> 2), so that the kernels' matrix index is k = bit(lo) + 2 * bit(hi).
static U4Mat u4_ascending(unsigned q0, unsigned q1, const double *u)
{
    static const int swap12[4] = {0, 2, 1, 3};
    U4Mat U;
    for (int r = 0; r < 4; r++)
        for (int k = 0; k < 4; k++) {
            const int sr = q0 > q1 ? swap12[r] : r, sk = q0 > q1 ? swap12[k] : k;
            U.m[(4 * r + k) * 2] = u[(4 * sr + sk) * 2]; U.m[(4 * r + k) * 2 + 1] = u[(4 * sr + sk) * 2 + 1];
        }
    return U;
}

// Form selection (DESIGN s4.5g).  Knobs: u2_variant (0 = the plan, 1 = quad form for every qubit pair), u2_nt, u2_streams_log2
// (-1: the plain gate takes the Hadamard plan's streams for hi, the controlled gate the phase gate's rule -- both taken over
// from kernels that walk two address streams, as guesses until tools/time_two_qubit_gate.py has measured the four-stream walk).
extern "C" int qcx_shard_two_qubit(void *amp, unsigned n_local, unsigned q0, unsigned q1, int ctl, const double *u, void *stream)
{
    if (!amp || !u || n_local == 0 || n_local > 40) return QCX_BAD_ARGUMENTS;
    if (q0 >= n_local || q1 >= n_local || q0 == q1) return QCX_BAD_QUBIT;
    if (ctl >= 0 && ((unsigned)ctl >= n_local || (unsigned)ctl == q0 || (unsigned)ctl == q1)) return QCX_BAD_QUBIT;
    hipStream_t st = (hipStream_t)stream;
    amp_t *a = (amp_t *)amp;
    const U4Mat U = u4_ascending(q0, q1, u);
    const unsigned lo = q0 < q1 ? q0 : q1, hi = q0 < q1 ? q1 : q0, c = ctl >= 0 ? (unsigned)ctl : 0u;
    const unsigned lowest = (ctl >= 0 && c < lo) ? c : lo;
    const uint64_t namps = (uint64_t)1 << n_local;
    const Tune t = tune_now();
    long want = t.u2_streams_log2;
    if (want < 0) want = ctl < 0 ? h_plan(hi).slog : (lowest >= 8 ? 1 : 2);
    const bool nt = t.u2_nt != 0;
    if (t.u2_variant == 0 && n_local >= 9 && lowest < 3) {
        // line forms: where each target sits in the lane numbering once a control >= 3 is squeezed out
        const bool csq = ctl >= 3;
        const unsigned plo = lo - ((csq && c < lo) ? 1u : 0u), phi = hi - ((csq && c < hi) ? 1u : 0u);
        const int ns = (plo < 6 ? 1 : 0) + (phi < 6 ? 1 : 0);
        unsigned s[2] = {0, 0}, nsq = 0;                       // (csq means lo < 3, so ns >= 1: never more than two bits)
        if (plo >= 6) s[nsq++] = lo;
        if (phi >= 6) s[nsq++] = hi;
        if (csq) s[nsq++] = c;
        if (nsq == 2 && s[1] < s[0]) std::swap(s[0], s[1]);
        const uint64_t count = namps >> nsq, cset = csq ? (uint64_t)1 << c : 0;
        const unsigned clow = (ctl >= 0 && !csq) ? 1u << c : 0u, mlo = 1u << (plo & 31u), mhi = 1u << (phi & 31u);
        const int store_all = (ctl >= 0 && c < 2) ? 1 : 0;
        const unsigned grid = grid_for(count, 64, 0, 64);
        unsigned glog, slog;
        stream_map(grid, (uint64_t)grid * 64, count, want, &glog, &slog);
        const auto lines = [&](auto nsv) { flag_dispatch(nt, [&](auto ntv) {
            hipLaunchKernelGGL((k_u2_lines<decltype(nsv)::value, decltype(ntv)::value>), dim3(grid), dim3(64), 0, st, a, lo, hi, mlo, mhi, nsq, s[0], s[1], cset, clow, store_all, U, count, glog, slog);
        }); };
        if (ns == 2)      lines(std::integral_constant<int, 2>());
        else if (ns == 1) lines(std::integral_constant<int, 1>());
        else              lines(std::integral_constant<int, 0>());
    } else {
        const bool ntq = nt && lowest >= 3;                    // nontemporal only where a wave instruction covers whole 128-B lines
        if (ctl < 0) { if (ntq) launch_u2_quad<true, false>(a, lo, hi, 0, U, namps >> 2, want, st); else launch_u2_quad<false, false>(a, lo, hi, 0, U, namps >> 2, want, st); }
        else         { if (ntq) launch_u2_quad<true, true>(a, lo, hi, c, U, namps >> 3, want, st);  else launch_u2_quad<false, true>(a, lo, hi, c, U, namps >> 3, want, st); }
    }
    return launch_status("two-qubit gate");
}

// ---- the argument checks the masked and the table gates share ------------------------------------------------------------------------
// Each caller runs them in the order its header documents, on n <= 40 qubits.  Only the first writes a text (`who` names the
// caller in it): the QCX_BAD_QUBIT refusals leave qcx_last_error() as it stands.
static int check_ctrl_values(const char *who, uint64_t cmask, uint64_t cvals)
{
    if (cvals & ~cmask) { set_error("%s: ctrl_values %#llx has bits outside ctrl_mask %#llx", who, (unsigned long long)cvals, (unsigned long long)cmask); return QCX_BAD_ARGUMENTS; }
    return QCX_NO_ERROR;
}
static int check_targets(unsigned n, unsigned k, const unsigned *targets, uint64_t *tmask)       // k distinct qubits below n; *tmask: their bits
{
    *tmask = 0;
    for (unsigned j = 0; j < k; j++) {
        if (targets[j] >= n || ((*tmask >> targets[j]) & 1u)) return QCX_BAD_QUBIT;
        *tmask |= (uint64_t)1 << targets[j];
    }
    return QCX_NO_ERROR;
}
static int check_range(unsigned n, unsigned first, unsigned num, uint64_t *range)                // [first, first + num) inside n qubits; *range (if asked for): its bits
{
    if (first > n || num > n - first) return QCX_BAD_QUBIT;
    if (range) *range = ((((uint64_t)1) << num) - 1u) << first;
    return QCX_NO_ERROR;
}
static int check_ctrl_mask(unsigned n, uint64_t cmask, uint64_t opmask)                          // no control at or above n or on a bit the operator acts on
{
    return ((cmask >> n) != 0 || (cmask & opmask) != 0) ? QCX_BAD_QUBIT : QCX_NO_ERROR;
}

// The ascending runs of set bits of `mask`, [run_pos[k], run_pos[k] + run_len[k]), k < *nruns.  false: more than `cap` of them
// (the first `cap` are listed).
static bool mask_runs(uint64_t mask, unsigned char *run_pos, unsigned char *run_len, unsigned cap, unsigned *nruns)
{
    for (*nruns = 0; mask != 0; ++*nruns) {
        const unsigned b = (unsigned)__builtin_ctzll(mask), len = (unsigned)__builtin_ctzll(~(mask >> b));
        if (*nruns == cap) return false;
        run_pos[*nruns] = (unsigned char)b; run_len[*nruns] = (unsigned char)len;
        mask &= ~(((((uint64_t)1) << len) - 1u) << b);
    }
    return true;
}

// ---- K17: a one- or two-qubit gate under a control mask (include/qcx_plan.h states the rule, DESIGN s4.5m) ------------------------
// the checks of the plan and of the gate calls, in the header's order
static int mc_check(const char *who, unsigned n, uint64_t cmask, uint64_t cvals, unsigned ntargets, unsigned q0, unsigned q1)
{
    const unsigned targets[2] = {q0, q1};
    uint64_t tmask;
    QCX_TRY(check_ctrl_values(who, cmask, cvals));
    QCX_TRY(check_targets(n, ntargets, targets, &tmask));
    return check_ctrl_mask(n, cmask, tmask);
}

// The ONE place that decides the form, the numbering and the launch geometry, for arguments that passed mc_check(); mc_launch()
// below launches what it returns.
static int mc_gate_rule(const Tune &t, unsigned n, uint64_t cmask, uint64_t cvals, unsigned ntargets, unsigned q0, unsigned q1, qcx_mc_plan *out)
{
    const uint64_t tmask = ((uint64_t)1 << q0) | (ntargets == 2 ? (uint64_t)1 << q1 : 0);
    memset(out, 0, sizeof *out);
    const unsigned lo = ntargets == 2 && q1 < q0 ? q1 : q0, hi = ntargets == 2 ? (q0 < q1 ? q1 : q0) : q0;
    const uint64_t high = cmask & ~(uint64_t)7;
    const unsigned low = (unsigned)cmask & 7u;
    // the forms that keep whole lines: a target or a control inside a 128-B line, registers of 2^9 amplitudes or more
    bool lines = (lo < 3 || low != 0) && n >= 9 && t.ph_lines != 0 && (ntargets == 1 || t.u2_variant == 0);
    uint64_t squeezed = 0;
    unsigned form = 0, ns = 0, plo = 0, phi = 0;
    if (lines) {
        squeezed = high;
        if (ntargets == 1) {
            if (lo >= 3) squeezed |= tmask;
            form = lo < 3 ? QCX_MC_LINE_SHFL : QCX_MC_LINE_PAIR;
        } else {
            // where each target sits in the lane numbering once the high controls are squeezed out (lo in registers puts hi there too)
            plo = lo - (unsigned)__builtin_popcountll(high & (((uint64_t)1 << lo) - 1));
            phi = hi - (unsigned)__builtin_popcountll(high & (((uint64_t)1 << hi) - 1));
            if (plo >= 6) squeezed |= (uint64_t)1 << lo;
            if (phi >= 6) squeezed |= (uint64_t)1 << hi;
            ns = (plo < 6 ? 1u : 0u) + (phi < 6 ? 1u : 0u);
            form = QCX_MC_LINES2;
        }
        // the shuffle forms need whole waves: below 64 work items the pair / quad form (its traffic is irrelevant at that size)
        if ((n - (unsigned)__builtin_popcountll(squeezed)) < 6) lines = false;
    }
    if (!lines) {
        squeezed = cmask | tmask;
        form = ntargets == 1 ? QCX_MC_PAIR : QCX_MC_QUAD;
        ns = 0;
    }
    out->form = form; out->ns = ns;
    out->count = (uint64_t)1 << (n - (unsigned)__builtin_popcountll(squeezed));
    if (!mask_runs(squeezed, out->run_pos, out->run_len, QCX_MC_MAX_RUNS, &out->nruns)) { set_error("mc gate: more than %d runs of squeezed positions", QCX_MC_MAX_RUNS); return QCX_UNSUPPORTED; }
    out->or_const = cvals & squeezed;
    if (lines) { out->low_mask = low; out->low_values = (unsigned)cvals & 7u; out->store_all = (low & 3u) ? 1 : 0; }
    if (form == QCX_MC_LINES2 && ns >= 1) out->shfl_lo = 1u << plo;
    if (form == QCX_MC_LINES2 && ns == 2) out->shfl_hi = 1u << phi;
    // nontemporal only where a wave instruction covers whole 128-B lines
    out->nt = ((ntargets == 1 ? t.ph_nt : t.u2_nt) != 0 && (squeezed & 7u) == 0) ? 1 : 0;      // (K12's knob, K13's knob)
    out->block = 64; out->items_per_thread = 1;
    out->grid = grid_for(out->count, 64, 0, 64);
    long want = ntargets == 1 ? t.ph_streams_log2 : t.u2_streams_log2;
    if (want < 0) want = (squeezed & 255u) == 0 ? 1 : 2;             // the phase gate's rule: 1 when the lowest squeezed bit is >= 8
    stream_map(out->grid, (uint64_t)out->grid * 64, out->count, want, &out->glog, &out->slog);
    const char *b = out->nt ? "true" : "false";
    if (form == QCX_MC_LINE_SHFL) snprintf(out->kernel, sizeof out->kernel, "k_mcu_shfl<%s>", b);
    else if (ntargets == 1)       snprintf(out->kernel, sizeof out->kernel, "k_mcu_pair<%s>", b);
    else if (ns == 0)             snprintf(out->kernel, sizeof out->kernel, "k_mcu2_quad<%s>", b);
    else                          snprintf(out->kernel, sizeof out->kernel, "k_mcu2_lines<%u, %s>", ns, b);
    return QCX_NO_ERROR;
}

extern "C" int qcx_mc_gate_plan(unsigned n, uint64_t ctrl_mask, uint64_t ctrl_values, unsigned ntargets, unsigned qubit0, unsigned qubit1,
                                qcx_mc_plan *out)
{
    if (!out || (ntargets != 1 && ntargets != 2) || n == 0 || n > 40) return QCX_BAD_ARGUMENTS;
    QCX_TRY(mc_check("mc gate", n, ctrl_mask, ctrl_values, ntargets, qubit0, qubit1));
    return mc_gate_rule(tune_now(), n, ctrl_mask, ctrl_values, ntargets, qubit0, qubit1, out);
}

// launches what the plan says (u: the caller's 8 or 32 doubles)
static int mc_launch(amp_t *a, unsigned n, uint64_t cmask, uint64_t cvals, unsigned ntargets, unsigned q0, unsigned q1, const double *u, hipStream_t st)
{
    qcx_mc_plan pl;
    QCX_TRY(mc_gate_rule(tune_now(), n, cmask, cvals, ntargets, q0, q1, &pl));
    static_assert(MC_MAP_RUNS == QCX_MC_MAX_RUNS, "McMap holds the runs of a qcx_mc_plan");
    McMap M; memset(&M, 0, sizeof M);
    M.nruns = pl.nruns; M.orc = pl.or_const;
    for (unsigned k = 0; k < pl.nruns; k++) M.run[k] = (uint32_t)pl.run_pos[k] | ((uint32_t)pl.run_len[k] << 8);
    const dim3 grid(pl.grid), block(pl.block);
    const int sa = (int)pl.store_all;
    if (ntargets == 1) {
        const UMat U = {u[0], u[1], u[2], u[3], u[4], u[5], u[6], u[7]};
        flag_dispatch(pl.nt != 0, [&](auto nt) {
            if (pl.form == QCX_MC_LINE_SHFL) hipLaunchKernelGGL((k_mcu_shfl<decltype(nt)::value>), grid, block, 0, st, a, q0, M, pl.low_mask, pl.low_values, sa, U, pl.count, pl.glog, pl.slog);
            else                             hipLaunchKernelGGL((k_mcu_pair<decltype(nt)::value>), grid, block, 0, st, a, q0, M, pl.low_mask, pl.low_values, sa, U, pl.count, pl.glog, pl.slog);
        });
    } else {
        const U4Mat U = u4_ascending(q0, q1, u);
        const unsigned lo = q0 < q1 ? q0 : q1, hi = q0 < q1 ? q1 : q0;
        flag_dispatch(pl.nt != 0, [&](auto nt) {
            auto lines = [&](auto ns) {
                hipLaunchKernelGGL((k_mcu2_lines<decltype(ns)::value, decltype(nt)::value>), grid, block, 0, st, a, lo, hi, pl.shfl_lo, pl.shfl_hi, M, pl.low_mask, pl.low_values, sa, U, pl.count, pl.glog, pl.slog);
            };
            if (pl.form == QCX_MC_LINES2 && pl.ns == 2)      lines(std::integral_constant<int, 2>());
            else if (pl.form == QCX_MC_LINES2 && pl.ns == 1) lines(std::integral_constant<int, 1>());
            else hipLaunchKernelGGL((k_mcu2_quad<decltype(nt)::value>), grid, block, 0, st, a, lo, hi, M, pl.low_mask, pl.low_values, sa, U, pl.count, pl.glog, pl.slog);
        });
    }
    return launch_status("mc gate");
}

// ---- K14 / K15: the units of work of a Pauli string (PauliTiles in qcx_kernels.h) ------------------------------------------------
// Tiles of the T = min(n, 12) lowest index bits.  shape: 0 = no X or Y in the string, 1 = the partner i ^ x_mask inside the tile,
// 2 = in another tile: the units are pairs of tiles (n > 12: whole tiles); full: the tile has all 2^12 elements.
struct PauliUnits { unsigned T; uint64_t nunits; int shape; bool full; };
template <int SHAPE, bool FULL> struct PauliForm { static constexpr int shape = SHAPE; static constexpr bool full = FULL; };

static PauliUnits pauli_units(unsigned n, uint64_t x_mask)
{
    const unsigned T = std::min(n, 12u);
    const uint64_t ntiles = ((uint64_t)1) << (n - T);
    if (x_mask >> T) return {T, ntiles >> 1, 2, true};
    return {T, ntiles, x_mask ? 1 : 0, T == 12};
}

// launch(PauliForm<shape, full>()): the five forms both kernels are built in
template <class Launch> static void pauli_dispatch(const PauliUnits &pu, Launch launch)
{
    if (pu.shape == 2) launch(PauliForm<2, true>());
    else if (pu.full) { if (pu.shape) launch(PauliForm<1, true>()); else launch(PauliForm<0, true>()); }
    else { if (pu.shape) launch(PauliForm<1, false>()); else launch(PauliForm<0, false>()); }
}

// ---- K15: the rotation about a Pauli string -----------------------------------------------------------------------------------
// One launch for any string: the units and the grid are k_pauli_leaves' (tiles of the T = min(n, 12) lowest bits, pairs of tiles
// when the partner lies in another tile, at most prot_grid_cap = 2048 workgroups).  c and s are cos and sin of theta / 2.
extern "C" int qcx_shard_pauli_rotation(void *amp, unsigned n_local, uint64_t x_mask, uint64_t z_mask, double c, double s, void *stream)
{
    if (!amp || n_local == 0 || n_local > 40) return QCX_BAD_ARGUMENTS;
    if ((x_mask | z_mask) >> n_local) return QCX_BAD_QUBIT;
    const unsigned g = (unsigned)__builtin_popcountll(x_mask & z_mask) & 3u;
    // -i i^g s: (+0, -s), (s, +0), (+0, s), (-s, +0)
    const PRot R = {c, 0.0, g == 1 ? s : (g == 3 ? -s : 0.0), g == 0 ? -s : (g == 2 ? s : 0.0)};
    const PauliUnits pu = pauli_units(n_local, x_mask);
    const unsigned grid = grid_for(pu.nunits, 1, tune_now().prot_grid_cap, 256);
    pauli_dispatch(pu, [&](auto f) {
        hipLaunchKernelGGL((k_pauli_rot<f.shape, f.full>), dim3(grid), dim3(256), 0, (hipStream_t)stream, (amp_t *)amp, pu.nunits, pu.T, x_mask, z_mask, g, R);
    });
    return launch_status("pauli rotation");
}

// ---- K18: a diagonal on a qubit range from a table ------------------------------------------------------------------------------
// the rule of include/qcx_plan.h, under one snapshot of the knobs
static int diagonal_plan(const Tune &t, unsigned n, unsigned first, unsigned num, qcx_diag_plan *out)
{
    if (!out || n == 0 || n > 40) return QCX_BAD_ARGUMENTS;
    QCX_TRY(check_range(n, first, num, nullptr));
    memset(out, 0, sizeof *out);
    const unsigned T = std::min(n, 12u);
    out->T = T; out->first = first; out->num = num;
    out->kmask = (((uint64_t)1) << num) - 1u;
    out->units = ((uint64_t)1) << (n - T);
    out->full = T == 12;
    out->elems = T > 8 ? 1u << (T - 8) : 1u;
    out->form = (num == 0 || first >= T) ? QCX_DIAG_TILE : (first >= 8 ? QCX_DIAG_GROUP : QCX_DIAG_LANE);
    out->slice_entries = out->form == QCX_DIAG_TILE ? 1 : ((uint64_t)1) << (std::min(first + num, T) - first);
    out->lds = out->form == QCX_DIAG_LANE && first + num <= 12 && t.diag_lds != 0;
    out->lds_bytes = out->lds ? 16u << num : 0;
    out->grid = grid_for(out->units, 1, t.diag_grid_cap, 256);
    out->block = 256;
    snprintf(out->kernel, sizeof out->kernel, "k_diagonal<%u, %s, %s>", out->form, out->full ? "true" : "false", out->lds ? "true" : "false");
    return QCX_NO_ERROR;
}

extern "C" int qcx_diagonal_plan(unsigned n, unsigned first, unsigned num, qcx_diag_plan *out)
{
    return diagonal_plan(tune_now(), n, first, num, out);
}

extern "C" int qcx_shard_diagonal(void *amp, unsigned n_local, unsigned first, unsigned num, const void *table_dev, void *stream)
{
    if (!amp || !table_dev) return QCX_BAD_ARGUMENTS;
    qcx_diag_plan pl;
    QCX_TRY(diagonal_plan(tune_now(), n_local, first, num, &pl));
    const dim3 grid(pl.grid), block(pl.block);
    // the (FORM, LDS) pairs the kernel is built in are written out below: only the lane form has an LDS variant
    const auto launch = [&](auto form, auto lds) { flag_dispatch(pl.full != 0, [&](auto full) {
        hipLaunchKernelGGL((k_diagonal<decltype(form)::value, decltype(full)::value, decltype(lds)::value>), grid, block, pl.lds_bytes,
                           (hipStream_t)stream, (amp_t *)amp, (const amp_t *)table_dev, pl.units, pl.T, pl.first, pl.kmask);
    }); };
    if (pl.form == QCX_DIAG_TILE)       launch(std::integral_constant<int, 0>(), std::false_type());
    else if (pl.form == QCX_DIAG_GROUP) launch(std::integral_constant<int, 1>(), std::false_type());
    else if (pl.lds)                    launch(std::integral_constant<int, 2>(), std::true_type());
    else                                launch(std::integral_constant<int, 2>(), std::false_type());
    return launch_status("diagonal gate");
}

// ---- the tile geometry K19 and K20 share ----------------------------------------------------------------------------------------
// Fills a plan's qcx_tile_geom in place by the rule include/qcx_plan.h states there, for an operator on the index bits `opmask`
// (num of them; the caller has checked them and the controls) and a tile of at most 2^want amplitudes.  strict: nothing is
// squeezed and no predicate is split; the caller takes the controls whole.
static void tile_geometry(unsigned n, uint64_t cmask, uint64_t cvals, uint64_t opmask, unsigned num, bool strict, unsigned want, qcx_tile_geom *G)
{
    memset(G, 0, sizeof *G);
    const uint64_t nmask = (((uint64_t)1) << n) - 1u;
    const uint64_t squeezed = strict ? 0 : cmask & ~(uint64_t)7;
    const unsigned unsq = n - (unsigned)__builtin_popcountll(squeezed);
    const unsigned T = std::min(std::min(12u, unsq), want);
    uint64_t tile = opmask, others = nmask & ~(squeezed | opmask);
    for (unsigned k = num; k < T; k++) { tile |= others & (0 - others); others &= others - 1; }
    G->T = T; G->tile_mask = tile; G->unit_mask = others;
    { unsigned k = 0; for (uint64_t m = tile; m; m &= m - 1) G->tile_bits[k++] = (unsigned char)__builtin_ctzll(m); }
    G->squeezed = squeezed; G->or_const = cvals & squeezed;
    (void)mask_runs(squeezed, G->run_pos, G->run_len, QCX_PERM_MAX_RUNS, &G->nruns);         // (at most 19 runs above bit 2 of 40 bits)
    if (!strict) {
        const uint64_t pmask = cmask & ~squeezed, pvals = cvals & ~squeezed;
        G->elem_mask = (unsigned)(pmask & tile); G->elem_values = (unsigned)(pvals & tile);
        G->unit_mask_low = (unsigned)(pmask & ~tile); G->unit_values_low = (unsigned)(pvals & ~tile);
    }
    G->units = ((uint64_t)1) << (unsq - T);
    G->form = (tile & 7u & nmask) == (7u & nmask) ? QCX_PERM_LINES : QCX_PERM_SHARED;
}

// ---- K19: a permutation of a qubit range's basis states from a table ---------------------------------------------------------------
static PermParams perm_params(const qcx_perm_plan &pl, uint64_t pmask, uint64_t pvals)        // pmask / pvals: the controls that are predicates
{
    const qcx_tile_geom &G = pl.geom;
    return {G.tile_mask, G.unit_mask, G.or_const, pmask, pvals, G.units, G.T, pl.range_pos, pl.num, (int)pl.store_all};
}

// the rule of include/qcx_plan.h, under one snapshot of the knobs.  strict: the pass of a register flagged non-finite -- nothing
// squeezed, every control a predicate (P->pmask); otherwise P->pmask holds the controls below bit 3
static int permutation_plan(const Tune &t, unsigned n, uint64_t cmask, uint64_t cvals, unsigned first, unsigned num, bool strict,
                            qcx_perm_plan *out, PermParams *P)
{
    if (!out || n == 0 || n > 40) return QCX_BAD_ARGUMENTS;
    uint64_t range;
    QCX_TRY(check_ctrl_values("permutation_gate", cmask, cvals));
    QCX_TRY(check_range(n, first, num, &range));
    QCX_TRY(check_ctrl_mask(n, cmask, range));
    if (num > QCX_PERM_MAX_QUBITS) {
        set_error("permutation_gate: a table over %u qubits is more than the %u a tile holds", num, (unsigned)QCX_PERM_MAX_QUBITS);
        return QCX_BAD_ARGUMENTS;
    }
    memset(out, 0, sizeof *out);
    const unsigned want = (unsigned)std::min<long>(12, std::max<long>(0, t.perm_tile_log2));
    qcx_tile_geom &G = out->geom;
    tile_geometry(n, cmask, cvals, range, num, strict, std::max(num + 3u, want), &G);
    const uint64_t pmask = cmask & ~G.squeezed, pvals = cvals & ~G.squeezed;
    out->first = first; out->num = num;
    out->range_pos = (unsigned)__builtin_popcountll(G.tile_mask & ((((uint64_t)1) << first) - 1u));
    out->block = G.T == 12 ? 1024 : 256;
    out->grid = grid_for(G.units, 1, t.perm_grid_cap, out->block);
    out->lds_bytes = (16u << G.T) + (((2u << num) + 15u) & ~15u);
    out->store_all = (!strict && t.perm_store_all != 0 && pmask != 0) ? 1 : 0;
    out->nt = (!strict && t.perm_nt != 0) ? 1 : 0;
    snprintf(out->kernel, sizeof out->kernel, "k_perm_tile<%s, %s>", strict ? "true" : "false", out->nt ? "true" : "false");
    if (P) *P = perm_params(*out, pmask, pvals);
    return QCX_NO_ERROR;
}

extern "C" int qcx_permutation_plan(unsigned n, uint64_t ctrl_mask, uint64_t ctrl_values, unsigned first, unsigned num, qcx_perm_plan *out)
{
    return permutation_plan(tune_now(), n, ctrl_mask, ctrl_values, first, num, false, out, nullptr);
}

// The table's check and its inverse, on the host: inv[perm[k]] = k for a bijection of [0, 2^num), num <= QCX_PERM_MAX_QUBITS; the
// first entry that is out of range or repeats a value is named.  moved = the number of k with perm[k] != k.
static int permutation_invert(unsigned num, const uint32_t *perm, uint16_t *inv, unsigned long *moved)
{
    const uint32_t entries = 1u << num;
    for (uint32_t k = 0; k < entries; k++) inv[k] = 0xFFFFu;               // (no entry: every value is below 2^12)
    *moved = 0;
    for (uint32_t k = 0; k < entries; k++) {
        const uint32_t v = perm[k];
        if (v >= entries) { set_error("permutation_gate: entry %u is %u, which is not below 2^%u", k, v, num); return QCX_BAD_ARGUMENTS; }
        if (inv[v] != 0xFFFFu) { set_error("permutation_gate: entry %u is %u, the value entry %u already has: not a bijection", k, v, (unsigned)inv[v]); return QCX_BAD_ARGUMENTS; }
        inv[v] = (uint16_t)k;
        if (v != k) ++*moved;
    }
    return QCX_NO_ERROR;
}

// launches what the plan says; inv_dev: the inverse table in device memory, complete in stream order
static int permutation_launch(amp_t *a, unsigned n, uint64_t cmask, uint64_t cvals, unsigned first, unsigned num, bool strict,
                              const uint16_t *inv_dev, hipStream_t st)
{
    qcx_perm_plan pl;
    PermParams P;
    QCX_TRY(permutation_plan(tune_now(), n, cmask, cvals, first, num, strict, &pl, &P));
    const dim3 grid(pl.grid), block(pl.block);
    if (strict)     hipLaunchKernelGGL((k_perm_tile<true, false>), grid, block, pl.lds_bytes, st, a, inv_dev, P, 1.0, 0.0);
    else if (pl.nt) hipLaunchKernelGGL((k_perm_tile<false, true>), grid, block, pl.lds_bytes, st, a, inv_dev, P, 1.0, 0.0);
    else            hipLaunchKernelGGL((k_perm_tile<false, false>), grid, block, pl.lds_bytes, st, a, inv_dev, P, 1.0, 0.0);
    return launch_status("permutation gate");
}

// ---- K20: a dense matrix on 1 .. 5 target qubits --------------------------------------------------------------------------------
static MultiParams multi_params(const qcx_multi_plan &pl)
{
    const qcx_tile_geom &G = pl.geom;
    unsigned emask = 0;
    for (unsigned j = 0; j < pl.num_targets; j++) emask |= 1u << pl.target_pos[j];
    return {G.tile_mask, G.unit_mask, G.or_const, G.units, G.elem_mask, G.elem_values, G.T, emask, (int)pl.store_all};
}

// the rule of include/qcx_plan.h, under one snapshot of the knobs: K19's geometry (tile_geometry) with the target set as the
// operator's bits.  (A register flagged non-finite does not come here: its strict pass has no tiles.)
static int multi_plan(const Tune &t, unsigned n, uint64_t cmask, uint64_t cvals, unsigned k, const unsigned *targets, qcx_multi_plan *out,
                      MultiParams *P)
{
    if (!out || !targets || n == 0 || n > 40) return QCX_BAD_ARGUMENTS;
    if (k == 0 || k > QCX_MULTI_MAX_TARGETS) {
        set_error("mc_multi_qubit_gate: %u targets; a matrix acts on 1 to %u qubits", k, (unsigned)QCX_MULTI_MAX_TARGETS);
        return QCX_BAD_ARGUMENTS;
    }
    uint64_t tmask;
    QCX_TRY(check_ctrl_values("mc_multi_qubit_gate", cmask, cvals));
    QCX_TRY(check_targets(n, k, targets, &tmask));
    QCX_TRY(check_ctrl_mask(n, cmask, tmask));
    memset(out, 0, sizeof *out);
    qcx_tile_geom &G = out->geom;
    tile_geometry(n, cmask, cvals, tmask, k, false, 12, &G);
    out->num_targets = k;
    for (unsigned j = 0; j < k; j++) {
        out->targets[j] = (unsigned char)targets[j];
        out->target_pos[j] = (unsigned char)__builtin_popcountll(G.tile_mask & ((((uint64_t)1) << targets[j]) - 1u));
    }
    out->rows_per_item = k == 1 ? 2 : 4;
    out->block = std::min(1024u, std::max(64u, (1u << G.T) / out->rows_per_item));
    out->grid = grid_for(G.units, 1, t.multi_grid_cap, out->block);
    out->lds_bytes = 16u << G.T;
    out->store_all = (t.multi_store_all != 0 && (cmask & ~G.squeezed) != 0) ? 1 : 0;
    out->nt = t.multi_nt != 0 ? 1 : 0;
    snprintf(out->kernel, sizeof out->kernel, "k_multi_tile<%u, %s>", k, out->nt ? "true" : "false");
    if (P) *P = multi_params(*out);
    return QCX_NO_ERROR;
}

extern "C" int qcx_multi_gate_plan(unsigned n, uint64_t ctrl_mask, uint64_t ctrl_values, unsigned num_targets, const unsigned *targets,
                                   qcx_multi_plan *out)
{
    return multi_plan(tune_now(), n, ctrl_mask, ctrl_values, num_targets, targets, out, nullptr);
}

// The matrix as the kernels take it: m = P u P, row and column c the c-th amplitude of a group in ascending state index, laid out
// column-major, mt[2 (c 2^k + r)] = m[r][c] (re, im).  rank[j] = how many targets lie below targets[j]: bit j of the caller's
// index is bit rank[j] of the ascending one.  sorted: the targets ascending.
static void multi_ascending(unsigned k, const unsigned *targets, const double *u, double *mt, unsigned char *sorted)
{
    unsigned rank[QCX_MULTI_MAX_TARGETS], given[1u << QCX_MULTI_MAX_TARGETS];
    for (unsigned j = 0; j < k; j++) {
        rank[j] = 0;
        for (unsigned i = 0; i < k; i++) rank[j] += targets[i] < targets[j];
        sorted[rank[j]] = (unsigned char)targets[j];
    }
    const unsigned d = 1u << k;
    for (unsigned c = 0; c < d; c++) {
        given[c] = 0;
        for (unsigned j = 0; j < k; j++) given[c] |= ((c >> rank[j]) & 1u) << j;
    }
    for (unsigned r = 0; r < d; r++)
        for (unsigned c = 0; c < d; c++) {
            const double *e = u + 2u * (given[r] * d + given[c]);
            mt[2u * (c * d + r)] = e[0]; mt[2u * (c * d + r) + 1u] = e[1];
        }
}

// launches what the plan says (strict: the one pass over every group of a register flagged non-finite); mt_dev: multi_ascending's
// matrix in device memory, complete in stream order; sorted: the targets ascending
static int multi_launch(amp_t *a, unsigned n, uint64_t cmask, uint64_t cvals, unsigned k, const unsigned *targets, const unsigned char *sorted,
                        bool strict, const double *mt_dev, hipStream_t st)
{
    if (strict) {
        MultiTargets tq; memset(&tq, 0, sizeof tq);
        for (unsigned j = 0; j < k; j++) tq.q[j] = sorted[j];
        const uint64_t dim = (uint64_t)1 << n;
        targets_dispatch(k, [&](auto kk) {
            hipLaunchKernelGGL((k_strict_multi<decltype(kk)::value>), dim3(grid_for(dim >> k, 256, 65536, 256)), dim3(256), 0, st, a, n, tq, cmask, cvals, mt_dev, 1.0, 0.0);
        });
        return launch_status("multi-qubit gate");
    }
    qcx_multi_plan pl;
    MultiParams P;
    QCX_TRY(multi_plan(tune_now(), n, cmask, cvals, k, targets, &pl, &P));
    const dim3 grid(pl.grid), block(pl.block);
    targets_dispatch(k, [&](auto kk) { flag_dispatch(pl.nt != 0, [&](auto nt) {
        hipLaunchKernelGGL((k_multi_tile<decltype(kk)::value, decltype(nt)::value>), grid, block, pl.lds_bytes, st, a, mt_dev, P);
    }); });
    return launch_status("multi-qubit gate");
}

// ---- K15b: a run of rotations in one pass (qcx_pauli_rotation_batch) -----------------------------------------------------------
extern "C" unsigned qcx_pauli_rotation_batch_width(void) { return QCX_PROT_RUN_W; }

// a mask's bits at and above 8: what a term asks of a pass's hot set
static inline uint64_t prot_hx(uint64_t x_mask) { return x_mask & ~(uint64_t)0xFF; }

// The passes of qcx_pauli_rotation_batch (include/qcx_plan.h states the rule): at most one pass is open; a wide term (more than
// four x bits at or above 8) closes it and is a pass of its own, any other joins it while it holds fewer than `width` terms and
// the hot set stays within four bits; a closing pass pads its hot set with the lowest qubits of [8, n) not in it.
extern "C" int qcx_pauli_rotation_batch_plan(unsigned n, unsigned long nterms, const uint64_t *x_masks, unsigned width,
                                             unsigned long *pass_of_term, unsigned long *npasses, unsigned *pass_kind, uint64_t *pass_hot)
{
    if (!npasses || width == 0 || n == 0 || n > 40 || (nterms && (!x_masks || !pass_of_term || !pass_kind || !pass_hot))) return QCX_BAD_ARGUMENTS;
    for (unsigned long k = 0; k < nterms; k++)
        if (x_masks[k] >> n) return QCX_BAD_QUBIT;
    const unsigned nhot = std::min(4u, std::max(n, 8u) - 8u);
    unsigned long np = 0;
    bool open = false;
    uint64_t H = 0;
    unsigned count = 0;
    auto close = [&]() {
        for (unsigned q = 8; q < n && (unsigned)__builtin_popcountll(H) < nhot; q++) H |= (uint64_t)1 << q;
        pass_kind[np] = 0; pass_hot[np] = H;
        np++; open = false;
    };
    for (unsigned long k = 0; k < nterms; k++) {
        const uint64_t hx = prot_hx(x_masks[k]);
        if (__builtin_popcountll(hx) > 4) {
            if (open) close();
            pass_kind[np] = 1; pass_hot[np] = 0;
            pass_of_term[k] = np++;
            continue;
        }
        if (open && !(count < width && __builtin_popcountll(H | hx) <= 4)) close();
        if (!open) { open = true; H = 0; count = 0; }
        H |= hx; count++;
        pass_of_term[k] = np;
    }
    if (open) close();
    *npasses = np;
    return QCX_NO_ERROR;
}

// One pass, the launch alone: the nterms <= W rotations (x_masks, z_masks, cs, ss)[0 .. nterms) in order, over the tile of index
// bits 0-7 and hot_mask.  hot_mask must be what the plan gives a pass: min(4, max(n, 8) - 8) bits of [8, n), covering every
// term's x bits at and above 8 (else QCX_BAD_ARGUMENTS: nothing outside the tile can be reached).
extern "C" int qcx_shard_pauli_rotation_run(void *amp, unsigned n_local, uint64_t hot_mask, unsigned nterms, const uint64_t *x_masks,
                                            const uint64_t *z_masks, const double *cs, const double *ss, void *stream)
{
    if (!amp || n_local == 0 || n_local > 40 || nterms == 0 || nterms > QCX_PROT_RUN_W || !x_masks || !z_masks || !cs || !ss) return QCX_BAD_ARGUMENTS;
    for (unsigned k = 0; k < nterms; k++)
        if ((x_masks[k] | z_masks[k]) >> n_local) return QCX_BAD_QUBIT;
    const unsigned nhot = std::min(4u, std::max(n_local, 8u) - 8u);
    if ((hot_mask & 0xFF) || (hot_mask >> n_local) || (unsigned)__builtin_popcountll(hot_mask) != nhot) {
        set_error("pauli rotation run: hot mask %#llx is not %u bits of [8, %u)", (unsigned long long)hot_mask, nhot, n_local);
        return QCX_BAD_ARGUMENTS;
    }
    unsigned hpos[4], nh = 0;
    for (unsigned q = 8; q < n_local; q++)
        if (hot_mask >> q & 1u) hpos[nh++] = q;
    for (unsigned q = 8; nh < 4; q++)                               // (n < 12: the tile-local bits that do not exist keep their own place)
        if (!(hot_mask >> q & 1u)) hpos[nh++] = q;
    std::sort(hpos, hpos + 4);
    auto local = [&](uint64_t m) {                                  // the tile's bits of a mask, squeezed: 0-7, then the hot bits
        unsigned v = (unsigned)m & 255u;
        for (unsigned b = 0; b < 4; b++) v |= (unsigned)(m >> hpos[b] & 1u) << (8u + b);
        return v;
    };
    PRotRun run = {};
    bool diag = true;
    for (unsigned k = 0; k < nterms; k++) {
        const uint64_t x = x_masks[k], z = z_masks[k];
        if (prot_hx(x) & ~hot_mask) {
            set_error("pauli rotation run: term %u's x_mask %#llx leaves the tile of hot mask %#llx", k, (unsigned long long)x, (unsigned long long)hot_mask);
            return QCX_BAD_ARGUMENTS;
        }
        const unsigned g = (unsigned)__builtin_popcountll(x & z) & 3u, x_loc = local(x), z_loc = local(z);
        const double c = cs[k], s = ss[k];
        unsigned odd = 0;
        for (unsigned j = 0; j < 16; j++) {
            odd |= (unsigned)(__builtin_popcount(j & (z_loc >> 8)) & 1) << j;
            odd |= (unsigned)((__builtin_popcount((j ^ (x_loc >> 8)) & (z_loc >> 8)) + __builtin_popcount(x_loc & z_loc & 255u)) & 1) << (16u + j);
        }
        run.t[k].z_mask = z;
        run.t[k].R = {c, 0.0, g == 1 ? s : (g == 3 ? -s : 0.0), g == 0 ? -s : (g == 2 ? s : 0.0)};      // (qcx_shard_pauli_rotation's)
        run.t[k].loc = x_loc | z_loc << 12 | g << 24;
        run.t[k].odd = odd;
        diag = diag && x_loc == 0;
    }
    const bool full = n_local >= 12;
    const uint64_t nunits = full ? ((uint64_t)1) << (n_local - 12) : 1;
    const unsigned grid = grid_for(nunits, 1, tune_now().prot_grid_cap, 256);
    const unsigned hot = hpos[0] | hpos[1] << 8 | hpos[2] << 16 | hpos[3] << 24;
#define QCX_PROT_RUN(DIAG, FULL) hipLaunchKernelGGL((k_prot_run<DIAG, FULL>), dim3(grid), dim3(256), 0, (hipStream_t)stream, (amp_t *)amp, nunits, n_local, hot, nterms, run)
    if (full) { if (diag) QCX_PROT_RUN(true, true); else QCX_PROT_RUN(false, true); }
    else      { if (diag) QCX_PROT_RUN(true, false); else QCX_PROT_RUN(false, false); }
#undef QCX_PROT_RUN
    return launch_status("pauli rotation run");
}

// ---- K12b / K13b: a run of one- and two-qubit gates in one pass (qcx_gate_batch) ------------------------------------------------
extern "C" unsigned qcx_gate_batch_width(void) { return QCX_GATE_RUN_W; }

// The passes of qcx_gate_batch (include/qcx_plan.h states the rule): qcx_pauli_rotation_batch_plan's walk with a budget in units
// instead of a term count, and no wide gate -- two targets never ask for more than two hot bits.  A gate always fits an empty pass.
extern "C" int qcx_gate_batch_plan(unsigned n, unsigned long ngates, const uint64_t *target_masks, const unsigned *units, unsigned width,
                                   unsigned long *pass_of_gate, unsigned long *npasses, uint64_t *pass_hot)
{
    if (!npasses || width == 0 || n == 0 || n > 40 || (ngates && (!target_masks || !units || !pass_of_gate || !pass_hot))) return QCX_BAD_ARGUMENTS;
    for (unsigned long k = 0; k < ngates; k++)
        if (units[k] != 1 && units[k] != 4) return QCX_BAD_ARGUMENTS;
    for (unsigned long k = 0; k < ngates; k++)
        if ((target_masks[k] >> n) || (unsigned)__builtin_popcountll(target_masks[k]) != (units[k] == 1 ? 1u : 2u)) return QCX_BAD_QUBIT;
    const unsigned nhot = std::min(4u, std::max(n, 8u) - 8u);
    unsigned long np = 0;
    bool open = false;
    uint64_t H = 0;
    unsigned long used = 0;
    auto close = [&]() {
        for (unsigned q = 8; q < n && (unsigned)__builtin_popcountll(H) < nhot; q++) H |= (uint64_t)1 << q;
        pass_hot[np] = H;
        np++; open = false;
    };
    for (unsigned long k = 0; k < ngates; k++) {
        const uint64_t hx = prot_hx(target_masks[k]);
        if (open && !(used + units[k] <= width && __builtin_popcountll(H | hx) <= 4)) close();
        if (!open) { open = true; H = 0; used = 0; }
        H |= hx; used += units[k];
        pass_of_gate[k] = np;
    }
    if (open) close();
    *npasses = np;
    return QCX_NO_ERROR;
}

// a gate's qubits against n: in range and distinct (the matrix is not looked at)
static bool gate_qubits_ok(const qcx_gate &g, unsigned n)
{
    if (g.qubit0 >= n) return false;
    if (g.ntargets == 2 && (g.qubit1 >= n || g.qubit1 == g.qubit0)) return false;
    if (g.control >= 0 && ((unsigned)g.control >= n || (unsigned)g.control == g.qubit0 || (g.ntargets == 2 && (unsigned)g.control == g.qubit1))) return false;
    return true;
}

static inline uint64_t gate_targets(const qcx_gate &g)
{
    return ((uint64_t)1 << g.qubit0) | (g.ntargets == 2 ? (uint64_t)1 << g.qubit1 : 0);
}

// One pass, the launch alone: the gates in order over the tile of index bits 0-7 and hot_mask.  hot_mask must be what the plan
// gives a pass and hold every gate's targets at and above 8 (else QCX_BAD_ARGUMENTS: nothing outside the tile can be reached).
extern "C" int qcx_shard_gate_run(void *amp, unsigned n_local, uint64_t hot_mask, unsigned ngates, const struct qcx_gate *gates, void *stream)
{
    if (!amp || n_local == 0 || n_local > 40 || ngates == 0 || ngates > QCX_GATE_RUN_W || !gates) return QCX_BAD_ARGUMENTS;
    unsigned units = 0;
    for (unsigned k = 0; k < ngates; k++) {
        if (gates[k].ntargets != 1 && gates[k].ntargets != 2) return QCX_BAD_ARGUMENTS;
        units += gates[k].ntargets == 2 ? 4u : 1u;
    }
    if (units > QCX_GATE_RUN_W) { set_error("gate run: %u units are more than the %u of one pass", units, (unsigned)QCX_GATE_RUN_W); return QCX_BAD_ARGUMENTS; }
    for (unsigned k = 0; k < ngates; k++)
        if (!gate_qubits_ok(gates[k], n_local)) return QCX_BAD_QUBIT;
    const unsigned nhot = std::min(4u, std::max(n_local, 8u) - 8u);
    if ((hot_mask & 0xFF) || (hot_mask >> n_local) || (unsigned)__builtin_popcountll(hot_mask) != nhot) {
        set_error("gate run: hot mask %#llx is not %u bits of [8, %u)", (unsigned long long)hot_mask, nhot, n_local);
        return QCX_BAD_ARGUMENTS;
    }
    unsigned hpos[4], nh = 0;
    for (unsigned q = 8; q < n_local; q++)
        if (hot_mask >> q & 1u) hpos[nh++] = q;
    for (unsigned q = 8; nh < 4; q++)                               // (n < 12: the tile-local bits that do not exist keep their own place)
        if (!(hot_mask >> q & 1u)) hpos[nh++] = q;
    std::sort(hpos, hpos + 4);
    auto local = [&](unsigned q) -> unsigned {                      // a qubit's tile-local position, 255: not in the tile
        if (q < 8) return q;
        for (unsigned b = 0; b < 4; b++)
            if (hpos[b] == q) return 8u + b;
        return 255u;
    };
    GateRun run = {};
    bool lds = false;
    unsigned at = 0;
    for (unsigned k = 0; k < ngates; k++) {
        const qcx_gate &g = gates[k];
        if (prot_hx(gate_targets(g)) & ~hot_mask) {
            set_error("gate run: gate %u's targets %#llx leave the tile of hot mask %#llx", k, (unsigned long long)gate_targets(g), (unsigned long long)hot_mask);
            return QCX_BAD_ARGUMENTS;
        }
        const bool two = g.ntargets == 2;
        const unsigned lo = two && g.qubit1 < g.qubit0 ? g.qubit1 : g.qubit0, hi = two ? (g.qubit0 ^ g.qubit1 ^ lo) : 0u;
        const uint64_t p0 = local(lo), p1 = two ? local(hi) : 0u;   // (the deposit is monotone: lo < hi stays p0 < p1)
        const uint64_t cloc = g.control >= 0 ? local((unsigned)g.control) : 255u, cfull = g.control >= 0 ? (unsigned)g.control : 255u;
        run.w[at] = p0 | p1 << 8 | cloc << 16 | cfull << 24 | (uint64_t)g.ntargets << 32;
        if (two) { const U4Mat U = u4_ascending(g.qubit0, g.qubit1, g.u); memcpy(&run.w[at + 2], U.m, sizeof U.m); }
        else memcpy(&run.w[at + 2], g.u, 8 * sizeof(double));
        at += two ? 4u * QCX_GATE_UNIT : QCX_GATE_UNIT;
        lds = lds || lo < 8;
    }
    const bool full = n_local >= 12;
    const uint64_t nunits = full ? ((uint64_t)1) << (n_local - 12) : 1;
    const unsigned grid = grid_for(nunits, 1, tune_now().prot_grid_cap, 256);
    const unsigned hot = hpos[0] | hpos[1] << 8 | hpos[2] << 16 | hpos[3] << 24;
#define QCX_GATE_RUN(LDS, FULL) hipLaunchKernelGGL((k_gate_run<LDS, FULL>), dim3(grid), dim3(256), 0, (hipStream_t)stream, (amp_t *)amp, nunits, n_local, hot, ngates, run)
    if (full) { if (lds) QCX_GATE_RUN(true, true); else QCX_GATE_RUN(false, true); }
    else      { if (lds) QCX_GATE_RUN(true, false); else QCX_GATE_RUN(false, false); }
#undef QCX_GATE_RUN
    return launch_status("gate run");
}

static unsigned gcd_u32(unsigned a, unsigned b) { while (b) { unsigned t = a % b; a = b; b = t; } return a; }

// modular inverse of a mod m (gcd(a, m) == 1, m >= 1); 0 when m == 1
static unsigned modinv_u32(unsigned a, unsigned m)
{
    if (m == 1) return 0;
    long long t = 0, nt = 1, r = m, nr = a % m;
    while (nr != 0) {
        long long qd = r / nr;
        long long tmp = t - qd * nt; t = nt; nt = tmp;
        tmp = r - qd * nr; r = nr; nr = tmp;
    }
    if (t < 0) t += m;
    return (unsigned)t;
}

// M > 12: the 2^M-block does not fit an LDS tile -> in place through the device's staging buffer, a batch of blocks at a time
// (K3b: k_cam_big_gather / k_cam_big_scatter).  Works on any view (a whole register, a shard, a slice of at least one block).
static int shard_camodc_large(amp_t *a, unsigned n_local, unsigned M, unsigned C, unsigned A, int ctl, hipStream_t st, const Tune &tn)
{
    if (M > 26) return QCX_UNSUPPORTED;
    const uint64_t blk = (uint64_t)1 << M;
    const uint64_t fmax = (C < blk ? C : blk) - 1;
    const bool wraps = (uint64_t)(C - 1) * fmax > 0xffffffffULL;
    const bool closed = (ctl < 0 || ctl >= (int)M) && C <= blk && !wraps;        // as in qcx_shard_camodc
    CamBig P;
    memset(&P, 0, sizeof P);
    P.M = M; P.C = C;
    P.ctl = (ctl >= (int)M) ? ctl : -1;               // a control inside the M register is encoded in the table
    P.R = closed ? C : (unsigned)blk;
    P.chunks = (P.R + 1023u) / 1024u;
    const uint64_t all_blocks = (uint64_t)1 << (n_local - M);
    const uint64_t touched = (P.ctl >= 0) ? all_blocks >> 1 : all_blocks;
    if (touched == 0) return QCX_NO_ERROR;

    Workspace *w;
    QCX_TRY(workspace(&w));
    std::lock_guard<std::mutex> use(g_ws_use[w - g_ws]);     // table and staging buffer are per-device scratch: one user at a time
    const size_t row_bytes = (size_t)P.R * sizeof(amp_t);
    const size_t want = std::max<size_t>(row_bytes, std::min<size_t>((size_t)std::max<long>(tn.cam_stage_mb, 1) << 20, row_bytes * touched));
    {
        std::lock_guard<std::mutex> lock(g_ws_mutex);
        if (w->cam_stage_cap < want) {
            HIP_TRY(hipStreamSynchronize(st));
            if (w->cam_stage) HIP_TRY(hipFree(w->cam_stage));
            w->cam_stage = nullptr; w->cam_stage_cap = 0;
            if (hipMalloc(&w->cam_stage, want) != hipSuccess) {
                (void)hipGetLastError();
                set_error("hipMalloc(%zu bytes) for the staging buffer of a modular multiply with M = %u", want, M);
                return QCX_INSUFFICIENT_MEMORY;
            }
            w->cam_stage_cap = want;
        }
    }
    const uint32_t *d_off = nullptr, *d_srcs = nullptr;
    if (closed) {
        P.d = gcd_u32(A, C); P.Cd = C / P.d; P.inv = modinv_u32(A / P.d, P.Cd);
    } else {
        // CSR of sources per destination built as Q:611-654 maps them
        std::vector<uint32_t> cnt(blk + 1, 0), dst(blk);
        for (uint64_t f = 0; f < blk; f++) {
            uint32_t d = (uint32_t)f;
            const bool on = (ctl >= 0 && ctl < (int)M) ? ((f >> ctl) & 1u) : true;
            if (on && f < C) d = (uint32_t)(((uint32_t)(A * (uint32_t)f)) % C) & (uint32_t)(blk - 1);
            dst[f] = d; cnt[d + 1]++;
        }
        for (uint64_t g = 0; g < blk; g++) cnt[g + 1] += cnt[g];
        std::vector<uint32_t> tab(2 * blk + 1);
        memcpy(tab.data(), cnt.data(), (blk + 1) * sizeof(uint32_t));
        std::vector<uint32_t> fill(cnt.begin(), cnt.end() - 1);
        for (uint64_t f = 0; f < blk; f++) tab[blk + 1 + fill[dst[f]]++] = (uint32_t)f;       // ascending f per destination
        const size_t need = tab.size() * sizeof(uint32_t);
        {
            std::lock_guard<std::mutex> lock(g_ws_mutex);
            if (w->tab_cap < need) {
                if (w->tab) HIP_TRY(hipFree(w->tab));
                w->tab = nullptr; w->tab_cap = 0;
                HIP_TRY(hipMalloc(&w->tab, need));
                w->tab_cap = need;
            }
        }
        HIP_TRY(hipStreamSynchronize(st));                   // the previous table may still be in use
        HIP_TRY(hipMemcpy(w->tab, tab.data(), need, hipMemcpyHostToDevice));
        d_off = w->tab; d_srcs = w->tab + blk + 1;
    }
    const uint64_t per_batch = std::max<uint64_t>(1, w->cam_stage_cap / row_bytes);
    for (uint64_t first = 0; first < touched; first += per_batch) {
        P.first = first; P.nblk = std::min<uint64_t>(per_batch, touched - first);
        const uint64_t items = ((P.nblk + 7) / 8) * P.chunks;                    // per XCD, at most
        const unsigned grid = 8u * (unsigned)std::min<uint64_t>(items, 1024);
        if (closed) hipLaunchKernelGGL((k_cam_big_gather<false>), dim3(grid), dim3(256), 0, st, (const amp_t *)a, w->cam_stage, P, d_off, d_srcs);
        else hipLaunchKernelGGL((k_cam_big_gather<true>), dim3(grid), dim3(256), 0, st, (const amp_t *)a, w->cam_stage, P, d_off, d_srcs);
        hipLaunchKernelGGL(k_cam_big_scatter, dim3(grid), dim3(256), 0, st, a, (const amp_t *)w->cam_stage, P);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));                       // rare path: table and staging buffer are free again when the lock is
    return QCX_NO_ERROR;
}

extern "C" int qcx_shard_camodc(void *amp, unsigned n_local, unsigned M, unsigned C, unsigned A, int ctl, void *stream)
{
    if (!amp || n_local > 40 || C == 0 || M > n_local) return QCX_BAD_ARGUMENTS;
    if (ctl >= (int)n_local) return QCX_BAD_QUBIT;
    A %= C;
    hipStream_t st = (hipStream_t)stream;
    amp_t *a = (amp_t *)amp;
    const Tune tn = tune_now();
    if (M > 12) return shard_camodc_large(a, n_local, M, C, A, ctl, st, tn);     // 2^M-block no longer fits the LDS tile

    CamodcParams P;
    memset(&P, 0, sizeof P);
    P.M = M;
    { const unsigned want = (unsigned)std::min<long>(12, std::max<long>(8, tn.cam_logT)); P.logT = (M < want) ? want : M; }     // tile: >= the 2^M block
    if (P.logT > n_local) P.logT = n_local;
    // a control at or above the M register is squeezed out of the tile numbering (tiles hold control-set amplitudes
    // only: half the vector is never read); that needs at least two tiles' worth of index space
    if (ctl >= (int)M && P.logT == n_local && P.logT > M) P.logT--;
    if (P.logT < M) return QCX_BAD_ARGUMENTS;
    P.ctl = ctl;
    P.C = C;
    P.skip = tn.cam_skip != 0; P.ntl = tn.cam_nt_lines != 0;
    const uint64_t blk = (uint64_t)1 << M;
    const uint64_t all_tiles = (uint64_t)1 << (n_local - P.logT);
    const uint64_t ctl_tiles = (ctl >= (int)M) ? all_tiles >> 1 : all_tiles;
    const size_t lds = ((size_t)16 << P.logT) + (((size_t)2 << M) + 15) / 16 * 16;       // tile + the source table of the permutation case

    // closed form is valid when the control is outside the M register, every residue fits the
    // register (C <= 2^M) and the reference's 32-bit product A*f cannot wrap (Q:598-600, Q:639)
    const uint64_t fmax = (C < blk ? C : blk) - 1;
    const bool wraps = (uint64_t)(C - 1) * fmax > 0xffffffffULL;
    const bool closed = (ctl < 0 || ctl >= (int)M) && C <= blk && !wraps;

    if (closed) {
        P.d = gcd_u32(A, C);            // gcd(0, C) = C
        P.Cd = C / P.d;
        P.inv = modinv_u32(A / P.d, P.Cd);
        P.ntiles = ctl_tiles;
        const unsigned grid = grid_for(P.ntiles, 1, tn.cam_grid_cap);
        // tiles of 2^12 amplitudes (M = 12) get 1024 threads: with 256 the two workgroups a CU's LDS holds are 8 waves, too few to
        // overlap their load -> barrier -> store chains (n = 30: 4.55 -> 3.25 ms; 2^11 tiles: 512 threads 3.27, 256 threads 3.14)
        const unsigned blockT = (tn.cam_block > 0) ? (unsigned)tn.cam_block : (P.logT >= 12 ? 1024u : 256u);
#define QCX_CAM_LAUNCH(B) hipLaunchKernelGGL((k_camodc<B>), dim3(grid), dim3(B), lds, st, a, P)
        if (blockT >= 1024) QCX_CAM_LAUNCH(1024); else if (blockT >= 512) QCX_CAM_LAUNCH(512); else QCX_CAM_LAUNCH(256);
#undef QCX_CAM_LAUNCH
        HIP_TRY(hipGetLastError());
        return QCX_NO_ERROR;
    }

    // generic path: CSR of sources per destination built as Q:611-654 maps them
    std::vector<uint32_t> cnt(blk + 1, 0), dst(blk);
    for (uint64_t f = 0; f < blk; f++) {
        uint32_t d = (uint32_t)f;
        const bool on = (ctl >= 0 && ctl < (int)M) ? ((f >> ctl) & 1u) : true;
        if (on && f < C) d = (uint32_t)(((uint32_t)(A * (uint32_t)f)) % C) & (uint32_t)(blk - 1);
        dst[f] = d;
        cnt[d + 1]++;
    }
    for (uint64_t g = 0; g < blk; g++) cnt[g + 1] += cnt[g];
    std::vector<uint32_t> tab(blk + 1 + blk);
    memcpy(tab.data(), cnt.data(), (blk + 1) * sizeof(uint32_t));
    std::vector<uint32_t> fill(cnt.begin(), cnt.end() - 1);
    for (uint64_t f = 0; f < blk; f++) tab[blk + 1 + fill[dst[f]]++] = (uint32_t)f;   // ascending f per destination

    Workspace *w;
    QCX_TRY(workspace(&w));
    std::lock_guard<std::mutex> use(g_ws_use[w - g_ws]);     // the table is per-device scratch: one user at a time
    const size_t need = tab.size() * sizeof(uint32_t);
    {
        std::lock_guard<std::mutex> lock(g_ws_mutex);
        if (w->tab_cap < need) {
            if (w->tab) HIP_TRY(hipFree(w->tab));
            w->tab = nullptr; w->tab_cap = 0;
            HIP_TRY(hipMalloc(&w->tab, need));
            w->tab_cap = need;
        }
    }
    HIP_TRY(hipStreamSynchronize(st));                       // the previous table may still be in use
    HIP_TRY(hipMemcpy(w->tab, tab.data(), need, hipMemcpyHostToDevice));
    CamodcParams Pt = P;
    Pt.d = 1; Pt.Cd = C; Pt.inv = 0;
    if (ctl >= 0 && ctl < (int)M) Pt.ctl = -1;               // the table already encodes the control
    Pt.ntiles = (Pt.ctl >= (int)M) ? all_tiles >> 1 : all_tiles;
    const unsigned grid = grid_for(Pt.ntiles, 1, tn.cam_grid_cap);
    hipLaunchKernelGGL((k_camodc_table<256>), dim3(grid), dim3(256), lds, st, a, Pt, w->tab, w->tab + blk + 1);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));                       // rare path: finish before the table can be replaced
    return QCX_NO_ERROR;
}

extern "C" int qcx_shard_swap_bits(const void *src, void *dst, unsigned n_local, unsigned npairs,
                                   const unsigned *pos_a, const unsigned *pos_b, void *stream)
{
    if (!src || !dst || src == dst || n_local > 40 || npairs > 8 || (npairs && (!pos_a || !pos_b))) return QCX_BAD_ARGUMENTS;
    SwapBits S;
    memset(&S, 0, sizeof S);
    S.npairs = npairs;
    for (unsigned m = 0; m < npairs; m++) {
        if (pos_a[m] >= n_local || pos_b[m] >= n_local || pos_a[m] == pos_b[m]) return QCX_BAD_QUBIT;
        S.a[m] = pos_a[m]; S.b[m] = pos_b[m];
    }
    const uint64_t count = (uint64_t)1 << n_local;
    hipLaunchKernelGGL((k_swap_bits<256>), dim3(grid_for(count, 256, 0, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const amp_t *)src, (amp_t *)dst, count, S);
    HIP_TRY(hipGetLastError());
    return QCX_NO_ERROR;
}

extern "C" int qcx_shard_norm2(const void *amp, unsigned n_local, double *out, void *stream)
{
    if (!amp || !out || n_local > 40) return QCX_BAD_ARGUMENTS;
    Workspace *w;
    QCX_TRY(workspace(&w));
    std::lock_guard<std::mutex> use(g_ws_use[w - g_ws]);
    hipStream_t st = (hipStream_t)stream;
    const uint64_t count = (uint64_t)1 << n_local;
    const unsigned grid = grid_for(count, 256 * 8, NORM_BLOCKS);
    hipLaunchKernelGGL((k_norm_partial<256>), dim3(grid), dim3(256), 0, st, (const amp_t *)amp, count, w->partials);
    hipLaunchKernelGGL(k_norm_final, dim3(1), dim3(64), 0, st, w->partials, grid, w->partials + NORM_BLOCKS);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(w->h_scalar, w->partials + NORM_BLOCKS, sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *out = *w->h_scalar;
    return QCX_NO_ERROR;
}

// the sampling scan's buffers (K4d): the record ends, the chunk carries of the segmented scan and its `bad` word
static int samp_reserve(Workspace *w, uint64_t nrec)
{
    std::lock_guard<std::mutex> lock(g_ws_mutex);
    if (w->samp_cap >= nrec) return QCX_NO_ERROR;
    if (w->samp_ends) { HIP_TRY(hipFree(w->samp_ends)); HIP_TRY(hipFree(w->samp_aux)); }
    w->samp_ends = nullptr; w->samp_aux = nullptr; w->samp_cap = 0;
    const uint64_t nch = (nrec + QCX_SAMP_CHUNK - 1) / QCX_SAMP_CHUNK;
    HIP_TRY(hipMalloc(&w->samp_ends, ((size_t)nrec + 1) * sizeof(double)));
    HIP_TRY(hipMalloc(&w->samp_aux, (2 * (size_t)nch + 2) * sizeof(SampCarry)));
    w->samp_cap = nrec;
    return QCX_NO_ERROR;
}

// The launches of one measurement scan of `count` amplitudes on stream st; the caller holds the device's scratch.  ends = true (the
// sampling scan, K4d): they also leave the exact running sum at the end of every record in w->samp_ends (2^*elog_out amplitudes per
// record, *nrec_out records) -- k_sample_seq where the single-wave scan would run, the ENDS forms of k_meas_fast / k_meas_walk
// otherwise, and then only the events' ends are there (*need_fill: the plain records' are still to be assembled).
static int meas_launch(Workspace *w, const void *amp, uint64_t count, double cum_in, double r, MeasureOut *res, hipStream_t st,
                       bool *parallel_out, bool ends, unsigned *elog_out, uint64_t *nrec_out, bool *need_fill)
{
    const Tune tn = tune_now();
    const bool parallel = tn.meas_parallel != 0 && count >= ((uint64_t)1 << tn.meas_min_log2);
    *parallel_out = parallel;
    if (!parallel && ends) {
        // (the sampling scan) the single-wave chain stores the sum at the end of every amplitude -- or of every 2^11 of a large register
        // scanned this way (meas_parallel = 0)
        const unsigned elog = count > ((uint64_t)1 << 16) ? 11u : 0u;
        const uint64_t nrec = (count + (((uint64_t)1 << elog) - 1)) >> elog;
        QCX_TRY(samp_reserve(w, nrec));
        hipLaunchKernelGGL(k_sample_seq, dim3(1), dim3(64), 0, st, (const amp_t *)amp, count, cum_in, elog, w->samp_ends);
        *elog_out = elog; *nrec_out = nrec; *need_fill = false;
    } else if (!parallel) {
        // small shards: the strictly sequential single-wave scan
        hipLaunchKernelGGL(k_measure_scan, dim3(1), dim3(64), 0, st, (const amp_t *)amp, count, cum_in, r, res);
    } else {
        // exact parallel form (qcx_kernels.h, K4c): one read of the state (look-back for the binade guesses), a few tiny group
        // launches, the tree walk.  A "block" of 2^blog amplitudes is one RECORD (one wave); a workgroup takes four of them.
        unsigned blog = (unsigned)tn.meas_block_log;
        if (blog == 0) {
            unsigned bits = 0;
            while (bits < 63 && ((uint64_t)1 << bits) < count) bits++;
            blog = bits ? (bits - 1) / 2 : 8;
        }
        blog = std::min<unsigned>(std::max<unsigned>(blog, 8u), 11u);     // a record is one wave's 2^8 .. 2^11 amplitudes
        // k_meas_onepass takes four records per 256-thread workgroup and a launch holds fewer than 2^32 threads: a record size
        // forced too small for the register (meas_block_log = 8 at n = 34) is raised, not refused
        while (blog < 11u && ((((count + (((uint64_t)1 << blog) - 1)) >> blog) + 3u) / 4u) * 256u > 0xffffffffULL) blog++;
        const uint64_t nb64 = (count + (((uint64_t)1 << blog) - 1)) >> blog;
        if (nb64 > 0x7fffffffULL) return QCX_UNSUPPORTED;
        const unsigned nblocks = (unsigned)nb64;
        {
            std::lock_guard<std::mutex> lock(g_ws_mutex);
            if (w->meas_cap < nblocks) {
                if (w->meas_blocks) { HIP_TRY(hipFree(w->meas_blocks)); HIP_TRY(hipFree(w->meas_look)); HIP_TRY(hipFree(w->meas_up)); }
                w->meas_blocks = nullptr; w->meas_cap = 0; w->meas_clean = false; w->meas_clean_slots = 0;
                w->meas_look = nullptr; w->meas_up = nullptr;
                HIP_TRY(hipMalloc(&w->meas_blocks, ((size_t)nblocks + 4) * sizeof(MeasBlock)));
                HIP_TRY(hipMalloc(&w->meas_look, (2 * (size_t)nblocks + 4 * ((size_t)nblocks / 64 + 2) + 8) * sizeof(meas_slot_t)));
                HIP_TRY(hipMalloc(&w->meas_up, ((size_t)nblocks / 32 + 16) * sizeof(MeasBlock)));
                w->meas_cap = nblocks;
            }
        }
        if (ends) {                                                 // every record "not redone yet" (all ones) before the scan
            QCX_TRY(samp_reserve(w, nblocks));
            HIP_TRY(hipMemsetAsync(w->samp_ends, 0xff, (size_t)nblocks * sizeof(double), st));
            *elog_out = blog; *nrec_out = nblocks; *need_fill = true;
        }
        double *const ends_p = ends ? w->samp_ends : nullptr;
        {
            const unsigned nwg = (nblocks + 3u) / 4u, ngrp = (nwg + 63u) / 64u;
            MeasLookback LB;
            LB.agg = w->meas_look; LB.incl = LB.agg + nwg; LB.gsum = LB.incl + nwg; LB.gincl = LB.gsum + ngrp;
            LB.ticket = w->meas_cands->ticket;                       // (a fixed address: the scan's last kernel leaves it at zero for the next one)
            const bool clean = w->meas_clean;
            const size_t nslots = 2 * (size_t)nwg + 2 * (size_t)ngrp;
            if (!clean || nslots > w->meas_clean_slots) HIP_TRY(hipMemsetAsync(w->meas_look, 0xff, nslots * sizeof(meas_slot_t), st));
            const size_t slots_after = clean ? std::max(w->meas_clean_slots, nslots) : nslots;
            w->meas_clean = false;                                  // (true again when this call has completed)
            if (!clean) HIP_TRY(hipMemsetAsync(w->meas_cands, 0, 6 * sizeof(unsigned), st));       // candidate count + ticket
            const unsigned spin = (unsigned)std::max<long>(1000, tn.meas_spin_limit);
#define QCX_ONEPASS(B) hipLaunchKernelGGL((k_meas_onepass<B>), dim3(nwg), dim3(256), 0, st, (const amp_t *)amp, count, cum_in, LB, w->meas_blocks, spin, (unsigned)tn.meas_dbg, r)
            switch (blog) {
            case 8: QCX_ONEPASS(8); break;   case 9: QCX_ONEPASS(9); break;   case 10: QCX_ONEPASS(10); break;
            default: QCX_ONEPASS(11); break;
            }
#undef QCX_ONEPASS
            MeasLevels T;
            memset(&T, 0, sizeof T);
            T.lv[0] = w->meas_blocks; T.n[0] = nblocks; T.top = 0;
            MeasBlock *up = w->meas_up;
            // the events of the scan go to k_meas_fast (the launch over the records lists them), the walk stands behind it
            const bool fast = tn.meas_fast != 0 && T.n[0] > 64u;
            while (T.n[T.top] > 64u && T.top < 4) {
                const unsigned nin = T.n[T.top], nout = (nin + 63u) / 64u;
                hipLaunchKernelGGL(k_meas_groups, dim3(nout), dim3(64), 0, st, T.lv[T.top], nin, up, (fast && T.top == 0) ? w->meas_cands : (MeasCands *)nullptr,
                                   T.top == 0 ? w->meas_look : (meas_slot_t *)nullptr, (unsigned)nslots);
                T.top++;
                T.lv[T.top] = up; T.n[T.top] = nout;
                up += nout;
            }
            if (fast) {
                if (ends)
                    hipLaunchKernelGGL(k_meas_fast<true>, dim3(1), dim3(512), 0, st, (const amp_t *)amp, count, T, cum_in, r, res, res->stats, blog,
                                       (const MeasCands *)w->meas_cands, w->meas_resume, (unsigned)tn.meas_dbg, ends_p);
                else
                    hipLaunchKernelGGL(k_meas_fast<false>, dim3(1), dim3(512), 0, st, (const amp_t *)amp, count, T, cum_in, r, res, res->stats, blog,
                                       (const MeasCands *)w->meas_cands, w->meas_resume, (unsigned)tn.meas_dbg, ends_p);
            }
            if (ends)
                hipLaunchKernelGGL(k_meas_walk<true>, dim3(1), dim3(64), 0, st, (const amp_t *)amp, count, T, cum_in, r, res, res->stats, blog,
                                   fast ? (const MeasResume *)w->meas_resume : (const MeasResume *)nullptr, w->meas_cands,
                                   T.top == 0 ? w->meas_look : (meas_slot_t *)nullptr, (unsigned)nslots, ends_p);
            else
                hipLaunchKernelGGL(k_meas_walk<false>, dim3(1), dim3(64), 0, st, (const amp_t *)amp, count, T, cum_in, r, res, res->stats, blog,
                                   fast ? (const MeasResume *)w->meas_resume : (const MeasResume *)nullptr, w->meas_cands,
                                   T.top == 0 ? w->meas_look : (meas_slot_t *)nullptr, (unsigned)nslots, ends_p);
            w->meas_slots_pending = slots_after;
        }
    }
    return QCX_NO_ERROR;
}

extern "C" int qcx_shard_measure_scan(const void *amp, unsigned n_local, uint64_t first_global,
                                      uint64_t last_excluded, double cum_in, double r,
                                      int *found, uint64_t *index, double *cum_out, void *stream)
{
    if (!amp || !found || !index || !cum_out || n_local > 40) return QCX_BAD_ARGUMENTS;
    Workspace *w;
    QCX_TRY(workspace(&w));
    std::lock_guard<std::mutex> use(g_ws_use[w - g_ws]);
    hipStream_t st = (hipStream_t)stream;
    uint64_t count = (uint64_t)1 << n_local;
    if (first_global >= last_excluded) count = 0;
    else if (last_excluded - first_global < count) count = last_excluded - first_global;
    if (count == 0) { *found = 0; *index = 0; *cum_out = cum_in; return QCX_NO_ERROR; }
    // The scan's last kernel writes its result (a MeasureOut, 32 bytes) STRAIGHT into pinned host memory (meas_host_out, round 5): the
    // copy back used to be one more operation on the stream -- a blit kernel, 6-10 us of an attempt that takes 27 us at n = 7 and
    // 100 us at n = 20.  The kernels only write it (what the fast scan leaves for the walk travels in MeasResume, device memory).
    MeasureOut *const res = tune_now().meas_host_out ? w->h_mout : w->mout;
    bool parallel = false, fill = false;
    unsigned elog = 0; uint64_t nrec = 0;
    QCX_TRY(meas_launch(w, amp, count, cum_in, r, res, st, &parallel, false, &elog, &nrec, &fill));
    HIP_TRY(hipGetLastError());
    if (res != w->h_mout) HIP_TRY(hipMemcpyAsync(w->h_mout, w->mout, sizeof(MeasureOut), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (parallel) { w->h_meas_stats[0] = w->h_mout->stats[0]; w->h_meas_stats[1] = w->h_mout->stats[1]; w->meas_clean = true; w->meas_clean_slots = w->meas_slots_pending; }
    *found = w->h_mout->found;
    *index = first_global + w->h_mout->index;
    *cum_out = w->h_mout->cum;
    return QCX_NO_ERROR;
}

// K4d: the answers of the measurement scan for `shots` draws r[] on the 2^n_local amplitudes at amp, from ONE scan of them, nothing
// written to the state.  out[i] (host) = the index (< last_excluded), QCX_SAMP_NOTFOUND or QCX_SAMP_FALLBACK (qcx_kernels.h)
static int sample_scan(const void *amp, unsigned n_local, uint64_t last_excluded, const double *r, size_t shots, uint64_t *out,
                       hipStream_t st)
{
    Workspace *w;
    QCX_TRY(workspace(&w));
    std::lock_guard<std::mutex> use(g_ws_use[w - g_ws]);
    const uint64_t count = (uint64_t)1 << n_local;
    MeasureOut *const res = tune_now().meas_host_out ? w->h_mout : w->mout;
    bool parallel = false, fill = false;
    unsigned elog = 0; uint64_t nrec = 0;
    QCX_TRY(meas_launch(w, amp, count, 0.0, INFINITY, res, st, &parallel, true, &elog, &nrec, &fill));
    SampCarry *const chunk_tot = w->samp_aux, *const chunk_pre = w->samp_aux + w->samp_nch_cap(), *const badw = chunk_pre + w->samp_nch_cap();
    unsigned *const bad = (unsigned *)badw;
    HIP_TRY(hipMemsetAsync(bad, 0, sizeof(unsigned), st));
    if (fill) {
        const uint64_t nch = (nrec + QCX_SAMP_CHUNK - 1) / QCX_SAMP_CHUNK;
        hipLaunchKernelGGL(k_samp_chunks, dim3((unsigned)nch), dim3(256), 0, st, (const MeasBlock *)w->meas_blocks, (const double *)w->samp_ends, nrec, chunk_tot);
        hipLaunchKernelGGL(k_samp_chunk_scan, dim3(1), dim3(256), 0, st, (const SampCarry *)chunk_tot, (unsigned)nch, chunk_pre);
        hipLaunchKernelGGL(k_samp_fill, dim3((unsigned)nch), dim3(256), 0, st, (const MeasBlock *)w->meas_blocks, w->samp_ends, nrec,
                           (const SampCarry *)chunk_pre, 0.0, bad);
    }
    HIP_TRY(hipGetLastError());
    // the shots, in batches (the draws in, the answers out: 16 bytes a shot)
    const size_t BATCH = (size_t)1 << 20;
    for (size_t s0 = 0; s0 < shots; s0 += BATCH) {
        const size_t k = std::min(BATCH, shots - s0);
        {
            std::lock_guard<std::mutex> lock(g_ws_mutex);
            if (w->samp_shot_cap < k) {
                if (w->samp_r) { HIP_TRY(hipFree(w->samp_r)); HIP_TRY(hipFree(w->samp_out)); }
                w->samp_r = nullptr; w->samp_out = nullptr; w->samp_shot_cap = 0;
                const size_t cap = std::max<size_t>(k, 1024);
                HIP_TRY(hipMalloc(&w->samp_r, cap * sizeof(double)));
                HIP_TRY(hipMalloc(&w->samp_out, cap * sizeof(uint64_t)));
                w->samp_shot_cap = cap;
            }
        }
        HIP_TRY(hipMemcpyAsync(w->samp_r, r + s0, k * sizeof(double), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_sample_shots, dim3((unsigned)((k + 3) / 4)), dim3(256), 0, st, (const amp_t *)amp, count, (const double *)w->samp_ends, nrec,
                           elog, 0.0, (const double *)w->samp_r, (uint64_t)k, last_excluded, (const unsigned *)bad, w->samp_out);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(out + s0, w->samp_out, k * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    if (parallel) { w->h_meas_stats[0] = w->h_mout->stats[0]; w->h_meas_stats[1] = w->h_mout->stats[1]; w->meas_clean = true; w->meas_clean_slots = w->meas_slots_pending; }
    return QCX_NO_ERROR;
}

// ---- K10: the stage plan of a marginal (include/qcx_plan.h, DESIGN s4.5d) ----------------------------------------------
// labels[b] = the register qubit that input index bit b stands for; a qubit in [first, first + num) is kept, the others summed.
// kind 0 / 1: tiles of up to 2^12 elements, the c = 3 (amplitudes) / 4 (partials) lowest bits first; kind 2 (compact blocks,
// >= 64 B each): up to 2^8 elements, c = 1.
static int marginal_plan_from(unsigned kind0, std::vector<unsigned> labels, uint64_t qubits0, unsigned first, unsigned num,
                              qcx_marginal_stage *stages, unsigned *n_stages)
{
    auto summed = [&](unsigned q) { return q < first || q >= first + num; };
    unsigned ns = 0;
    uint64_t off = 0;
    for (unsigned kind = kind0;; kind = 1) {
        if (ns >= QCX_MARGINAL_MAX_STAGES) return QCX_UNKNOWN_ERROR;
        const unsigned m = (unsigned)labels.size();
        const unsigned Tmax = kind == 2 ? 8u : 12u, cmin = kind == 0 ? 3u : (kind == 1 ? 4u : 1u);
        const unsigned c = std::min(cmin, m);
        uint64_t tile = c ? ((((uint64_t)1) << c) - 1u) : 0u;
        unsigned T = c;
        for (unsigned b = c; b < m && T < Tmax; b++)
            if (summed(labels[b])) { tile |= (uint64_t)1 << b; T++; }
        for (unsigned b = c; b < m && T < Tmax; b++)          // (no summed bit left outside the tile: fill it with kept bits)
            if (!(tile >> b & 1u)) { tile |= (uint64_t)1 << b; T++; }
        uint64_t sum = 0, qb = ns == 0 ? qubits0 : 0;
        for (unsigned b = 0; b < m; b++)
            if ((tile >> b & 1u) && summed(labels[b])) { sum |= (uint64_t)1 << b; qb |= (uint64_t)1 << labels[b]; }
        std::vector<unsigned> rest;
        bool more = false;
        for (unsigned b = 0; b < m; b++)
            if (!(sum >> b & 1u)) { rest.push_back(labels[b]); more |= summed(labels[b]); }
        qcx_marginal_stage &S = stages[ns++];
        memset(&S, 0, sizeof S);
        S.kind = kind; S.in_bits = m; S.T = T; S.c = c; S.tile_mask = tile; S.sum_mask = sum; S.qubits = qb;
        S.out_bits = (unsigned)rest.size();
        S.final_stage = more ? 0u : 1u;
        S.out_offset = more ? off : 0u;
        if (more) off += (uint64_t)1 << S.out_bits;
        labels.swap(rest);
        if (!more) break;
    }
    *n_stages = ns;
    return QCX_NO_ERROR;
}

extern "C" int qcx_marginal_plan(unsigned n, unsigned first, unsigned num, qcx_marginal_stage *stages, unsigned *n_stages)
{
    if (!stages || !n_stages) return QCX_BAD_ARGUMENTS;
    if (n < 1 || n > 40 || (uint64_t)first + num > n) return QCX_BAD_QUBIT;
    if (num > 30) return QCX_UNSUPPORTED;
    std::vector<unsigned> labels(n);
    for (unsigned b = 0; b < n; b++) labels[b] = b;
    return marginal_plan_from(0, labels, 0, first, num, stages, n_stages);
}

extern "C" int qcx_marginal_plan_compact(unsigned n, unsigned M, unsigned first, unsigned num, qcx_marginal_stage *stages, unsigned *n_stages)
{
    if (!stages || !n_stages) return QCX_BAD_ARGUMENTS;
    if (n < 1 || n > 40 || (uint64_t)first + num > n) return QCX_BAD_QUBIT;
    if (num > 30) return QCX_UNSUPPORTED;
    if (M < 1 || M >= n || first < M) return QCX_BAD_ARGUMENTS;
    std::vector<unsigned> labels(n - M);
    for (unsigned b = 0; b < n - M; b++) labels[b] = M + b;
    return marginal_plan_from(2, labels, (((uint64_t)1) << M) - 1u, first, num, stages, n_stages);
}

// ---- K16: the stage plan of a reduced density matrix (include/qcx_plan.h, DESIGN s4.5j) -----------------------------------------
// Stage 0 (k_rdm_leaves / k_rdm_small) sums the lowest summed qubits of every component: all of them below 12 qubits, else the
// 12 - num that share a unit of 2^12 amplitudes with the range and, from 22 qubits on, min(n - 21, 4) more: a workgroup adds the
// roots of that many consecutive units itself (at least 2^9 groups stay: two workgroups a CU).  Behind it the rows x 2^rest_bits partials are ONE marginal input
// whose kept bits are the row number, on top: the marginal's own planner cuts the rest of the tree.
extern "C" unsigned qcx_rdm_max_qubits(void) { return QCX_RDM_MAX_QUBITS; }

extern "C" int qcx_rdm_plan(unsigned n, unsigned first, unsigned num, qcx_rdm_stage0 *s0, qcx_marginal_stage *stages, unsigned *n_stages)
{
    if (!s0 || !stages || !n_stages) return QCX_BAD_ARGUMENTS;
    if (n < 1 || n > 40 || (uint64_t)first + num > n) return QCX_BAD_QUBIT;
    if (num > QCX_RDM_MAX_QUBITS) return QCX_UNSUPPORTED;
    memset(s0, 0, sizeof *s0);
    s0->group_bits = n > 21 ? std::min(n - 21u, (unsigned)QCX_RDM_MAX_GROUP_BITS) : 0u;
    s0->sum_bits = std::min(n, 12u) - num + s0->group_bits;
    s0->rest_bits = n - num - s0->sum_bits;
    for (unsigned q = 0, k = 0; q < n && k < s0->sum_bits; q++)
        if (q < first || q >= first + num) { s0->sum_mask |= (uint64_t)1 << q; k++; }
    s0->rows = 1u << (2u * num);
    s0->row_stride = ((uint64_t)1) << s0->rest_bits;
    *n_stages = 0;
    if (s0->rest_bits == 0) return QCX_NO_ERROR;                     // stage 0 writes the components themselves
    const unsigned m = s0->rest_bits + 2u * num;
    std::vector<unsigned> labels(m);
    for (unsigned b = 0; b < m; b++) labels[b] = b;
    QCX_TRY(marginal_plan_from(1, labels, 0, s0->rest_bits, 2u * num, stages, n_stages));
    s0->scratch = (uint64_t)s0->rows << s0->rest_bits;
    for (unsigned i = 0; i < *n_stages; i++)
        if (!stages[i].final_stage) {
            stages[i].out_offset += (uint64_t)s0->rows << s0->rest_bits;
            s0->scratch = std::max<uint64_t>(s0->scratch, stages[i].out_offset + (((uint64_t)1) << stages[i].out_bits));
        }
    return QCX_NO_ERROR;
}

// the kernel's parameters of one planned stage (tile-local bits, tree levels, output bits, tile-number segments)
static void marginal_params(const qcx_marginal_stage &S, MargParams *P)
{
    memset(P, 0, sizeof *P);
    const uint64_t all = S.in_bits >= 64 ? ~(uint64_t)0 : ((((uint64_t)1) << S.in_bits) - 1u);
    auto out_pos = [&](unsigned b) { return (unsigned)__builtin_popcountll(~S.sum_mask & all & ((((uint64_t)1) << b) - 1u)); };
    unsigned j = 0, kept = 0;
    for (unsigned b = 0; b < S.in_bits; b++) {
        if (!(S.tile_mask >> b & 1u)) continue;
        P->tpos[j++] = (uint8_t)b;
        if (S.sum_mask >> b & 1u) P->lvl_q[P->nlvl++] = (uint8_t)kept;
        else P->kpos[kept++] = (uint8_t)out_pos(b);
    }
    P->T = j; P->nkeep = kept;
    unsigned i = 0;                                     // bit i of the tile number = the i-th input bit outside the tile
    for (unsigned b = 0; b < S.in_bits; b++) {
        if (S.tile_mask >> b & 1u) continue;
        const unsigned o = out_pos(b);
        MargSeg *g = P->nseg ? &P->seg[P->nseg - 1] : nullptr;
        if (g && g->src + g->len == i && g->dst_in + g->len == b && g->dst_out + g->len == o) g->len++;
        else P->seg[P->nseg++] = MargSeg{(uint8_t)i, (uint8_t)b, (uint8_t)o, 1};
        i++;
    }
    P->ntiles = ((uint64_t)1) << (S.in_bits - S.T);
}

// diagnostics of the last parallel measurement scan on the current device: blocks redone sequentially / blocks
extern "C" int qcx_measure_last_stats(unsigned *slow_blocks, unsigned *blocks)
{
    Workspace *w;
    QCX_TRY(workspace(&w));
    if (slow_blocks) *slow_blocks = w->h_meas_stats[0];
    if (blocks) *blocks = w->h_meas_stats[1];
    return QCX_NO_ERROR;
}

// ---------------------------------------------------------------------------
// register (single-GPU handle): one in-place amplitude buffer in HBM
// ---------------------------------------------------------------------------
// What an observer's last call read (the *_last_stats getters): where the state came from, and the passes that read amplitudes.
// SRC_COMPACT is the marginal's alone; SRC_EXPANDED: the compact result expanded into the register first, the compact form kept.
enum { SRC_REGISTER = 0, SRC_COMPACT = 1, SRC_BASIS = 2 /* no kernel */, SRC_EXPANDED = 3 };
struct ReadStats { unsigned source; unsigned long reads; };

// A small host array on its way to the device (K18's table, K19's inverse table, K20's matrix): through a pinned buffer into a
// device buffer, on the register's stream, so the caller's array is free when the call returns and the kernel finds the data
// behind the copy.  The next call waits for that copy (ev) before it overwrites the pinned buffer; the device buffer is only
// ever touched in stream order.  All zero: empty.
struct StagedUpload {
    void      *dev, *pinned;
    size_t     cap;             // bytes each holds
    hipEvent_t ev;              // the copy out of `pinned` has been passed by the stream

    // `pinned` free to take `bytes`: both buffers grown to a power-of-two multiple of min_bytes if need be.  A failed allocation
    // is QCX_INSUFFICIENT_MEMORY and leaves the member empty.
    int reserve(size_t bytes, size_t min_bytes, hipStream_t stream)
    {
        if (!ev) HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        else HIP_TRY(hipEventSynchronize(ev));
        if (cap >= bytes) return QCX_NO_ERROR;
        if (cap) {
            HIP_TRY(hipStreamSynchronize(stream));                // (a kernel may still be reading the old buffer)
            (void)hipFree(dev); (void)hipHostFree(pinned);
            dev = pinned = nullptr; cap = 0;
        }
        size_t want = min_bytes;
        while (want < bytes) want <<= 1;
        if (hipMalloc(&dev, want) != hipSuccess) { (void)hipGetLastError(); dev = nullptr; return QCX_INSUFFICIENT_MEMORY; }
        if (hipHostMalloc(&pinned, want) != hipSuccess) { (void)hipGetLastError(); (void)hipFree(dev); dev = pinned = nullptr; return QCX_INSUFFICIENT_MEMORY; }
        cap = want;
        return QCX_NO_ERROR;
    }
    int send(size_t bytes, hipStream_t stream)
    {
        HIP_TRY(hipMemcpyAsync(dev, pinned, bytes, hipMemcpyHostToDevice, stream));
        HIP_TRY(hipEventRecord(ev, stream));
        return QCX_NO_ERROR;
    }
    void release()
    {
        if (cap) { (void)hipFree(dev); (void)hipHostFree(pinned); }
        if (ev) (void)hipEventDestroy(ev);
    }
};

struct qcx_register {
    int        L, M;
    unsigned   n;
    uint64_t   dim;
    amp_t     *amp;
    hipStream_t own_stream, stream;
    hipEvent_t ev0, ev1;
    hipEvent_t *events;
    unsigned   n_events;
    amp_t     *scratch;         // second buffer, allocated on first use (chained passes)
    int        no_chain;        // the buffer pointer was handed out (qcx_device_pointer) or no second buffer fits: passes work in place
    int        nonfinite;       // the caller wrote a component that is not finite (or >= 2^500): every gate runs as a STRICT pass (K9: the
                                // mat-vec's own products, identity rows included) until a reset, a fill or a measurement replaces the state
    int        zeros_dirty;     // 1: the caller wrote amplitudes (qcx_state_write / _load): they may hold -0, which the reference's gates would
                                // canonicalise (Q:393-413); one k_canon_zeros pass runs before the next gate.  2: a tolerance-mode flush
                                // ran merged diagonals, which leave -0 as well (plan_has_diagonals, qcx_fuse.inc.h): the same pass, but
                                // not before another tolerance-mode flush
    int        fusion;          // 1: every gate call is queued (fused passes, qcx_fuse.inc.h); 0: only the whole-circuit entry points; -1: nothing
    int        composite;       // > 0 while a whole-circuit entry point is queueing its gates
    struct GateQueue *queue;
    int        basis_pending;   // the state IS the basis state basis_index (reset / collapse) but has not been written yet:
    uint64_t   basis_index;     // the next flush writes it, together with a closed-form gate prefix if the queue has one
    unsigned long fronts;       // basis-state fronts executed as one write pass (K0b)
    // a compact chain left the state in its compact form (qcx_fuse.inc.h, compact_chain): r->amp is stale until expand_pending()
    // runs -- at the next flush, unless measure_state gets there first (it scans the compact form and collapses lazily)
    int        compact_pending;
    unsigned long compact_measures;            // measurements that scanned the compact form
    amp_t     *compact_amp;     // inside r->scratch
    ExpandParams compact_E;     // ... and its layout: M, column bits, orbit (compact_params)
    unsigned long samp_scans, samp_fallback;   // the last qcx_sample_states call: whole-state scans launched / shots a per-shot scan answered
    double    *marg_buf;        // K10 (qcx_marginal_probabilities): the stages' partials, the output and the `bad` word; its own buffer
    size_t     marg_cap;        // doubles marg_buf holds
    ReadStats  marg, exp, rdm;  // the last marginal / pauli_expectation(_sum, _batch) / reduced_density_matrix call
    ReadStats  coll;            // the last measure_qubits / postselect call: the marginal's reads behind its probabilities ...
    unsigned long coll_writes;  // ... and collapse passes launched (0 or 1)
    unsigned long rotb_passes, rotb_wide;    // the last pauli_rotation_batch call: its passes, and those of them that are one wide term (K15)
    unsigned   diag_form;       // the last diagonal_gate call: the plan's form ...
    unsigned long diag_entries; // ... and its table's entries
    StagedUpload diag_up;       // K18, host form: the table, 2^12 entries or more
    unsigned   perm_form;       // the last permutation_gate call: the plan's form ...
    unsigned long perm_moved;   // ... and the entries of its table that are not fixed points
    StagedUpload perm_up;       // K19: the inverse table, 2^12 entries
    unsigned   multi_form;      // the last mc_multi_qubit_gate call: the plan's form ...
    unsigned   multi_k;         // ... and its number of targets
    StagedUpload multi_up;      // K20: the ascending matrix, 2 * 4^5 doubles
    unsigned long gateb_passes, gateb_lds;   // the last gate_batch call: its passes, and the gates in them that exchanged through LDS (K12b / K13b)
    struct ShardSet *sh;     // non-null: the register is sharded over several GPUs by this process (qcx_sharded.inc.h)
};

static int reg_camodc(qcx_register *r, unsigned C, unsigned A, unsigned ctl);

// a state the caller wrote may hold -0 components; the reference's next gate would turn them into +0 wherever they sit
// (Q:393-413), the gate kernels only where they act: one pass over the state before the first gate after such a write
static int canon_if_dirty(qcx_register *r)
{
    if (!r->zeros_dirty) return QCX_NO_ERROR;
    r->zeros_dirty = 0;
    return qcx_shard_canon_zeros(r->amp, r->n, r->stream);
}

#include "qcx_fuse.inc.h"
#include "qcx_sharded.inc.h"

#define FLUSH(r) QCX_TRY(fuse_flush(r))

static int reg_camodc(qcx_register *r, unsigned C, unsigned A, unsigned ctl)
{
    return qcx_shard_camodc(r->amp, r->n, (unsigned)r->M, C, A, (int)ctl, r->stream);
}

extern "C" int qcx_register_create_sharded(int L, int M, unsigned nshards, const int *devices, qcx_register **out)
{
    if (!out) return QCX_BAD_ARGUMENTS;
    *out = nullptr;
    if (L < 0 || M < 0 || L + M < 1 || L + M > 40) return QCX_BAD_ARGUMENTS;
    if (nshards == 1 && !(devices && devices[0] < 0)) {
        if (devices) QCX_TRY(qcx_set_device(devices[0]));
        return qcx_register_create(L, M, out);
    }
    qcx_register *r = (qcx_register *)calloc(1, sizeof(qcx_register));
    if (!r) return QCX_INSUFFICIENT_MEMORY;
    r->L = L; r->M = M; r->n = (unsigned)(L + M); r->dim = (uint64_t)1 << r->n;
    const int s = sh_create(L, M, nshards, devices, &r->sh);
    if (s != QCX_NO_ERROR) { free(r); return s; }
    if (!r->sh->dry && (hipEventCreate(&r->ev0) != hipSuccess || hipEventCreate(&r->ev1) != hipSuccess)) { sh_free(r->sh); free(r); return QCX_HIP_ERROR; }
    if (const char *e = getenv("QCX_SHARD_RELAYS")) {             // "4,5,6,7": GPUs without a shard that relay stripes of every trade
        int devs[8], nr = 0;
        for (const char *p = e; *p && nr < 8; nr++) { devs[nr] = atoi(p); while (*p && *p != ',') p++; if (*p == ',') p++; }
        const int rs = sh_set_relays(r->sh, (unsigned)nr, devs);
        if (rs != QCX_NO_ERROR) { sh_free(r->sh); (void)hipEventDestroy(r->ev0); (void)hipEventDestroy(r->ev1); free(r); return rs; }
    }
    *out = r;
    return QCX_NO_ERROR;
}

extern "C" int qcx_sharded_set_relays(qcx_register *r, unsigned nrelays, const int *devices)
{
    if (!r || !r->sh) return QCX_BAD_ARGUMENTS;
    return sh_set_relays(r->sh, nrelays, devices);
}

extern "C" int qcx_sharded_overlap_stats(qcx_register *r, unsigned *slices_log2, unsigned long *gates_in_windows)     // diagnostics
{
    if (!r || !r->sh) return QCX_BAD_ARGUMENTS;
    if (slices_log2) *slices_log2 = r->sh->sigma;
    if (gates_in_windows) *gates_in_windows = r->sh->overlapped_gates;
    return QCX_NO_ERROR;
}

extern "C" int qcx_sharded_relay_stats(qcx_register *r, unsigned *nrelays, unsigned long *relayed_bytes)     // diagnostics
{
    if (!r || !r->sh) return QCX_BAD_ARGUMENTS;
    if (nrelays) *nrelays = (unsigned)r->sh->relay_dev.size();
    if (relayed_bytes) *relayed_bytes = r->sh->relayed_bytes;
    return QCX_NO_ERROR;
}

// where qcx_register_create_sharded(devices = NULL) puts the shards when `visible` devices can be seen (visible <= 0: ask HIP)
extern "C" int qcx_spread_devices(unsigned nshards, int visible, int *devices_out)
{
    if (!devices_out || nshards < 1 || nshards > 16 || (nshards & (nshards - 1))) return QCX_BAD_ARGUMENTS;
    if (visible <= 0) { QCX_TRY(qcx_device_count(&visible)); if (visible < 1) { set_error("no HIP device"); return QCX_HIP_ERROR; } }
    sh_spread(nshards, visible, devices_out);
    return QCX_NO_ERROR;
}

// the pre-flight exchange check on demand (it runs by itself at creation when the shards sit on different devices)
extern "C" int qcx_sharded_selfcheck(qcx_register *r)
{
    if (!r || !r->sh) return QCX_BAD_ARGUMENTS;
    if (r->sh->dry) return QCX_UNSUPPORTED;
    std::vector<int> rel(r->sh->relay_dev);
    int prev = 0;
    (void)hipGetDevice(&prev);
    const int s = sh_selfcheck(r->sh, (unsigned)rel.size(), rel.data());
    (void)hipSetDevice(prev);
    return s;
}

extern "C" unsigned long qcx_sharded_selfchecks(const qcx_register *r) { return (r && r->sh) ? r->sh->selfchecks : 0ul; }

extern "C" unsigned qcx_register_shards(const qcx_register *r) { return r ? (r->sh ? r->sh->W : 1u) : 0u; }

extern "C" int qcx_sharded_stats(qcx_register *r, unsigned long *exchanges, unsigned long *pack_passes)
{
    if (!r) return QCX_BAD_ARGUMENTS;
    if (exchanges) *exchanges = r->sh ? r->sh->exchanges : 0;
    if (pack_passes) *pack_passes = r->sh ? r->sh->pack_passes : 0;
    return QCX_NO_ERROR;
}

// diagnostics (not in the public header): the step list a dry-run register has scheduled since the last call, and the
// restoration of the identity layout on demand (measurement and read-back do it themselves)
extern "C" int qcx_sharded_trace(qcx_register *r, char *buf, size_t cap, size_t *need)
{
    if (!r || !r->sh || !need) return QCX_BAD_ARGUMENTS;
    *need = r->sh->trace.size() + 1;
    if (!buf || cap < *need) return QCX_INSUFFICIENT_MEMORY;
    memcpy(buf, r->sh->trace.c_str(), *need);
    r->sh->trace.clear();
    return QCX_NO_ERROR;
}
extern "C" int qcx_sharded_restore_identity(qcx_register *r) { return (r && r->sh) ? sh_identity(r->sh) : QCX_BAD_ARGUMENTS; }
extern "C" int qcx_sharded_layout(qcx_register *r, unsigned *perm, unsigned cap)
{
    if (!r || !r->sh || !perm || cap < r->n) return QCX_BAD_ARGUMENTS;
    for (unsigned q = 0; q < r->n; q++) perm[q] = r->sh->perm[q];
    return QCX_NO_ERROR;
}

extern "C" int qcx_register_create(int L, int M, qcx_register **out)
{
    if (!out) return QCX_BAD_ARGUMENTS;
    *out = nullptr;
    // QCX_SHARDS=N (N = 2, 4, 8, 16): every register this process creates is sharded over N devices -- how a program
    // written against the reference's interface (qcx_compat.h, host/qcx_shor) gets onto the 8 GPUs of a node without
    // an edit.  QCX_SHARD_DEVICES="0,0,1,1" places the shards (default: shard r on device r).
    if (const char *e = getenv("QCX_SHARDS")) {
        const int ns = atoi(e);
        if (ns > 1) {
            int devs[16];
            const char *d = getenv("QCX_SHARD_DEVICES");
            if (d && *d) {
                int i = 0;
                for (const char *p = d; *p && i < 16; i++) { devs[i] = atoi(p); while (*p && *p != ',') p++; if (*p == ',') p++; }
                for (int j = i; j < 16; j++) devs[j] = devs[i ? i - 1 : 0];
            }
            return qcx_register_create_sharded(L, M, (unsigned)ns, (d && *d) ? devs : nullptr, out);    // no list: spread over the visible devices
        }
    }
    if (L < 0 || M < 0 || L + M < 1 || L + M > 36) return QCX_BAD_ARGUMENTS;
    int ndev = 0;
    QCX_TRY(qcx_device_count(&ndev));
    if (ndev < 1) { snprintf(g_last_error, sizeof g_last_error, "no HIP device"); return QCX_HIP_ERROR; }
    qcx_register *r = (qcx_register *)calloc(1, sizeof(qcx_register));
    if (!r) return QCX_INSUFFICIENT_MEMORY;
    r->L = L; r->M = M; r->n = (unsigned)(L + M); r->dim = (uint64_t)1 << r->n;
    hipError_t e = hipMalloc(&r->amp, r->dim * sizeof(amp_t));
    if (e != hipSuccess) { free(r); snprintf(g_last_error, sizeof g_last_error, "hipMalloc: %s", hipGetErrorString(e)); return QCX_INSUFFICIENT_MEMORY; }
    // (each step is undone on a later failure: nothing of a half-built register stays behind)
    bool ok = hipStreamCreate(&r->own_stream) == hipSuccess;
    const bool have_stream = ok;
    const bool have_ev0 = ok && hipEventCreate(&r->ev0) == hipSuccess;
    const bool have_ev1 = have_ev0 && hipEventCreate(&r->ev1) == hipSuccess;
    ok = have_ev1;
    r->stream = r->own_stream;
    // the reference's buffers start zeroed by calloc-like GSL allocs only after reset; be deterministic
    if (ok && hipMemsetAsync(r->amp, 0, r->dim * sizeof(amp_t), r->stream) != hipSuccess) ok = false;
    if (!ok) {
        snprintf(g_last_error, sizeof g_last_error, "qcx_register_create: %s", hipGetErrorString(hipGetLastError()));
        if (have_ev1) (void)hipEventDestroy(r->ev1);
        if (have_ev0) (void)hipEventDestroy(r->ev0);
        if (have_stream) (void)hipStreamDestroy(r->own_stream);
        (void)hipFree(r->amp); free(r);
        return QCX_HIP_ERROR;
    }
    *out = r;
    return QCX_NO_ERROR;
}

extern "C" int qcx_register_destroy(qcx_register *r)
{
    if (!r) return QCX_NO_ERROR;
    if (r->sh) {
        const bool dry = r->sh->dry;
        sh_free(r->sh);
        if (!dry) { (void)hipEventDestroy(r->ev0); (void)hipEventDestroy(r->ev1); }
        free(r);
        return QCX_NO_ERROR;
    }
    (void)fuse_flush(r);
    (void)hipStreamSynchronize(r->stream);
    queue_free(r->queue);
    (void)hipEventDestroy(r->ev0); (void)hipEventDestroy(r->ev1);
    for (unsigned i = 0; i < r->n_events; i++) (void)hipEventDestroy(r->events[i]);
    free(r->events);
    (void)hipStreamDestroy(r->own_stream);
    (void)hipFree(r->amp);
    if (r->scratch) (void)hipFree(r->scratch);
    if (r->marg_buf) (void)hipFree(r->marg_buf);
    r->diag_up.release(); r->perm_up.release(); r->multi_up.release();
    free(r);
    return QCX_NO_ERROR;
}

extern "C" unsigned qcx_num_qubits(const qcx_register *r) { return r ? r->n : 0; }
extern "C" unsigned long qcx_num_states(const qcx_register *r) { return r ? (unsigned long)r->dim : 0; }
extern "C" int qcx_L_size(const qcx_register *r) { return r ? r->L : 0; }
extern "C" int qcx_M_size(const qcx_register *r) { return r ? r->M : 0; }
extern "C" void *qcx_device_pointer(qcx_register *r)
{
    if (!r || r->sh) return nullptr;
    (void)fuse_flush(r);
    r->no_chain = 1;             // the caller may keep the pointer: from now on the state stays in THIS buffer (no chained passes, which alternate between two)
    return (void *)r->amp;
}

// shard-level gate list through the fusion scheduler: one queue (record buffers + the event that guards them) per
// (device, stream), one user at a time.  A queue's event is only ever recorded on its own stream; the owner of a
// stream drops the queue before destroying the stream (qcx_shard_release_stream) -- an event whose last record was on
// a destroyed stream must not be synchronised any more.
struct ShardQueue { GateQueue q; std::mutex use; };
static std::mutex g_shard_queue_mutex;
static std::map<std::pair<int, hipStream_t>, ShardQueue *> g_shard_queues;

extern "C" int qcx_shard_release_stream(void *stream)
{
    std::vector<ShardQueue *> gone;
    {
        std::lock_guard<std::mutex> lock(g_shard_queue_mutex);
        for (auto it = g_shard_queues.begin(); it != g_shard_queues.end();)
            if (it->first.second == (hipStream_t)stream) { gone.push_back(it->second); it = g_shard_queues.erase(it); } else ++it;
    }
    for (ShardQueue *sq : gone) {
        std::lock_guard<std::mutex> use(sq->use);
        if (sq->q.ev_valid) { (void)hipEventSynchronize(sq->q.ev); (void)hipEventDestroy(sq->q.ev); sq->q.ev_valid = false; }
        if (sq->q.d_ops) (void)hipFree(sq->q.d_ops);
        if (sq->q.h_ops) (void)hipHostFree(sq->q.h_ops);
        sq->q.d_ops = nullptr; sq->q.h_ops = nullptr;
    }
    for (ShardQueue *sq : gone) delete sq;
    return QCX_NO_ERROR;
}

static int descs_to_gates(unsigned n_local, unsigned M, unsigned count, const qcx_gate_desc *gates, std::vector<QGate> &out)
{
    for (unsigned k = 0; k < count; k++) {
        const qcx_gate_desc &d = gates[k];
        QGate g; memset(&g, 0, sizeof g);
        if (d.type == 0) {
            if (d.q >= n_local) return QCX_BAD_QUBIT;
            g.type = FUSE_H; g.q = d.q;
        } else if (d.type == 1) {
            if (n_local < 64 && (d.mask >> n_local) != 0) return QCX_BAD_QUBIT;
            if (__builtin_popcountll(d.mask) > 2) return QCX_BAD_ARGUMENTS;
            g.type = FUSE_PHASE; g.mask = d.mask; g.c = d.c; g.s = d.s;
        } else if (d.type == 2) {
            if (d.C == 0 || (d.q != 0xffffffffu && d.q >= n_local)) return QCX_BAD_ARGUMENTS;
            g.q = d.q; g.C = d.C; g.A = d.A % d.C;
            const bool closed = (d.q == 0xffffffffu) ? camodc_closed_form(n_local, M, d.C, g.A, M)   // "control" outside M
                                                     : camodc_closed_form(n_local, M, d.C, g.A, d.q);
            g.type = closed ? (uint32_t)FUSE_CAMODC : 99u;          // (M > 12: the planner keeps it out of the tile passes -- K3b, stand-alone)
        } else return QCX_BAD_ARGUMENTS;
        out.push_back(g);
    }
    return QCX_NO_ERROR;
}

// the leading descriptors that can be part of a circuit front (Hadamards and multiplies), as gates: the front ends at the first
// descriptor that cannot -- a phase, or one that is not valid
static std::vector<QGate> front_prefix(unsigned n, unsigned M, unsigned count, const qcx_gate_desc *gates)
{
    std::vector<QGate> q;
    for (unsigned k = 0; k < count; k++)
        if (gates[k].type == 1 || descs_to_gates(n, M, 1, gates + k, q) != QCX_NO_ERROR) break;
    return q;
}

// ---- compact circuits for a one-process-per-GPU host (quantumcomputer_amd/sharded.py; the C host: sh_compact) ----------------
// qcx_compact_plan: pure host.  The closed-form front of `gates` on basis state `basis` (as qcx_shard_basis_front consumes it)
// and, when the M register stays on a small orbit behind it (compact_orbit), the compact form's column bits and the orbit.
// *ncols = 0: no compact form.  Every rank calls it with the same arguments and gets the same answer.
extern "C" int qcx_compact_plan(unsigned n, unsigned M, uint64_t basis, unsigned count, const qcx_gate_desc *gates,
                                unsigned *used, unsigned *cb, unsigned *ncols, uint16_t *orbit16)
{
    if (!used || !cb || !ncols || !orbit16 || n == 0 || n > 40 || M > n || (count && !gates) || (basis >> n)) return QCX_BAD_ARGUMENTS;
    *used = *cb = *ncols = 0;
    const std::vector<QGate> q = front_prefix(n, M, count, gates);
    BasisFront B;
    const Tune tn = tune_now();
    const size_t k = (M <= 26) ? front_plan(n, M, basis, tn, q, &B) : 0;
    *used = (unsigned)k;
    std::vector<uint16_t> orbit;
    unsigned c = 0;
    if (!k || !tn.fuse_compact || !compact_orbit(B, M, orbit, &c)) return QCX_NO_ERROR;
    *cb = c; *ncols = (unsigned)orbit.size();
    for (size_t j = 0; j < orbit.size(); j++) orbit16[j] = orbit[j];
    return QCX_NO_ERROR;
}

// this rank's part of the front, written in the compact form ([L register][orbit column]); count = the front's gates (*used of
// qcx_compact_plan), first_global = REAL global index of the rank's amplitude 0, n_local_compact = n_local - M + cb
extern "C" int qcx_shard_compact_front(void *compact, unsigned n_local_compact, uint64_t first_global, unsigned n, unsigned M, uint64_t basis,
                                       unsigned count, const qcx_gate_desc *gates, unsigned cb, unsigned ncols, const uint16_t *orbit16, void *stream)
{
    if (!compact || !orbit16 || !count || !gates || n == 0 || n > 40 || M > n || ncols == 0 || ncols > 16 || cb < 2 || cb > 4 || (1u << cb) < ncols ||
        n_local_compact <= cb || n_local_compact > 40) return QCX_BAD_ARGUMENTS;
    std::vector<QGate> q;
    QCX_TRY(descs_to_gates(n, M, count, gates, q));
    BasisFront B;
    if (front_plan(n, M, basis, tune_now(), q, &B) != count) return QCX_BAD_ARGUMENTS;
    B.first = first_global;
    const ExpandParams E = compact_params(M, cb, orbit16, ncols);
    const uint64_t nblocks = (uint64_t)1 << (n_local_compact - cb);
    hipLaunchKernelGGL(k_basis_front_compact, dim3(grid_for(nblocks, 256, 65536)), dim3(256), 0, (hipStream_t)stream, (amp_t *)compact, n_local_compact, B, E);
    HIP_TRY(hipGetLastError());
    return QCX_NO_ERROR;
}

// a rank's part of the real register from its compact form (n_local - M >= 6)
extern "C" int qcx_shard_expand_compact(const void *compact, void *real, unsigned n_local, unsigned M, unsigned cb, unsigned ncols,
                                        const uint16_t *orbit16, void *stream)
{
    if (!compact || !real || !orbit16 || n_local > 40 || M > 12 || n_local < M + 6 || ncols == 0 || ncols > 16 || cb < 2 || cb > 4 || (1u << cb) < ncols) return QCX_BAD_ARGUMENTS;
    return launch_expand_compact((const amp_t *)compact, (amp_t *)real, n_local, compact_params(M, cb, orbit16, ncols), (hipStream_t)stream);
}

extern "C" int qcx_shard_run_fused_mode(int mode, void *amp, unsigned n_local, unsigned M, unsigned count, const qcx_gate_desc *gates, void *stream);

extern "C" int qcx_shard_run_fused(void *amp, unsigned n_local, unsigned M, unsigned count, const qcx_gate_desc *gates, void *stream)
{
    return qcx_shard_run_fused_mode(1, amp, n_local, M, count, gates, stream);
}

// mode 1: bit-exact passes; 2: the tolerance mode's passes (merged diagonals; a phase with ONE mask bit -- its other qubit
// is a constant 1 of the shard -- joins the diagonal of its run as a constant factor)
extern "C" int qcx_shard_run_fused_mode(int mode, void *amp, unsigned n_local, unsigned M, unsigned count, const qcx_gate_desc *gates, void *stream)
{
    if (!amp || n_local == 0 || n_local > 40 || M > n_local || (count && !gates)) return QCX_BAD_ARGUMENTS;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64) return QCX_HIP_ERROR;
    ShardQueue *sq;
    {
        std::lock_guard<std::mutex> lock(g_shard_queue_mutex);
        ShardQueue *&slot = g_shard_queues[std::make_pair(dev, (hipStream_t)stream)];
        if (!slot) slot = new ShardQueue();
        sq = slot;
    }
    std::lock_guard<std::mutex> use(sq->use);
    qcx_register tmp = reg_view(n_local - M, M, (amp_t *)amp, nullptr, (hipStream_t)stream, (hipStream_t)stream, mode == 2 ? 2 : 1);
    tmp.queue = &sq->q;
    tmp.no_chain = 1;                                    // a view of somebody else's memory: there is no second buffer behind it
    tmp.queue->gates.clear();
    QCX_TRY(descs_to_gates(n_local, M, count, gates, tmp.queue->gates));
    return fuse_flush(&tmp);
}

// The planner alone, on the host (no GPU needed): which passes / stand-alone gates a gate list becomes and the
// records the pass kernels would interpret.  actions[k] describes action k; records receives the raw 32-byte
// records of all passes back to back (action.rec_off / rec_cnt index into it, in records).
extern "C" int qcx_fusion_plan_mode(int mode, unsigned n_local, unsigned M, unsigned count, const qcx_gate_desc *gates,
                                    qcx_plan_action *actions, unsigned max_actions, unsigned *n_actions,
                                    qcx_fuse_record *records, size_t max_records, size_t *n_records);

extern "C" int qcx_fusion_plan(unsigned n_local, unsigned M, unsigned count, const qcx_gate_desc *gates,
                               qcx_plan_action *actions, unsigned max_actions, unsigned *n_actions,
                               qcx_fuse_record *records, size_t max_records, size_t *n_records)
{
    return qcx_fusion_plan_mode(1, n_local, M, count, gates, actions, max_actions, n_actions, records, max_records, n_records);
}

extern "C" int qcx_fusion_plan_mode(int mode, unsigned n_local, unsigned M, unsigned count, const qcx_gate_desc *gates,
                                    qcx_plan_action *actions, unsigned max_actions, unsigned *n_actions,
                                    qcx_fuse_record *records, size_t max_records, size_t *n_records)
{
    if (n_local == 0 || n_local > 40 || M > n_local || (count && !gates) || !n_actions || !n_records) return QCX_BAD_ARGUMENTS;
    if ((mode & 3) != 1 && (mode & 3) != 2) return QCX_BAD_ARGUMENTS;
    static_assert(sizeof(qcx_fuse_record) == sizeof(FuseOp), "record layout");
    const qcx_register tmp = reg_view(n_local - M, M, nullptr, nullptr, nullptr, nullptr, 0);
    std::vector<QGate> q;
    QCX_TRY(descs_to_gates(n_local, M, count, gates, q));
    std::vector<FuseAction> acts;
    std::vector<FuseOp> ops;
    // mode | 4: with chained passes (a register with a second buffer); | 8: as compact_chain_plan plans the virtual register of a compact
    // chain (the first pass generated by columns: a tile of the M register's bits x 8 hot bits)
    const Tune tn = tune_now();
    const bool tol = (mode & 3) == 2;
    fuse_plan(&tmp, tn, q, acts, ops, tol, (mode & 4) != 0, (mode & 8) ? compact_first_cols(tn, tol) : 0);
    *n_actions = (unsigned)acts.size();
    *n_records = ops.size();
    if (acts.size() > max_actions || ops.size() > max_records || (!actions && !acts.empty()) || (!records && !ops.empty()))
        return QCX_INSUFFICIENT_MEMORY;
    for (size_t k = 0; k < acts.size(); k++) {
        const FuseAction &a = acts[k];
        qcx_plan_action &o = actions[k];
        memset(&o, 0, sizeof o);
        o.fused = a.fused;
        if (!a.fused) { o.first_gate = (unsigned)a.gate; o.ngates = 1; continue; }
        o.first_gate = (unsigned)a.first_gate; o.ngates = (unsigned)a.ngates;
        o.T = a.P.T; o.c = a.P.c; o.nh = a.P.nh; o.nopipe = (unsigned)a.nopipe;
        memcpy(o.hbit, a.P.hbit, sizeof o.hbit);
        o.rounds_form = (unsigned)a.P.cam_ctl_local[0];
        o.rec_off = a.op_off; o.rec_cnt = a.op_cnt; o.nops = a.P.nops;
        o.table_bytes = (unsigned)a.P.cam_ctl_local[1]; o.table_rec_off = (unsigned)a.P.cam_ctl_local[2];
        o.diag_cnt = a.P.dg_cnt; o.diag_rec_off = a.P.dg_rec_off;
        o.chained = a.P.chained;
        memcpy(o.tl, a.tl, sizeof o.tl);
        memcpy(o.in_pos, a.P.in_pos, sizeof o.in_pos); memcpy(o.st_loc, a.P.st_loc, sizeof o.st_loc); memcpy(o.st_pos, a.P.st_pos, sizeof o.st_pos);
        o.nseg_in = a.P.nseg_in; o.nseg_out = a.P.nseg_out; o.nseg_lg = a.P.nseg_lg;
        static_assert(sizeof o.seg_in == sizeof a.P.seg_in, "segment layout");
        memcpy(o.seg_in, a.P.seg_in, sizeof o.seg_in); memcpy(o.seg_out, a.P.seg_out, sizeof o.seg_out); memcpy(o.seg_lg, a.P.seg_lg, sizeof o.seg_lg);
        PassLaunch L;
        if (pass_launch_plan(pass_launch_in(a.P, n_local, M, a.P.chained != 0), tn, L) == QCX_NO_ERROR) {
            snprintf(o.kernel, sizeof o.kernel, "%s", pass_kernel_text(L.kernel));
            o.grid = L.grid; o.block = L.block; o.lds_bytes = (unsigned)L.lds;
        }
    }
    if (!ops.empty()) memcpy(records, ops.data(), ops.size() * sizeof(FuseOp));
    return QCX_NO_ERROR;
}

// The launch plan of one pass on its own (include/qcx_plan.h): pass_launch_plan under the knobs of the moment.
extern "C" int qcx_pass_launch_plan(const qcx_pass_launch_in *in, qcx_pass_launch_out *out)
{
    if (!in || !out || in->n == 0 || in->n > 40) return QCX_BAD_ARGUMENTS;
    memset(out, 0, sizeof *out);
    qcx_pass_launch_in I = *in;
    if (I.T > I.n) I.tables_cover = 0;
    const Tune tn = tune_now();
    out->expanding_store_ok = pass_expanding_store_ok(I, tn);
    PassLaunch L;
    if (pass_launch_plan(I, tn, L) != QCX_NO_ERROR) { set_error("%s", L.err); return QCX_UNKNOWN_ERROR; }
    snprintf(out->kernel, sizeof out->kernel, "%s", pass_kernel_text(L.kernel));
    out->grid = L.grid; out->block = L.block; out->lds_bytes = (unsigned)L.lds; out->waves = L.waves;
    out->xm_off = L.xm_off; out->dg_lds_off = L.dg_lds_off; out->gen_lds_off = L.gen_lds_off; out->table_lds_off = (unsigned)L.table_lds_off; out->dbg = L.dbg;
    return QCX_NO_ERROR;
}

// One shard's part of the basis state |basis> of an (n, M) register -- amplitudes [first_global, first_global + 2^n_local) --
// written together with the longest prefix of `gates` (GLOBAL qubit numbers, identity layout) that has the closed form on
// a basis state: Hadamards on distinct qubits, then controlled modular multiplies (K0b).  Every rank of a multi-process
// host calls it with the same list and gets the same *used; no communication.  used = 0: the plain basis state.
extern "C" int qcx_shard_basis_front(void *amp, unsigned n_local, uint64_t first_global, unsigned n, unsigned M, uint64_t basis,
                                     unsigned count, const qcx_gate_desc *gates, unsigned *used, void *stream)
{
    if (!amp || !used || n_local == 0 || n_local > 40 || n < n_local || n > 40 || M > n_local || (count && !gates)) return QCX_BAD_ARGUMENTS;
    if (basis >> n) return QCX_BAD_ARGUMENTS;
    if (first_global & (((uint64_t)1 << n_local) - 1)) return QCX_BAD_ARGUMENTS;
    *used = 0;
    const std::vector<QGate> q = front_prefix(n, M, count, gates);
    BasisFront B;
    size_t k = 0;
    if (M <= 26) k = front_plan(n, M, basis, tune_now(), q, &B);
    hipStream_t st = (hipStream_t)stream;
    if (k == 0) {
        const uint64_t per = (uint64_t)1 << n_local;
        const bool mine = basis >= first_global && basis - first_global < per;
        return qcx_shard_collapse(amp, n_local, mine ? (int64_t)(basis - first_global) : -1, st);
    }
    B.first = first_global;
    QCX_TRY(launch_basis_front((amp_t *)amp, n_local, B, st));
    *used = (unsigned)k;
    return QCX_NO_ERROR;
}

// The host half of the basis-state circuit front alone (no GPU needed; test interface, not in the public header): how many
// leading gates of the list have the closed form on basis state `basis` of an (n_local, M) register, and the parameters
// k_basis_front would get (struct BasisFront, csrc/qcx_kernels.h).
extern "C" int qcx_front_plan(unsigned n_local, unsigned M, uint64_t basis, unsigned count, const qcx_gate_desc *gates,
                              unsigned *used, void *front_out, size_t front_bytes)
{
    if (n_local == 0 || n_local > 40 || M > n_local || (count && !gates) || !used || !front_out || front_bytes < sizeof(BasisFront)) return QCX_BAD_ARGUMENTS;
    std::vector<QGate> q;
    QCX_TRY(descs_to_gates(n_local, M, count, gates, q));
    BasisFront B;
    *used = (unsigned)front_plan(n_local, M, basis, tune_now(), q, &B);
    memcpy(front_out, &B, sizeof B);
    return QCX_NO_ERROR;
}

// gate fusion: 1 = queue gates and run them as fused LDS-tile passes; results are
// bit-identical to the per-gate kernels.  Observing calls (read, norm, measure, synchronize, timers) flush.
extern "C" int qcx_set_fusion(qcx_register *r, int enable)
{
    if (!r) return QCX_BAD_ARGUMENTS;
    if (r->sh) { QCX_TRY(sh_flush(r->sh)); r->sh->fusion = enable >= 2 ? 2 : (enable >= 0 ? 1 : -1); return QCX_NO_ERROR; }   // (gates are always queued; -1 = one launch per gate, 2 = tolerance mode per shard)
    FLUSH(r);
    r->fusion = enable >= 2 ? 2 : (enable > 0 ? 1 : (enable < 0 ? -1 : 0));
    return QCX_NO_ERROR;
}

extern "C" int qcx_flush(qcx_register *r)
{
    if (!r) return QCX_BAD_ARGUMENTS;
    if (r->sh) return sh_flush(r->sh);
    FLUSH(r);
    return QCX_NO_ERROR;
}

extern "C" int qcx_fusion_stats(qcx_register *r, unsigned long *passes, unsigned long *gates)
{
    if (!r) return QCX_BAD_ARGUMENTS;
    if (r->sh) { if (passes) *passes = r->sh->fronts; if (gates) *gates = 0; return QCX_NO_ERROR; }     // (circuit fronts written in one pass; the per-device pass queues are not counted: see qcx_sharded_stats)
    if (passes) *passes = (r->queue ? r->queue->passes_launched : 0) + r->fronts;
    if (gates) *gates = r->queue ? r->queue->gates_fused : 0;
    return QCX_NO_ERROR;
}

// diagnostics (not in the public header): fused passes that went out of place through the second buffer; circuit fronts
// that were generated inside the first pass behind them instead of being written by a pass of their own
extern "C" int qcx_chain_stats(qcx_register *r, unsigned long *chained_passes)
{
    if (!r || !chained_passes) return QCX_BAD_ARGUMENTS;
    *chained_passes = (!r->sh && r->queue) ? r->queue->chained_passes : 0;
    return QCX_NO_ERROR;
}
// ... fused passes that carried merged diagonals (tolerance mode: a flush without one ran the exact interpreter throughout)
extern "C" int qcx_diag_stats(qcx_register *r, unsigned long *diag_passes)
{
    if (!r || !diag_passes) return QCX_BAD_ARGUMENTS;
    *diag_passes = (!r->sh && r->queue) ? r->queue->diag_passes : 0;
    return QCX_NO_ERROR;
}
extern "C" int qcx_gen_stats(qcx_register *r, unsigned long *generated_fronts)
{
    if (!r || !generated_fronts) return QCX_BAD_ARGUMENTS;
    *generated_fronts = (!r->sh && r->queue) ? r->queue->gen_fronts : 0;
    return QCX_NO_ERROR;
}
extern "C" int qcx_gen_cols_stats(qcx_register *r, unsigned long *by_columns)
{
    if (!r || !by_columns) return QCX_BAD_ARGUMENTS;
    *by_columns = (!r->sh && r->queue) ? r->queue->gen_cols : 0;
    return QCX_NO_ERROR;
}
extern "C" int qcx_compact_stats(qcx_register *r, unsigned long *compact_chains)
{
    if (!r || !compact_chains) return QCX_BAD_ARGUMENTS;
    *compact_chains = r->sh ? r->sh->compact_circuits : (r->queue ? r->queue->compact_chains : 0);
    return QCX_NO_ERROR;
}

// host logic only (no GPU): the expanding-store tables compact_chain would give the last pass of a compact chain -- T = 12, the
// pass's store order (st_pos / st_loc as qcx_fusion_plan reports them for the plan of the VIRTUAL register, mode | 8), an M
// register of M bits and cb column bits.  *ok = 0: that pass does not qualify (the separate expansion runs).
extern "C" int qcx_expand_store_plan(unsigned T, const unsigned char *st_pos, const unsigned char *st_loc, unsigned M, unsigned cb,
                                     unsigned char *xp_pos24, unsigned char *xp_loc24, unsigned char *xp_colloc4, int *ok)
{
    if (!st_pos || !st_loc || !xp_pos24 || !xp_loc24 || !xp_colloc4 || !ok || T > 16) return QCX_BAD_ARGUMENTS;
    FusePass P;
    memset(&P, 0, sizeof P);
    P.T = T;
    memcpy(P.st_pos, st_pos, 16); memcpy(P.st_loc, st_loc, 16);
    const std::vector<uint16_t> none;
    *ok = xp_setup(P, M, cb, none) ? 1 : 0;
    memcpy(xp_pos24, P.xp_pos, 24); memcpy(xp_loc24, P.xp_loc, 24); memcpy(xp_colloc4, P.xp_colloc, 4);
    return QCX_NO_ERROR;
}

// diagnostics: flushes that took their plan from the plan cache (GateQueue::pc)
extern "C" int qcx_plan_cache_stats(qcx_register *r, unsigned long *hits)
{
    if (!r || !hits) return QCX_BAD_ARGUMENTS;
    *hits = (!r->sh && r->queue) ? r->queue->plan_hits : 0;
    return QCX_NO_ERROR;
}

// diagnostics: compact chains whose LAST pass stored the real register itself (no k_expand_compact launch)
extern "C" int qcx_expanding_store_stats(qcx_register *r, unsigned long *expanding_stores)
{
    if (!r || !expanding_stores) return QCX_BAD_ARGUMENTS;
    *expanding_stores = (!r->sh && r->queue) ? r->queue->expanding_stores : 0;
    return QCX_NO_ERROR;
}

// diagnostics: measurements that scanned the compact form of a circuit's result instead of the register (no expansion written)
extern "C" int qcx_compact_measure_stats(qcx_register *r, unsigned long *compact_measures)
{
    if (!r || !compact_measures) return QCX_BAD_ARGUMENTS;
    *compact_measures = r->sh ? r->sh->compact_measures : r->compact_measures;
    return QCX_NO_ERROR;
}

extern "C" int qcx_register_set_stream(qcx_register *r, void *hip_stream)
{
    if (!r) return QCX_BAD_ARGUMENTS;
    if (r->sh) return QCX_UNSUPPORTED;                 // one stream per shard, owned by the register
    FLUSH(r);
    HIP_TRY(hipStreamSynchronize(r->stream));
    r->stream = hip_stream ? (hipStream_t)hip_stream : r->own_stream;
    return QCX_NO_ERROR;
}

extern "C" int qcx_synchronize(qcx_register *r)
{
    if (!r) return QCX_BAD_ARGUMENTS;
    if (r->sh) return sh_sync(r->sh);
    FLUSH(r);
    HIP_TRY(hipStreamSynchronize(r->stream));
    return QCX_NO_ERROR;
}

// ---- strict gates (K9): a register that was handed non-finite amplitudes -------------------------------------------------------
// What a scan kernel ORs into the workspace's device flag word: the word cleared, launch(word) enqueued on the stream, its value
// to *flag behind one sync.  The pinned word it is read through doubles as the last measurement scan's statistics: put back.
template <typename Launch>
static int scan_flag_word(hipStream_t stream, Launch launch, unsigned *flag)
{
    Workspace *w;
    QCX_TRY(workspace(&w));
    std::lock_guard<std::mutex> use(g_ws_use[w - g_ws]);
    HIP_TRY(hipMemsetAsync(w->meas_stats, 0, sizeof(unsigned), stream));
    launch(w->meas_stats);
    HIP_TRY(hipGetLastError());
    const unsigned keep = w->h_meas_stats[0];
    HIP_TRY(hipMemcpyAsync(w->h_meas_stats, w->meas_stats, sizeof(unsigned), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    *flag = w->h_meas_stats[0];
    w->h_meas_stats[0] = keep;
    return QCX_NO_ERROR;
}

// did the caller just write something that is not finite (or >= 2^500) into [first, first + count)?  (scanned on the device)
static int note_nonfinite(qcx_register *r, uint64_t first, uint64_t count)
{
    if (!count || r->nonfinite) return QCX_NO_ERROR;
    unsigned found = 0;
    QCX_TRY(scan_flag_word(r->stream, [&](unsigned *word) {
        hipLaunchKernelGGL(k_scan_nonfinite, dim3(grid_for(count, 256 * 8, 65536, 256)), dim3(256), 0, r->stream, (const amp_t *)(r->amp + first), count, word);
    }, &found));
    if (found) r->nonfinite = 1;
    return QCX_NO_ERROR;
}

static int strict_gate(qcx_register *r, const QGate &g)
{
    FLUSH(r);                                       // (nothing is queued in this mode; a pending reset would have cleared it)
    r->zeros_dirty = 0;                             // every strict pass rewrites every amplitude as 0 + ...: canonical zeros
    const uint64_t dim = r->dim;
    if (g.type == FUSE_H) {
        if (r->n < 1) return QCX_BAD_ARGUMENTS;
        hipLaunchKernelGGL(k_strict_h, dim3(grid_for(dim >> 1, 256, 65536, 256)), dim3(256), 0, r->stream, r->amp, r->n, g.q, M_SQRT1_2, 0.0);
    } else if (g.type == FUSE_PHASE) {
        hipLaunchKernelGGL(k_strict_phase, dim3(grid_for(dim, 256, 65536, 256)), dim3(256), 0, r->stream, r->amp, dim, g.mask, g.c, g.s, 1.0, 0.0);
    } else {
        const unsigned M = (unsigned)r->M;
        if (M > 12) { set_error("c_amodc_gate on a state with non-finite amplitudes: M = %u > 12 is not supported", M); return QCX_UNSUPPORTED; }
        const size_t lds = ((size_t)16 << M) + ((size_t)2 << M);
        hipLaunchKernelGGL(k_strict_camodc, dim3(grid_for(dim >> M, 1, 65536, 256)), dim3(256), lds, r->stream, r->amp, r->n, M, g.C, g.A, (int)g.q, 1.0, 0.0);
    }
    HIP_TRY(hipGetLastError());
    return QCX_NO_ERROR;
}

extern "C" int qcx_reset_register(qcx_register *r)
{
    if (!r) return QCX_BAD_ARGUMENTS;
    if (r->sh) return sh_reset(r->sh);
    if (r->queue) r->queue->gates.clear();         // pending gates act on a state that is being overwritten
    r->nonfinite = 0;
    r->zeros_dirty = 0;
    r->compact_pending = 0;
    if (r->fusion >= 0 && r->n >= 1) {             // lazily: the write happens at the next flush, fused with the circuit front (K0b)
        r->basis_pending = 1; r->basis_index = 1;
        return QCX_NO_ERROR;
    }
    r->basis_pending = 0;
    return qcx_shard_reset(r->amp, r->n, 1, r->stream);
}

// the same gate as the sharded queue takes it: LOGICAL qubits q (and q2) in the place of a mask
static SGate sharded_gate(const QGate &g, unsigned q, unsigned q2 = 0)
{
    SGate s; memset(&s, 0, sizeof s); s.type = g.type; s.q = q; s.q2 = q2; s.c = g.c; s.s = g.s; s.C = g.C; s.A = g.A;
    return s;
}

extern "C" int qcx_hadamard_gate(unsigned q, qcx_register *r)
{
    if (!r) return QCX_BAD_ARGUMENTS;
    if (q >= r->n) return QCX_BAD_QUBIT;
    QGate g; memset(&g, 0, sizeof g);
    g.type = FUSE_H; g.q = q;
    if (r->sh) return sh_push(r->sh, sharded_gate(g, q));
    if (r->nonfinite) return strict_gate(r, g);
    if (r->fusion > 0 || r->composite) return fuse_push(r, g);
    FLUSH(r);                                         // (a lazily pending reset / collapse is written first)
    QCX_TRY(canon_if_dirty(r));
    return qcx_shard_hadamard(r->amp, r->n, q, r->stream);
}

// e^{i theta} the way the reference obtains it: gsl_complex_polar(1.0, theta) = (1*cos, 1*sin) (Q:526), which
// gcc -O2 compiles to ONE glibc sincos() call (cos and sin of the same argument are merged).  glibc's sincos
// and its stand-alone sin/cos can differ in the last bit (e.g. sin(0.20966817126512538)), so sincos is called
// explicitly here and in the oracle instead of leaving the choice to each compiler.
extern "C" void qcx_polar(double theta, double *cos_out, double *sin_out)
{
    double sn, cs;
    sincos(theta, &sn, &cs);
    *cos_out = 1.0 * cs;
    *sin_out = 1.0 * sn;
}

extern "C" int qcx_c_phase_shift_gate(unsigned c, unsigned t, double theta, qcx_register *r)
{
    if (!r) return QCX_BAD_ARGUMENTS;
    if (c >= r->n || t >= r->n || c == t) return QCX_BAD_QUBIT;
    double er, ei;
    qcx_polar(theta, &er, &ei);
    QGate g; memset(&g, 0, sizeof g);
    g.type = FUSE_PHASE; g.mask = ((uint64_t)1 << c) | ((uint64_t)1 << t); g.c = er; g.s = ei;
    if (r->sh) return sh_push(r->sh, sharded_gate(g, c, t));
    if (r->nonfinite) return strict_gate(r, g);
    if (r->fusion > 0 || r->composite) return fuse_push(r, g);
    FLUSH(r);
    QCX_TRY(canon_if_dirty(r));
    return qcx_shard_phase(r->amp, r->n, g.mask, er, ei, r->stream);
}

// each component of a gate's matrix must be finite with |.| <= 1 (u: ncomp doubles, re and im interleaved)
static int check_matrix(const char *who, const double *u, int ncomp)
{
    for (int k = 0; k < ncomp; k++)
        if (!(fabs(u[k]) <= 1.0)) { set_error("%s: matrix component %d is %g (each must be finite with |.| <= 1)", who, k, u[k]); return QCX_BAD_ARGUMENTS; }
    return QCX_NO_ERROR;
}

// What a gate that is never queued (K12, K13, K15) does behind its argument checks: a sharded register is refused; queued gates,
// a pending basis state or a compact circuit result are flushed; a pass that rewrites every amplitude as 0 + ... -- the strict
// pass of a non-finite register, or a kernel that always does (rewrites_all) -- leaves canonical zeros, any other needs them.
static int unqueued_gate(qcx_register *r, const char *who, bool rewrites_all)
{
    if (r->sh) { set_error("%s: not available on a sharded register", who); return QCX_UNSUPPORTED; }
    FLUSH(r);
    if (r->nonfinite || rewrites_all) { r->zeros_dirty = 0; return QCX_NO_ERROR; }
    return canon_if_dirty(r);
}

// A gate on 1 or 2 targets under the controls (cmask, cvals) as the STRICT pass of a register flagged non-finite (K9): one plain
// pass over all pairs / quads, the two-qubit matrix permuted to lo < hi as every K13 kernel takes it.
static int strict_controlled_gate(qcx_register *r, uint64_t cmask, uint64_t cvals, unsigned ntargets, unsigned q0, unsigned q1, const double *u)
{
    if (ntargets == 1) {
        const UMat U = {u[0], u[1], u[2], u[3], u[4], u[5], u[6], u[7]};
        hipLaunchKernelGGL(k_strict_mcu, dim3(grid_for(r->dim >> 1, 256, 65536, 256)), dim3(256), 0, r->stream, r->amp, r->n, q0, cmask, cvals, U, 1.0, 0.0);
    } else {
        const U4Mat U = u4_ascending(q0, q1, u);
        const unsigned lo = q0 < q1 ? q0 : q1, hi = q0 < q1 ? q1 : q0;
        hipLaunchKernelGGL(k_strict_mcu2, dim3(grid_for(r->dim >> 2, 256, 65536, 256)), dim3(256), 0, r->stream, r->amp, r->n, lo, hi, cmask, cvals, U, 1.0, 0.0);
    }
    HIP_TRY(hipGetLastError());
    return QCX_NO_ERROR;
}

// Any one-qubit gate (ctl < 0: plain).  Never queued, in any fusion mode: the fused passes know H and phase only, so the call
// flushes what is pending and launches its own kernel (K12); the fusion statistics do not count it.
static int one_qubit_gate(int ctl, unsigned q, const double *u, qcx_register *r, const char *who)
{
    if (!r || !u) return QCX_BAD_ARGUMENTS;
    QCX_TRY(check_matrix(who, u, 8));
    if (q >= r->n || (ctl >= 0 && ((unsigned)ctl >= r->n || (unsigned)ctl == q))) return QCX_BAD_QUBIT;
    QCX_TRY(unqueued_gate(r, who, false));
    if (r->nonfinite && ctl >= 0) return strict_controlled_gate(r, (uint64_t)1 << ctl, (uint64_t)1 << ctl, 1, q, 0, u);     // (the plain kernels already are strict)
    return qcx_shard_one_qubit(r->amp, r->n, q, ctl, u, r->stream);
}

extern "C" int qcx_one_qubit_gate(unsigned q, const double *u, qcx_register *r)
{
    return one_qubit_gate(-1, q, u, r, "one_qubit_gate");
}

extern "C" int qcx_c_one_qubit_gate(unsigned c, unsigned q, const double *u, qcx_register *r)
{
    if (r && c >= r->n) return QCX_BAD_QUBIT;         // (before the cast: a control >= 2^31 is a bad qubit, not "no control")
    return one_qubit_gate((int)c, q, u, r, "c_one_qubit_gate");
}

// Any two-qubit gate (ctl < 0: plain).  one_qubit_gate()'s sequence: never queued, in any fusion mode; the call flushes what
// is pending and launches its own kernel (K13); the fusion statistics do not count it.
static int two_qubit_gate(int ctl, unsigned q0, unsigned q1, const double *u, qcx_register *r, const char *who)
{
    if (!r || !u) return QCX_BAD_ARGUMENTS;
    QCX_TRY(check_matrix(who, u, 32));
    if (q0 >= r->n || q1 >= r->n || q0 == q1) return QCX_BAD_QUBIT;
    if (ctl >= 0 && ((unsigned)ctl >= r->n || (unsigned)ctl == q0 || (unsigned)ctl == q1)) return QCX_BAD_QUBIT;
    QCX_TRY(unqueued_gate(r, who, false));
    if (r->nonfinite && ctl >= 0) return strict_controlled_gate(r, (uint64_t)1 << ctl, (uint64_t)1 << ctl, 2, q0, q1, u);   // (the plain kernels already are strict)
    return qcx_shard_two_qubit(r->amp, r->n, q0, q1, ctl, u, r->stream);
}

extern "C" int qcx_two_qubit_gate(unsigned q0, unsigned q1, const double *u, qcx_register *r)
{
    return two_qubit_gate(-1, q0, q1, u, r, "two_qubit_gate");
}

extern "C" int qcx_c_two_qubit_gate(unsigned c, unsigned q0, unsigned q1, const double *u, qcx_register *r)
{
    if (r && c >= r->n) return QCX_BAD_QUBIT;         // (before the cast: a control >= 2^31 is a bad qubit, not "no control")
    return two_qubit_gate((int)c, q0, q1, u, r, "c_two_qubit_gate");
}

// A one- or two-qubit gate under a control mask (K17).  one_qubit_gate()'s sequence behind the checks of include/qcx.h, in their
// order.  No control and one positive control ARE the calls above -- the same kernels and launches -- unless mc_generic is set.
static int mc_gate(uint64_t cmask, uint64_t cvals, unsigned ntargets, unsigned q0, unsigned q1, const double *u, qcx_register *r, const char *who)
{
    if (!r || !u) return QCX_BAD_ARGUMENTS;
    QCX_TRY(check_matrix(who, u, ntargets == 1 ? 8 : 32));
    QCX_TRY(mc_check(who, r->n, cmask, cvals, ntargets, q0, q1));          // (mc_launch() plans without repeating them)
    if (tune_now().mc_generic == 0 && (cmask == 0 || (cmask == cvals && (cmask & (cmask - 1)) == 0))) {
        const int ctl = cmask ? (int)__builtin_ctzll(cmask) : -1;
        return ntargets == 1 ? one_qubit_gate(ctl, q0, u, r, who) : two_qubit_gate(ctl, q0, q1, u, r, who);
    }
    QCX_TRY(unqueued_gate(r, who, false));
    if (r->nonfinite) return strict_controlled_gate(r, cmask, cvals, ntargets, q0, q1, u);
    return mc_launch(r->amp, r->n, cmask, cvals, ntargets, q0, q1, u, r->stream);
}

extern "C" int qcx_mc_one_qubit_gate(uint64_t ctrl_mask, uint64_t ctrl_values, unsigned q, const double *u, qcx_register *r)
{
    return mc_gate(ctrl_mask, ctrl_values, 1, q, 0, u, r, "mc_one_qubit_gate");
}

extern "C" int qcx_mc_two_qubit_gate(uint64_t ctrl_mask, uint64_t ctrl_values, unsigned q0, unsigned q1, const double *u, qcx_register *r)
{
    return mc_gate(ctrl_mask, ctrl_values, 2, q0, q1, u, r, "mc_two_qubit_gate");
}

// The passes of a batch plan, in order: pass_of is non-decreasing over the items, a pass a run of equal values.  each(first item,
// count, pass number) returns a status; the first that is not QCX_NO_ERROR ends the walk and is returned.
template <typename Each>
static int for_each_pass(const std::vector<unsigned long> &pass_of, Each each)
{
    for (unsigned long k = 0, n = pass_of.size(); k < n;) {
        unsigned cnt = 1;
        while (k + cnt < n && pass_of[k + cnt] == pass_of[k]) cnt++;
        QCX_TRY(each(k, cnt, pass_of[k]));
        k += cnt;
    }
    return QCX_NO_ERROR;
}

// exp(-i theta/2 P) of the Pauli string (x_mask, z_mask).  one_qubit_gate()'s sequence: never queued, in any fusion mode; the
// call flushes what is pending and launches its own kernel (K15); the fusion statistics do not count it.  The kernel rewrites
// every amplitude from its own row's products, so it is its own strict pass: a non-finite register keeps its flag and runs it too.
extern "C" int qcx_pauli_rotation(uint64_t x_mask, uint64_t z_mask, double theta, qcx_register *r)
{
    if (!r) return QCX_BAD_ARGUMENTS;
    if (!std::isfinite(theta)) { set_error("pauli_rotation: theta is %g", theta); return QCX_BAD_ARGUMENTS; }
    if ((x_mask | z_mask) >> r->n) {
        set_error("pauli_rotation: masks %#llx / %#llx reach past the %u qubits", (unsigned long long)x_mask, (unsigned long long)z_mask, r->n);
        return QCX_BAD_QUBIT;
    }
    QCX_TRY(unqueued_gate(r, "pauli_rotation", true));
    double c, s;
    qcx_polar(theta / 2.0, &c, &s);
    return qcx_shard_pauli_rotation(r->amp, r->n, x_mask, z_mask, c, s, r->stream);
}

// A list of rotations, in order, as the passes of qcx_pauli_rotation_batch_plan: a run of terms whose partners stay inside one
// tile is one k_prot_run launch (K15b), a wide term its own k_pauli_rot launch.  Every term is K15's arithmetic with its own
// (c, s) = polar(theta / 2), so the state is what the loop of qcx_pauli_rotation leaves; everything else is that call's sequence.
extern "C" int qcx_pauli_rotation_batch(qcx_register *r, unsigned long nterms, const uint64_t *x_masks, const uint64_t *z_masks,
                                        const double *thetas)
{
    if (!r || (nterms && (!x_masks || !z_masks || !thetas))) return QCX_BAD_ARGUMENTS;
    for (unsigned long k = 0; k < nterms; k++)
        if (!std::isfinite(thetas[k])) { set_error("pauli_rotation_batch: theta of term %lu is %g", k, thetas[k]); return QCX_BAD_ARGUMENTS; }
    for (unsigned long k = 0; k < nterms; k++)
        if ((x_masks[k] | z_masks[k]) >> r->n) {
            set_error("pauli_rotation_batch: term %lu's masks %#llx / %#llx reach past the %u qubits", k, (unsigned long long)x_masks[k],
                      (unsigned long long)z_masks[k], r->n);
            return QCX_BAD_QUBIT;
        }
    if (r->sh) { set_error("pauli_rotation_batch: not available on a sharded register"); return QCX_UNSUPPORTED; }
    r->rotb_passes = 0; r->rotb_wide = 0;
    if (nterms == 0) return QCX_NO_ERROR;
    std::vector<unsigned long> pass_of(nterms);
    std::vector<unsigned> kind(nterms);
    std::vector<uint64_t> hot(nterms);
    unsigned long np = 0;
    QCX_TRY(qcx_pauli_rotation_batch_plan(r->n, nterms, x_masks, QCX_PROT_RUN_W, pass_of.data(), &np, kind.data(), hot.data()));
    QCX_TRY(unqueued_gate(r, "pauli_rotation_batch", true));
    return for_each_pass(pass_of, [&](unsigned long k, unsigned cnt, unsigned long p) {
        double cs[QCX_PROT_RUN_W], ss[QCX_PROT_RUN_W];
        for (unsigned c = 0; c < cnt; c++) qcx_polar(thetas[k + c] / 2.0, &cs[c], &ss[c]);
        if (kind[p] == 1) { QCX_TRY(qcx_shard_pauli_rotation(r->amp, r->n, x_masks[k], z_masks[k], cs[0], ss[0], r->stream)); r->rotb_wide++; }
        else QCX_TRY(qcx_shard_pauli_rotation_run(r->amp, r->n, hot[p], cnt, x_masks + k, z_masks + k, cs, ss, r->stream));
        r->rotb_passes++;
        return (int)QCX_NO_ERROR;
    });
}

extern "C" int qcx_rotation_batch_last_stats(qcx_register *r, unsigned long *passes, unsigned long *wide_terms)
{
    if (!r) return QCX_BAD_ARGUMENTS;
    if (passes) *passes = r->rotb_passes;
    if (wide_terms) *wide_terms = r->rotb_wide;
    return QCX_NO_ERROR;
}

// ---- the diagonal of a qubit range from a table (K18) ---------------------------------------------------------------------------
#define QCX_DIAG_HOST_MAX 20u
extern "C" unsigned qcx_diagonal_host_max_qubits(void) { return QCX_DIAG_HOST_MAX; }

extern "C" void qcx_polar_array(unsigned long count, const double *thetas, double *out_re_im)
{
    for (unsigned long k = 0; k < count; k++) qcx_polar(thetas[k], out_re_im + 2 * k, out_re_im + 2 * k + 1);
}

// behind the checks: qcx_pauli_rotation's sequence, then the launch the plan gives
static int diagonal_run(qcx_register *r, const char *who, unsigned first, unsigned num, const amp_t *tab_dev)
{
    QCX_TRY(unqueued_gate(r, who, true));
    qcx_diag_plan pl;
    QCX_TRY(qcx_diagonal_plan(r->n, first, num, &pl));
    r->diag_form = pl.form; r->diag_entries = (unsigned long)(pl.kmask + 1);
    return qcx_shard_diagonal(r->amp, r->n, first, num, tab_dev, r->stream);
}

// The host form: the table goes to the device as a StagedUpload (r->diag_up, grown on demand), sent before the flush.
extern "C" int qcx_diagonal_gate(unsigned first, unsigned num, const double *d, qcx_register *r)
{
    if (!r || !d) return QCX_BAD_ARGUMENTS;
    QCX_TRY(check_range(r->n, first, num, nullptr));
    if (num > QCX_DIAG_HOST_MAX) {
        set_error("diagonal_gate: a table over %u qubits is more than the host form takes (%u); build it on the device and call qcx_diagonal_gate_device", num, QCX_DIAG_HOST_MAX);
        return QCX_BAD_ARGUMENTS;
    }
    const size_t entries = (size_t)1 << num;
    for (size_t k = 0; k < 2 * entries; k++)
        if (!(fabs(d[k]) <= 1.0)) {
            set_error("diagonal_gate: entry %zu's %s part is %g (each component must be finite with |.| <= 1)", k >> 1, (k & 1) ? "imaginary" : "real", d[k]);
            return QCX_BAD_ARGUMENTS;
        }
    if (r->sh) { set_error("diagonal_gate: not available on a sharded register"); return QCX_UNSUPPORTED; }
    QCX_TRY(r->diag_up.reserve(entries * sizeof(amp_t), 4096 * sizeof(amp_t), r->stream));
    memcpy(r->diag_up.pinned, d, entries * sizeof(amp_t));
    QCX_TRY(r->diag_up.send(entries * sizeof(amp_t), r->stream));
    return diagonal_run(r, "diagonal_gate", first, num, (const amp_t *)r->diag_up.dev);
}

// The device form: the caller's table in place.  Where it lies is checked on the host; what it holds, on the device, on the
// register's stream (k_diag_scan through scan_flag_word: one sync) -- before the flush, so a refusal touches nothing.
extern "C" int qcx_diagonal_gate_device(unsigned first, unsigned num, const void *d_device, qcx_register *r)
{
    if (!r || !d_device) return QCX_BAD_ARGUMENTS;
    QCX_TRY(check_range(r->n, first, num, nullptr));
    const uint64_t entries = ((uint64_t)1) << num, bytes = entries * sizeof(amp_t);
    hipPointerAttribute_t at;
    memset(&at, 0, sizeof at);
    if (hipPointerGetAttributes(&at, d_device) != hipSuccess || at.type != hipMemoryTypeDevice) {
        (void)hipGetLastError();
        set_error("diagonal_gate_device: the table at %p is not device memory", d_device);
        return QCX_BAD_ARGUMENTS;
    }
    if (((uintptr_t)d_device & 15u) != 0) { set_error("diagonal_gate_device: the table at %p is not aligned to 16 bytes", d_device); return QCX_BAD_ARGUMENTS; }
    void *base = nullptr; size_t size = 0;
    if (hipMemGetAddressRange((hipDeviceptr_t *)&base, &size, (hipDeviceptr_t)d_device) == hipSuccess) {
        if ((uintptr_t)d_device + bytes > (uintptr_t)base + size) {
            set_error("diagonal_gate_device: 2^%u entries from %p run past the end of their allocation", num, d_device);
            return QCX_BAD_ARGUMENTS;
        }
    } else (void)hipGetLastError();
    if (r->sh) { set_error("diagonal_gate_device: not available on a sharded register"); return QCX_UNSUPPORTED; }
    hipPointerAttribute_t ra;
    memset(&ra, 0, sizeof ra);
    HIP_TRY(hipPointerGetAttributes(&ra, r->amp));
    if (at.device != ra.device) {
        set_error("diagonal_gate_device: the table lies on device %d, the register on device %d", at.device, ra.device);
        return QCX_BAD_ARGUMENTS;
    }
    const uintptr_t t0 = (uintptr_t)d_device, t1 = t0 + bytes;
    const auto overlaps = [&](const amp_t *p) { const uintptr_t a0 = (uintptr_t)p, a1 = a0 + (uintptr_t)(r->dim * sizeof(amp_t)); return p && t0 < a1 && a0 < t1; };
    if (overlaps(r->amp) || overlaps(r->scratch)) { set_error("diagonal_gate_device: the table overlaps the register's buffer"); return QCX_BAD_ARGUMENTS; }
    unsigned bad = 0;
    QCX_TRY(scan_flag_word(r->stream, [&](unsigned *word) {
        hipLaunchKernelGGL(k_diag_scan, dim3(grid_for(entries, 256 * 8, 65536, 256)), dim3(256), 0, r->stream, (const amp_t *)d_device, entries, word);
    }, &bad));
    if (bad) { set_error("diagonal_gate_device: the table holds a component that is not finite or exceeds 1 in absolute value"); return QCX_BAD_ARGUMENTS; }
    return diagonal_run(r, "diagonal_gate_device", first, num, (const amp_t *)d_device);
}

extern "C" int qcx_diagonal_last_stats(qcx_register *r, unsigned *form, unsigned long *table_entries)
{
    if (!r) return QCX_BAD_ARGUMENTS;
    if (form) *form = r->diag_form;
    if (table_entries) *table_entries = r->diag_entries;
    return QCX_NO_ERROR;
}

// ---- a permutation of a qubit range's basis states from a table (K19) -------------------------------------------------------------
extern "C" unsigned qcx_permutation_max_qubits(void) { return QCX_PERM_MAX_QUBITS; }

// one_qubit_gate()'s sequence behind the checks of include/qcx.h, in their order.  The inverse table goes to the device as a
// StagedUpload (r->perm_up), reserved before the flush and sent behind it; the identity sends nothing.
extern "C" int qcx_permutation_gate(uint64_t cmask, uint64_t cvals, unsigned first, unsigned num, const uint32_t *perm, qcx_register *r)
{
    if (!r || !perm) return QCX_BAD_ARGUMENTS;
    qcx_perm_plan pl;
    QCX_TRY(qcx_permutation_plan(r->n, cmask, cvals, first, num, &pl));        // (the argument checks, in the header's order)
    uint16_t inv[1u << QCX_PERM_MAX_QUBITS];
    unsigned long moved = 0;
    QCX_TRY(permutation_invert(num, perm, inv, &moved));
    if (r->sh) { set_error("permutation_gate: not available on a sharded register"); return QCX_UNSUPPORTED; }
    QCX_TRY(r->perm_up.reserve(sizeof inv, sizeof inv, r->stream));
    QCX_TRY(unqueued_gate(r, "permutation_gate", false));
    r->perm_form = pl.geom.form; r->perm_moved = moved;
    if (moved == 0 && !r->nonfinite) return QCX_NO_ERROR;                      // the identity on finite amplitudes whose zeros are +0
    const size_t bytes = sizeof(uint16_t) << num;
    memcpy(r->perm_up.pinned, inv, bytes);
    QCX_TRY(r->perm_up.send(bytes, r->stream));
    return permutation_launch(r->amp, r->n, cmask, cvals, first, num, r->nonfinite != 0, (const uint16_t *)r->perm_up.dev, r->stream);
}

extern "C" int qcx_permutation_last_stats(qcx_register *r, unsigned *form, unsigned long *moved)
{
    if (!r) return QCX_BAD_ARGUMENTS;
    if (form) *form = r->perm_form;
    if (moved) *moved = r->perm_moved;
    return QCX_NO_ERROR;
}

// ---- a dense matrix on 1 .. 5 target qubits under a control mask (K20) ---------------------------------------------------------------
extern "C" unsigned qcx_multi_qubit_max_targets(void) { return QCX_MULTI_MAX_TARGETS; }

// mc_gate()'s sequence behind the checks of include/qcx.h, in their order.  One and two targets ARE mc_gate() -- the same kernels
// and launches -- unless multi_generic is set.  The ascending matrix is written straight into the pinned buffer of a
// StagedUpload (r->multi_up), reserved before the flush and sent behind it.
extern "C" int qcx_mc_multi_qubit_gate(uint64_t cmask, uint64_t cvals, unsigned k, const unsigned *targets, const double *u, qcx_register *r)
{
    const char *who = "mc_multi_qubit_gate";
    if (!r || !u || !targets) return QCX_BAD_ARGUMENTS;
    if (k == 0 || k > QCX_MULTI_MAX_TARGETS) {
        set_error("%s: %u targets; a matrix acts on 1 to %u qubits", who, k, (unsigned)QCX_MULTI_MAX_TARGETS);
        return QCX_BAD_ARGUMENTS;
    }
    QCX_TRY(check_matrix(who, u, 2 << (2 * k)));
    qcx_multi_plan pl;
    QCX_TRY(qcx_multi_gate_plan(r->n, cmask, cvals, k, targets, &pl));         // (the other argument checks, in the header's order)
    if (r->sh) { set_error("%s: not available on a sharded register", who); return QCX_UNSUPPORTED; }
    if (k <= 2 && tune_now().multi_generic == 0) {
        r->multi_form = pl.geom.form; r->multi_k = k;
        return mc_gate(cmask, cvals, k, targets[0], k == 2 ? targets[1] : 0, u, r, who);
    }
    constexpr size_t cap = sizeof(double) * (2u << (2 * QCX_MULTI_MAX_TARGETS));
    QCX_TRY(r->multi_up.reserve(cap, cap, r->stream));
    QCX_TRY(unqueued_gate(r, who, false));
    r->multi_form = pl.geom.form; r->multi_k = k;
    unsigned char sorted[QCX_MULTI_MAX_TARGETS];
    multi_ascending(k, targets, u, (double *)r->multi_up.pinned, sorted);
    QCX_TRY(r->multi_up.send(sizeof(double) * (2u << (2 * k)), r->stream));
    return multi_launch(r->amp, r->n, cmask, cvals, k, targets, sorted, r->nonfinite != 0, (const double *)r->multi_up.dev, r->stream);
}

extern "C" int qcx_multi_qubit_last_stats(qcx_register *r, unsigned *form, unsigned *num_targets)
{
    if (!r) return QCX_BAD_ARGUMENTS;
    if (form) *form = r->multi_form;
    if (num_targets) *num_targets = r->multi_k;
    return QCX_NO_ERROR;
}

// A list of one- and two-qubit gates, in order, as the passes of qcx_gate_batch_plan: a run of gates whose targets lie inside one
// tile is one k_gate_run launch (K12b / K13b).  Every output amplitude is its own row of K12's / K13's arithmetic, so the state is
// what the loop of the four gate calls leaves; everything else is one_qubit_gate()'s sequence.  A register flagged non-finite
// runs that loop itself: its controlled gates need the strict kernels, which rewrite the control-clear amplitudes too.
extern "C" int qcx_gate_batch(qcx_register *r, unsigned long ngates, const qcx_gate *gates)
{
    if (!r || (ngates && !gates)) return QCX_BAD_ARGUMENTS;
    for (unsigned long k = 0; k < ngates; k++)
        if (gates[k].ntargets != 1 && gates[k].ntargets != 2) { set_error("gate_batch: gate %lu has %u targets (1 or 2)", k, gates[k].ntargets); return QCX_BAD_ARGUMENTS; }
    for (unsigned long k = 0; k < ngates; k++)
        for (int c = 0, nc = gates[k].ntargets == 2 ? 32 : 8; c < nc; c++)
            if (!(fabs(gates[k].u[c]) <= 1.0)) {
                set_error("gate_batch: gate %lu's matrix component %d is %g (each must be finite with |.| <= 1)", k, c, gates[k].u[c]);
                return QCX_BAD_ARGUMENTS;
            }
    for (unsigned long k = 0; k < ngates; k++)
        if (!gate_qubits_ok(gates[k], r->n)) {
            set_error("gate_batch: gate %lu's qubits (control %d, qubit0 %u, qubit1 %u with %u targets) are not distinct qubits of the %u", k,
                      gates[k].control, gates[k].qubit0, gates[k].qubit1, gates[k].ntargets, r->n);
            return QCX_BAD_QUBIT;
        }
    if (r->sh) { set_error("gate_batch: not available on a sharded register"); return QCX_UNSUPPORTED; }
    r->gateb_passes = 0; r->gateb_lds = 0;
    if (ngates == 0) return QCX_NO_ERROR;
    std::vector<uint64_t> masks(ngates), hot(ngates);
    std::vector<unsigned> units(ngates);
    std::vector<unsigned long> pass_of(ngates);
    for (unsigned long k = 0; k < ngates; k++) { masks[k] = gate_targets(gates[k]); units[k] = gates[k].ntargets == 2 ? 4u : 1u; }
    unsigned long np = 0;
    QCX_TRY(qcx_gate_batch_plan(r->n, ngates, masks.data(), units.data(), QCX_GATE_RUN_W, pass_of.data(), &np, hot.data()));
    QCX_TRY(unqueued_gate(r, "gate_batch", false));
    if (r->nonfinite) {
        for (unsigned long k = 0; k < ngates; k++) {
            const qcx_gate &g = gates[k];
            if (g.ntargets == 2) QCX_TRY(two_qubit_gate(g.control < 0 ? -1 : g.control, g.qubit0, g.qubit1, g.u, r, "gate_batch"));
            else QCX_TRY(one_qubit_gate(g.control < 0 ? -1 : g.control, g.qubit0, g.u, r, "gate_batch"));
            r->gateb_passes++;
        }
        return QCX_NO_ERROR;
    }
    return for_each_pass(pass_of, [&](unsigned long k, unsigned cnt, unsigned long p) {
        QCX_TRY(qcx_shard_gate_run(r->amp, r->n, hot[p], cnt, gates + k, r->stream));
        for (unsigned c = 0; c < cnt; c++)
            if (masks[k + c] & 0xFF) r->gateb_lds++;
        r->gateb_passes++;
        return (int)QCX_NO_ERROR;
    });
}

extern "C" int qcx_gate_batch_last_stats(qcx_register *r, unsigned long *passes, unsigned long *lds_gates)
{
    if (!r) return QCX_BAD_ARGUMENTS;
    if (passes) *passes = r->gateb_passes;
    if (lds_gates) *lds_gates = r->gateb_lds;
    return QCX_NO_ERROR;
}

extern "C" int qcx_c_amodc_gate(unsigned C, unsigned long long atox, unsigned c, qcx_register *r)
{
    if (!r || C == 0) return QCX_BAD_ARGUMENTS;
    if (c >= r->n) return QCX_BAD_QUBIT;
    QGate g; memset(&g, 0, sizeof g);
    g.type = FUSE_CAMODC; g.q = c; g.C = C; g.A = (unsigned)(atox % C);
    if (r->sh) return sh_push(r->sh, sharded_gate(g, c));
    if (r->nonfinite) return strict_gate(r, g);
    if (r->fusion > 0 || r->composite) {
        if (!camodc_closed_form(r->n, (unsigned)r->M, C, g.A, c)) g.type = 99u;      // (queued, but runs stand-alone)
        return fuse_push(r, g);
    }
    FLUSH(r);
    QCX_TRY(canon_if_dirty(r));
    return reg_camodc(r, C, g.A, c);
}

extern "C" int qcx_swap_states(qcx_register *r) { return r ? QCX_NO_ERROR : QCX_BAD_ARGUMENTS; }

// The whole-circuit entry points know their complete gate list, so unless the register is in strict per-gate mode
// (qcx_set_fusion(reg, -1)) they hand it to the pass scheduler in one piece: same bits, one HBM round trip per pass
// instead of one per gate.  Nested use (quantum_computation -> inverse_QFT) flushes once, at the outermost exit.
struct CircuitScope {
    qcx_register *r;
    bool mine;
    explicit CircuitScope(qcx_register *r_) : r(r_), mine(!r_->sh && r_->fusion == 0) { if (mine) r->composite++; }
    int done(int status)
    {
        if (!mine) return status;
        mine = false;
        if (--r->composite == 0) { const int f = fuse_flush(r, true); if (status == QCX_NO_ERROR) status = f; }     // (a compact chain's result may stay compact)
        return status;
    }
    ~CircuitScope() { (void)done(QCX_NO_ERROR); }
};

static int inverse_qft_body(qcx_register *r)
{
    for (int l = r->L + r->M - 1; l >= r->M; l--) {
        QCX_TRY(qcx_hadamard_gate((unsigned)l, r));
        for (int k = l - 1; k >= r->M; k--) {
            const double theta = M_PI / (double)((uint64_t)1 << (unsigned)(l - k));   // Q:686
            QCX_TRY(qcx_c_phase_shift_gate((unsigned)l, (unsigned)k, theta, r));
        }
    }
    return QCX_NO_ERROR;
}

extern "C" int qcx_inverse_QFT(qcx_register *r)
{
    if (!r) return QCX_BAD_ARGUMENTS;
    CircuitScope scope(r);
    return scope.done(inverse_qft_body(r));
}

// the reference's INT_POW (Q:158-159) as x86-64 gcc evaluates it: pow, +0.5, truncation to a
// signed 64-bit integer (out of range gives 0x8000000000000000), low 32 bits kept
extern "C" unsigned qcx_ref_int_pow(double base, double power)
{
    const double d = pow(base, power) + 0.5;
    if (!(d > -9223372036854775808.0 && d < 9223372036854775808.0)) return 0u;
    return (unsigned)(unsigned long long)(long long)d;
}

static int quantum_computation_body(unsigned C, unsigned a, int intpow_mode, qcx_register *r);

extern "C" int qcx_quantum_computation(unsigned C, unsigned a, int intpow_mode, qcx_register *r)
{
    if (!r || C == 0) return QCX_BAD_ARGUMENTS;
    CircuitScope scope(r);
    return scope.done(quantum_computation_body(C, a, intpow_mode, r));
}

static int quantum_computation_body(unsigned C, unsigned a, int intpow_mode, qcx_register *r)
{
    const unsigned lo = r->n - (unsigned)r->L;
    for (unsigned l = lo; l < r->n; l++) QCX_TRY(qcx_hadamard_gate(l, r));
    unsigned x = 1;                                   // Q:714
    unsigned long long exact = a % C;                 // a^(2^k) mod C by repeated squaring
    for (unsigned l = lo; l < r->n; l++) {
        const unsigned long long atox = intpow_mode ? (unsigned long long)qcx_ref_int_pow((double)a, (double)x) : exact;
        QCX_TRY(qcx_c_amodc_gate(C, atox, l, r));
        x *= 2;                                       // Q:730
        exact = (exact * exact) % C;
    }
    return inverse_qft_body(r);
}

// the observers' prologue: the queue flushed, a compact chain's result kept compact -- its deferred last pass run as an ordinary
// pass, since the observers read the compact form
static int settle_for_read(qcx_register *r)
{
    QCX_TRY(fuse_flush(r, true));
    return compact_finish_last(r, false);
}

// the state is the lazily pending basis state (amplitude 1 at basis_index) with no gate queued behind it: answered on the host
static bool basis_only(const qcx_register *r)
{
    return r->basis_pending && (!r->queue || r->queue->gates.empty());
}

// The scan of Q:283-292 on whichever form holds the state (after settle_for_read).  On the compact form the amplitudes left out
// are +0 and add exactly nothing to the running sum, and the compact order IS the index order (orbit ascending), so the first
// compact element with cum >= r is the first real one -- except for r <= 0, where the reference stops at index 0 whatever it
// holds.  A hit in a padding column is not mapped through stale orbit slots: the state is expanded (same bits) and the register
// scanned.
static int scan_state(qcx_register *r, double rnd, uint64_t *idx)
{
    int found = 0; uint64_t i = 0; double cum = 0.0;
    *idx = r->dim - 1;                                                      // Q:283 fall-through
    if (r->compact_pending) {
        const ExpandParams &E = r->compact_E;
        if (rnd <= 0.0) { *idx = 0; return QCX_NO_ERROR; }
        QCX_TRY(qcx_shard_measure_scan(r->compact_amp, r->n - E.M + E.cb, 0, compact_scan_end(r->n, E), 0.0, rnd, &found, &i, &cum, r->stream));
        if (!found || compact_real_index(E, i, idx)) return QCX_NO_ERROR;
        QCX_TRY(expand_pending(r));
    }
    QCX_TRY(qcx_shard_measure_scan(r->amp, r->n, 0, r->dim - 1, 0.0, rnd, &found, &i, &cum, r->stream));
    if (found) *idx = i;
    return QCX_NO_ERROR;
}

extern "C" int qcx_measure_state_r(qcx_register *r, double rnd, unsigned long *state_num)
{
    if (!r || !state_num) return QCX_BAD_ARGUMENTS;
    if (r->sh) return sh_measure(r->sh, rnd, state_num);
    QCX_TRY(settle_for_read(r));
    const bool compact = r->compact_pending != 0;
    uint64_t idx = 0;
    QCX_TRY(scan_state(r, rnd, &idx));
    if (compact) { r->compact_pending = 0; r->compact_measures++; }
    r->zeros_dirty = 0;                                                     // (the collapse replaces the whole state)
    r->nonfinite = 0;
    if (r->fusion >= 0) { r->basis_pending = 1; r->basis_index = idx; }     // Q:302-303, written at the next flush (or never: a reset may follow)
    else QCX_TRY(qcx_shard_collapse(r->amp, r->n, (int64_t)idx, r->stream));
    *state_num = (unsigned long)idx;
    return QCX_NO_ERROR;
}

extern "C" int qcx_measure_state(qcx_register *r, qcx_rng *rng, unsigned long *state_num)
{
    if (!rng) return QCX_BAD_ARGUMENTS;
    return qcx_measure_state_r(r, qcx_rng_uniform(rng), state_num);         // Q:281
}

// K4d: many shots from the current state, which stays exactly as it is (include/qcx.h).  out[i] = what qcx_measure_state_r(r, rs[i])
// would return: the same scan on the same form of the state -- the register, or the compact form of a circuit's result --, one
// scan for all shots; a shot the fast path cannot vouch for is answered by that very scan of its own (no collapse).
static int sample_fallback_shot(qcx_register *r, double rnd, unsigned long *out)
{
    uint64_t idx = 0;
    r->samp_scans++; r->samp_fallback++;
    QCX_TRY(scan_state(r, rnd, &idx));
    *out = (unsigned long)idx;
    return QCX_NO_ERROR;
}

extern "C" int qcx_sample_states_r(qcx_register *r, const double *rs, unsigned long shots, unsigned long *state_nums)
{
    if (!r) return QCX_BAD_ARGUMENTS;
    if (shots == 0) return QCX_NO_ERROR;
    if (!rs || !state_nums) return QCX_BAD_ARGUMENTS;
    if (r->sh) return QCX_UNSUPPORTED;
    r->samp_scans = 0; r->samp_fallback = 0;
    if (basis_only(r)) {
        // the running sum is 0 before the basis state k and 1 from k on -- nothing to scan, and the state stays unwritten
        const unsigned long k = (unsigned long)r->basis_index;
        for (unsigned long i = 0; i < shots; i++) state_nums[i] = rs[i] <= 0.0 ? 0ul : (rs[i] <= 1.0 ? k : (unsigned long)(r->dim - 1));
        return QCX_NO_ERROR;
    }
    QCX_TRY(settle_for_read(r));
    if (r->nonfinite) {                                                     // the fast path's arithmetic wants finite sums: every shot its own scan
        for (unsigned long i = 0; i < shots; i++) QCX_TRY(sample_fallback_shot(r, rs[i], &state_nums[i]));
        return QCX_NO_ERROR;
    }
    std::vector<uint64_t> res(shots);
    const bool compact = r->compact_pending != 0;
    const ExpandParams &E = r->compact_E;
    if (compact) {
        QCX_TRY(sample_scan(r->compact_amp, r->n - E.M + E.cb, compact_scan_end(r->n, E), rs, shots, res.data(), r->stream));
        r->compact_measures++;
    } else
        QCX_TRY(sample_scan(r->amp, r->n, r->dim - 1, rs, shots, res.data(), r->stream));
    r->samp_scans = 1;
    for (unsigned long i = 0; i < shots; i++) {
        const uint64_t v = res[i];
        uint64_t idx = v;
        if (rs[i] <= 0.0) state_nums[i] = 0;                                // Q:289 (the compact scan's element 0 need not be index 0)
        else if (v == QCX_SAMP_NOTFOUND) state_nums[i] = (unsigned long)(r->dim - 1);
        else if (v == QCX_SAMP_FALLBACK || (compact && !compact_real_index(E, v, &idx)))
            QCX_TRY(sample_fallback_shot(r, rs[i], &state_nums[i]));
        else state_nums[i] = (unsigned long)idx;
    }
    return QCX_NO_ERROR;
}

extern "C" int qcx_sample_states(qcx_register *r, qcx_rng *rng, unsigned long shots, unsigned long *state_nums)
{
    if (!r || (!rng && shots)) return QCX_BAD_ARGUMENTS;
    if (shots == 0) return QCX_NO_ERROR;
    if (!state_nums) return QCX_BAD_ARGUMENTS;
    if (r->sh) return QCX_UNSUPPORTED;
    std::vector<double> rs(shots);
    for (unsigned long i = 0; i < shots; i++) rs[i] = qcx_rng_uniform(rng);  // Q:281, one draw a shot
    return qcx_sample_states_r(r, rs.data(), shots, state_nums);
}

extern "C" int qcx_sample_last_stats(qcx_register *r, unsigned long *state_scans, unsigned long *fallback_shots)
{
    if (!r) return QCX_BAD_ARGUMENTS;
    if (state_scans) *state_scans = r->samp_scans;
    if (fallback_shots) *fallback_shots = r->samp_fallback;
    return QCX_NO_ERROR;
}

// the buffer of K10's and K14's stages: at least `need` doubles
static int marg_reserve(qcx_register *r, size_t need)
{
    if (r->marg_cap >= need) return QCX_NO_ERROR;
    if (r->marg_buf) HIP_TRY(hipFree(r->marg_buf));
    r->marg_buf = nullptr; r->marg_cap = 0;
    HIP_TRY(hipMalloc(&r->marg_buf, need * sizeof(double)));
    r->marg_cap = need;
    return QCX_NO_ERROR;
}

// the doubles a plan's partials take: every stage but the final one writes 2^out_bits of them at its out_offset
static size_t stages_scratch(const qcx_marginal_stage *st, unsigned ns)
{
    size_t scratch = 0;
    for (unsigned i = 0; i < ns; i++)
        if (!st[i].final_stage) scratch = std::max<size_t>(scratch, (size_t)(st[i].out_offset + (((uint64_t)1) << st[i].out_bits)));
    return scratch;
}

// Stages [from, ns) of a plan, each a k_marginal<MARG_DBL> launch on r->stream: a stage reads the partials of the stage before it
// at base + out_offset (stage 0: at base), the final one writes to out.  That kernel never looks at `bad` (MARG_COMPACT's word).
static int later_stages(qcx_register *r, const qcx_marginal_stage *st, unsigned from, unsigned ns, double *base, double *out, unsigned *bad)
{
    for (unsigned i = from; i < ns; i++) {
        MargParams P;
        marginal_params(st[i], &P);
        P.src = i == 0 ? base : base + st[i - 1].out_offset;
        P.dst = st[i].final_stage ? out : base + st[i].out_offset;
        P.bad = bad;
        hipLaunchKernelGGL(k_marginal<MARG_DBL>, dim3((unsigned)std::min<uint64_t>(P.ntiles, 2048)), dim3(256), 0, r->stream, P);
        HIP_TRY(hipGetLastError());
    }
    return QCX_NO_ERROR;
}

// K10: the marginal of bits [first, first + num) (include/qcx.h, DESIGN s4.5d).  The planned stages run on r->stream: the first
// reads the state (the register, or the compact form in place), the others only the partials; then one copy of the output.
static int marginal_launch(qcx_register *r, const void *src, bool compact, unsigned first, unsigned num, double *probs, bool *bad_out)
{
    qcx_marginal_stage st[QCX_MARGINAL_MAX_STAGES];
    unsigned ns = 0;
    if (compact) QCX_TRY(qcx_marginal_plan_compact(r->n, (unsigned)r->M, first, num, st, &ns));
    else QCX_TRY(qcx_marginal_plan(r->n, first, num, st, &ns));
    const size_t scratch = stages_scratch(st, ns), nout = (size_t)1 << num;
    QCX_TRY(marg_reserve(r, scratch + nout + 1));
    double *const out = r->marg_buf + scratch;
    unsigned *const bad = (unsigned *)(out + nout);
    if (compact) HIP_TRY(hipMemsetAsync(bad, 0, sizeof(unsigned), r->stream));
    {
        MargParams P;
        marginal_params(st[0], &P);
        P.src = src;
        P.dst = st[0].final_stage ? out : r->marg_buf + st[0].out_offset;
        P.bad = bad;
        const unsigned grid = (unsigned)std::min<uint64_t>(P.ntiles, 2048);
        if (st[0].kind == 2) {
            // the sparse tree of one block's 2^M leaves: +0 everywhere but at the orbit residues (columns, ascending)
            const unsigned M = (unsigned)r->M;
            std::vector<std::pair<unsigned, unsigned>> nodes;          // (position at this level, slot)
            for (unsigned j = 0; j < r->compact_E.ncols; j++) nodes.push_back({r->compact_E.orbit[j], j});
            std::sort(nodes.begin(), nodes.end());
            for (unsigned h = 0; h < M; h++) {
                std::vector<std::pair<unsigned, unsigned>> up;
                for (size_t k = 0; k < nodes.size(); k++) {
                    if (k + 1 < nodes.size() && (nodes[k].first >> 1) == (nodes[k + 1].first >> 1)) {
                        P.prog_a[P.nprog] = (uint8_t)nodes[k].second; P.prog_b[P.nprog] = (uint8_t)nodes[k + 1].second; P.nprog++;
                        up.push_back({nodes[k].first >> 1, nodes[k].second});
                        k++;
                    } else
                        up.push_back({nodes[k].first >> 1, nodes[k].second});
                }
                nodes.swap(up);
            }
            if (nodes.size() != 1 || nodes[0].second != 0) {         // the root sits in the slot of the lowest residue: column 0
                snprintf(g_last_error, sizeof g_last_error, "compact orbit is not ascending");
                return QCX_UNKNOWN_ERROR;
            }
            P.cb = r->compact_E.cb; P.ncols = r->compact_E.ncols;
            hipLaunchKernelGGL(k_marginal<MARG_COMPACT>, dim3(grid), dim3(256), 0, r->stream, P);
        } else
            hipLaunchKernelGGL(k_marginal<MARG_AMP>, dim3(grid), dim3(256), 0, r->stream, P);
        HIP_TRY(hipGetLastError());
    }
    QCX_TRY(later_stages(r, st, 1, ns, r->marg_buf, out, bad));
    unsigned hbad = 0;
    HIP_TRY(hipMemcpyAsync(probs, out, nout * sizeof(double), hipMemcpyDeviceToHost, r->stream));
    if (compact) HIP_TRY(hipMemcpyAsync(&hbad, bad, sizeof(unsigned), hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    *bad_out = hbad != 0;
    return QCX_NO_ERROR;
}

// Behind an observer's checks and its basis shortcut: r->amp holds the state.  A compact result is expanded into the register's
// buffer (stale while the state is compact) and stays what later calls see; *source then says SRC_EXPANDED.
static int state_into_register(qcx_register *r, unsigned *source)
{
    QCX_TRY(settle_for_read(r));
    if (!r->compact_pending) return QCX_NO_ERROR;
    QCX_TRY(launch_expand_compact(r->compact_amp, r->amp, r->n, r->compact_E, r->stream));
    *source = SRC_EXPANDED;
    return QCX_NO_ERROR;
}

extern "C" int qcx_marginal_probabilities(qcx_register *r, unsigned first, unsigned num, double *probs)
{
    if (!r || !probs) return QCX_BAD_ARGUMENTS;
    if (r->sh) return QCX_UNSUPPORTED;
    if ((uint64_t)first + num > r->n) return QCX_BAD_QUBIT;
    if (num > 30) return QCX_UNSUPPORTED;
    r->marg = {SRC_REGISTER, 0};
    const uint64_t nout = (uint64_t)1 << num;
    if (basis_only(r)) {
        // 1 at the basis state's range value, +0 everywhere else -- no kernel, the state stays unwritten
        const uint64_t v = (r->basis_index >> first) & (nout - 1u);
        for (uint64_t i = 0; i < nout; i++) probs[i] = i == v ? 1.0 : 0.0;
        r->marg.source = SRC_BASIS;
        return QCX_NO_ERROR;
    }
    bool bad = false;
    if (first >= (unsigned)r->M) {
        QCX_TRY(settle_for_read(r));
        if (r->compact_pending) {                         // a range above the M register: the compact form in place
            QCX_TRY(marginal_launch(r, r->compact_amp, true, first, num, probs, &bad));
            r->marg = {SRC_COMPACT, 1};
            r->compact_measures++;
            if (!bad) return QCX_NO_ERROR;
            // a padding column that is not +0: the compact premise broke -- as qcx_measure_state_r, expand (same bits) and
            // read the register
            QCX_TRY(expand_pending(r));
        }
    } else
        QCX_TRY(state_into_register(r, &r->marg.source));
    QCX_TRY(marginal_launch(r, r->amp, false, first, num, probs, &bad));
    r->marg.reads += 1;
    if (r->marg.source == SRC_COMPACT) r->marg.source = SRC_EXPANDED;
    return QCX_NO_ERROR;
}

// the body of an observer's *_last_stats getter, on its ReadStats member of the register
static int last_stats(const qcx_register *r, const ReadStats qcx_register::*which, unsigned *source, unsigned long *state_reads)
{
    if (!r) return QCX_BAD_ARGUMENTS;
    if (source) *source = (r->*which).source;
    if (state_reads) *state_reads = (r->*which).reads;
    return QCX_NO_ERROR;
}

extern "C" int qcx_marginal_last_stats(qcx_register *r, unsigned *source, unsigned long *state_reads)
{
    return last_stats(r, &qcx_register::marg, source, state_reads);
}

// K14 / K14b: the stages of a Pauli string's value are those of qcx_marginal_plan(n, 0, 0) -- "sum everything" --, with a Pauli
// kernel in the place of stage 0.  row: the doubles of the non-final stages' outputs, one string's partials.
struct PauliStages { qcx_marginal_stage st[QCX_MARGINAL_MAX_STAGES]; unsigned ns, T; size_t row; };
static int pauli_stages(qcx_register *r, PauliStages *ps)
{
    ps->ns = 0;
    QCX_TRY(qcx_marginal_plan(r->n, 0, 0, ps->st, &ps->ns));
    const qcx_marginal_stage *st = ps->st;
    const unsigned T = ps->T = st[0].T;
    const uint64_t low = (((uint64_t)1) << T) - 1u;
    // what the Pauli kernels take for granted of stage 0: tiles of the T = min(n, 12) lowest bits, all summed, tile t -> output t
    if (st[0].kind != 0 || T != std::min(r->n, 12u) || st[0].tile_mask != low || st[0].sum_mask != low || st[0].out_bits != r->n - T) {
        set_error("qcx_pauli_expectation: unexpected first stage in the plan of n = %u", r->n);
        return QCX_UNKNOWN_ERROR;
    }
    ps->row = stages_scratch(st, ps->ns);
    return QCX_NO_ERROR;
}

// K14: <psi|P|psi> of the Pauli string (x, z) on the state in r->amp (include/qcx.h, DESIGN s4.5h); partials and result in marg_buf.
static int pauli_launch(qcx_register *r, uint64_t x, uint64_t z, double *value)
{
    PauliStages ps;
    QCX_TRY(pauli_stages(r, &ps));
    QCX_TRY(marg_reserve(r, ps.row + 2));
    double *const out = r->marg_buf + ps.row;
    const unsigned g = (unsigned)__builtin_popcountll(x & z) & 3u;
    const PauliUnits pu = pauli_units(r->n, x);                    // (pu.T == ps.T: checked against the plan)
    double *const dst0 = ps.st[0].final_stage ? out : r->marg_buf + ps.st[0].out_offset;
    pauli_dispatch(pu, [&](auto f) {
        hipLaunchKernelGGL((k_pauli_leaves<f.shape, f.full>), dim3((unsigned)std::min<uint64_t>(pu.nunits, 2048)), dim3(256), 0, r->stream, (const amp_t *)r->amp, dst0, pu.nunits, ps.T, x, z, g);
    });
    HIP_TRY(hipGetLastError());
    QCX_TRY(later_stages(r, ps.st, 1, ps.ns, r->marg_buf, out, nullptr));
    HIP_TRY(hipMemcpyAsync(value, out, sizeof(double), hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    return QCX_NO_ERROR;
}

// ---- K14b: the terms of a call that share an x_mask, QCX_PAULI_BATCH_W at the most, from one read of the state -------------------
extern "C" unsigned qcx_pauli_batch_width(void) { return QCX_PAULI_BATCH_W; }

// The passes of qcx_pauli_expectation_batch (include/qcx_plan.h): term k joins the open pass of its x_mask while that holds fewer
// than `width` terms, otherwise it opens a new one; passes are numbered in the order they are opened.
extern "C" int qcx_pauli_batch_plan(unsigned long nterms, const uint64_t *x_masks, unsigned width, unsigned long *pass_of_term,
                                    unsigned long *npasses)
{
    if (!npasses || width == 0 || (nterms && (!x_masks || !pass_of_term))) return QCX_BAD_ARGUMENTS;
    std::map<uint64_t, std::pair<unsigned long, unsigned>> open;     // x_mask -> (its open pass, terms in it)
    unsigned long np = 0;
    for (unsigned long k = 0; k < nterms; k++) {
        auto it = open.find(x_masks[k]);
        if (it == open.end() || it->second.second >= width) {
            open[x_masks[k]] = {np, 1u};
            pass_of_term[k] = np++;
        } else {
            it->second.second++;
            pass_of_term[k] = it->second.first;
        }
    }
    *npasses = np;
    return QCX_NO_ERROR;
}

// One pass: the K terms idx[0 .. K) of (xs, zs), all with the x_mask x.  k_pauli_leaves_batch writes term k's tile roots to row k
// of the stage buffer; the later stages are K14's, row by row, and the K results, side by side behind the rows, come back in
// one copy.
static int pauli_batch_launch(qcx_register *r, uint64_t x, unsigned K, const unsigned long *idx, const uint64_t *zs, double *values,
                              unsigned rows /* of the call's widest pass: one allocation for all of them */)
{
    PauliStages ps;
    QCX_TRY(pauli_stages(r, &ps));
    if (K == 0 || K > rows || rows > QCX_PAULI_BATCH_W) {
        set_error("qcx_pauli_expectation_batch: a pass of %u terms", K);
        return QCX_UNKNOWN_ERROR;
    }
    QCX_TRY(marg_reserve(r, (ps.row + 1) * rows));
    double *const out = r->marg_buf + ps.row * rows;
    const uint64_t low = (((uint64_t)1) << ps.T) - 1u;
    PauliBatchTerms tm = {};
    bool odd = false;
    for (unsigned k = 0; k < K; k++) {
        const uint64_t z = zs[idx[k]];
        const unsigned g = (unsigned)__builtin_popcountll(x & z) & 3u, xi = (unsigned)(x & low) & 15u, zi = (unsigned)(z & low) & 15u;
        unsigned iodd = 0;
        for (unsigned i = 0; i < 16; i++) iodd |= (unsigned)(__builtin_popcount((i ^ xi) & zi) & 1) << i;
        tm.z[k] = z;
        tm.meta[k] = iodd | g << 16;
        odd = odd || (g & 1u);
    }
    const PauliUnits pu = pauli_units(r->n, x);                    // (pu.T == ps.T: checked against the plan)
    double *const dst0 = ps.st[0].final_stage ? out : r->marg_buf + ps.st[0].out_offset;
    const uint64_t stride0 = ps.st[0].final_stage ? 1 : ps.row;
    const unsigned grid = (unsigned)std::min<uint64_t>(pu.nunits, 2048);
    pauli_dispatch(pu, [&](auto f) {
        if (odd) hipLaunchKernelGGL((k_pauli_leaves_batch<f.shape, f.full, true>), dim3(grid), dim3(256), 0, r->stream, (const amp_t *)r->amp, dst0, stride0, pu.nunits, ps.T, x, K, tm);
        else hipLaunchKernelGGL((k_pauli_leaves_batch<f.shape, f.full, false>), dim3(grid), dim3(256), 0, r->stream, (const amp_t *)r->amp, dst0, stride0, pu.nunits, ps.T, x, K, tm);
    });
    HIP_TRY(hipGetLastError());
    for (unsigned k = 0; k < K; k++) QCX_TRY(later_stages(r, ps.st, 1, ps.ns, r->marg_buf + k * ps.row, out + k, nullptr));
    double got[QCX_PAULI_BATCH_W];
    HIP_TRY(hipMemcpyAsync(got, out, K * sizeof(double), hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    for (unsigned k = 0; k < K; k++) values[idx[k]] = got[k];
    return QCX_NO_ERROR;
}

// the passes of qcx_pauli_batch_plan, in the order they were opened; values is not null here.  Every pass goes through K14b, a
// pass of one term too: it measured faster than K14 in every shape (DESIGN s4.5h).
static int pauli_batches(qcx_register *r, unsigned long nterms, const uint64_t *xs, const uint64_t *zs, double *values)
{
    std::vector<unsigned long> pass_of(nterms);
    unsigned long np = 0;
    QCX_TRY(qcx_pauli_batch_plan(nterms, xs, QCX_PAULI_BATCH_W, pass_of.data(), &np));
    std::vector<std::vector<unsigned long>> members(np);
    for (unsigned long k = 0; k < nterms; k++) members[pass_of[k]].push_back(k);
    size_t rows = 1;
    for (unsigned long p = 0; p < np; p++) rows = std::max(rows, members[p].size());
    for (unsigned long p = 0; p < np; p++) {
        const std::vector<unsigned long> &m = members[p];
        QCX_TRY(pauli_batch_launch(r, xs[m[0]], (unsigned)m.size(), m.data(), zs, values, (unsigned)rows));
        r->exp.reads += 1;
    }
    return QCX_NO_ERROR;
}

// the terms of one call, in order; values may be null (not with batch).  Everything is checked before anything runs.
// batch: the terms run as the passes of qcx_pauli_expectation_batch, otherwise one by one.
static int pauli_terms(qcx_register *r, unsigned long nterms, const uint64_t *xs, const uint64_t *zs, double *values, bool batch = false)
{
    for (unsigned long k = 0; k < nterms; k++)
        if ((xs[k] | zs[k]) >> r->n) {
            set_error("qcx_pauli_expectation: masks %#llx / %#llx reach past the %u qubits", (unsigned long long)xs[k],
                      (unsigned long long)zs[k], r->n);
            return QCX_BAD_QUBIT;
        }
    r->exp = {SRC_REGISTER, 0};
    if (nterms == 0) return QCX_NO_ERROR;
    if (basis_only(r)) {
        // amplitude 1 at basis_index: a string with an X or a Y has no diagonal entry there, a Z-type one reads the parity
        for (unsigned long k = 0; k < nterms; k++) {
            const double v = xs[k] ? 0.0 : ((__builtin_popcountll(r->basis_index & zs[k]) & 1) ? -1.0 : 1.0);
            if (values) values[k] = v;
        }
        r->exp.source = SRC_BASIS;
        return QCX_NO_ERROR;
    }
    QCX_TRY(state_into_register(r, &r->exp.source));
    if (batch) return pauli_batches(r, nterms, xs, zs, values);
    for (unsigned long k = 0; k < nterms; k++) {
        double v = 0.0;
        QCX_TRY(pauli_launch(r, xs[k], zs[k], &v));
        r->exp.reads += 1;
        if (values) values[k] = v;
    }
    return QCX_NO_ERROR;
}

extern "C" int qcx_pauli_expectation(qcx_register *r, uint64_t x_mask, uint64_t z_mask, double *value)
{
    if (!r || !value) return QCX_BAD_ARGUMENTS;
    if (r->sh) return QCX_UNSUPPORTED;
    return pauli_terms(r, 1, &x_mask, &z_mask, value);
}

// qcx_pauli_expectation_sum and qcx_pauli_expectation_batch: the same call but for how the terms share reads of the state
static int pauli_sum(qcx_register *r, unsigned long nterms, const uint64_t *x_masks, const uint64_t *z_masks, const double *coeffs,
                     double *values, double *total, bool batch)
{
    if (!r || !total || (nterms && (!x_masks || !z_masks || !coeffs))) return QCX_BAD_ARGUMENTS;
    if (r->sh) return QCX_UNSUPPORTED;
    std::vector<double> own;
    if (!values && nterms) { own.resize(nterms); values = own.data(); }
    QCX_TRY(pauli_terms(r, nterms, x_masks, z_masks, values, batch));
    double acc = 0.0;
    for (unsigned long k = 0; k < nterms; k++) acc = acc + coeffs[k] * values[k];      // (each rounded on its own: -ffp-contract=off)
    *total = acc;
    return QCX_NO_ERROR;
}

extern "C" int qcx_pauli_expectation_sum(qcx_register *r, unsigned long nterms, const uint64_t *x_masks, const uint64_t *z_masks,
                                         const double *coeffs, double *values, double *total)
{
    return pauli_sum(r, nterms, x_masks, z_masks, coeffs, values, total, false);
}

extern "C" int qcx_pauli_expectation_batch(qcx_register *r, unsigned long nterms, const uint64_t *x_masks, const uint64_t *z_masks,
                                           const double *coeffs, double *values, double *total)
{
    return pauli_sum(r, nterms, x_masks, z_masks, coeffs, values, total, true);
}

extern "C" int qcx_expectation_last_stats(qcx_register *r, unsigned *source, unsigned long *state_reads)
{
    return last_stats(r, &qcx_register::exp, source, state_reads);
}

// ---- K16: the reduced density matrix of bits [first, first + num) (include/qcx.h, DESIGN s4.5j) -----------------------------------
// Stage 0 reads the state in r->amp once and writes every component's partial roots; the planned marginal stages take all rows
// through each launch; the 4^num components come back in one copy.
static int rdm_launch(qcx_register *r, unsigned first, unsigned num, double *comps)
{
    qcx_rdm_stage0 s0;
    qcx_marginal_stage st[QCX_MARGINAL_MAX_STAGES];
    unsigned ns = 0;
    QCX_TRY(qcx_rdm_plan(r->n, first, num, &s0, st, &ns));
    QCX_TRY(marg_reserve(r, (size_t)s0.scratch + s0.rows));
    double *const out = r->marg_buf + s0.scratch;
    double *const dst0 = ns ? r->marg_buf : out;
    const uint64_t stride0 = ns ? s0.row_stride : 1, ngroups = s0.row_stride;
    const unsigned grid = (unsigned)std::min<uint64_t>(ngroups, 2048), ug = s0.group_bits;
    const amp_t *amp = (const amp_t *)r->amp;
    if (r->n < 12)
        hipLaunchKernelGGL(k_rdm_small, dim3(1), dim3(256), 0, r->stream, amp, dst0, r->n, first, num);
    else {
        // EXCH: the range begins below the 12 - num summed bits of a unit, so a unit is 2^12 consecutive amplitudes
        const bool exch = first < 12u - num;
#define QCX_RDM_LAUNCH(NUM) \
        do { \
            if (exch) hipLaunchKernelGGL((k_rdm_leaves<NUM, true>), dim3(grid), dim3(256), 0, r->stream, amp, dst0, stride0, ngroups, ug, first); \
            else hipLaunchKernelGGL((k_rdm_leaves<NUM, false>), dim3(grid), dim3(256), 0, r->stream, amp, dst0, stride0, ngroups, ug, first); \
        } while (0)
        switch (num) {
        case 0: QCX_RDM_LAUNCH(0); break;
        case 1: QCX_RDM_LAUNCH(1); break;
        case 2: QCX_RDM_LAUNCH(2); break;
        case 3: QCX_RDM_LAUNCH(3); break;
        default: QCX_RDM_LAUNCH(4); break;
        }
#undef QCX_RDM_LAUNCH
    }
    HIP_TRY(hipGetLastError());
    QCX_TRY(later_stages(r, st, 0, ns, r->marg_buf, out, nullptr));
    HIP_TRY(hipMemcpyAsync(comps, out, s0.rows * sizeof(double), hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    return QCX_NO_ERROR;
}

extern "C" int qcx_reduced_density_matrix(qcx_register *r, unsigned first, unsigned num, double *rho)
{
    if (!r || !rho) return QCX_BAD_ARGUMENTS;
    if (r->sh) return QCX_UNSUPPORTED;
    if ((uint64_t)first + num > r->n) return QCX_BAD_QUBIT;
    if (num > QCX_RDM_MAX_QUBITS) return QCX_UNSUPPORTED;
    r->rdm = {SRC_REGISTER, 0};
    const unsigned nv = 1u << num;
    if (basis_only(r)) {
        // amplitude 1 at basis_index: the projector on its range value -- no kernel, the state stays unwritten
        const unsigned v = (unsigned)((r->basis_index >> first) & (nv - 1u));
        for (unsigned i = 0; i < 2u * nv * nv; i++) rho[i] = 0.0;
        rho[2u * (v * nv + v)] = 1.0;
        r->rdm.source = SRC_BASIS;
        return QCX_NO_ERROR;
    }
    QCX_TRY(state_into_register(r, &r->rdm.source));
    double comps[1u << (2 * QCX_RDM_MAX_QUBITS)];
    QCX_TRY(rdm_launch(r, first, num, comps));
    r->rdm.reads = 1;
    // row v nv + w, v <= w, holds Re rho[v][w], row w nv + v its imaginary part; the lower triangle is the conjugate
    for (unsigned v = 0; v < nv; v++) {
        rho[2u * (v * nv + v)] = comps[v * nv + v];
        rho[2u * (v * nv + v) + 1u] = 0.0;
        for (unsigned w = v + 1u; w < nv; w++) {
            const double re = comps[v * nv + w], im = comps[w * nv + v];
            rho[2u * (v * nv + w)] = re; rho[2u * (v * nv + w) + 1u] = im;
            rho[2u * (w * nv + v)] = re; rho[2u * (w * nv + v) + 1u] = 0.0 - im;
        }
    }
    return QCX_NO_ERROR;
}

extern "C" int qcx_rdm_last_stats(qcx_register *r, unsigned *source, unsigned long *state_reads)
{
    return last_stats(r, &qcx_register::rdm, source, state_reads);
}

// K11: measure or post-select the qubits [first, first + num) and collapse the state (include/qcx.h, DESIGN s4.5e).  Two passes:
// the marginal above gives P (its code path, its summation order), the host picks the outcome by the scan of Q:283-292 on P, then
// k_collapse_range rewrites the state in the register's current buffer.
static int launch_collapse(qcx_register *r, unsigned first, unsigned num, uint64_t outcome, double s)
{
    const Tune tn = tune_now();
    const bool perm = tn.collapse_perm && first >= 3 && first < 6 && num >= 1 && r->n >= num + 6;
    const unsigned U = tn.collapse_upt == 8 ? 8u : 4u;
    const unsigned grid = grid_for(r->dim, 256 * U, tn.collapse_grid_cap, 256);
#define QCX_COLLAPSE(PERM, UPT) hipLaunchKernelGGL((k_collapse_range<PERM, UPT>), dim3(grid), dim3(256), 0, r->stream, r->amp, r->dim, first, num, outcome, s)
    if (perm) { if (U == 8) QCX_COLLAPSE(true, 8); else QCX_COLLAPSE(true, 4); }
    else { if (U == 8) QCX_COLLAPSE(false, 8); else QCX_COLLAPSE(false, 4); }
#undef QCX_COLLAPSE
    HIP_TRY(hipGetLastError());
    return QCX_NO_ERROR;
}

// rnd is used when `given` is null (the measure forms), else *given is the caller's outcome (post-selection)
static int collapse_range(qcx_register *r, unsigned first, unsigned num, double rnd, const unsigned long *given,
                          unsigned long *outcome_out, double *prob_out)
{
    if ((uint64_t)first + num > r->n) return QCX_BAD_QUBIT;
    if (num > 30) return QCX_UNSUPPORTED;
    const uint64_t nout = (uint64_t)1 << num;
    if (given && (uint64_t)*given >= nout) {
        set_error("qcx_postselect_qubits: outcome %lu does not fit %u qubits", *given, num);
        return QCX_BAD_ARGUMENTS;
    }
    r->coll = {SRC_REGISTER, 0}; r->coll_writes = 0;
    const bool was_basis = basis_only(r);
    std::vector<double> P(nout);
    QCX_TRY(qcx_marginal_probabilities(r, first, num, P.data()));
    r->coll.reads = r->marg.reads;
    r->coll.source = was_basis ? SRC_BASIS : (r->marg.source == SRC_COMPACT || r->marg.source == SRC_EXPANDED) ? SRC_EXPANDED : SRC_REGISTER;
    uint64_t v = nout - 1;                                                  // Q:283 fall-through
    if (given) v = *given;
    else {
        double cum = 0.0;
        for (uint64_t k = 0; k + 1 < nout; k++) {
            cum += P[k];                                                    // Q:286-287 on the range's values
            if (cum >= rnd) { v = k; break; }
        }
    }
    const double p = P[v];
    if (outcome_out) *outcome_out = (unsigned long)v;
    if (prob_out) *prob_out = p;
    const double s = 1.0 / sqrt(p);
    if (!(p > 0.0) || !std::isfinite(p) || !std::isfinite(s)) {
        set_error("qubits [%u, %u): outcome %lu has probability %.17g: the state cannot be collapsed onto it", first, first + num,
                  (unsigned long)v, p);
        return QCX_BAD_ARGUMENTS;
    }
    if (was_basis) return QCX_NO_ERROR;                                     // P = 1, s = 1: the pending basis state is the result
    QCX_TRY(expand_pending(r));                                             // (a compact result: collapsed in the register)
    QCX_TRY(launch_collapse(r, first, num, v, s));
    r->coll_writes = 1;
    r->zeros_dirty = 1;                                                     // kept -0 stay -0, products may underflow to -0: as caller data
    return QCX_NO_ERROR;
}

extern "C" int qcx_measure_qubits_r(qcx_register *r, unsigned first, unsigned num, double rnd, unsigned long *outcome, double *probability)
{
    if (!r || !outcome) return QCX_BAD_ARGUMENTS;
    if (r->sh) return QCX_UNSUPPORTED;
    return collapse_range(r, first, num, rnd, nullptr, outcome, probability);
}

extern "C" int qcx_measure_qubits(qcx_register *r, qcx_rng *rng, unsigned first, unsigned num, unsigned long *outcome, double *probability)
{
    if (!r || !rng || !outcome) return QCX_BAD_ARGUMENTS;
    if (r->sh) return QCX_UNSUPPORTED;
    if ((uint64_t)first + num > r->n) return QCX_BAD_QUBIT;                 // (no draw for a call that cannot run)
    if (num > 30) return QCX_UNSUPPORTED;
    return collapse_range(r, first, num, qcx_rng_uniform(rng), nullptr, outcome, probability);   // Q:281
}

extern "C" int qcx_postselect_qubits(qcx_register *r, unsigned first, unsigned num, unsigned long outcome, double *probability)
{
    if (!r) return QCX_BAD_ARGUMENTS;
    if (r->sh) return QCX_UNSUPPORTED;
    return collapse_range(r, first, num, 0.0, &outcome, nullptr, probability);
}

// diagnostics (tools/time_measure_qubits.py): the collapse pass alone, on the register's current state
extern "C" int qcx_collapse_pass(qcx_register *r, unsigned first, unsigned num, unsigned long outcome, double s)
{
    if (!r || r->sh) return QCX_BAD_ARGUMENTS;
    if ((uint64_t)first + num > r->n || num > 30 || (uint64_t)outcome >= ((uint64_t)1 << num)) return QCX_BAD_ARGUMENTS;
    FLUSH(r);
    r->zeros_dirty = 1;
    return launch_collapse(r, first, num, outcome, s);
}

extern "C" int qcx_collapse_last_stats(qcx_register *r, unsigned *source, unsigned long *state_reads, unsigned long *state_writes)
{
    QCX_TRY(last_stats(r, &qcx_register::coll, source, state_reads));
    if (state_writes) *state_writes = r->coll_writes;
    return QCX_NO_ERROR;
}

extern "C" int qcx_state_read(qcx_register *r, unsigned long first, unsigned long count, double *out)
{
    if (!r || (!out && count)) return QCX_BAD_ARGUMENTS;
    if ((uint64_t)first > r->dim || (uint64_t)count > r->dim - first) return QCX_BAD_ARGUMENTS;
    if (r->sh) return sh_copy(r->sh, first, count, out, true);
    FLUSH(r);
    HIP_TRY(hipStreamSynchronize(r->stream));
    if (count) HIP_TRY(hipMemcpy(out, r->amp + first, (size_t)count * sizeof(amp_t), hipMemcpyDeviceToHost));
    return QCX_NO_ERROR;
}

extern "C" int qcx_state_write(qcx_register *r, unsigned long first, unsigned long count, const double *in)
{
    if (!r || (!in && count)) return QCX_BAD_ARGUMENTS;
    if ((uint64_t)first > r->dim || (uint64_t)count > r->dim - first) return QCX_BAD_ARGUMENTS;
    if (r->sh) return sh_copy(r->sh, first, count, const_cast<double *>(in), false);
    FLUSH(r);
    HIP_TRY(hipStreamSynchronize(r->stream));
    if (count) {
        HIP_TRY(hipMemcpy(r->amp + first, in, (size_t)count * sizeof(amp_t), hipMemcpyHostToDevice));
        r->zeros_dirty = 1;
        QCX_TRY(note_nonfinite(r, first, count));
    }
    return QCX_NO_ERROR;
}

// ---- state files (golden-vector I/O, debugging, checkpoint) -------------------------------
// 64-byte header, then the 2^n amplitudes as interleaved little-endian binary64 (re, im), index order.  Streamed
// through a pinned staging buffer, so a 16 GiB state needs 64 MiB of host memory.  The checksum is FNV-1a 64 over the
// payload bytes.  The payload goes straight to the device chunk by chunk, so a load that fails half-way (truncated
// file, checksum mismatch) leaves a partial copy in the register and says so (QCX_UNKNOWN_ERROR + qcx_last_error).
struct StateFileHeader {
    char     magic[8];          // "QCXSTATE"
    uint32_t version;           // 1
    uint32_t bytes_per_amp;     // 16
    int32_t  L, M;
    uint64_t dim;               // 2^(L+M)
    uint64_t checksum;          // FNV-1a 64 of the payload
    uint8_t  pad[24];
};
static_assert(sizeof(StateFileHeader) == 64, "state file header");

static uint64_t fnv1a64(const unsigned char *p, size_t len, uint64_t h)
{
    for (size_t k = 0; k < len; k++) { h ^= p[k]; h *= 0x100000001b3ull; }
    return h;
}

extern "C" int qcx_state_save(qcx_register *r, const char *path)
{
    if (!r || !path) return QCX_BAD_ARGUMENTS;
    if (r->sh) QCX_TRY(sh_identity(r->sh)); else { FLUSH(r); HIP_TRY(hipStreamSynchronize(r->stream)); }
    FILE *f = fopen(path, "wb");
    if (!f) { set_error("qcx_state_save: cannot open %s", path); return QCX_BAD_ARGUMENTS; }
    StateFileHeader h;
    memset(&h, 0, sizeof h);
    memcpy(h.magic, "QCXSTATE", 8); h.version = 1; h.bytes_per_amp = (uint32_t)sizeof(amp_t);
    h.L = r->L; h.M = r->M; h.dim = r->dim;
    int st = QCX_NO_ERROR;
    void *stage = nullptr;
    const size_t chunk = (size_t)std::min<uint64_t>(r->dim, (uint64_t)1 << 22);          // 4 Mi amplitudes = 64 MiB
    if (hipHostMalloc(&stage, chunk * sizeof(amp_t)) != hipSuccess) { fclose(f); return QCX_INSUFFICIENT_MEMORY; }
    uint64_t sum = 0xcbf29ce484222325ull;
    if (fwrite(&h, sizeof h, 1, f) != 1) st = QCX_UNKNOWN_ERROR;
    for (uint64_t at = 0; st == QCX_NO_ERROR && at < r->dim; at += chunk) {
        const size_t cnt = (size_t)std::min<uint64_t>(chunk, r->dim - at);
        if (r->sh ? sh_copy(r->sh, at, cnt, (double *)stage, true) != QCX_NO_ERROR
                  : hipMemcpy(stage, r->amp + at, cnt * sizeof(amp_t), hipMemcpyDeviceToHost) != hipSuccess) { st = QCX_HIP_ERROR; break; }
        sum = fnv1a64((const unsigned char *)stage, cnt * sizeof(amp_t), sum);
        if (fwrite(stage, sizeof(amp_t), cnt, f) != cnt) st = QCX_UNKNOWN_ERROR;
    }
    if (st == QCX_NO_ERROR) {
        h.checksum = sum;
        if (fseek(f, 0, SEEK_SET) != 0 || fwrite(&h, sizeof h, 1, f) != 1) st = QCX_UNKNOWN_ERROR;
    }
    (void)hipHostFree(stage);
    if (fclose(f) != 0 && st == QCX_NO_ERROR) st = QCX_UNKNOWN_ERROR;
    if (st != QCX_NO_ERROR) set_error("qcx_state_save: writing %s failed", path);
    return st;
}

extern "C" int qcx_state_load(qcx_register *r, const char *path)
{
    if (!r || !path) return QCX_BAD_ARGUMENTS;
    if (r->sh) QCX_TRY(sh_identity(r->sh)); else { FLUSH(r); HIP_TRY(hipStreamSynchronize(r->stream)); }
    r->zeros_dirty = 1;                              // (a sharded register: sh_copy notes it per set)
    FILE *f = fopen(path, "rb");
    if (!f) { set_error("qcx_state_load: cannot open %s", path); return QCX_BAD_ARGUMENTS; }
    StateFileHeader h;
    if (fread(&h, sizeof h, 1, f) != 1 || memcmp(h.magic, "QCXSTATE", 8) != 0 || h.version != 1 || h.bytes_per_amp != sizeof(amp_t)) {
        fclose(f); set_error("qcx_state_load: %s is not a state file of this version", path); return QCX_BAD_ARGUMENTS;
    }
    if (h.L != r->L || h.M != r->M || h.dim != r->dim) {
        fclose(f); set_error("qcx_state_load: %s holds L=%d M=%d, the register is L=%d M=%d", path, h.L, h.M, r->L, r->M);
        return QCX_BAD_ARGUMENTS;
    }
    void *stage = nullptr;
    const size_t chunk = (size_t)std::min<uint64_t>(r->dim, (uint64_t)1 << 22);
    if (hipHostMalloc(&stage, chunk * sizeof(amp_t)) != hipSuccess) { fclose(f); return QCX_INSUFFICIENT_MEMORY; }
    int st = QCX_NO_ERROR;
    uint64_t sum = 0xcbf29ce484222325ull;
    for (uint64_t at = 0; st == QCX_NO_ERROR && at < r->dim; at += chunk) {
        const size_t cnt = (size_t)std::min<uint64_t>(chunk, r->dim - at);
        if (fread(stage, sizeof(amp_t), cnt, f) != cnt) { st = QCX_UNKNOWN_ERROR; break; }
        sum = fnv1a64((const unsigned char *)stage, cnt * sizeof(amp_t), sum);
        if (r->sh ? sh_copy(r->sh, at, cnt, (double *)stage, false) != QCX_NO_ERROR
                  : hipMemcpy(r->amp + at, stage, cnt * sizeof(amp_t), hipMemcpyHostToDevice) != hipSuccess) st = QCX_HIP_ERROR;
    }
    (void)hipHostFree(stage);
    fclose(f);
    if (st == QCX_NO_ERROR && sum != h.checksum) st = QCX_UNKNOWN_ERROR;
    if (st != QCX_NO_ERROR) set_error("qcx_state_load: %s is truncated or corrupt (the register now holds a partial copy)", path);
    if (!r->sh) { const int nf = note_nonfinite(r, 0, r->dim); if (st == QCX_NO_ERROR) st = nf; }
    return st;
}

extern "C" int qcx_norm2(qcx_register *r, double *out)
{
    if (!r || !out) return QCX_BAD_ARGUMENTS;
    if (r->sh) return sh_norm2(r->sh, out);
    FLUSH(r);
    return qcx_shard_norm2(r->amp, r->n, out, r->stream);
}

// T:28-37 exactly: the reference's check_normalisation adds |amp|^2 one by one in index order.  The exact scan of the
// measurement (run to the end: r = +inf is never reached) returns that very sum, bit for bit; qcx_norm2 above is the
// faster tree sum.
extern "C" int qcx_total_probability(qcx_register *r, double *out)
{
    if (!r || !out) return QCX_BAD_ARGUMENTS;
    int found = 0; uint64_t idx = 0; double cum = 0.0;
    if (r->sh) {
        ShardSet *sh = r->sh;
        QCX_TRY(sh_identity(sh));
        if (sh->dry) return QCX_UNSUPPORTED;
        QCX_TRY(sh_sync(sh));
        for (unsigned s = 0; s < sh->W; s++) {
            HIP_TRY(hipSetDevice(sh->dev[s]));
            double c2 = cum;
            QCX_TRY(qcx_shard_measure_scan(sh->buf[sh->cur][s], sh->n_local, (uint64_t)s << sh->n_local, r->dim, cum, INFINITY,
                                           &found, &idx, &c2, sh->st[s]));
            cum = c2;
        }
        *out = cum;
        return QCX_NO_ERROR;
    }
    FLUSH(r);
    QCX_TRY(qcx_shard_measure_scan(r->amp, r->n, 0, r->dim, 0.0, INFINITY, &found, &idx, &cum, r->stream));
    *out = cum;
    return QCX_NO_ERROR;
}

extern "C" int qcx_state_fill_random(qcx_register *r, uint64_t seed)
{
    if (!r) return QCX_BAD_ARGUMENTS;
    if (r->sh) return sh_fill_random(r->sh, seed);
    if (r->queue) r->queue->gates.clear();
    r->basis_pending = 0;                           // everything is overwritten
    r->compact_pending = 0;
    r->nonfinite = 0;
    r->zeros_dirty = 0;
    // U(-0.5, 0.5) components have variance 1/12: this scale makes the expected norm 1
    return qcx_shard_fill_random(r->amp, r->n, 0, seed, sqrt(6.0 / (double)r->dim), r->stream);
}

// a pool of HIP events on the register's stream: record between gates inside a timed region,
// read the differences afterwards (per-kernel durations for the roofline, bench.py)
extern "C" int qcx_events_create(qcx_register *r, unsigned count)
{
    if (!r || count > 65536) return QCX_BAD_ARGUMENTS;
    if (r->sh) return QCX_UNSUPPORTED;               // per-gate event pools are a single-GPU bench tool; use qcx_timer_start/stop
    for (unsigned i = 0; i < r->n_events; i++) (void)hipEventDestroy(r->events[i]);
    free(r->events);
    r->events = nullptr; r->n_events = 0;
    if (count == 0) return QCX_NO_ERROR;
    r->events = (hipEvent_t *)calloc(count, sizeof(hipEvent_t));
    if (!r->events) return QCX_INSUFFICIENT_MEMORY;
    for (unsigned i = 0; i < count; i++) { HIP_TRY(hipEventCreate(&r->events[i])); r->n_events = i + 1; }
    return QCX_NO_ERROR;
}

extern "C" int qcx_event_record(qcx_register *r, unsigned slot)
{
    if (!r || slot >= r->n_events) return QCX_BAD_ARGUMENTS;
    FLUSH(r);
    HIP_TRY(hipEventRecord(r->events[slot], r->stream));
    return QCX_NO_ERROR;
}

extern "C" int qcx_event_elapsed(qcx_register *r, unsigned from_slot, unsigned to_slot, double *ms)
{
    if (!r || !ms || from_slot >= r->n_events || to_slot >= r->n_events) return QCX_BAD_ARGUMENTS;
    HIP_TRY(hipEventSynchronize(r->events[to_slot]));
    float f = 0.f;
    HIP_TRY(hipEventElapsedTime(&f, r->events[from_slot], r->events[to_slot]));
    *ms = (double)f;
    return QCX_NO_ERROR;
}

extern "C" int qcx_timer_start(qcx_register *r)
{
    if (!r) return QCX_BAD_ARGUMENTS;
    if (r->sh) {                                     // all shards idle, then the start event on shard 0's stream
        if (r->sh->dry) return QCX_UNSUPPORTED;
        QCX_TRY(sh_sync(r->sh));
        HIP_TRY(hipSetDevice(r->sh->dev[0]));
        HIP_TRY(hipEventRecord(r->ev0, r->sh->st[0]));
        return QCX_NO_ERROR;
    }
    FLUSH(r);
    HIP_TRY(hipEventRecord(r->ev0, r->stream));
    return QCX_NO_ERROR;
}

extern "C" int qcx_timer_stop(qcx_register *r, double *ms)
{
    if (!r || !ms) return QCX_BAD_ARGUMENTS;
    if (r->sh) {                                     // everything queued has run on every shard, then the stop event
        if (r->sh->dry) return QCX_UNSUPPORTED;
        QCX_TRY(sh_sync(r->sh));
        HIP_TRY(hipSetDevice(r->sh->dev[0]));
        HIP_TRY(hipEventRecord(r->ev1, r->sh->st[0]));
        HIP_TRY(hipEventSynchronize(r->ev1));
        float f = 0.f;
        HIP_TRY(hipEventElapsedTime(&f, r->ev0, r->ev1));
        *ms = (double)f;
        return QCX_NO_ERROR;
    }
    FLUSH(r);
    HIP_TRY(hipEventRecord(r->ev1, r->stream));
    HIP_TRY(hipEventSynchronize(r->ev1));
    float f = 0.f;
    HIP_TRY(hipEventElapsedTime(&f, r->ev0, r->ev1));
    *ms = (double)f;
    return QCX_NO_ERROR;
}

// ---------------------------------------------------------------------------
// MT19937 with gsl_rng_mt19937 semantics (GSL 2.6 rng/mt.c: 2002 seeding, seed 0 -> 4357,
// uniform = u32 / 2^32).  Restated from the published generator definition.
// ---------------------------------------------------------------------------
struct qcx_rng {
    uint32_t s[624];
    int pos;
};

extern "C" qcx_rng *qcx_rng_alloc(void)
{
    qcx_rng *g = (qcx_rng *)malloc(sizeof(qcx_rng));
    if (g) qcx_rng_set(g, 0);
    return g;
}

extern "C" void qcx_rng_free(qcx_rng *g) { free(g); }

extern "C" void qcx_rng_set(qcx_rng *g, unsigned long seed)
{
    uint32_t v = (uint32_t)(seed & 0xffffffffUL);
    if (v == 0) v = 4357u;
    for (int i = 0; i < 624; i++) {
        g->s[i] = v;
        v = 1812433253u * (v ^ (v >> 30)) + (uint32_t)(i + 1);
    }
    g->pos = 624;
}

extern "C" unsigned long qcx_rng_get(qcx_rng *g)
{
    if (g->pos == 624) {
        uint32_t *s = g->s;
        auto twist = [](uint32_t u, uint32_t v) { uint32_t y = (u & 0x80000000u) | (v & 0x7fffffffu); return (y >> 1) ^ ((v & 1u) ? 0x9908b0dfu : 0u); };
        int k = 0;
        for (; k < 624 - 397; k++) s[k] = s[k + 397] ^ twist(s[k], s[k + 1]);
        for (; k < 623; k++)       s[k] = s[k + 397 - 624] ^ twist(s[k], s[k + 1]);
        s[623] = s[396] ^ twist(s[623], s[0]);
        g->pos = 0;
    }
    uint32_t y = g->s[g->pos++];
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    return (unsigned long)y;
}

extern "C" double qcx_rng_uniform(qcx_rng *g) { return (double)qcx_rng_get(g) / 4294967296.0; }
